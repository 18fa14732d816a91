// Conv3x3 weight gradient for narrow channels — direct MFMA kernel, gfx950.
//
//   dW[co,ky,kx,ci] = sum_{img,y,x} dy[img,y,x,co] * x[img,y+ky-1,x+kx-1,ci]
//   db[co]          = sum dy[...,co]                          (when asked)
//
// 3x3, stride 1, SAME; bf16 operands, fp32 accumulation and results;
// Cin % 32 == 0, Cout % 32 == 0, Cout <= 128, any H, W >= 1. This is the
// wgrad of the convs conv3x3_halo.hip runs forward; conv3x3_wgrad.hip keeps
// the wide shapes (its block is a fixed 128 co x 64 ci tile).
//
// Per tap the GEMM is M x N = Cout x Cin (tiny) with K = every pixel of the
// batch (10^6 at the bench shape), so the kernel is bound by the bytes of x
// and dy and is built to move each of them once:
//
//  * Wave tile: 32 co x 32 ci for all nine taps — nine
//    mfma_f32_32x32x16_bf16 accumulators (144 fp32), K step = 16 pixels of
//    one image row. Both operands are pixel-major, so both fragments come
//    from row-major pixel images in LDS through ds_read_b64_tr_b16. ky pairs
//    dy row r with x rows r-1, r, r+1 of an LDS ring; kx is a one-pixel
//    address shift against an x row staged with a one-pixel halo. Rows -1
//    and H of an image are staged as zeros, so every step issues all nine
//    MFMAs without a branch. (The tap scheme of conv3x3_wgrad.hip.)
//  * Block: all of Cout x a ci tile of 32 (Cin % 64 != 0) or 64 channels:
//    NT = (Cout/32) x (ci tile/32) wave tiles. With NT < 8 the block runs
//    KS = 8/NT waves per tile, and these split the K steps of every staged
//    round among them (step j goes to wave j % KS): an intra-block split-K
//    on the same staged bytes. Their accumulators are summed through LDS in
//    log2(KS) halving rounds, so a block issues one set of global atomics.
//  * Grid: ci tiles x split-K over contiguous (image, row) ranges, one block
//    per CU (144 accumulators + fragments allow two waves per SIMD, which
//    is one 8-wave block). Blocks of one range (different ci tiles) are kept
//    on one XCD by the bijective remap, so the re-read of dy hits its L2.
//    A block walks its range with the accumulators in registers and flushes
//    once with fp32 atomicAdd into the zeroed (Cout,3,3,Cin) result.
//  * Staging: global_load_lds, 16 B per lane. The next round's rows are
//    issued before the MFMAs of the current one. A round holds gr rows
//    (128-256 pixels) so that short rows still give every wave a K step.
//  * LDS layout: pixel rows are unpadded (stride = 2*C bytes). A transpose
//    read serves 32 lanes from 4 pixel rows x 64 contiguous bytes; the four
//    rows must fall in the four 64 B quarters of the 256 B bank line. Strides
//    of 64 and 192 B do that as they are. At 128 and 256 B the 64 B units of
//    a pixel row are XOR-swizzled by the pixel index ((p>>1)&1, resp. p&3):
//    the staging lanes fetch the swizzled source unit (the LDS side of
//    global_load_lds stays 1 KiB contiguous per wave), the reads add the
//    same term, which is a per-lane constant per kx.
//
// No scalar stores, no printf/assert; out-of-image pixels are loaded from a
// zero buffer, and a tile is addressed inside its own image only.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "common.h"

namespace {

struct WnShape {
  int IMG, H, W, Cin, Cout;
  int PW;       // column-tile width: min(ceil16(W), 128)
  int nks;      // K steps per tile row = PW / 16
  int nct;      // column tiles per row
  int gr;       // rows staged per barrier round
  int rs;       // x ring slots, power of two >= 2*gr + 2
  int units;    // IMG * H * nct row tiles
  int nb_n;     // ci tiles
  int sk;       // split-K factor over unit ranges
  int with_bias;
};

// 64 B unit swizzle of a pixel row of `S` bytes, by pixel index
template <int S>
__device__ __forceinline__ int unit_swz(int pixel) {
  if (S == 128) return (pixel >> 1) & 1;
  if (S == 256) return pixel & 3;
  return 0;
}

// NCO = Cout/32, NCI = ci tile/32
template <int NCO, int NCI>
__global__ __launch_bounds__(64 * (NCO * NCI) * (8 / (NCO * NCI)))
void conv3x3_wgrad_narrow_kernel(const bf16* __restrict__ x,
                                 const bf16* __restrict__ dy,
                                 const bf16* __restrict__ zbuf,
                                 float* __restrict__ dwacc,
                                 float* __restrict__ dbacc,
                                 WnShape s) {
  constexpr int NT = NCO * NCI;
  constexpr int KS = 8 / NT;   // 8,4,2,2,1,1 for NT 1,2,3,4,6,8
  constexpr int NW = NT * KS;
  constexpr int SDY = NCO * 64;             // bytes per staged dy pixel
  constexpr int SX = NCI * 64;              // bytes per staged x pixel

  // block decode with the bijective XCD remap: ids that share a range
  // (different ci tiles) are consecutive after the remap, i.e. on one XCD
  int bid = blockIdx.x;
  {
    const int nwg = s.sk * s.nb_n;
    const int q = nwg / 8, r = nwg % 8;
    const int xcd = bid % 8, idx = bid / 8;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  const int bn = bid % s.nb_n;
  const int sk = bid / s.nb_n;
  const int ci0 = bn * (NCI * 32);

  const int per = (s.units + s.sk - 1) / s.sk;
  const int u0 = sk * per;
  const int u1 = min(s.units, u0 + per);
  if (u0 >= u1) return;   // whole block, before any barrier

  extern __shared__ __attribute__((aligned(16))) char smem[];
  // layout: [dy buf 0][dy buf 1][x slot 0 .. rs-1]
  const int dy_bytes = s.gr * s.PW * SDY;
  const int x_bytes = (s.PW + 2) * SX;
  char* xbase = smem + 2 * dy_bytes;

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int tile = wave % NT;
  const int ks = wave / NT;     // K slice of this wave
  const int wm = tile / NCI;    // co tile
  const int wn = tile % NCI;    // ci tile within the block

  // transpose-read lane geometry: the two reads of a fragment cover pixel
  // rows tr_prow and tr_prow + 4 (same swizzle term), 8 bytes at tr_chb of
  // the wave's 64 B channel unit
  const int g = lane >> 4;
  const int m16 = lane & 15;
  const int tr_prow = (g >> 1) * 8 + (m16 >> 2);
  const int tr_chb = ((g & 1) * 16 + 4 * (m16 & 3)) * 2;
  const int a_off = tr_prow * SDY + ((wm ^ unit_swz<SDY>(tr_prow)) << 6)
                    + tr_chb;
  int b_off[3];
#pragma unroll
  for (int kx = 0; kx < 3; ++kx) {
    b_off[kx] = (tr_prow + kx) * SX
                + ((wn ^ unit_swz<SX>(tr_prow + kx)) << 6) + tr_chb;
  }

  const long rowstride_x = (long)s.W * s.Cin;
  const long rowstride_dy = (long)s.W * s.Cout;

  // dy rows [rbase, rbase+nrows) of (img, ct) -> buf, [row][PW pixels][Cout]
  auto stage_dy = [&](int img, int rbase, int nrows, int ct, int buf) {
    const long base = ((long)img * s.H + rbase) * rowstride_dy;
    char* dst = smem + buf * dy_bytes;
    const int bytes = nrows * s.PW * SDY;
    for (int o = wave * 1024 + lane * 16; o < bytes; o += NW * 1024) {
      const int pxf = o / SDY;
      const int w = o % SDY;
      const int rig = pxf / s.PW;
      const int px = ct * s.PW + (pxf - rig * s.PW);
      const int ch = ((((w >> 6) ^ unit_swz<SDY>(pxf)) << 6) + (w & 63)) >> 1;
      const bf16* src = zbuf;
      if (px < s.W) {
        src = dy + base + (long)rig * rowstride_dy + (long)px * s.Cout + ch;
      }
      __builtin_amdgcn_global_load_lds(as_global(src),
          as_shared(dst + (o - lane * 16)), 16, 0, 0);
    }
  };

  // x row r of (img, ct) with a one-pixel halo -> ring slot; rows outside
  // the image and pixels outside the row are zeros
  auto stage_x = [&](int img, int r, int ct, int slot) {
    const bool row_ok = r >= 0 && r < s.H;
    const long base = ((long)img * s.H + r) * rowstride_x + ci0;
    const int px0 = ct * s.PW - 1;   // image pixel of halo index 0
    char* dst = xbase + slot * x_bytes;
    for (int o = wave * 1024 + lane * 16; o < x_bytes; o += NW * 1024) {
      const int pxi = o / SX;
      const int w = o % SX;
      const int px = px0 + pxi;
      const int ch = ((((w >> 6) ^ unit_swz<SX>(pxi)) << 6) + (w & 63)) >> 1;
      const bf16* src = zbuf;
      if (row_ok && px >= 0 && px < s.W) {
        src = x + base + (long)px * s.Cin + ch;
      }
      __builtin_amdgcn_global_load_lds(as_global(src),
          as_shared(dst + (o - lane * 16)), 16, 0, 0);
    }
  };

  float acc[9][16];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
  float dbsum = 0.f;
  const bool do_bias = s.with_bias && bn == 0 && wn == 0;

  const int rsm = s.rs - 1;
  int u = u0;
  while (u < u1) {
    const int ct = u / (s.IMG * s.H);
    const int vr = u % (s.IMG * s.H);
    const int img = vr / s.H;
    const int r0 = vr % s.H;
    // segment = the run of rows of this (img, ct) inside the block's range
    const int rend = min(s.H, r0 + (u1 - u));

    const int cnt0 = min(s.gr, rend - r0);
    for (int rr = r0 - 1; rr <= r0 + cnt0; ++rr) {
      stage_x(img, rr, ct, (rr + 1) & rsm);
    }
    stage_dy(img, r0, cnt0, ct, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    int gbuf = 0;
    for (int gs = r0; gs < rend; gs += s.gr) {
      const int cnt = min(s.gr, rend - gs);
      const int nxt = gs + cnt;
      if (nxt < rend) {
        const int ncnt = min(s.gr, rend - nxt);
        stage_dy(img, nxt, ncnt, ct, gbuf ^ 1);
        for (int rr = nxt + 1; rr <= nxt + ncnt; ++rr) {
          stage_x(img, rr, ct, (rr + 1) & rsm);
        }
      }
      // K steps of this round, dealt to the tile's KS waves
      const int nsteps = cnt * s.nks;
      const char* abuf = smem + gbuf * dy_bytes + a_off;
#pragma unroll 1
      for (int j = ks; j < nsteps; j += KS) {
        const int ri = j / s.nks;
        const int p0 = (j - ri * s.nks) * 16;
        const int r = gs + ri;
        const char* pa = abuf + (ri * s.PW + p0) * SDY;
        bf16x8 af = tr16x8(pa, pa + 4 * SDY);
        if (do_bias) {
#pragma unroll
          for (int e = 0; e < 8; ++e) dbsum += (float)af[e];
        }
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
          const int slot = (r + ky) & rsm;   // x row r + ky - 1
          const char* bb = xbase + slot * x_bytes + p0 * SX;
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) {
            const char* pb = bb + b_off[kx];
            bf16x8 bf = tr16x8(pb, pb + 4 * SX);
            *reinterpret_cast<f32x16*>(acc[ky * 3 + kx]) =
                __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                    af, bf, *reinterpret_cast<f32x16*>(acc[ky * 3 + kx]),
                    0, 0, 0);
          }
        }
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      gbuf ^= 1;
    }
    u += rend - r0;
  }

  // ---- sum the KS waves of a tile through LDS (halving rounds) ----------
  // red[(slot*144 + t*16 + e)*64 + lane]; the last barrier of the main loop
  // has retired every read of the staging buffers.
  if (KS > 1) {
    float* red = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int h = KS / 2; h >= 1; h >>= 1) {
      if (ks >= h && ks < 2 * h) {
        float* dst = red + ((ks - h) * NT + tile) * (144 * 64) + lane;
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
          for (int e = 0; e < 16; ++e) dst[(t * 16 + e) * 64] = acc[t][e];
      }
      __syncthreads();
      if (ks < h) {
        const float* src = red + (ks * NT + tile) * (144 * 64) + lane;
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
          for (int e = 0; e < 16; ++e) acc[t][e] += src[(t * 16 + e) * 64];
      }
      __syncthreads();
    }
  }

  // ---- flush: fp32 atomics into dwacc -----------------------------------
  // D layout (mfma_f32_32x32x16): col = lane&31 (ci), row = (e&3) + 8*(e>>2)
  // + 4*(lane>>5) (co)
  if (ks == 0) {
    const int ci = ci0 + wn * 32 + (lane & 31);
    const int co_base = wm * 32 + 4 * (lane >> 5);
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int co = co_base + (e & 3) + 8 * (e >> 2);
        atomicAdd(dwacc + ((long)co * 9 + t) * s.Cin + ci, acc[t][e]);
      }
  }
  if (do_bias) {
    // lanes l and l+32 hold the same co (different pixels); every K slice
    // adds the steps it took
    dbsum += __shfl_xor(dbsum, 32, NVS_WAVE);
    if (lane < 32) atomicAdd(dbacc + wm * 32 + lane, dbsum);
  }
}

template <int NCO, int NCI>
void launch(const WnShape& s, size_t lds, hipStream_t stream, const bf16* x,
            const bf16* dy, const bf16* zbuf, float* dw, float* db) {
  constexpr int NT = NCO * NCI;
  constexpr int KS = 8 / NT;
  auto kern = conv3x3_wgrad_narrow_kernel<NCO, NCI>;
  hipLaunchKernelGGL(kern, dim3(s.sk * s.nb_n), dim3(64 * NT * KS), lds,
                     stream, x, dy, zbuf, dw, db, s);
}

}  // namespace

std::vector<at::Tensor> conv3x3_wgrad_narrow(const at::Tensor& x,
                                             const at::Tensor& dy,
                                             bool with_bias) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && dy.is_contiguous());
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16 &&
              dy.scalar_type() == torch::kBFloat16);
  const int nd = x.dim();
  TORCH_CHECK((nd == 4 || nd == 5) && dy.dim() == nd);
  WnShape s;
  auto xs = x.sizes();
  const long img = nd == 5 ? xs[0] * xs[1] : xs[0];
  s.IMG = (int)img;
  s.H = xs[nd - 3]; s.W = xs[nd - 2]; s.Cin = xs[nd - 1];
  s.Cout = dy.size(nd - 1);
  TORCH_CHECK(s.IMG >= 1 && s.H >= 1 && s.W >= 1);
  TORCH_CHECK(s.Cin % 32 == 0 && s.Cout % 32 == 0 && s.Cin >= 32 &&
              s.Cout >= 32 && s.Cout <= 128,
              "conv3x3_wgrad_narrow: Cin % 32, Cout % 32, Cout <= 128");
  TORCH_CHECK(x.numel() == img * s.H * s.W * s.Cin &&
              dy.numel() == img * s.H * s.W * s.Cout);
  TORCH_CHECK(img * s.H * ((s.W + 15) / 16) < (1L << 30),
              "conv3x3_wgrad_narrow: too many row tiles");

  const int nco = s.Cout / 32;
  const int nci = s.Cin % 64 == 0 ? 2 : 1;
  const int nt = nco * nci;
  const int ks = 8 / nt;
  s.PW = std::min((s.W + 15) / 16 * 16, 128);
  s.nks = s.PW / 16;
  s.nct = (s.W + s.PW - 1) / s.PW;
  s.units = s.IMG * s.H * s.nct;
  s.nb_n = s.Cin / (32 * nci);
  s.with_bias = with_bias ? 1 : 0;

  // rows per round: 256 pixels for the narrowest tiles, else 128; halved
  // until the staging buffers fit
  const int round_px = (s.Cout + 32 * nci <= 96) ? 256 : 128;
  const size_t lds_max = 160 * 1024;
  size_t stage = 0;
  for (s.gr = std::max(1, std::min(8, round_px / s.PW));; s.gr /= 2) {
    s.rs = 4;
    while (s.rs < 2 * s.gr + 2) s.rs *= 2;
    stage = 2 * (size_t)(s.gr * s.PW) * (s.Cout * 2)
            + (size_t)s.rs * (s.PW + 2) * (nci * 64);
    if (stage <= lds_max || s.gr == 1) break;
  }
  const size_t red = ks > 1 ? (size_t)(ks / 2) * nt * 144 * 64 * 4 : 0;
  const size_t lds = std::max(stage, red);
  TORCH_CHECK(lds <= lds_max, "conv3x3_wgrad_narrow LDS overflow: ", lds);

  // one block per CU over ci tiles x ranges; a range holds at least one
  // full round of rows
  const int cus = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  s.sk = std::max(1, std::min(s.units / s.gr, std::max(1, cus / s.nb_n)));

  auto opts = x.options().dtype(torch::kFloat);
  auto dw = torch::zeros({s.Cout, 3, 3, s.Cin}, opts);
  torch::Tensor db;
  if (with_bias) db = torch::zeros({s.Cout}, opts);
  static torch::Tensor zbuf;
  if (!zbuf.defined() || zbuf.device() != x.device()) {
    zbuf = torch::zeros({64}, x.options());
  }

  auto stream = at::hip::getCurrentHIPStream();
  auto xp = reinterpret_cast<const bf16*>(x.data_ptr());
  auto dyp = reinterpret_cast<const bf16*>(dy.data_ptr());
  auto zp = reinterpret_cast<const bf16*>(zbuf.data_ptr());
  float* dwp = dw.data_ptr<float>();
  float* dbp = with_bias ? db.data_ptr<float>() : nullptr;
#define NVS_WN_CASE(A, B)                                                  \
  if (nco == A && nci == B) {                                              \
    launch<A, B>(s, lds, stream, xp, dyp, zp, dwp, dbp);                   \
  } else
  NVS_WN_CASE(1, 1) NVS_WN_CASE(1, 2) NVS_WN_CASE(2, 1) NVS_WN_CASE(2, 2)
  NVS_WN_CASE(3, 1) NVS_WN_CASE(3, 2) NVS_WN_CASE(4, 1) NVS_WN_CASE(4, 2)
  { TORCH_CHECK(false, "conv3x3_wgrad_narrow: no instantiation"); }
#undef NVS_WN_CASE
  if (with_bias) return {dw, db};
  return {dw};
}
