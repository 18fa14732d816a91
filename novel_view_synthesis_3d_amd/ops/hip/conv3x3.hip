// Implicit-GEMM 3x3 SAME stride-1 conv, NHWC bf16, MFMA — CDNA4 gfx950.
//
// The model's only conv type (kernel (1,3,3) over frames). GEMM view:
//   out[M, N] = sum_k A[M, k] * B[k, N]
//   M = B*F*H*W pixels, N = Cout, k = (plane dy*3+dx, ci), K = 9*Cin.
// A is the im2col image, never materialized: each K-step (one kernel plane,
// 64 input channels) is gathered straight into LDS. B is the weight, whose
// OHWI storage (Cout, 3, 3, Cin) is ALREADY (n, k) row-major.
//
// Staging: both tiles stream global->LDS with global_load_lds (16 B per
// lane, no register round trip). The LDS image of a glds is lane-linear, so
// the ((row&7)<<4) byte-XOR bank swizzle is applied to the per-lane SOURCE
// address instead; the MFMA fragment reads apply the same XOR. SAME padding
// and the M tail are handled by pointing out-of-range lanes at a 128 B
// buffer of zeros, so the main loops carry no masks.
//
// Two kernels, selected on the host (use256):
//   conv3x3_igemm      128x128 tile, 4 waves (2x2 of 64x64), 64 KiB LDS,
//                      one barrier per K-step;
//   conv3x3_igemm_256  256x256 tile, 8 waves (2Mx4N), 128 KiB LDS, where
//                      that tiling still fills the chip.
// Both are BK=64, mfma_f32_16x16x32_bf16, double-buffered, and share the
// block swizzle, the pixel-row decode, the A source address and the
// epilogue (accumulators -> LDS -> coalesced bf16 stores with fused bias,
// residual and scale) below. Their main loops are different structures and
// stay separate.
//
// The same kernels compute dgrad: conv3x3(dy, w~) with
// w~[ci, ey, ex, co] = w[co, 2-ey, 2-ex, ci] (host-side transform).
// Constraints: Cin % 64 == 0, Cout % 128 == 0. ops/hip_ops.py routes every
// other shape (stem 3ch, strided pose-emb 144ch, head 3ch, small configs)
// to the im2col + hipBLASLt GEMM path.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "common.h"

namespace {

constexpr int BK = 64;
// LDS tile: [rows][BK] bf16, byte-swizzled. row stride = BK*2 = 128B.
__device__ __forceinline__ int swz(int row, int k_elem) {
  int byte = row * (BK * 2) + k_elem * 2;
  return byte ^ ((row & 7) << 4);
}

struct ConvShape {
  int IMG;       // B*F images
  int H, W;      // spatial
  int Cin, Cout;
  int M;         // IMG*H*W
  int ksteps;    // 9*Cin / BK
  int steps_per_plane;  // Cin / BK
};

// XCD-aware block swizzle (bijective form): hardware deals consecutive
// block ids round-robin over the 8 XCDs; remap so that each XCD walks
// consecutive M-blocks within one N-column and its L2 keeps the weight
// panel.
__device__ __forceinline__ int xcd_swizzle(int bid, int nwg) {
  const int q = nwg / 8, r = nwg % 8;
  const int xcd = bid % 8, idx = bid / 8;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// One output pixel (tile row m) as the A gather sees it.
struct PixRow {
  int h, w;    // position in its image
  int ok;      // m < M (rows past the M tail read zeros)
  long base;   // element offset of the image in x
};

__device__ __forceinline__ PixRow decode_row(const ConvShape& s, int m) {
  PixRow r;
  r.w = m % s.W;
  r.h = (m / s.W) % s.H;
  r.ok = m < s.M;
  r.base = ((long)(m / (s.W * s.H)) * s.H) * s.W * s.Cin;
  return r;
}

// Source of one 16 B A chunk: pixel r shifted by kernel plane (dy, dx),
// 16 B chunk kp of the channels [ci0, ci0+64). Padding and tail rows read
// the zero buffer.
__device__ __forceinline__ const bf16* a_src(const bf16* x, const bf16* zbuf,
                                             const ConvShape& s,
                                             const PixRow& r, int dy, int dx,
                                             int ci0, int kp) {
  const int hh = r.h + dy;
  const int ww = r.w + dx;
  const bool valid = r.ok & (hh >= 0) & (hh < s.H) & (ww >= 0) & (ww < s.W);
  return valid
      ? x + r.base + ((long)hh * s.W + ww) * s.Cin + ci0 + kp * 8
      : zbuf;
}

// Epilogue of a TILE x TILE block run by NT threads: acc (+bias) -> bf16
// tile in LDS -> coalesced 16 B stores, optionally y = (v + residual) *
// out_scale (the ResnetBlock tail) in fp32 with one rounding. Each wave
// owns MI x 4 accumulator fragments of 16x16 whose top-left corner in the
// tile is (wrow0, wcol0).
template <int TILE, int NT, int MI>
__device__ __forceinline__ void store_tile(
    char* smem, const float (&acc)[MI][4][4], int wrow0, int wcol0,
    int m0, int n0, const ConvShape& s, const float* __restrict__ bias,
    const bf16* __restrict__ residual, float out_scale,
    bf16* __restrict__ out) {
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  bf16* ldsC = reinterpret_cast<bf16*>(smem);  // [TILE][TILE] bf16
  __syncthreads();  // done with A/B buffers
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int col = wcol0 + j * 16 + (lane & 15);
    const float bj = bias != nullptr ? bias[n0 + col] : 0.f;
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const int rbase = wrow0 + i * 16 + ((lane >> 4) << 2);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        ldsC[(rbase + r) * TILE + col] = __float2bfloat16(acc[i][j][r] + bj);
      }
    }
  }
  __syncthreads();
  constexpr int PACKS = TILE / 8;  // 16 B packs per tile row
#pragma unroll
  for (int it = 0; it < TILE * PACKS / NT; ++it) {
    const int p = tid + it * NT;
    const int row = p / PACKS;
    const int cp = p % PACKS;
    const int m = m0 + row;
    if (m < s.M) {
      Pack<bf16, 8> v = *reinterpret_cast<Pack<bf16, 8>*>(
          ldsC + row * TILE + cp * 8);
      const long goff = (long)m * s.Cout + n0 + cp * 8;
      if (residual != nullptr) {
        Pack<bf16, 8> rv = pload<bf16, 8>(residual + goff);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          from_f32((to_f32(v.v[j]) + to_f32(rv.v[j])) * out_scale, v.v[j]);
        }
      } else if (out_scale != 1.0f) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          from_f32(to_f32(v.v[j]) * out_scale, v.v[j]);
        }
      }
      pstore<bf16, 8>(out + goff, v);
    }
  }
}

// ---------------------------------------------------------------------------
// 128x128 tile, 4 waves
// ---------------------------------------------------------------------------

constexpr int BM = 128;
constexpr int BN = 128;
constexpr int THREADS = 256;

__global__ __launch_bounds__(THREADS)
void conv3x3_igemm(const bf16* __restrict__ x,   // (IMG,H,W,Cin)
                   const bf16* __restrict__ w,   // (Cout, 9*Cin) rows=co
                   const float* __restrict__ bias,  // (Cout,) or null
                   const bf16* __restrict__ zbuf,   // 128B of zeros (padding)
                   const bf16* __restrict__ residual,  // out-shaped or null
                   float out_scale,              // y=(conv+bias+res)*scale
                   bf16* __restrict__ out,       // (IMG,H,W,Cout)
                   ConvShape s, int nblocks_m) {
  const int bid = xcd_swizzle(blockIdx.x, nblocks_m * (s.Cout / BN));
  const int bm = bid % nblocks_m;
  const int bn = bid / nblocks_m;
  const int m0 = bm * BM;
  const int n0 = bn * BN;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16* ldsA = reinterpret_cast<bf16*>(smem);               // 2 x 16KB
  bf16* ldsB = reinterpret_cast<bf16*>(smem + 2 * BM * BK * 2);  // 2 x 16KB

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wr = wave >> 1;   // 0..1: M half
  const int wc = wave & 1;    // 0..1: N half

  // One glds instruction fills 1 KiB: 16 per 16KB tile = 4 per wave; slot s
  // of this wave covers LDS bytes [(wave*4+s)*1024, +1024).
  // Lane's element under the swizzle: row = o/128 (XOR keeps the row),
  // k-byte = (o ^ ((row&7)<<4)) % 128, with o = slot*1024 + lane*16.
  PixRow a_row[4];
  int kp[4], b_co[4];
#pragma unroll
  for (int slot = 0; slot < 4; ++slot) {
    const int o = (wave * 4 + slot) * 1024 + lane * 16;
    const int row = o >> 7;
    const int kb = (o ^ ((row & 7) << 4)) & 127;
    kp[slot] = kb >> 4;
    b_co[slot] = n0 + row;
    a_row[slot] = decode_row(s, m0 + row);
  }

  float acc[4][4][4];  // [mi][nj][reg] f32x4 fragments
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.f;

  auto stage_glds = [&](int kstep, int buf) {
    const int plane = kstep / s.steps_per_plane;
    const int ci0 = (kstep % s.steps_per_plane) * BK;
    const int dy = plane / 3 - 1;
    const int dx = plane % 3 - 1;
    char* baseA = reinterpret_cast<char*>(ldsA) + buf * BM * BK * 2
                  + wave * 4 * 1024;
    char* baseB = reinterpret_cast<char*>(ldsB) + buf * BN * BK * 2
                  + wave * 4 * 1024;
#pragma unroll
    for (int slot = 0; slot < 4; ++slot) {
      const bf16* srcA = a_src(x, zbuf, s, a_row[slot], dy, dx,
                               ci0, kp[slot]);
      __builtin_amdgcn_global_load_lds(as_global(srcA),
          as_shared(baseA + slot * 1024), 16, 0, 0);
      const bf16* srcB = w + (long)b_co[slot] * (9 * s.Cin) + kstep * BK
                         + kp[slot] * 8;
      __builtin_amdgcn_global_load_lds(as_global(srcB),
          as_shared(baseB + slot * 1024), 16, 0, 0);
    }
  };

  auto compute = [&](int buf) {
    const char* baseA = reinterpret_cast<const char*>(ldsA) + buf * BM * BK * 2;
    const char* baseB = reinterpret_cast<const char*>(ldsB) + buf * BN * BK * 2;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 af[4], bf[4];
      const int kbase = kk * 32 + (lane >> 4) * 8;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = wr * 64 + i * 16 + (lane & 15);
        af[i] = *reinterpret_cast<const bf16x8*>(baseA + swz(row, kbase));
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = wc * 64 + j * 16 + (lane & 15);
        bf[j] = *reinterpret_cast<const bf16x8*>(baseB + swz(row, kbase));
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          *reinterpret_cast<f32x4*>(acc[i][j]) =
              __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  af[i], bf[j], *reinterpret_cast<f32x4*>(acc[i][j]),
                  0, 0, 0);
        }
    }
  };

  // --- main loop: glds double-buffer, one barrier per K-step ----------
  stage_glds(0, 0);
  __syncthreads();  // drains the glds (vmcnt(0) inside the barrier)
  for (int t = 0; t < s.ksteps; ++t) {
    const int cur = t & 1;
    if (t + 1 < s.ksteps) stage_glds(t + 1, cur ^ 1);
    compute(cur);
    __syncthreads();  // glds for t+1 landed; LDS reads of buf cur done
  }

  store_tile<BM, THREADS, 4>(smem, acc, wr * 64, wc * 64, m0, n0, s, bias,
                             residual, out_scale, out);
}

// ---------------------------------------------------------------------------
// 256x256 tile, 8 waves as 2Mx4N: halves the staging traffic per FLOP and
// runs 64 MFMA per wave between barriers (vs 32 in the 128² kernel).
// Per K-tile: 4 quadrant phases with no internal barriers (each wave reads
// its own A/B halves); ONE vmcnt(0)+barrier per K-tile. A/B staged by glds
// in 4 half-tiles (128 rows x 64 k each), double-buffered (4 x 16KB x 2 =
// 128 KiB LDS).
// ---------------------------------------------------------------------------

constexpr int BM2 = 256;
constexpr int BN2 = 256;
constexpr int T2 = 512;

__global__ __launch_bounds__(T2)
void conv3x3_igemm_256(const bf16* __restrict__ x,
                       const bf16* __restrict__ w,   // (Cout, 9*Cin)
                       const float* __restrict__ bias,
                       const bf16* __restrict__ zbuf,
                       const bf16* __restrict__ residual,
                       float out_scale,
                       bf16* __restrict__ out,
                       ConvShape s, int nblocks_m) {
  const int bid = xcd_swizzle(blockIdx.x, nblocks_m * (s.Cout / BN2));
  const int bm = bid % nblocks_m;
  const int bn = bid / nblocks_m;
  const int m0 = bm * BM2;
  const int n0 = bn * BN2;

  // LDS: [buf(2)][operand A=0/B=1][half(2)][16KB]
  extern __shared__ __attribute__((aligned(16))) char smem[];
  auto half_base = [&](int buf, int op, int half) -> char* {
    return smem + (((buf * 2 + op) * 2 + half) << 14);
  };

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;   // 0..7
  const int wm = wave >> 2;    // A half this wave consumes
  const int wn = wave & 3;     // B cols: half wn>>1, sub (wn&1)*64

  // glds slot decode: wave issues 2 glds per half-tile; slot s covers LDS
  // bytes [(wave*2+s)*1024, +1024) of that half (lane-linear). Element under
  // the ((row&7)<<4) XOR swizzle: row = o>>7, kp = ((o ^ ((row&7)<<4)) & 127) >> 4.
  PixRow a_row[2][2];  // [half][slot]
  int kp[2], b_co[2][2];
#pragma unroll
  for (int half = 0; half < 2; ++half) {
#pragma unroll
    for (int slot = 0; slot < 2; ++slot) {
      const int o = (wave * 2 + slot) * 1024 + lane * 16;
      const int row = o >> 7;             // 0..127 within the half
      kp[slot] = ((o ^ ((row & 7) << 4)) & 127) >> 4;
      a_row[half][slot] = decode_row(s, m0 + half * 128 + row);
      b_co[half][slot] = n0 + half * 128 + row;
    }
  }

  auto stage_tile = [&](int kstep, int buf) {
    const int plane = kstep / s.steps_per_plane;
    const int ci0 = (kstep % s.steps_per_plane) * BK;
    const int dy = plane / 3 - 1;
    const int dx = plane % 3 - 1;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
      for (int slot = 0; slot < 2; ++slot) {
        const bf16* srcA = a_src(x, zbuf, s, a_row[half][slot], dy, dx,
                                 ci0, kp[slot]);
        __builtin_amdgcn_global_load_lds(as_global(srcA),
            as_shared(half_base(buf, 0, half) + (wave * 2 + slot) * 1024),
            16, 0, 0);
        const bf16* srcB = w + (long)b_co[half][slot] * (9 * s.Cin)
                           + kstep * BK + kp[slot] * 8;
        __builtin_amdgcn_global_load_lds(as_global(srcB),
            as_shared(half_base(buf, 1, half) + (wave * 2 + slot) * 1024),
            16, 0, 0);
      }
    }
  };

  float acc[8][4][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.f;

  stage_tile(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  for (int t = 0; t < s.ksteps; ++t) {
    const int cur = t & 1;
    const char* baseA = half_base(cur, 0, wm);
    const char* baseB = half_base(cur, 1, wn >> 1);
    // B fragments for the whole K-tile (shared by all 4 quadrants)
    bf16x8 bfr[4][2];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const int row = (wn & 1) * 64 + j * 16 + (lane & 15);
        bfr[j][kk] = *reinterpret_cast<const bf16x8*>(
            baseB + swz(row, kk * 32 + (lane >> 4) * 8));
      }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (q == 0 && t + 1 < s.ksteps) {
        stage_tile(t + 1, cur ^ 1);  // overlaps the whole tile's compute
      }
      bf16x8 afr[2][2];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          const int row = q * 32 + i * 16 + (lane & 15);
          afr[i][kk] = *reinterpret_cast<const bf16x8*>(
              baseA + swz(row, kk * 32 + (lane >> 4) * 8));
        }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int kk = 0; kk < 2; ++kk) {
            *reinterpret_cast<f32x4*>(acc[q * 2 + i][j]) =
                __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    afr[i][kk], bfr[j][kk],
                    *reinterpret_cast<f32x4*>(acc[q * 2 + i][j]), 0, 0, 0);
          }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

  store_tile<BM2, T2, 8>(smem, acc, wm * 128, wn * 64, m0, n0, s, bias,
                         residual, out_scale, out);
}

}  // namespace

torch::Tensor conv3x3_fwd(torch::Tensor x, torch::Tensor w,
                          c10::optional<torch::Tensor> bias,
                          c10::optional<torch::Tensor> residual,
                          double out_scale) {
  // x: (B,F,H,W,Cin) or (IMG,H,W,Cin) bf16 contiguous; w: (Cout,3,3,Cin)
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && w.is_contiguous());
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16 &&
              w.scalar_type() == torch::kBFloat16);
  auto xs = x.sizes();
  const int nd = x.dim();
  TORCH_CHECK(nd == 4 || nd == 5);
  ConvShape s;
  s.IMG = nd == 5 ? xs[0] * xs[1] : xs[0];
  s.H = xs[nd - 3]; s.W = xs[nd - 2]; s.Cin = xs[nd - 1];
  s.Cout = w.size(0);
  TORCH_CHECK(w.size(1) == 3 && w.size(2) == 3 && w.size(3) == s.Cin);
  TORCH_CHECK(s.Cin % BK == 0, "Cin must be multiple of 64");
  TORCH_CHECK(s.Cout % BN == 0, "Cout must be multiple of 128");
  s.M = s.IMG * s.H * s.W;
  s.steps_per_plane = s.Cin / BK;
  s.ksteps = 9 * s.steps_per_plane;

  std::vector<int64_t> oshape(xs.begin(), xs.end());
  oshape[nd - 1] = s.Cout;
  auto out = torch::empty(oshape, x.options());

  torch::Tensor biasf;
  if (bias.has_value()) biasf = bias->to(torch::kFloat).contiguous();
  static torch::Tensor zbuf;  // 128B zero pad source for OOB glds lanes
  if (!zbuf.defined() || zbuf.device() != x.device()) {
    zbuf = torch::zeros({64}, x.options());
  }

  auto stream = at::hip::getCurrentHIPStream();
  if (residual.has_value()) {
    TORCH_CHECK(residual->is_contiguous()
                && residual->sizes() == out.sizes()
                && residual->scalar_type() == torch::kBFloat16);
  }
  auto launch = [&](auto kernel, int tile, int threads, size_t lds) {
    const int nblocks_m = (s.M + tile - 1) / tile;
    hipLaunchKernelGGL(kernel, dim3(nblocks_m * (s.Cout / tile)),
        dim3(threads), lds, stream,
        reinterpret_cast<const bf16*>(x.data_ptr()),
        reinterpret_cast<const bf16*>(w.data_ptr()),
        bias.has_value() ? biasf.data_ptr<float>() : nullptr,
        reinterpret_cast<const bf16*>(zbuf.data_ptr()),
        residual.has_value()
            ? reinterpret_cast<const bf16*>(residual->data_ptr()) : nullptr,
        (float)out_scale,
        reinterpret_cast<bf16*>(out.data_ptr()), s, nblocks_m);
  };
  // 256x256-tile variant where it fills the chip (L0-L2 full-config convs)
  const bool use256 = (s.M % 256 == 0) && (s.Cout % 256 == 0)
      && ((long)(s.M / 256) * (s.Cout / 256) >= 128);
  if (use256) {
    launch(conv3x3_igemm_256, BM2, T2, 128 * 1024);
  } else {
    launch(conv3x3_igemm, BM, THREADS, 2 * (BM + BN) * BK * 2);  // 64 KB
  }
  return out;
}
