// Halo-tile 3x3 SAME stride-1 conv for narrow channels, NHWC bf16, MFMA —
// CDNA4 gfx950. Covers Cin % 32 == 0, Cout % 32 == 0, Cout <= 128, any H, W:
// the small X-UNet config, whose GEMM N of 32..128 the 128/256-wide igemm
// tiles of conv3x3.hip cannot serve.
//
// Work split: a block (4 waves) owns a 16x16 tile of output pixels of ONE
// image and ALL of Cout; wave v owns tile rows 4v..4v+3, one row of 16
// pixels per MFMA fragment. Accumulators (4 x Cout/16 fragments of
// mfma_f32_16x16x32_bf16) stay in registers over the Cin loop. Blocks are
// persistent: block b takes tiles b, b+grid, ...
//
// Data movement, per (tile, 32-channel chunk of Cin):
//   * the 18x18 halo patch goes global -> registers -> LDS once, pixel-major,
//     64 B (32 channels) per pixel; loads are predicated, so SAME padding and
//     everything outside the image (never a neighbouring frame) is zeros.
//     All nine taps read their fragments from that patch at a pixel shift of
//     ky*18 + kx. The loads of the next patch are issued before the MFMAs of
//     this one and land in LDS after them.
//   * the chunk's filter (9 x Cout rows of 64 B) is staged in LDS; with one
//     chunk (Cin == 32) it is staged once per block and stays for all tiles.
//
// The MFMA runs transposed, D[cout][pixel] = W[cout][k] * X[k][pixel]: the
// weight is the A operand, the pixels are B. A lane of D then holds four
// consecutive rows (couts) of one pixel. The filter rows of a fragment pair
// (2j, 2j+1) are permuted while staging so that those are couts
// 32j + 8g + {0..3} and + {4..7} (g = lane >> 4): eight consecutive channels
// of one pixel per lane, i.e. the epilogue is one 16 B store per lane
// straight from registers, (acc + bias + residual) * out_scale in fp32 with
// one rounding, masked per pixel at ragged edges. No LDS round trip.
//
// LDS rows are 64 B = four 16 B chunks, chunk c of row r stored at chunk
// c ^ ((r >> 2) & 3), where r is the filter row, or the pixel COLUMN of a
// patch row (18 x 64 B, a multiple of 128 B, so rows do not enter). A
// ds_read_b128 group is 16 lanes on 16 consecutive r and one chunk: each
// 64 B quarter of the 256 B bank line (address bits 6-7, r & 3 up to a
// constant) is hit by four of them, whose r >> 2 are four consecutive
// numbers, so the XOR sends them to four different chunks — 16 distinct
// 16 B slots for any start, hence for every tap shift. The XOR term depends
// on the lane and kx only, so every fragment address is one of four lane
// bases plus an immediate. The staging stores (4 lanes per row, 16 lanes on
// 256 contiguous bytes) are conflict-free as well.
//
// dgrad is the same kernel on w~[ci,ey,ex,co] = w[co,2-ey,2-ex,ci].

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "common.h"

namespace {

constexpr int TH = 16, TW = 16;            // output tile
constexpr int PH = TH + 2, PW = TW + 2;    // halo patch
constexpr int KC = 32;                     // Cin chunk = K of one MFMA
constexpr int ROWB = KC * 2;               // bytes of one LDS row
constexpr int PATCH_PIX = PH * PW;
constexpr int PATCH_BYTES = PATCH_PIX * ROWB;              // 20736
constexpr int NT = 256;
constexpr int PATCH_LOADS = PH / 3;  // passes of three patch rows

using u32x4 = __attribute__((ext_vector_type(4))) unsigned;

// byte offset of 16 B chunk c of LDS row `row` (see the bank argument above)
__device__ __forceinline__ int row_off(int row, int c) {
  return row * ROWB + ((c ^ ((row >> 2) & 3)) << 4);
}
// the same for patch pixel (py, px), swizzled by the pixel column
__device__ __forceinline__ int patch_off(int py, int px, int c) {
  return (py * PW + px) * ROWB + ((c ^ ((px >> 2) & 3)) << 4);
}

struct HaloShape {
  int H, W, Cin;
  int tiles_x, tiles_y, ntiles;  // ntiles = IMG * tiles_y * tiles_x
  int nchunks;                   // Cin / KC
};

// waves per SIMD that the LDS footprint (20.25 KiB + 9 KiB per 16 couts, of
// 160 KiB per CU) admits; the register budget is held to the same figure
constexpr int halo_waves(int nf) { return nf == 2 ? 4 : nf <= 6 ? 2 : 1; }

template <int NF>  // Cout / 16
__global__ __launch_bounds__(NT, halo_waves(NF))
void conv3x3_halo_kernel(const bf16* __restrict__ x,     // (IMG,H,W,Cin)
                         const bf16* __restrict__ w,     // (Cout,3,3,Cin)
                         const float* __restrict__ bias,  // (Cout,) or null
                         const bf16* __restrict__ residual,  // out-shaped/null
                         float out_scale,
                         bf16* __restrict__ out,         // (IMG,H,W,Cout)
                         HaloShape s) {
  constexpr int COUT = NF * 16;
  constexpr int WCHUNKS = 9 * COUT * 4;  // 16 B chunks of one staged filter
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* ldsX = smem;                // [PATCH_PIX][64 B]
  char* ldsW = smem + PATCH_BYTES;  // [9][COUT][64 B], rows in fragment order

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int l15 = lane & 15;
  const int kg = lane >> 4;  // k group of an operand lane, row group of D

  // host launches grid <= ntiles
  const int my_tiles = (s.ntiles - (int)blockIdx.x + (int)gridDim.x - 1)
                       / (int)gridDim.x;
  const int nsteps = my_tiles * s.nchunks;

  struct Tile { int img, y0, x0; };
  auto tile_of = [&](int step) {
    const int t = blockIdx.x + (step / s.nchunks) * gridDim.x;
    Tile r;
    r.x0 = (t % s.tiles_x) * TW;
    r.y0 = ((t / s.tiles_x) % s.tiles_y) * TH;
    r.img = t / (s.tiles_x * s.tiles_y);
    return r;
  };

  // Patch staging: three patch rows per pass (18 pixels x 4 chunks = 72
  // lanes a row, 216 of the 256 lanes busy), six passes. A lane keeps its
  // (pixel column, chunk) and moves down three rows per pass, so its global
  // and LDS addresses advance by a uniform stride.
  const int prow = tid / (PW * 4);       // 0..2; 3 = idle
  const int pcol = (tid % (PW * 4)) >> 2;
  const int pch = tid & 3;  // (tid % 72) & 3: 72 is a multiple of 4
  const int plds = patch_off(prow, pcol, pch);

  u32x4 pre[PATCH_LOADS];
  auto load_patch = [&](int step) {
    const Tile t = tile_of(step);
    const int ci0 = (step % s.nchunks) * KC;
    const int gx = t.x0 - 1 + pcol;
    const bool okx = (prow < 3) & (gx >= 0) & (gx < s.W);
    const bf16* src = x + (((long)t.img * s.H + (t.y0 - 1 + prow)) * s.W + gx)
                          * s.Cin + ci0 + pch * 8;
    const long pass_stride = 3L * s.W * s.Cin;
#pragma unroll
    for (int it = 0; it < PATCH_LOADS; ++it) {
      const int gy = t.y0 - 1 + prow + it * 3;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (okx & (gy >= 0) & (gy < s.H)) {
        v = *reinterpret_cast<const u32x4*>(src + it * pass_stride);
      }
      pre[it] = v;
    }
  };
  auto store_patch = [&]() {
    if (prow < 3) {
#pragma unroll
      for (int it = 0; it < PATCH_LOADS; ++it) {
        *reinterpret_cast<u32x4*>(ldsX + plds + it * 3 * PW * ROWB) = pre[it];
      }
    }
  };

  // Filter staging: 64 LDS rows per pass, as two groups of 32 (one per wave
  // pair, so the group index g = 2*pass + (wave>>1) is wave-uniform). Group
  // g is tap g / (COUT/32), couts 32j.. with j = g % (COUT/32). LDS row
  // 32j + 16h + i of a tap holds cout 32j + 8(i>>2) + 4h + (i&3).
  constexpr int J = COUT / 32;
  constexpr int WPASSES = (9 * J + 1) / 2;
  const int wsel = __builtin_amdgcn_readfirstlane(tid >> 7);
  const int wrow = (tid >> 2) & 31;
  const int wco = ((wrow & 0xC) << 1) | ((wrow & 0x10) >> 2) | (wrow & 3);
  const int wlds = row_off(wrow, pch);
  auto stage_weights = [&](int ci0) {
    const bf16* src = w + (long)wco * 9 * s.Cin + ci0 + pch * 8;
#pragma unroll
    for (int p0 = 0; p0 < WPASSES; p0 += 4) {
      u32x4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int g = 2 * (p0 + u) + wsel;
        if (p0 + u < WPASSES && g < 9 * J) {
          const int tap = g / J, j = g % J;
          v[u] = *reinterpret_cast<const u32x4*>(
              src + ((long)j * 32 * 9 + tap) * s.Cin);
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int g = 2 * (p0 + u) + wsel;
        if (p0 + u < WPASSES && g < 9 * J) {
          const int tap = g / J, j = g % J;
          *reinterpret_cast<u32x4*>(
              ldsW + (tap * COUT + j * 32) * ROWB + wlds) = v[u];
        }
      }
    }
  };

  f32x4 acc[4][NF];  // [tile row of this wave][cout fragment]
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int f = 0; f < NF; ++f) acc[i][f] = f32x4{0.f, 0.f, 0.f, 0.f};

  // fragment reads: lane base + a compile-time offset per (row, tap, f)
  int xlds[3];
#pragma unroll
  for (int kx = 0; kx < 3; ++kx) xlds[kx] = patch_off(wave * 4, kx + l15, kg);
  const int wfrag = row_off(l15, kg);

  if (nsteps > 0) load_patch(0);
  for (int step = 0; step < nsteps; ++step) {
    const int chunk = step % s.nchunks;
    __syncthreads();  // every wave is done reading the previous patch/filter
    store_patch();
    if (s.nchunks > 1 || step == 0) stage_weights(chunk * KC);
    __syncthreads();
    if (step + 1 < nsteps) load_patch(step + 1);  // in flight over the MFMAs

#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int ky = tap / 3, kx = tap % 3;
      bf16x8 xb[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        xb[i] = *reinterpret_cast<const bf16x8*>(
            ldsX + xlds[kx] + (i + ky) * PW * ROWB);
      }
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        const bf16x8 wa = *reinterpret_cast<const bf16x8*>(
            ldsW + wfrag + (tap * COUT + f * 16) * ROWB);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          acc[i][f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              wa, xb[i], acc[i][f], 0, 0, 0);
        }
      }
    }

    if (chunk + 1 < s.nchunks) continue;

    // epilogue: lane = pixel (row wave*4+i, column l15), couts 32j+8kg..+8
    const Tile t = tile_of(step);
    const int gx = t.x0 + l15;
#pragma unroll
    for (int j = 0; j < NF / 2; ++j) {
      const int co0 = j * 32 + kg * 8;
      float bj[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) bj[e] = bias != nullptr ? bias[co0 + e] : 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int gy = t.y0 + wave * 4 + i;
        if (gy < s.H && gx < s.W) {
          const long goff = (((long)t.img * s.H + gy) * s.W + gx) * COUT + co0;
          float r[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) r[e] = 0.f;
          if (residual != nullptr) {
            const Pack<bf16, 8> rv = pload<bf16, 8>(residual + goff);
#pragma unroll
            for (int e = 0; e < 8; ++e) r[e] = to_f32(rv.v[e]);
          }
          Pack<bf16, 8> o;
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float a = acc[i][2 * j + (e >> 2)][e & 3];
            from_f32((a + bj[e] + r[e]) * out_scale, o.v[e]);
          }
          pstore<bf16, 8>(out + goff, o);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int f = 0; f < NF; ++f) acc[i][f] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
}

}  // namespace

torch::Tensor conv3x3_halo_fwd(torch::Tensor x, torch::Tensor w,
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
  const long IMG = nd == 5 ? xs[0] * xs[1] : xs[0];
  HaloShape s;
  s.H = xs[nd - 3]; s.W = xs[nd - 2]; s.Cin = xs[nd - 1];
  const int Cout = w.size(0);
  TORCH_CHECK(w.dim() == 4 && w.size(1) == 3 && w.size(2) == 3
              && w.size(3) == s.Cin);
  TORCH_CHECK(s.Cin % KC == 0, "Cin must be a multiple of 32");
  TORCH_CHECK(Cout % 32 == 0 && Cout <= 128,
              "Cout must be a multiple of 32, at most 128");
  TORCH_CHECK(IMG >= 1 && s.H >= 1 && s.W >= 1);
  TORCH_CHECK((uintptr_t)x.data_ptr() % 16 == 0
              && (uintptr_t)w.data_ptr() % 16 == 0, "16 B aligned x, w");
  s.tiles_x = (s.W + TW - 1) / TW;
  s.tiles_y = (s.H + TH - 1) / TH;
  const long ntiles = IMG * s.tiles_y * s.tiles_x;
  TORCH_CHECK(ntiles < (1L << 31) && IMG * s.H < (1L << 31));
  s.ntiles = (int)ntiles;
  s.nchunks = s.Cin / KC;

  std::vector<int64_t> oshape(xs.begin(), xs.end());
  oshape[nd - 1] = Cout;
  auto out = torch::empty(oshape, x.options());

  torch::Tensor biasf;
  if (bias.has_value()) {
    TORCH_CHECK(bias->numel() == Cout && bias->device() == x.device());
    biasf = bias->to(torch::kFloat).contiguous();
  }
  if (residual.has_value()) {
    TORCH_CHECK(residual->is_contiguous()
                && residual->sizes() == out.sizes()
                && residual->scalar_type() == torch::kBFloat16
                && residual->device() == x.device()
                && (uintptr_t)residual->data_ptr() % 16 == 0);
  }

  // persistent blocks: enough to fill every CU at the kernel's occupancy
  const int cus = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  const int grid = (int)std::min<long>(ntiles, (long)cus * 4);
  const size_t lds = PATCH_BYTES + (size_t)9 * Cout * ROWB;
  auto stream = at::hip::getCurrentHIPStream();
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(NT), lds, stream,
        reinterpret_cast<const bf16*>(x.data_ptr()),
        reinterpret_cast<const bf16*>(w.data_ptr()),
        bias.has_value() ? biasf.data_ptr<float>() : nullptr,
        residual.has_value()
            ? reinterpret_cast<const bf16*>(residual->data_ptr()) : nullptr,
        (float)out_scale, reinterpret_cast<bf16*>(out.data_ptr()), s);
  };
  switch (Cout) {
    case 32: launch(conv3x3_halo_kernel<2>); break;
    case 64: launch(conv3x3_halo_kernel<4>); break;
    case 96: launch(conv3x3_halo_kernel<6>); break;
    default: launch(conv3x3_halo_kernel<8>); break;
  }
  return out;
}
