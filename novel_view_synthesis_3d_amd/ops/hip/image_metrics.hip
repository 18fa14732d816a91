// Fused PSNR + SSIM over a batch of image pairs — CDNA4 gfx950.
//
// pred, target: contiguous (N,H,W,3) in [-1,1], fp32 or bf16. Per element
//   u = clamp(x,-1,1)*0.5 + 0.5            (data_range 1)
//   u = trunc(u*255)/255                   (quantize, pred only: the 8-bit
//                                           value written to PNG; the target
//                                           is a dataset image already)
// PSNR = 10 log10(1/mse) over all H*W*3 elements of one image. SSIM is Wang
// et al. 2004 per channel: 11-tap Gaussian window (sigma 1.5, normalised),
// population moments, C1 = 0.01^2, C2 = 0.03^2, mean over the VALID
// (H-10)*(W-10) window positions x 3 channels (no padding).
//
// Two launches for the whole batch, no host sync, no float atomics:
//   image_metrics_kernel    grid (tiles, N); a block owns a TILE x TILE patch
//       of valid window positions. Per channel it stages the patch plus its
//       10-pixel halo of both images into LDS as fp32, runs the horizontal
//       11-tap pass for the five moments into LDS, the vertical pass from
//       there, forms S and sums it. The squared error of every staged
//       element the block OWNS is summed in the same pass: a block owns the
//       pixels at its window centres, and the first / last tile of a row or
//       column also owns the 5-pixel image border next to it, so every
//       input element is counted exactly once. Each block stores its two
//       sums to partials (N, tiles, 2).
//   image_metrics_finalize  one block per image adds the partials in double
//       in a fixed order and writes psnr[n], ssim[n].
// Every reduction order is fixed by the index math alone: equal inputs give
// equal bits.
//
// Numerics: E[x^2] - mu^2 in fp32 cancels badly in flat regions (C2 = 9e-4
// is small), so the moments are accumulated in fp64: the LDS stage holds
// exact fp32 values (the clamped input, or the integer 8-bit level of a
// quantised pred), the affine map to [0,1] is applied in fp64 as a value is
// read, and both filter passes, the horizontal intermediates and S are
// fp64. fp32 x fp32 products are exact in fp64, so a flat window gives a
// variance of ~1e-17 instead of ~1e-7. The per-thread and per-block sums of
// S (values in [-1,1]) are fp32.
//
// Loads: a staged row is one contiguous run of at most 34*3 elements. It is
// read in 16-byte packs aligned relative to the tensor base (the run's first
// and last pack may hold neighbours' elements, which are dropped); a base
// pointer that is not 16-byte aligned (storage offset) takes scalar loads.
// No load leaves [0, N*H*W*3).

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <cmath>

#include "common.h"

namespace {

constexpr int WIN = 11;                 // window taps
constexpr int HALO = WIN - 1;           // 10
constexpr int TILE = 24;                // valid window positions per side
constexpr int IN = TILE + HALO;         // 34 staged pixels per side
constexpr int NT = 256;                 // threads per block

struct Window {
  double w[WIN];
};

__device__ __forceinline__ float clamp1(float x) {
  return fminf(fmaxf(x, -1.0f), 1.0f);
}

// 8-bit level of a clamped value, with sample.py's fp32 arithmetic
__device__ __forceinline__ float level255(float c) {
  return truncf((c * 0.5f + 0.5f) * 255.0f);
}

// staged fp32 value -> u in [0,1]
__device__ __forceinline__ double unit(float s, bool is_level) {
  return is_level ? (double)s / 255.0 : 0.5 * (double)s + 0.5;
}

// sum over the block in a fixed order; the result is valid in thread 0
__device__ __forceinline__ float block_sum(float x, float* wsum) {
  x = wave_reduce_sum(x);
  const int lane = threadIdx.x & (NVS_WAVE - 1);
  const int wave = threadIdx.x / NVS_WAVE;
  __syncthreads();  // wsum may still be read from the previous call
  if (lane == 0) wsum[wave] = x;
  __syncthreads();
  float tot = wsum[0];
#pragma unroll
  for (int w = 1; w < NT / NVS_WAVE; ++w) tot += wsum[w];
  return tot;
}

// V: elements per load (16 B / sizeof(T), or 1 for an unaligned base).
template <typename T, int V>
__global__ void __launch_bounds__(NT)
image_metrics_kernel(const T* __restrict__ pred, const T* __restrict__ targ,
                     float* __restrict__ partials, int H, int W, int tiles_x,
                     int tiles, int quantize, Window win) {
  __shared__ float sx[IN][IN];           // pred: clamped x, or its 8-bit level
  __shared__ float sy[IN][IN];           // target: clamped y
  __shared__ double hq[5][IN][TILE];     // row-filtered moments
  __shared__ float wsum[NT / NVS_WAVE];

  const int tid = threadIdx.x;
  const int tile = blockIdx.x;
  const int n = blockIdx.y;
  const int ty = tile / tiles_x, tx = tile % tiles_x;
  const int Hv = H - HALO, Wv = W - HALO;
  const int y0 = ty * TILE, x0 = tx * TILE;
  const int th = min(TILE, Hv - y0), tw = min(TILE, Wv - x0);
  const int rows = th + HALO, cols = tw + HALO;  // staged patch, inside image
  // owned pixels, in patch coordinates
  const int orow0 = ty == 0 ? 0 : HALO / 2;
  const int orow1 = y0 + th == Hv ? rows : th + HALO / 2;
  const int ocol0 = tx == 0 ? 0 : HALO / 2;
  const int ocol1 = x0 + tw == Wv ? cols : tw + HALO / 2;

  const long total = (long)gridDim.y * H * W * 3;
  const int run = cols * 3;                       // elements per staged row
  constexpr int MAXPK = (IN * 3 + V - 1) / V + 1; // packs a run can touch
  const bool q = quantize != 0;

  float acc_s = 0.f, acc_e = 0.f;

  for (int ch = 0; ch < 3; ++ch) {
    // ---- stage channel ch of the patch, both images -----------------------
    for (int it = tid; it < rows * MAXPK; it += NT) {
      const int r = it / MAXPK, j = it % MAXPK;
      const long e0 = (((long)n * H + (y0 + r)) * W + x0) * 3;
      const long pk = e0 / V + j;                 // pack index from the base
      const long eb = pk * V;                     // its first element
      if (eb >= e0 + run) continue;
      float vx[V], vy[V];
      if (V > 1 && eb + V <= total) {
        const Pack<T, V> a = pload<T, V>(pred + eb);
        const Pack<T, V> b = pload<T, V>(targ + eb);
#pragma unroll
        for (int i = 0; i < V; ++i) {
          vx[i] = to_f32(a.v[i]);
          vy[i] = to_f32(b.v[i]);
        }
      } else {
#pragma unroll
        for (int i = 0; i < V; ++i) {
          const long e = eb + i < total ? eb + i : total - 1;
          vx[i] = to_f32(pred[e]);
          vy[i] = to_f32(targ[e]);
        }
      }
#pragma unroll
      for (int i = 0; i < V; ++i) {
        const int off = (int)(eb + i - e0);       // element within the run
        if (off < 0 || off >= run) continue;
        const int c = off / 3;
        if (off - c * 3 != ch) continue;
        const float cx = clamp1(vx[i]), cy = clamp1(vy[i]);
        const float stx = q ? level255(cx) : cx;
        sx[r][c] = stx;
        sy[r][c] = cy;
        if (r >= orow0 && r < orow1 && c >= ocol0 && c < ocol1) {
          // unquantised: u_x - u_y = 0.5*(x - y), exact for equal images
          const float d = q ? (float)(unit(stx, true) - unit(cy, false))
                            : 0.5f * (cx - cy);
          acc_e += d * d;
        }
      }
    }
    __syncthreads();

    // ---- horizontal pass: five moments, fp64 ------------------------------
    for (int it = tid; it < rows * TILE; it += NT) {
      const int r = it / TILE, c = it % TILE;
      if (c >= tw) continue;
      double ma = 0.0, mb = 0.0, aa = 0.0, bb = 0.0, ab = 0.0;
#pragma unroll
      for (int k = 0; k < WIN; ++k) {
        const double a = unit(sx[r][c + k], q), b = unit(sy[r][c + k], false);
        const double wa = win.w[k] * a, wb = win.w[k] * b;
        ma += wa;
        mb += wb;
        aa += wa * a;
        bb += wb * b;
        ab += wa * b;
      }
      hq[0][r][c] = ma;
      hq[1][r][c] = mb;
      hq[2][r][c] = aa;
      hq[3][r][c] = bb;
      hq[4][r][c] = ab;
    }
    __syncthreads();

    // ---- vertical pass + SSIM map -----------------------------------------
    for (int it = tid; it < th * TILE; it += NT) {
      const int oy = it / TILE, ox = it % TILE;
      if (ox >= tw) continue;
      double ma = 0.0, mb = 0.0, aa = 0.0, bb = 0.0, ab = 0.0;
#pragma unroll
      for (int k = 0; k < WIN; ++k) {
        const double w = win.w[k];
        ma += w * hq[0][oy + k][ox];
        mb += w * hq[1][oy + k][ox];
        aa += w * hq[2][oy + k][ox];
        bb += w * hq[3][oy + k][ox];
        ab += w * hq[4][oy + k][ox];
      }
      const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
      const double vx = aa - ma * ma, vy = bb - mb * mb, cov = ab - ma * mb;
      acc_s += (float)(((2.0 * ma * mb + C1) * (2.0 * cov + C2))
                       / ((ma * ma + mb * mb + C1) * (vx + vy + C2)));
    }
    __syncthreads();  // sx/sy/hq are rewritten for the next channel
  }

  const float tot_s = block_sum(acc_s, wsum);
  const float tot_e = block_sum(acc_e, wsum);
  if (tid == 0) {
    float* p = partials + ((long)n * tiles + tile) * 2;
    p[0] = tot_s;
    p[1] = tot_e;
  }
}

// One block per image: fixed-order double sums of the tile partials.
__global__ void __launch_bounds__(NT)
image_metrics_finalize_kernel(const float* __restrict__ partials, int tiles,
                              double inv_windows, double inv_elems,
                              float* __restrict__ psnr,
                              float* __restrict__ ssim) {
  __shared__ double rs[NT];
  __shared__ double re[NT];
  const int n = blockIdx.x;
  const float* p = partials + (long)n * tiles * 2;
  double s = 0.0, e = 0.0;
  for (int i = threadIdx.x; i < tiles; i += NT) {
    s += (double)p[2 * i];
    e += (double)p[2 * i + 1];
  }
  rs[threadIdx.x] = s;
  re[threadIdx.x] = e;
  __syncthreads();
  for (int k = NT / 2; k > 0; k >>= 1) {
    if (threadIdx.x < k) {
      rs[threadIdx.x] += rs[threadIdx.x + k];
      re[threadIdx.x] += re[threadIdx.x + k];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double mse = re[0] * inv_elems;
    ssim[n] = (float)(rs[0] * inv_windows);
    psnr[n] = mse == 0.0 ? INFINITY : (float)(10.0 * log10(1.0 / mse));
  }
}

Window gaussian_window() {
  double g[WIN], sum = 0.0;
  for (int k = 0; k < WIN; ++k) {
    const double x = k - (WIN - 1) / 2.0;
    g[k] = std::exp(-(x * x) / (2.0 * 1.5 * 1.5));
    sum += g[k];
  }
  Window w;
  for (int k = 0; k < WIN; ++k) w.w[k] = g[k] / sum;
  return w;
}

}  // namespace

int64_t image_metrics_tile() { return TILE; }

std::vector<torch::Tensor> image_metrics(torch::Tensor pred,
                                         torch::Tensor target,
                                         bool quantize) {
  TORCH_CHECK(pred.is_cuda() && target.is_cuda(),
              "image_metrics: inputs must be on the GPU");
  TORCH_CHECK(pred.dim() == 4 && pred.size(3) == 3
              && pred.sizes() == target.sizes(),
              "image_metrics: pred and target must both be (N,H,W,3)");
  const auto dt = pred.scalar_type();
  TORCH_CHECK((dt == torch::kFloat || dt == torch::kBFloat16)
              && target.scalar_type() == dt,
              "image_metrics: fp32 or bf16, both the same dtype");
  TORCH_CHECK(pred.is_contiguous() && target.is_contiguous(),
              "image_metrics: inputs must be contiguous");
  const long N = pred.size(0), H = pred.size(1), W = pred.size(2);
  TORCH_CHECK(H >= WIN && W >= WIN, "image_metrics: H and W must be >= 11");
  TORCH_CHECK(N >= 1 && N <= 65535, "image_metrics: 1 <= N <= 65535");
  TORCH_CHECK(H < (1 << 24) && W < (1 << 24));
  const long tiles_y = (H - HALO + TILE - 1) / TILE;
  const long tiles_x = (W - HALO + TILE - 1) / TILE;
  const long tiles = tiles_x * tiles_y;
  TORCH_CHECK(tiles < (1L << 31), "image_metrics: image too large");

  auto fopt = pred.options().dtype(torch::kFloat);
  auto partials = torch::empty({N, tiles, 2}, fopt);
  auto psnr = torch::empty({N}, fopt);
  auto ssim = torch::empty({N}, fopt);
  const Window win = gaussian_window();
  const bool al = reinterpret_cast<uintptr_t>(pred.data_ptr()) % 16 == 0
                  && reinterpret_cast<uintptr_t>(target.data_ptr()) % 16 == 0;

  auto stream = at::hip::getCurrentHIPStream();
  auto launch = [&](auto* tag, auto vtag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    constexpr int V = decltype(vtag)::value;
    hipLaunchKernelGGL((image_metrics_kernel<T, V>),
        dim3((unsigned)tiles, (unsigned)N), dim3(NT), 0, stream,
        reinterpret_cast<const T*>(pred.data_ptr()),
        reinterpret_cast<const T*>(target.data_ptr()),
        partials.data_ptr<float>(), (int)H, (int)W, (int)tiles_x,
        (int)tiles, quantize ? 1 : 0, win);
  };
  if (dt == torch::kBFloat16) {
    if (al) launch((bf16*)nullptr, std::integral_constant<int, 8>{});
    else launch((bf16*)nullptr, std::integral_constant<int, 1>{});
  } else {
    if (al) launch((float*)nullptr, std::integral_constant<int, 4>{});
    else launch((float*)nullptr, std::integral_constant<int, 1>{});
  }
  hipLaunchKernelGGL(image_metrics_finalize_kernel, dim3((unsigned)N),
      dim3(NT), 0, stream, partials.data_ptr<float>(), (int)tiles,
      1.0 / ((double)(H - HALO) * (double)(W - HALO) * 3.0),
      1.0 / ((double)H * (double)W * 3.0), psnr.data_ptr<float>(),
      ssim.data_ptr<float>());
  return {psnr, ssim};
}
