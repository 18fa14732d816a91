// Fused multi-tensor Adam — CDNA4 gfx950. SURVEY.md §2.4 K18.
//
// The reference uses optax.adam (/root/reference/train.py:45,74-76); eager
// torch launches per-tensor foreach kernels. Here ONE launch updates every
// parameter: the host packs (p, g, m, v) pointers + a chunk map into device
// buffers once (pointers are stable across steps), and each block processes
// one 64K-element chunk with 16-byte vectorized fp32 loads/stores.
//
//   m = b1*m + (1-b1)*g;  v = b2*v + (1-b2)*g^2
//   p -= lr * (m/bc1) / (sqrt(v/bc2) + eps),  bc_i = 1 - beta_i^step
//
// Training recipe on the same plan (docs/kernels.md "K18"):
//   grad_sqnorm_kernel   one read of g, one fp32 partial per chunk
//   grad_norm_finalize   one block: partials -> ctrl {norm, scale, skip, n}
//   adam_kernel<CLIP,EMA>  g*scale, skip on a non-finite norm, and
//                          ema = d*ema + (1-d)*p_new in the same pass
// The clip factor and the skip decision stay on the device: the update
// kernel reads them from ctrl by pointer. Every reduction runs in a fixed
// order (no float atomics), so equal gradients give an equal clip factor on
// every data-parallel rank.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "common.h"

namespace {

constexpr int CHUNK = 1 << 16;  // elements per block
constexpr int T = 256;

// ctrl buffer layout (fp32[4])
constexpr int CTRL_NORM = 0;
constexpr int CTRL_SCALE = 1;
constexpr int CTRL_SKIP = 2;
constexpr int CTRL_NSKIPPED = 3;

struct AdamScalars {
  float lr, b1, b2, eps, inv_bc1, inv_bc2;
  float scale;  // CLIP only
  float d;      // EMA only
};

// The one copy of the update math. <false,false> never touches g.
template <bool CLIP, bool EMA>
__device__ __forceinline__ void adam_elem(float& p, float g, float& m,
                                          float& v, float& e,
                                          const AdamScalars& s) {
  const float gj = CLIP ? g * s.scale : g;
  const float mj = s.b1 * m + (1.f - s.b1) * gj;
  const float vj = s.b2 * v + (1.f - s.b2) * gj * gj;
  m = mj;
  v = vj;
  p -= s.lr * (mj * s.inv_bc1) / (sqrtf(vj * s.inv_bc2) + s.eps);
  if (EMA) e = s.d * e + (1.f - s.d) * p;
}

__device__ __forceinline__ bool aligned16(unsigned long long a) {
  return (a & 15ull) == 0;
}

template <bool CLIP, bool EMA>
__global__ void adam_kernel(const unsigned long long* __restrict__ ptrs, // (n,4)
                            const unsigned long long* __restrict__ ema_ptrs, // (n,)
                            const int* __restrict__ chunk_tensor,
                            const long* __restrict__ chunk_off,
                            const long* __restrict__ numels,
                            const float* __restrict__ ctrl,
                            float lr, float b1, float b2, float eps,
                            float bc1, float bc2, float ema_d) {
  AdamScalars s;
  s.lr = lr; s.b1 = b1; s.b2 = b2; s.eps = eps;
  s.inv_bc1 = 1.f / bc1;
  s.inv_bc2 = 1.f / bc2;
  s.scale = 1.f;
  s.d = ema_d;
  if (CLIP) {
    // non-finite gradient norm: leave p, m, v and ema untouched
    if (ctrl[CTRL_SKIP] != 0.f) return;
    s.scale = ctrl[CTRL_SCALE];
  }

  const int ci = blockIdx.x;
  const int tidx = chunk_tensor[ci];
  const long off = chunk_off[ci];
  const long n = min((long)CHUNK, numels[tidx] - off);
  const unsigned long long ap = ptrs[tidx * 4 + 0], ag = ptrs[tidx * 4 + 1];
  const unsigned long long am = ptrs[tidx * 4 + 2], av = ptrs[tidx * 4 + 3];
  const unsigned long long ae = EMA ? ema_ptrs[tidx] : 0ull;
  float* p = reinterpret_cast<float*>(ap) + off;
  const float* g = reinterpret_cast<const float*>(ag) + off;
  float* m = reinterpret_cast<float*>(am) + off;
  float* v = reinterpret_cast<float*>(av) + off;
  float* e = EMA ? reinterpret_cast<float*>(ae) + off : nullptr;

  // off is a multiple of CHUNK, so the base pointers decide alignment. A
  // gradient that is a view into a flat data-parallel bucket is only 4-byte
  // aligned: such a chunk takes the scalar loop for all of its elements.
  const bool vec = aligned16(ap) && aligned16(ag) && aligned16(am) &&
                   aligned16(av) && aligned16(ae);
  float unused = 0.f;

  if (vec) {
    const long stride = (long)T * 4;
    // vectorized body (n multiple of 4 within the bulk)
    for (long i = (long)threadIdx.x * 4; i + 3 < n; i += stride) {
      Pack<float, 4> pg = pload<float, 4>(g + i);
      Pack<float, 4> pm = pload<float, 4>(m + i);
      Pack<float, 4> pv = pload<float, 4>(v + i);
      Pack<float, 4> pp = pload<float, 4>(p + i);
      Pack<float, 4> pe;
      if (EMA) pe = pload<float, 4>(e + i);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        adam_elem<CLIP, EMA>(pp.v[j], pg.v[j], pm.v[j], pv.v[j],
                             EMA ? pe.v[j] : unused, s);
      }
      pstore<float, 4>(m + i, pm);
      pstore<float, 4>(v + i, pv);
      pstore<float, 4>(p + i, pp);
      if (EMA) pstore<float, 4>(e + i, pe);
    }
  }
  // scalar loop: the tail of a vectorized chunk, or all of an unaligned one
  for (long i = (vec ? (n & ~3L) : 0L) + threadIdx.x; i < n; i += T) {
    adam_elem<CLIP, EMA>(p[i], g[i], m[i], v[i], EMA ? e[i] : unused, s);
  }
}

// Sum of g^2 over one chunk -> partials[partial_off + chunk]. Each thread
// keeps 4 fp32 accumulators (longest add chain: CHUNK/(T*4) = 64 FMAs, at
// most 3 tail adds, then 2 adds, 6 shuffle levels and 3 LDS adds); the order
// is fixed by the index math alone, so the same gradients always give the
// same bits.
__global__ void grad_sqnorm_kernel(const unsigned long long* __restrict__ ptrs,
                                   const int* __restrict__ chunk_tensor,
                                   const long* __restrict__ chunk_off,
                                   const long* __restrict__ numels,
                                   float* __restrict__ partials) {
  const int ci = blockIdx.x;
  const int tidx = chunk_tensor[ci];
  const long off = chunk_off[ci];
  const long n = min((long)CHUNK, numels[tidx] - off);
  const unsigned long long ag = ptrs[tidx * 4 + 1];
  const float* g = reinterpret_cast<const float*>(ag) + off;

  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  if (aligned16(ag)) {
    const long stride = (long)T * 4;
#pragma unroll 4
    for (long i = (long)threadIdx.x * 4; i + 3 < n; i += stride) {
      Pack<float, 4> pg = pload<float, 4>(g + i);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] += pg.v[j] * pg.v[j];
    }
    for (long i = (n & ~3L) + threadIdx.x; i < n; i += T) {
      acc[0] += g[i] * g[i];
    }
  } else {
    // 4-byte aligned gradient view: coalesced scalar loads, 4 per round
    long base = 0;
    for (; base + (long)T * 4 <= n; base += (long)T * 4) {
      float x[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) x[j] = g[base + j * T + threadIdx.x];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] += x[j] * x[j];
    }
    for (long i = base + threadIdx.x; i < n; i += T) {
      acc[0] += g[i] * g[i];
    }
  }
  float x = wave_reduce_sum((acc[0] + acc[1]) + (acc[2] + acc[3]));

  __shared__ float wsum[T / NVS_WAVE];
  const int lane = threadIdx.x & (NVS_WAVE - 1);
  const int wave = threadIdx.x / NVS_WAVE;
  if (lane == 0) wsum[wave] = x;
  __syncthreads();
  if (threadIdx.x == 0) {
    float tot = wsum[0];
#pragma unroll
    for (int w = 1; w < T / NVS_WAVE; ++w) tot += wsum[w];
    partials[ci] = tot;
  }
}

// One block: sum the partials in a fixed order in double, then write
// ctrl = {norm, scale, skip, skipped_steps}.
__global__ void grad_norm_finalize_kernel(const float* __restrict__ partials,
                                          int nparts, float max_norm,
                                          float* __restrict__ ctrl) {
  __shared__ double red[T];
  double a = 0.0;
  for (int i = threadIdx.x; i < nparts; i += T) a += (double)partials[i];
  red[threadIdx.x] = a;
  __syncthreads();
  for (int s = T / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(red[0]);
    const bool bad = !isfinite(norm);
    ctrl[CTRL_NORM] = norm;
    ctrl[CTRL_SCALE] = bad ? 0.f : fminf(1.f, max_norm / (norm + 1e-6f));
    ctrl[CTRL_SKIP] = bad ? 1.f : 0.f;
    ctrl[CTRL_NSKIPPED] += bad ? 1.f : 0.f;
  }
}

void check_plan(const torch::Tensor& ptrs, const torch::Tensor& chunk_tensor,
                const torch::Tensor& chunk_off, const torch::Tensor& numels) {
  TORCH_CHECK(ptrs.is_cuda() && ptrs.scalar_type() == torch::kUInt64);
  TORCH_CHECK(chunk_tensor.is_cuda() &&
              chunk_tensor.scalar_type() == torch::kInt32);
  TORCH_CHECK(chunk_off.is_cuda() && chunk_off.scalar_type() == torch::kInt64);
  TORCH_CHECK(numels.is_cuda() && numels.scalar_type() == torch::kInt64);
  TORCH_CHECK(chunk_off.size(0) == chunk_tensor.size(0));
  TORCH_CHECK(ptrs.numel() == 4 * numels.numel());
}

void check_ctrl(const torch::Tensor& ctrl) {
  TORCH_CHECK(ctrl.is_cuda() && ctrl.scalar_type() == torch::kFloat32 &&
              ctrl.is_contiguous() && ctrl.numel() >= 4,
              "ctrl must be a contiguous fp32[4] device tensor");
}

template <bool CLIP, bool EMA>
void launch_adam(const torch::Tensor& ptrs, const unsigned long long* ema_ptrs,
                 const torch::Tensor& chunk_tensor,
                 const torch::Tensor& chunk_off, const torch::Tensor& numels,
                 const float* ctrl, double lr, double b1, double b2,
                 double eps, int64_t step, double ema_decay) {
  const int nchunks = chunk_tensor.size(0);
  if (nchunks == 0) return;
  const float bc1 = 1.f - powf((float)b1, (float)step);
  const float bc2 = 1.f - powf((float)b2, (float)step);
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL((adam_kernel<CLIP, EMA>), dim3(nchunks), dim3(T), 0,
      stream,
      reinterpret_cast<const unsigned long long*>(ptrs.data_ptr()),
      ema_ptrs, chunk_tensor.data_ptr<int>(), chunk_off.data_ptr<long>(),
      numels.data_ptr<long>(), ctrl,
      (float)lr, (float)b1, (float)b2, (float)eps, bc1, bc2,
      (float)ema_decay);
}

}  // namespace

void fused_adam(torch::Tensor ptrs, torch::Tensor chunk_tensor,
                torch::Tensor chunk_off, torch::Tensor numels,
                double lr, double b1, double b2, double eps, int64_t step) {
  TORCH_CHECK(ptrs.is_cuda() && ptrs.scalar_type() == torch::kUInt64);
  launch_adam<false, false>(ptrs, nullptr, chunk_tensor, chunk_off, numels,
                            nullptr, lr, b1, b2, eps, step, 0.0);
}

// Adam with the optional recipe parts: ctrl given -> clip + skip,
// ema_ptrs given -> EMA with decay ema_decay.
void fused_adam_recipe(torch::Tensor ptrs,
                       c10::optional<torch::Tensor> ema_ptrs,
                       torch::Tensor chunk_tensor, torch::Tensor chunk_off,
                       torch::Tensor numels,
                       c10::optional<torch::Tensor> ctrl,
                       double lr, double b1, double b2, double eps,
                       int64_t step, double ema_decay) {
  check_plan(ptrs, chunk_tensor, chunk_off, numels);
  const unsigned long long* ep = nullptr;
  if (ema_ptrs.has_value()) {
    TORCH_CHECK(ema_ptrs->is_cuda() &&
                ema_ptrs->scalar_type() == torch::kUInt64 &&
                ema_ptrs->numel() == numels.numel(),
                "ema_ptrs must be a (n,) uint64 device tensor");
    ep = reinterpret_cast<const unsigned long long*>(ema_ptrs->data_ptr());
  }
  const float* cp = nullptr;
  if (ctrl.has_value()) {
    check_ctrl(*ctrl);
    cp = ctrl->data_ptr<float>();
  }
  if (cp && ep) {
    launch_adam<true, true>(ptrs, ep, chunk_tensor, chunk_off, numels, cp,
                            lr, b1, b2, eps, step, ema_decay);
  } else if (cp) {
    launch_adam<true, false>(ptrs, ep, chunk_tensor, chunk_off, numels, cp,
                             lr, b1, b2, eps, step, ema_decay);
  } else if (ep) {
    launch_adam<false, true>(ptrs, ep, chunk_tensor, chunk_off, numels, cp,
                             lr, b1, b2, eps, step, ema_decay);
  } else {
    launch_adam<false, false>(ptrs, ep, chunk_tensor, chunk_off, numels, cp,
                              lr, b1, b2, eps, step, ema_decay);
  }
}

// partials[partial_off + c] = sum of g^2 over chunk c of this plan
void grad_sqnorm(torch::Tensor ptrs, torch::Tensor chunk_tensor,
                 torch::Tensor chunk_off, torch::Tensor numels,
                 torch::Tensor partials, int64_t partial_off) {
  check_plan(ptrs, chunk_tensor, chunk_off, numels);
  const int64_t nchunks = chunk_tensor.size(0);
  TORCH_CHECK(partials.is_cuda() &&
              partials.scalar_type() == torch::kFloat32 &&
              partials.is_contiguous());
  TORCH_CHECK(partial_off >= 0 && partial_off + nchunks <= partials.numel(),
              "partials buffer too small");
  if (nchunks == 0) return;
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(grad_sqnorm_kernel, dim3((int)nchunks), dim3(T), 0,
      stream,
      reinterpret_cast<const unsigned long long*>(ptrs.data_ptr()),
      chunk_tensor.data_ptr<int>(), chunk_off.data_ptr<long>(),
      numels.data_ptr<long>(), partials.data_ptr<float>() + partial_off);
}

void grad_norm_finalize(torch::Tensor partials, torch::Tensor ctrl,
                        double max_norm) {
  TORCH_CHECK(partials.is_cuda() &&
              partials.scalar_type() == torch::kFloat32 &&
              partials.is_contiguous());
  check_ctrl(ctrl);
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(grad_norm_finalize_kernel, dim3(1), dim3(T), 0, stream,
      partials.data_ptr<float>(), (int)partials.numel(), (float)max_norm,
      ctrl.data_ptr<float>());
}
