// Stochastic-conditioning sampler step kernels — CDNA4 gfx950.
//
//  * cond_emb_select: per-level FiLM input silu(logsnr_emb + pose feature),
//    where frame 0 of the conditional CFG half is GATHERED from a bank of
//    per-view source features by a device-side index, frame 0 of the
//    unconditional half is the (view-independent) null feature and frame 1 is
//    the target-frame feature. Replaces the eager add + silu passes of
//    XUNet.forward's emb_at at the same memory traffic.
//  * ddpm_cfg_step: CFG combine + x0 prediction (+clamp) + posterior mean +
//    noise, in place on z, coefficients read from the device step tables at
//    the device step counter; a second small kernel writes the next step's
//    model input x from the image bank and publishes the advanced counter.
//  * solver_cfg_step: the same step for any solver of diffusion/solvers.py
//    (ddpm, ddim, dpmpp2m): z' = coef_z z + coef_x0 x0 + coef_hist x0_prev
//    + sigma noise, with one optional history buffer (the previous step's x0)
//    and optional noise; the same gather kernel follows when there is a bank.
//
// Index rule (shared with ops/reference.py stochastic_index):
//   idx[s,b] = min(floor(u[s,b] * k), k-1) in fp32, s = device step counter,
//   k = device scalar (number of valid bank entries).
// Nothing that varies per step comes from the host, so one captured hipGraph
// serves every step of every view. Both kernels are bandwidth-bound: 16-byte
// packs, grid-stride, plain vector stores, no LDS, wave64-agnostic.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "common.h"

namespace {

__device__ __forceinline__ long clampl(long v, long lo, long hi) {
  return v < lo ? lo : (v > hi ? hi : v);
}

// The index rule. S/Kcap clamps keep every derived address in bounds even
// for a counter or k the host left out of range.
__device__ __forceinline__ int bank_index(const float* __restrict__ u,
                                          long s, int S, int B, int b,
                                          long k, int Kcap) {
  s = clampl(s, 0, S - 1);
  const int kk = (int)clampl(k, 1, Kcap);
  const float uu = u[s * B + b];
  int j = (int)floorf(uu * (float)kk);
  j = j < kk - 1 ? j : kk - 1;
  return j > 0 ? j : 0;
}

__device__ __forceinline__ float silu_f32(float x) {
  return x / (1.0f + expf(-x));
}

// out (2B,2,HW,E) = silu(lemb[r] + feat); one pack of V channels per thread.
// blockIdx.y = (row r, frame f): the source plane is chosen once per block
// and the plane is walked with a 32-bit index (plane = HW*E/V packs), so
// the only per-pack division is one 32-bit modulo for the channel.
template <typename T, int V>
__global__ void cond_emb_select_kernel(
    const T* __restrict__ lemb, const T* __restrict__ bank,
    const T* __restrict__ nullf, const T* __restrict__ tgt,
    const float* __restrict__ u, const long* __restrict__ step,
    const long* __restrict__ kvalid, T* __restrict__ out,
    unsigned plane, int B, int HW, int E, int S, int Kcap, int null_b) {
  const unsigned Ep = (unsigned)(E / V);
  const int f = (int)(blockIdx.y & 1);
  const int r = (int)(blockIdx.y >> 1);
  const long plane_elems = (long)HW * E;
  const T* src;
  if (f == 1) {
    src = tgt + (long)r * plane_elems;
  } else if (r < B) {
    const int j = bank_index(u, step[0], S, B, r, kvalid[0], Kcap);
    src = bank + ((long)j * B + r) * plane_elems;
  } else {
    src = nullf + (long)(null_b == 1 ? 0 : r - B) * plane_elems;
  }
  const T* le = lemb + (long)r * E;
  T* dst = out + (long)blockIdx.y * plane_elems;
  const unsigned gstride = gridDim.x * blockDim.x;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < plane;
       i += gstride) {
    const unsigned c = (i % Ep) * V;
    Pack<T, V> a = pload<T, V>(le + c);
    Pack<T, V> v = pload<T, V>(src + (long)i * V);
    Pack<T, V> o;
#pragma unroll
    for (int j = 0; j < V; ++j)
      from_f32(silu_f32(to_f32(a.v[j]) + to_f32(v.v[j])), o.v[j]);
    pstore<T, V>(dst + (long)i * V, o);
  }
}

__device__ __forceinline__ float ddpm_elem(float z, float oc, float ou,
                                           float nz, float w, float ca,
                                           float cb, float c1, float c2,
                                           float sg, bool clip) {
  const float eps = (1.0f + w) * oc - w * ou;
  float x0 = ca * z - cb * eps;
  if (clip) x0 = fminf(fmaxf(x0, -1.0f), 1.0f);
  return c1 * x0 + c2 * z + sg * nz;
}

// z (n) <- posterior sample; out holds the conditional half at [0,n) and the
// unconditional half at [n,2n). 4-element packs (16 B of fp32) + scalar
// tail. ALIGNED_U: n % 4 == 0, so the unconditional half is pack-aligned;
// otherwise its loads are scalar.
template <typename TO, bool ALIGNED_U>
__global__ void ddpm_cfg_step_kernel(
    float* __restrict__ z, const TO* __restrict__ out,
    const float* __restrict__ noise, const float* __restrict__ t_ca,
    const float* __restrict__ t_cb, const float* __restrict__ t_c1,
    const float* __restrict__ t_c2, const float* __restrict__ t_sigma,
    const long* __restrict__ step, long* __restrict__ step_next,
    long n, int S, float w, float noise_scale, int clip) {
  const long s_raw = step[0];
  const long s = clampl(s_raw, 0, S - 1);
  const float ca = t_ca[s], cb = t_cb[s], c1 = t_c1[s], c2 = t_c2[s];
  const float sg = noise_scale * t_sigma[s];
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long gstride = (long)gridDim.x * blockDim.x;
  const long npack = n / 4;
  for (long i = tid; i < npack; i += gstride) {
    Pack<float, 4> vz = pload<float, 4>(z + i * 4);
    Pack<float, 4> vn = pload<float, 4>(noise + i * 4);
    Pack<TO, 4> vc = pload<TO, 4>(out + i * 4);
    Pack<TO, 4> vu;
    if (ALIGNED_U) {
      vu = pload<TO, 4>(out + n + i * 4);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) vu.v[j] = out[n + i * 4 + j];
    }
    Pack<float, 4> o;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      o.v[j] = ddpm_elem(vz.v[j], to_f32(vc.v[j]), to_f32(vu.v[j]), vn.v[j],
                         w, ca, cb, c1, c2, sg, clip != 0);
    pstore<float, 4>(z + i * 4, o);
  }
  // scalar tail: n % 4 trailing elements
  const long i = npack * 4 + tid;
  if (i < n)
    z[i] = ddpm_elem(z[i], to_f32(out[i]), to_f32(out[n + i]), noise[i], w,
                     ca, cb, c1, c2, sg, clip != 0);
  // The advanced counter goes to a shadow slot: other blocks of this launch
  // may still be reading step[0]. The gather kernel publishes it.
  if (tid == 0) step_next[0] = s_raw + 1;
}

// One step of a solver of diffusion/solvers.py on one element:
//   x0 = ca z - cb eps (clamped);  z' = cz z + cx x0 [+ ch h] [+ sg nz].
// Explicit fma chain: the rounding does not depend on the contraction mode.
struct SolverCoef {
  float w, ca, cb, cz, cx, ch, sg;
  bool clip, rd_hist, use_noise;
};

__device__ __forceinline__ float solver_elem(float z, float oc, float ou,
                                             float h, float nz,
                                             const SolverCoef& c,
                                             float& x0_out) {
  const float eps = fmaf(-c.w, ou, (1.0f + c.w) * oc);
  float x0 = fmaf(-c.cb, eps, c.ca * z);
  if (c.clip) x0 = fminf(fmaxf(x0, -1.0f), 1.0f);
  x0_out = x0;
  float r = fmaf(c.cx, x0, c.cz * z);
  if (c.rd_hist) r = fmaf(c.ch, h, r);
  if (c.use_noise) r = fmaf(c.sg, nz, r);
  return r;
}

// z (n) <- solver step, hist (n) <- x0; layout of `out`, packs, tail and
// ALIGNED_U as in ddpm_cfg_step_kernel. hist and noise may be null. hist is
// READ only when the step's coef_hist is nonzero (0 * NaN would reach z
// otherwise) and written whenever it is given; noise is read only when it is
// given. All three conditions are uniform over the launch.
template <typename TO, bool ALIGNED_U>
__global__ void solver_cfg_step_kernel(
    float* __restrict__ z, float* __restrict__ hist,
    const TO* __restrict__ out, const float* __restrict__ noise,
    const float* __restrict__ t_ca, const float* __restrict__ t_cb,
    const float* __restrict__ t_cz, const float* __restrict__ t_cx,
    const float* __restrict__ t_ch, const float* __restrict__ t_sigma,
    const long* __restrict__ step, long* __restrict__ step_next,
    long n, int S, float w, float noise_scale, int clip) {
  const long s_raw = step[0];
  const long s = clampl(s_raw, 0, S - 1);
  SolverCoef c;
  c.w = w;
  c.ca = t_ca[s], c.cb = t_cb[s], c.cz = t_cz[s], c.cx = t_cx[s];
  c.ch = t_ch[s];
  c.sg = noise_scale * t_sigma[s];
  c.clip = clip != 0;
  c.rd_hist = hist != nullptr && c.ch != 0.0f;
  c.use_noise = noise != nullptr;
  const bool wr_hist = hist != nullptr;
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long gstride = (long)gridDim.x * blockDim.x;
  const long npack = n / 4;
  for (long i = tid; i < npack; i += gstride) {
    Pack<float, 4> vz = pload<float, 4>(z + i * 4);
    Pack<float, 4> vh = {}, vn = {};
    if (c.rd_hist) vh = pload<float, 4>(hist + i * 4);
    if (c.use_noise) vn = pload<float, 4>(noise + i * 4);
    Pack<TO, 4> vc = pload<TO, 4>(out + i * 4);
    Pack<TO, 4> vu;
    if (ALIGNED_U) {
      vu = pload<TO, 4>(out + n + i * 4);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) vu.v[j] = out[n + i * 4 + j];
    }
    Pack<float, 4> o, x0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      o.v[j] = solver_elem(vz.v[j], to_f32(vc.v[j]), to_f32(vu.v[j]),
                           vh.v[j], vn.v[j], c, x0.v[j]);
    pstore<float, 4>(z + i * 4, o);
    if (wr_hist) pstore<float, 4>(hist + i * 4, x0);
  }
  // scalar tail: n % 4 trailing elements
  const long i = npack * 4 + tid;
  if (i < n) {
    float x0;
    const float h = c.rd_hist ? hist[i] : 0.0f;
    const float nz = c.use_noise ? noise[i] : 0.0f;
    z[i] = solver_elem(z[i], to_f32(out[i]), to_f32(out[n + i]), h, nz, c,
                       x0);
    if (wr_hist) hist[i] = x0;
  }
  // shadow slot, as in ddpm_cfg_step_kernel: other blocks of this launch
  // may still be reading step[0]
  if (tid == 0) step_next[0] = s_raw + 1;
}

// Publishes the advanced counter when there is no bank (and so no gather
// kernel to do it): a launch of its own, after every reader of step[0].
__global__ void publish_step_kernel(const long* __restrict__ step_next,
                                    long* __restrict__ step) {
  if (blockIdx.x == 0 && threadIdx.x == 0) step[0] = step_next[0];
}

// x (2B, m) <- bank_img[idx_next[b], b] for both CFG halves, where idx_next
// is the index rule at the ADVANCED counter; then publish the counter.
template <int V>
__global__ void next_x_gather_kernel(
    const float* __restrict__ bank_img, float* __restrict__ x,
    const float* __restrict__ u, const long* __restrict__ step_next,
    const long* __restrict__ kvalid, long* __restrict__ step,
    long total, int B, long m, int S, int Kcap) {
  const long s1 = step_next[0];
  const long k = kvalid[0];
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  // after the last step of a view there is no next step: x is left alone
  // (the host rewrites it when it resets the per-view state)
  if (s1 >= 0 && s1 < S) {
    const long mp = m / V;
    const long gstride = (long)gridDim.x * blockDim.x;
    for (long i = tid; i < total; i += gstride) {
      const int b = (int)(i / mp);
      const long e = (i % mp) * V;
      const int j = bank_index(u, s1, S, B, b, k, Kcap);
      Pack<float, V> v =
          pload<float, V>(bank_img + ((long)j * B + b) * m + e);
      pstore<float, V>(x + (long)b * m + e, v);
      pstore<float, V>(x + ((long)B + b) * m + e, v);
    }
  }
  // nobody in this launch reads step[0]
  if (tid == 0) step[0] = s1;
}

int grid_for(long work) {
  return (int)std::max<long>(1, std::min<long>((work + 255) / 256, 8192));
}

bool aligned16(const torch::Tensor& t) {
  return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
}

void check_index_inputs(const torch::Tensor& u, const torch::Tensor& step,
                        const torch::Tensor& kvalid, int B) {
  TORCH_CHECK(u.is_cuda() && u.is_contiguous() && u.dim() == 2
              && u.scalar_type() == torch::kFloat && u.size(1) == B
              && u.size(0) >= 1, "u must be a contiguous fp32 (S,B) table");
  TORCH_CHECK(step.is_cuda() && step.scalar_type() == torch::kLong
              && step.numel() == 1, "step must be a device int64 scalar");
  TORCH_CHECK(kvalid.is_cuda() && kvalid.scalar_type() == torch::kLong
              && kvalid.numel() == 1, "k must be a device int64 scalar");
}

}  // namespace

torch::Tensor cond_emb_select(torch::Tensor lemb, torch::Tensor bank,
                              torch::Tensor nullf, torch::Tensor tgt,
                              torch::Tensor u, torch::Tensor step,
                              torch::Tensor kvalid) {
  TORCH_CHECK(bank.is_cuda() && lemb.is_cuda() && nullf.is_cuda()
              && tgt.is_cuda(), "cond_emb_select: inputs must be on the GPU");
  TORCH_CHECK(bank.dim() == 5 && tgt.dim() == 4 && nullf.dim() == 4
              && lemb.dim() == 2);
  const auto dt = bank.scalar_type();
  TORCH_CHECK(dt == torch::kBFloat16 || dt == torch::kFloat,
              "cond_emb_select: bf16 or fp32 only");
  TORCH_CHECK(lemb.scalar_type() == dt && nullf.scalar_type() == dt
              && tgt.scalar_type() == dt, "cond_emb_select: dtype mismatch");
  TORCH_CHECK(lemb.is_contiguous() && bank.is_contiguous()
              && nullf.is_contiguous() && tgt.is_contiguous());
  const int Kcap = bank.size(0), B = bank.size(1);
  const int Hh = bank.size(2), Ww = bank.size(3), E = bank.size(4);
  const int HW = Hh * Ww;
  TORCH_CHECK(Kcap >= 1 && B >= 1 && HW >= 1 && E >= 1);
  // grid.y = 4B planes, each walked with a 32-bit pack index
  TORCH_CHECK(4L * B <= 65535 && (long)HW * E < (1L << 31),
              "cond_emb_select: batch or level too large");
  TORCH_CHECK(lemb.size(0) == 2 * B && lemb.size(1) == E);
  TORCH_CHECK(tgt.size(0) == 2 * B && tgt.size(1) == Hh && tgt.size(2) == Ww
              && tgt.size(3) == E);
  TORCH_CHECK((nullf.size(0) == 1 || nullf.size(0) == B)
              && nullf.size(1) == Hh && nullf.size(2) == Ww
              && nullf.size(3) == E);
  check_index_inputs(u, step, kvalid, B);
  const int S = u.size(0);
  const int null_b = nullf.size(0);

  auto out = torch::empty({2 * B, 2, Hh, Ww, E}, bank.options());
  const bool vec = E % 8 == 0 && aligned16(lemb) && aligned16(bank)
                   && aligned16(nullf) && aligned16(tgt) && aligned16(out);
  auto stream = at::hip::getCurrentHIPStream();
  auto launch = [&](auto* tag, auto vtag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    constexpr int V = decltype(vtag)::value;
    const unsigned plane = (unsigned)((long)HW * E / V);
    hipLaunchKernelGGL((cond_emb_select_kernel<T, V>),
        dim3(grid_for(plane), 4 * B), dim3(256), 0, stream,
        reinterpret_cast<const T*>(lemb.data_ptr()),
        reinterpret_cast<const T*>(bank.data_ptr()),
        reinterpret_cast<const T*>(nullf.data_ptr()),
        reinterpret_cast<const T*>(tgt.data_ptr()), u.data_ptr<float>(),
        reinterpret_cast<const long*>(step.data_ptr()),
        reinterpret_cast<const long*>(kvalid.data_ptr()),
        reinterpret_cast<T*>(out.data_ptr()), plane, B, HW, E, S, Kcap,
        null_b);
  };
  if (dt == torch::kBFloat16) {
    if (vec) launch((bf16*)nullptr, std::integral_constant<int, 8>{});
    else launch((bf16*)nullptr, std::integral_constant<int, 1>{});
  } else {
    if (vec) launch((float*)nullptr, std::integral_constant<int, 4>{});
    else launch((float*)nullptr, std::integral_constant<int, 1>{});
  }
  return out;
}

void ddpm_cfg_step(torch::Tensor z, torch::Tensor out, torch::Tensor noise,
                   torch::Tensor t_ca, torch::Tensor t_cb, torch::Tensor t_c1,
                   torch::Tensor t_c2, torch::Tensor t_sigma,
                   torch::Tensor step, torch::Tensor step_next,
                   torch::Tensor u, torch::Tensor kvalid,
                   torch::Tensor bank_img, torch::Tensor x, double w,
                   bool clip, double noise_scale) {
  TORCH_CHECK(z.is_cuda() && z.is_contiguous()
              && z.scalar_type() == torch::kFloat && z.dim() == 4);
  TORCH_CHECK(noise.is_contiguous() && noise.scalar_type() == torch::kFloat
              && noise.numel() == z.numel());
  TORCH_CHECK(out.is_contiguous() && out.numel() == 2 * z.numel()
              && (out.scalar_type() == torch::kBFloat16
                  || out.scalar_type() == torch::kFloat));
  const int B = z.size(0);
  const long n = z.numel();
  const long m = n / B;
  check_index_inputs(u, step, kvalid, B);
  const int S = u.size(0);
  for (const auto* t : {&t_ca, &t_cb, &t_c1, &t_c2, &t_sigma})
    TORCH_CHECK(t->is_cuda() && t->is_contiguous()
                && t->scalar_type() == torch::kFloat && t->numel() == S,
                "step tables must be fp32 (S,) matching u's S");
  TORCH_CHECK(step_next.is_cuda() && step_next.scalar_type() == torch::kLong
              && step_next.numel() == 1
              && step_next.data_ptr() != step.data_ptr());
  TORCH_CHECK(bank_img.is_cuda() && bank_img.is_contiguous()
              && bank_img.scalar_type() == torch::kFloat
              && bank_img.dim() == 5 && bank_img.size(0) >= 1
              && bank_img.size(1) == B && bank_img.numel()
                 == bank_img.size(0) * n);
  TORCH_CHECK(x.is_cuda() && x.is_contiguous()
              && x.scalar_type() == torch::kFloat && x.numel() == 2 * n);
  const int Kcap = bank_img.size(0);
  TORCH_CHECK(aligned16(z) && aligned16(noise) && aligned16(out),
              "ddpm_cfg_step: z/noise/out must be 16-byte aligned");

  auto stream = at::hip::getCurrentHIPStream();
  const int grid = grid_for((n + 3) / 4);
  auto launch = [&](auto* tag, auto atag) {
    using TO = std::remove_pointer_t<decltype(tag)>;
    constexpr bool AL = decltype(atag)::value;
    hipLaunchKernelGGL((ddpm_cfg_step_kernel<TO, AL>), dim3(grid), dim3(256),
        0, stream, z.data_ptr<float>(),
        reinterpret_cast<const TO*>(out.data_ptr()), noise.data_ptr<float>(),
        t_ca.data_ptr<float>(), t_cb.data_ptr<float>(),
        t_c1.data_ptr<float>(), t_c2.data_ptr<float>(),
        t_sigma.data_ptr<float>(),
        reinterpret_cast<const long*>(step.data_ptr()),
        reinterpret_cast<long*>(step_next.data_ptr()), n, S, (float)w,
        (float)noise_scale, clip ? 1 : 0);
  };
  const bool al = n % 4 == 0;
  if (out.scalar_type() == torch::kBFloat16) {
    if (al) launch((bf16*)nullptr, std::true_type{});
    else launch((bf16*)nullptr, std::false_type{});
  } else {
    if (al) launch((float*)nullptr, std::true_type{});
    else launch((float*)nullptr, std::false_type{});
  }

  const bool vec = m % 4 == 0 && aligned16(bank_img) && aligned16(x);
  auto gather = [&](auto vtag) {
    constexpr int V = decltype(vtag)::value;
    const long total = n / V;
    hipLaunchKernelGGL((next_x_gather_kernel<V>), dim3(grid_for(total)),
        dim3(256), 0, stream, bank_img.data_ptr<float>(),
        x.data_ptr<float>(), u.data_ptr<float>(),
        reinterpret_cast<const long*>(step_next.data_ptr()),
        reinterpret_cast<const long*>(kvalid.data_ptr()),
        reinterpret_cast<long*>(step.data_ptr()), total, B, m, S, Kcap);
  };
  if (vec) gather(std::integral_constant<int, 4>{});
  else gather(std::integral_constant<int, 1>{});
}

// Solver step (ddpm / ddim / dpmpp2m tables). hist and noise are optional;
// u, kvalid, bank_img and x come together or not at all: with them the next
// step's x is gathered and the gather kernel publishes the counter, without
// them a one-thread kernel does.
void solver_cfg_step(torch::Tensor z, c10::optional<torch::Tensor> hist,
                     torch::Tensor out, c10::optional<torch::Tensor> noise,
                     torch::Tensor t_ca, torch::Tensor t_cb,
                     torch::Tensor t_cz, torch::Tensor t_cx,
                     torch::Tensor t_ch, torch::Tensor t_sigma,
                     torch::Tensor step, torch::Tensor step_next,
                     c10::optional<torch::Tensor> u,
                     c10::optional<torch::Tensor> kvalid,
                     c10::optional<torch::Tensor> bank_img,
                     c10::optional<torch::Tensor> x, double w, bool clip,
                     double noise_scale) {
  TORCH_CHECK(z.is_cuda() && z.is_contiguous()
              && z.scalar_type() == torch::kFloat && z.dim() == 4
              && z.numel() >= 1);
  const int B = z.size(0);
  const long n = z.numel();
  const long m = n / B;
  auto same_as_z = [&](const torch::Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.is_contiguous()
                && t.scalar_type() == torch::kFloat && t.numel() == n
                && aligned16(t) && t.data_ptr() != z.data_ptr(),
                "solver_cfg_step: ", name, " must be a contiguous 16-byte "
                "aligned fp32 GPU tensor of z's size, distinct from z");
  };
  if (hist.has_value()) same_as_z(*hist, "hist");
  if (noise.has_value()) same_as_z(*noise, "noise");
  TORCH_CHECK(out.is_cuda() && out.is_contiguous()
              && out.numel() == 2 * n
              && (out.scalar_type() == torch::kBFloat16
                  || out.scalar_type() == torch::kFloat));
  TORCH_CHECK(aligned16(z) && aligned16(out),
              "solver_cfg_step: z/out must be 16-byte aligned");
  const long S = t_ca.numel();
  TORCH_CHECK(S >= 1 && S < (1L << 31));
  for (const auto* t : {&t_ca, &t_cb, &t_cz, &t_cx, &t_ch, &t_sigma})
    TORCH_CHECK(t->is_cuda() && t->is_contiguous()
                && t->scalar_type() == torch::kFloat && t->numel() == S,
                "step tables must be fp32 (S,) of one length");
  TORCH_CHECK(step.is_cuda() && step.scalar_type() == torch::kLong
              && step.numel() == 1, "step must be a device int64 scalar");
  TORCH_CHECK(step_next.is_cuda() && step_next.scalar_type() == torch::kLong
              && step_next.numel() == 1
              && step_next.data_ptr() != step.data_ptr());
  const bool bank = bank_img.has_value();
  TORCH_CHECK(u.has_value() == bank && kvalid.has_value() == bank
              && x.has_value() == bank,
              "solver_cfg_step: u, k, bank_img and x come together");
  if (bank) {
    check_index_inputs(*u, step, *kvalid, B);
    TORCH_CHECK(u->size(0) == S, "u must have one row per table entry");
    TORCH_CHECK(bank_img->is_cuda() && bank_img->is_contiguous()
                && bank_img->scalar_type() == torch::kFloat
                && bank_img->dim() == 5 && bank_img->size(0) >= 1
                && bank_img->size(1) == B && bank_img->numel()
                   == bank_img->size(0) * n);
    TORCH_CHECK(x->is_cuda() && x->is_contiguous()
                && x->scalar_type() == torch::kFloat && x->numel() == 2 * n);
  }

  auto stream = at::hip::getCurrentHIPStream();
  const int grid = grid_for((n + 3) / 4);
  auto launch = [&](auto* tag, auto atag) {
    using TO = std::remove_pointer_t<decltype(tag)>;
    constexpr bool AL = decltype(atag)::value;
    hipLaunchKernelGGL((solver_cfg_step_kernel<TO, AL>), dim3(grid),
        dim3(256), 0, stream, z.data_ptr<float>(),
        hist.has_value() ? hist->data_ptr<float>() : nullptr,
        reinterpret_cast<const TO*>(out.data_ptr()),
        noise.has_value() ? noise->data_ptr<float>() : nullptr,
        t_ca.data_ptr<float>(), t_cb.data_ptr<float>(),
        t_cz.data_ptr<float>(), t_cx.data_ptr<float>(),
        t_ch.data_ptr<float>(), t_sigma.data_ptr<float>(),
        reinterpret_cast<const long*>(step.data_ptr()),
        reinterpret_cast<long*>(step_next.data_ptr()), n, (int)S, (float)w,
        (float)noise_scale, clip ? 1 : 0);
  };
  const bool al = n % 4 == 0;
  if (out.scalar_type() == torch::kBFloat16) {
    if (al) launch((bf16*)nullptr, std::true_type{});
    else launch((bf16*)nullptr, std::false_type{});
  } else {
    if (al) launch((float*)nullptr, std::true_type{});
    else launch((float*)nullptr, std::false_type{});
  }

  if (!bank) {
    hipLaunchKernelGGL(publish_step_kernel, dim3(1), dim3(64), 0, stream,
        reinterpret_cast<const long*>(step_next.data_ptr()),
        reinterpret_cast<long*>(step.data_ptr()));
    return;
  }
  const bool vec = m % 4 == 0 && aligned16(*bank_img) && aligned16(*x);
  auto gather = [&](auto vtag) {
    constexpr int V = decltype(vtag)::value;
    const long total = n / V;
    hipLaunchKernelGGL((next_x_gather_kernel<V>), dim3(grid_for(total)),
        dim3(256), 0, stream, bank_img->data_ptr<float>(),
        x->data_ptr<float>(), u->data_ptr<float>(),
        reinterpret_cast<const long*>(step_next.data_ptr()),
        reinterpret_cast<const long*>(kvalid->data_ptr()),
        reinterpret_cast<long*>(step.data_ptr()), total, B, m, (int)S,
        (int)bank_img->size(0));
  };
  if (vec) gather(std::integral_constant<int, 4>{});
  else gather(std::integral_constant<int, 1>{});
}
