// Common helpers for the nvs3d CDNA4 (gfx950) kernels.
// Wavefront = 64 lanes; block sizes are multiples of 64.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#define NVS_WAVE 64

using bf16 = __hip_bfloat16;
// MFMA operand / accumulator fragments
using bf16x4 = __attribute__((ext_vector_type(4))) __bf16;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using f32x16 = __attribute__((ext_vector_type(16))) float;

// ---------------------------------------------------------------------------
// Packed vector load/store: Pack<T,V> is an aligned V-element chunk. hipcc
// emits global_load_dwordx4 / dwordx2 for the 16B/8B cases.
// ---------------------------------------------------------------------------
template <typename T, int V>
struct alignas(sizeof(T) * V) Pack {
  T v[V];
};

template <typename T, int V>
__device__ __forceinline__ Pack<T, V> pload(const T* p) {
  return *reinterpret_cast<const Pack<T, V>*>(p);
}

template <typename T, int V>
__device__ __forceinline__ void pstore(T* p, const Pack<T, V>& x) {
  *reinterpret_cast<Pack<T, V>*>(p) = x;
}

__device__ __forceinline__ float to_f32(float x) { return x; }
__device__ __forceinline__ float to_f32(__hip_bfloat16 x) {
  return __bfloat162float(x);
}
__device__ __forceinline__ void from_f32(float x, float& o) { o = x; }
__device__ __forceinline__ void from_f32(float x, __hip_bfloat16& o) {
  o = __float2bfloat16(x);
}

// ---------------------------------------------------------------------------
// LDS helpers for the MFMA kernels
// ---------------------------------------------------------------------------
// address-space casts for global_load_lds (via integer, the sanctioned way)
using as1_cvp = const __attribute__((address_space(1))) void*;
using as3_vp = __attribute__((address_space(3))) void*;
__device__ __forceinline__ as1_cvp as_global(const void* p) {
  return (as1_cvp)(unsigned long long)(uintptr_t)p;
}
__device__ __forceinline__ as3_vp as_shared(void* p) {
  return (as3_vp)(unsigned int)(uintptr_t)p;
}

// 8-element MFMA fragment from two ds_read_b64_tr_b16 hardware transpose
// reads (p1 is p0 four tile rows further on)
using as3_bf16x4p = __attribute__((address_space(3))) bf16x4*;
__device__ __forceinline__ bf16x8 tr16x8(const char* p0, const char* p1) {
  bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
      (as3_bf16x4p)(const_cast<char*>(p0)));
  bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
      (as3_bf16x4p)(const_cast<char*>(p1)));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// byte offset of (row, byte_in_row) in a row-major LDS tile whose 16 B
// chunks are XOR-swizzled by row to spread ds_read_b128 over the banks
__device__ __forceinline__ int swz_row(int row, int byte_in_row,
                                       int row_bytes) {
  return (row * row_bytes + byte_in_row) ^ ((row & 7) << 4);
}

// ---------------------------------------------------------------------------
// Wave + block reductions
// ---------------------------------------------------------------------------
__device__ __forceinline__ float wave_reduce_sum(float x) {
#pragma unroll
  for (int off = NVS_WAVE / 2; off > 0; off >>= 1) {
    x += __shfl_down(x, off, NVS_WAVE);
  }
  return x;
}

__device__ __forceinline__ float sigmoidf_fast(float x) {
  return 1.0f / (1.0f + __expf(-x));
}

static inline int ceil_div_host(long a, long b) {
  return static_cast<int>((a + b - 1) / b);
}

#define NVS_CHECK_HIP(expr)                                        \
  do {                                                             \
    hipError_t _e = (expr);                                        \
    TORCH_CHECK(_e == hipSuccess, "HIP error: ",                   \
                hipGetErrorString(_e));                            \
  } while (0)
