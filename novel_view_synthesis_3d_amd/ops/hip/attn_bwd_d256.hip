// Attention backward, dkv kernel for head dim 256 — CDNA4 gfx950.
// (The math, attn_delta, the dq kernel and the d <= 128 dkv template are in
// attn_bwd.hip, which launches this kernel through attn_bwd_dkv256_launch.)
//
// One block = (b, h, 128-key tile), 8 waves x 16 keys, K/V A-fragments and
// the dk/dv accumulators in registers, as in the template. The template
// cannot be instantiated at d = 256: its four images per q-tile (Q, DO, Q^T,
// DO^T), double-buffered, would need ~280 KB of LDS. Here only Q and DO are
// staged, row-major, and the contraction-over-i B-fragments of
// dv += P^T.DO and dk += dS^T.Q come out of the same images through
// ds_read_b64_tr_b16, so a buffer set is 2*64*512 + 512 = 66 048 B and two
// sets plus the per-wave P/dS tiles are 148 480 B.
//
// Registers. K/V fragments are 64 VGPRs a wave, S^T/dP^T 32, and dk/dv for
// all 256 columns would be 128 more; with two waves per SIMD (256 registers
// each) the compiler spills that: 76 VGPRs in one pass, 41 with two passes of
// 128 columns (docs/kernels.md has the table). So dk/dv are accumulated in
// NH = 4 passes over the q-tiles, 64 columns each, while S^T and dP^T still
// contract over all 256: 231 VGPRs, no scratch, at the price of recomputing
// S^T/dP^T four times (2.5x the MFMA work of one pass).
//
// Row layout: 512 B rows, unpadded; the byte offset inside a row is XORed
// with swz256(row) = (row&7)<<5 | (row&8)<<1. LDS has 64 banks x 4 B.
//  * row reads (ds_read_b128, S^T and dP^T): the 16 lanes that share a k
//    group read the same 16 B column of rows r..r+15. Bits 0-2 of the row
//    pick one of eight 32 B granules, bit 3 the half of it: 16 distinct
//    16 B chunks = all 64 banks once.
//  * transpose reads: a 16-lane block covers 4 rows x 32 B; the 32 lanes
//    served together (blocks g, g+1) cover rows 8a..8a+7 of one 32 B column
//    (the i index of the contraction is permuted so that they do, see
//    ipos below): bit 3 is common, bits 0-2 give eight distinct granules
//    = all 64 banks once.
// A padded stride cannot do both: +16 B serves the row reads but makes
// the 4 x 32 B block of a transpose read overlap itself, +32 B serves the
// transpose reads but folds rows r and r+8 of a row read onto each other.
//
// Staging is global_load_lds (16 B per lane, no VGPR round trip). The LDS
// side of that instruction is lane-linear, so the swizzle is applied to the
// global side: lane l of a 1 KB piece fetches the chunk that belongs at its
// LDS slot. A 512 B row is still one contiguous run of global lines.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "common.h"

namespace {

constexpr int D = 256;
constexpr int KVB = 128;               // keys per block
constexpr int QTB = 64;                // q rows per tile
constexpr int NW = 8;                  // waves, 16 keys each
constexpr int NH = 4;                  // passes over the q-tiles
constexpr int DC = D / 32;             // MFMA k-chunks of S^T / dP^T
constexpr int DFH = D / 16 / NH;       // accumulator fragments per pass
constexpr int ROWB = D * 2;            // bytes per staged row
constexpr int TILE = QTB * ROWB;       // one [64][256] bf16 image
constexpr int QSET = 2 * TILE + 2 * QTB * 4;   // Q | DO | lse | delta
constexpr size_t LDS_BYTES = 2 * (size_t)QSET + NW * 16 * QTB * 2;

struct Dkv256Shape {
  int L, Lk, H;
  float scale;
  long sqb, sqt;   // q strides (elements); head stride = D, d contiguous
  long skb, skt;   // k
  long svb, svt;   // v
  int kv_swap;     // the queries of batch b^1 attend the keys of batch b
};

__device__ __forceinline__ int swz256(int row) {
  return ((row & 7) << 5) | ((row & 8) << 1);
}

__global__ __launch_bounds__(NW * 64)
void attn_bwd_dkv256_kernel(const bf16* __restrict__ q,
                            const bf16* __restrict__ k,
                            const bf16* __restrict__ v,
                            const bf16* __restrict__ dout,  // (B,L,H,D)
                            const float* __restrict__ lse,  // (B,L,H)
                            const float* __restrict__ delta,
                            bf16* __restrict__ dk,          // (B,Lk,H,D)
                            bf16* __restrict__ dv,
                            Dkv256Shape s) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* ldsP = smem + 2 * QSET;                 // 8 waves x 16 x 64 bf16

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int g = lane >> 4;      // k group of the MFMA operand layouts
  const int m16 = lane & 15;

  int bid = blockIdx.x;
  const int kvtiles = s.Lk / KVB;
  const int kvt = bid % kvtiles; bid /= kvtiles;
  const int head = bid % s.H;
  const int b = bid / s.H;

  // keys of batch b are attended by batch b^1's queries under kv_swap
  const int bq = s.kv_swap ? (b ^ 1) : b;
  const bf16* qbase = q + (long)bq * s.sqb + head * D;
  const bf16* kbase = k + (long)b * s.skb + head * D;
  const bf16* vbase = v + (long)b * s.svb + head * D;
  const int HD = s.H * D;
  const bf16* dobase = dout + (long)bq * s.L * HD + head * D;
  // threads 0..63 carry lse, 64..127 delta of the q row tid&63
  const float* ldbase = (tid < QTB ? lse : delta)
                        + ((long)bq * s.L + (tid & (QTB - 1))) * s.H + head;

  // ---- this wave's K (prescaled, 1/16 is exact) and V rows as A-fragments
  const int k0 = kvt * KVB + wave * 16;
  bf16x8 ka[DC], va[DC];
#pragma unroll
  for (int dc = 0; dc < DC; ++dc) {
    const int off = dc * 32 + g * 8;
    Pack<bf16, 8> pk = pload<bf16, 8>(kbase + (long)(k0 + m16) * s.skt + off);
    Pack<bf16, 8> pv = pload<bf16, 8>(vbase + (long)(k0 + m16) * s.svt + off);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      ka[dc][j] = (__bf16)__float2bfloat16(to_f32(pk.v[j]) * s.scale);
      va[dc][j] = (__bf16)pv.v[j];
    }
  }

  char* pw = ldsP + wave * (16 * QTB * 2);   // [16 keys][64 ipos]

  // Q and DO rows of q-tile t -> buffer set `buf`
  auto stage_qtile = [&](int t, int buf) {
    char* dst = smem + buf * QSET;
#pragma unroll 1
    for (int it = 0; it < TILE / (NW * 1024); ++it) {
      const int o = (it * NW + wave) * 1024 + lane * 16;   // LDS slot
      const int row = o / ROWB;
      const int col = ((o % ROWB) ^ swz256(row)) >> 1;     // element there
      const long grow = (long)t * QTB + row;
      __builtin_amdgcn_global_load_lds(
          as_global(qbase + grow * s.sqt + col),
          as_shared(dst + (o - lane * 16)), 16, 0, 0);
      __builtin_amdgcn_global_load_lds(
          as_global(dobase + grow * HD + col),
          as_shared(dst + TILE + (o - lane * 16)), 16, 0, 0);
    }
  };
  auto ld_slot = [&](int buf) {
    return reinterpret_cast<float*>(smem + buf * QSET + 2 * TILE) + tid;
  };

  // per-lane offsets inside an image. Row reads: row c*16 + m16, bytes
  // dc*64 + g*16. Transpose reads: lane (g, m16) addresses 4 elements of
  // row g*4 + (m16>>2) (+ kc*32, + 16 for the second read) at column
  // f*16 + 4*(m16&3) and receives column f*16 + m16 of the block's 4 rows.
  const int rd_row = m16 * ROWB;
  const int rd_x = (g * 16) ^ swz256(m16);
  const int tr_r = g * 4 + (m16 >> 2);
  const int tr_row = tr_r * ROWB;
  const int tr_x = (8 * (m16 & 3)) ^ swz256(tr_r);
  // contraction index i = c*16 + m16 of a 64-row tile sits at position
  // ipos in the P/dS tile, so that one 16 B A-fragment read at
  // kc*32 + g*8 holds rows {g*4..+3, 16 + g*4..+3} of chunk kc — the rows
  // the two transpose reads of lane group g deliver
  auto ipos = [&](int c) {
    return (c >> 1) * 32 + (m16 >> 2) * 8 + (c & 1) * 4 + (m16 & 3);
  };

  // acc[f] += tile(P^T or dS^T) . img, the contraction over the 64 rows of
  // the row-major image `img` through transpose reads; tr_xh = tr_x with
  // the pass's column offset folded in. Step j = (kc, two f). Its reads are
  // issued one step ahead by hand, and the scheduling barriers keep the
  // compiler from hoisting more of them than there are registers for.
  auto accumulate = [&](const char* img, int tr_xh, f32x4 (&acc)[DFH]) {
    bf16x8 a[QTB / 32];
#pragma unroll
    for (int kc = 0; kc < QTB / 32; ++kc)
      a[kc] = *reinterpret_cast<const bf16x8*>(
          pw + swz_row(m16, (kc * 32 + g * 8) * 2, QTB * 2));
    bf16x8 bt[2][2];
    auto rd_tr = [&](int j) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const char* p0 = img + (j / (DFH / 2)) * 32 * ROWB + tr_row
                         + ((((j % (DFH / 2)) * 2 + u) * 32) ^ tr_xh);
        bt[j & 1][u] = tr16x8(p0, p0 + 16 * ROWB);
      }
    };
    rd_tr(0);
#pragma unroll
    for (int j = 0; j < QTB / 32 * DFH / 2; ++j) {
      if (j + 1 < QTB / 32 * DFH / 2) rd_tr(j + 1);
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int f = (j % (DFH / 2)) * 2 + u;
        acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            a[j / (DFH / 2)], bt[j & 1][u], acc[f], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  const int qtiles = s.L / QTB;
  // output staging: 8 KB a wave, 64 KB in all = exactly the Q | DO images
  // of buffer set 0
  char* ow = smem + wave * (16 * ROWB);
  // pass h accumulates columns h*64 .. h*64+63 of dk/dv
#pragma unroll 1
  for (int h = 0; h < NH; ++h) {
    const int hb = h * (D / NH) * 2;   // byte offset of the pass's columns
    const int tr_xh = hb ^ tr_x;
    f32x4 dvacc[DFH], dkacc[DFH];
#pragma unroll
    for (int f = 0; f < DFH; ++f) {
      dvacc[f] = f32x4{0.f, 0.f, 0.f, 0.f};
      dkacc[f] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    stage_qtile(0, 0);
    if (tid < 2 * QTB) *ld_slot(0) = ldbase[0];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int t = 0; t < qtiles; ++t) {
      const int buf = t & 1;
      const bool more = t + 1 < qtiles;
      float ld_next = 0.f;
      if (more) {
        if (tid < 2 * QTB) ld_next = ldbase[(long)(t + 1) * QTB * s.H];
        stage_qtile(t + 1, buf ^ 1);
      }
      const char* ldsQ = smem + buf * QSET;
      const char* ldsDO = ldsQ + TILE;
      const float* ldsLse = reinterpret_cast<const float*>(ldsDO + TILE);
      const float* ldsDel = ldsLse + QTB;

      // ---- S^T = K.Q^T and dP^T = V.DO^T (rows = keys, cols = q rows);
      // step i = (c, dc), reads one step ahead as in accumulate ----
      f32x4 st[4], dpt[4];
      bf16x8 qf[2], df[2];
      auto rd_rows = [&](int i) {
        const int off = (i >> 3) * 16 * ROWB + rd_row
                        + (((i & 7) * 64) ^ rd_x);
        qf[i & 1] = *reinterpret_cast<const bf16x8*>(ldsQ + off);
        df[i & 1] = *reinterpret_cast<const bf16x8*>(ldsDO + off);
      };
      rd_rows(0);
#pragma unroll
      for (int i = 0; i < 4 * DC; ++i) {
        const int c = i >> 3, dc = i & 7;
        if (i + 1 < 4 * DC) rd_rows(i + 1);
        if (dc == 0) {
          st[c] = f32x4{0.f, 0.f, 0.f, 0.f};
          dpt[c] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        st[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            ka[dc], qf[i & 1], st[c], 0, 0, 0);
        dpt[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            va[dc], df[i & 1], dpt[c], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }

      // ---- P^T = exp(S^T - lse_i) -> per-wave tile [16 keys][64 ipos] ----
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float l_i = ldsLse[c * 16 + m16];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = __expf(st[c][r] - l_i);
          st[c][r] = p;  // kept in fp32 for dS^T
          *reinterpret_cast<bf16*>(
              pw + swz_row(g * 4 + r, ipos(c) * 2, QTB * 2)) =
              __float2bfloat16(p);
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);

      // ---- dv += P^T . DO ----
      accumulate(ldsDO, tr_xh, dvacc);

      // ---- dS^T = P^T * (dP^T - delta_i) * scale -> same wave tile ----
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float d_i = ldsDel[c * 16 + m16];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float ds = st[c][r] * (dpt[c][r] - d_i) * s.scale;
          *reinterpret_cast<bf16*>(
              pw + swz_row(g * 4 + r, ipos(c) * 2, QTB * 2)) =
              __float2bfloat16(ds);
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);

      // ---- dk += dS^T . Q ----
      accumulate(ldsQ, tr_xh, dkacc);
      // the next tile's rows have landed in buf^1 and every wave is done
      // with buf before tile t+2 overwrites it
      if (more && tid < 2 * QTB) *ld_slot(buf ^ 1) = ld_next;
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }

    // ---- dv, then dk: C layout (row = key, col = d) -> this wave's 8 KB
    // of `ow` (same row swizzle) -> coalesced 16 B stores. The barrier
    // that ended the tile loop makes the images free to overwrite. ----
    auto write_out = [&](const f32x4 (&acc)[DFH], bf16* out) {
#pragma unroll
      for (int f = 0; f < DFH; ++f) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = g * 4 + r;
          *reinterpret_cast<bf16*>(
              ow + row * ROWB + (((f * 16 + m16) * 2) ^ swz256(row))) =
              __float2bfloat16(acc[f][r]);
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int it = 0; it < 16 * (D / NH) / 8 / 64; ++it) {
        const int p = lane + it * 64;
        const int row = p / (D / NH / 8);
        const int d0 = (p % (D / NH / 8)) * 8;
        Pack<bf16, 8> pv = *reinterpret_cast<Pack<bf16, 8>*>(
            ow + row * ROWB + ((d0 * 2) ^ swz256(row)));
        pstore<bf16, 8>(out + ((long)b * s.Lk + k0 + row) * HD + head * D
                        + (hb >> 1) + d0, pv);
      }
    };
    write_out(dvacc, dv);
    write_out(dkacc, dk);
    // the next pass stages tile 0 over the 64 KB the waves just read
    __syncthreads();
  }
}

}  // namespace

// q, k, v: (B,L,H,256) bf16 with a contiguous (head, d) tail; dout, dk, dv
// contiguous; L and Lk multiples of 128 (checked by attn_bwd_fused)
void attn_bwd_dkv256_launch(const torch::Tensor& q, const torch::Tensor& k,
                            const torch::Tensor& v, const torch::Tensor& dout,
                            const torch::Tensor& lse,
                            const torch::Tensor& delta, torch::Tensor& dk,
                            torch::Tensor& dv, bool kv_swap,
                            hipStream_t stream) {
  TORCH_CHECK(q.size(3) == D && q.size(1) % KVB == 0 && k.size(1) % KVB == 0);
  Dkv256Shape s;
  s.L = q.size(1); s.Lk = k.size(1); s.H = q.size(2);
  s.scale = 1.0f / 16.0f;
  s.sqb = q.stride(0); s.sqt = q.stride(1);
  s.skb = k.stride(0); s.skt = k.stride(1);
  s.svb = v.stride(0); s.svt = v.stride(1);
  s.kv_swap = kv_swap ? 1 : 0;
  const int B = q.size(0);
  hipLaunchKernelGGL(attn_bwd_dkv256_kernel,
      dim3(B * s.H * (s.Lk / KVB)), dim3(NW * 64), LDS_BYTES, stream,
      reinterpret_cast<const bf16*>(q.data_ptr()),
      reinterpret_cast<const bf16*>(k.data_ptr()),
      reinterpret_cast<const bf16*>(v.data_ptr()),
      reinterpret_cast<const bf16*>(dout.data_ptr()),
      lse.data_ptr<float>(), delta.data_ptr<float>(),
      reinterpret_cast<bf16*>(dk.data_ptr()),
      reinterpret_cast<bf16*>(dv.data_ptr()), s);
}
