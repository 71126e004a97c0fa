// Cross-attention probabilities as an output (spmm_attn_probs, include/spmm_hip.h): P = softmax(Q K^T / 8 + cross mask) per head, and
// the mean over the heads, in fp32.  Replaces BertSelfAttention.forward xbert.py:305-340 up to `attention_probs` (scores :305, /sqrt(d)
// :323, additive encoder mask :327 from invert_attention_mask :1038-1043, softmax :335), without the dropout of :344 -- the part of the
// layer that csrc/attention.hip and csrc/xattn.hip keep only as bf16-rounded, un-normalised MFMA operands in registers.
//
// Shape of the work: at most rows x Lkv x 4 bytes out for rows x nH x 128 bytes in -- output-bound.  One wave64 workgroup per (sequence,
// 32-query tile); the head loop is inside, so the head mean is summed in ascending head order in the registers of the one wave that owns
// the rows: no atomics, no second launch.  Scores are computed transposed (S^T = K Q^T, v_mfma_f32_32x32x16_bf16, K rows as the A
// operand straight from HBM / L2, as attention.hip does from LDS): a lane owns one query row and 16 keys of each 32-key tile, so the row
// maximum and row sum need one exchange with lane ^ 32.  Two passes over the key tiles per head (running maximum and sum, then the
// probabilities): the scores are recomputed, not kept -- 8 MFMAs per tile against 128 more registers, and the MFMAs are idle anyway.
// Everything after the MFMA is fp32; nothing is rounded to bf16.  A tile leaves through 4.5 KiB of LDS so that every store instruction
// writes two 128-byte row pieces (plain 4-byte vector stores: the outputs are only 4-byte aligned and ldp is free).
//
// Determinism: a key past the source's length or masked by kmask has bias -inf, so it contributes exp2(-inf) = +0 to the sum, leaves the
// maximum alone and comes out as exactly 0; a whole tile past the length is skipped, which is the same arithmetic.  The tile order, the
// register order inside a tile and the lane ^ 32 exchange depend on nothing but the sequence itself: its rows have the same bits wherever
// it sits in the launch, whatever Lkv >= its source length the launch has, and however its source is reached.
#include "common.h"
#include "attn_tiles.h"
#include "../../include/spmm_hip.h"

namespace {

struct MapP {
  const bf16* Q; long ldq;
  const bf16* K; long ldk;
  const int* kmask; const int* kv_seq; const int* q_row0; const int* q_len; const int* kv_row0; const int* kv_len;
  float* Pm; float* Ph; long ldp, head_stride;
  int nseq, nH, Lq, Lkv;
};

constexpr int TP = 36;      // floats per row of the transposition tile: 16-byte aligned rows, the 32 lanes of a column write spread over the banks

// scores of key tile t in units of log2 e, bias added: register 4*gq + j of lane (q = lane & 31, g = lane >> 5) holds key t*32 + 8*gq + 4*g + j
__device__ __forceinline__ f32x16 score_tile(const bf16* Kh, long ldk, int Lsrc, int t, const bf16x8 (&qf)[4], const float* mb, int lane) {
  const int g = lane >> 5;
  int krow = t * 32 + (lane & 31);
  krow = krow < Lsrc ? krow : Lsrc - 1;             // rows past the source re-read its last row (finite; their bias is -inf).  Lsrc >= 1 here.
  const bf16* kp = Kh + (long)krow * ldk + g * 8;
  f32x16 acc = zero16();
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) acc = MFMA32(*(const bf16x8*)(kp + kk * 16), qf[kk], acc);
#pragma unroll
  for (int gq = 0; gq < 4; ++gq) {
    const f32x4 b = *(const f32x4*)(mb + t * 32 + 8 * gq + 4 * g);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[gq * 4 + j] = __builtin_fmaf(acc[gq * 4 + j], 0.125f * LOG2E, b[j]);
  }
  return acc;
}

// [32 keys of tile t] x [32 queries] in registers -> rows of `out` (the sequence's first row), through the wave's LDS tile
__device__ __forceinline__ void store_tile(float* T, const f32x16& v, float* out, long ldp, int q0, int Lq, int kv0, int Lkv, int lane) {
  const int q = lane & 31, g = lane >> 5;
  __syncthreads();                                  // (one wave: the reads of the previous tile are done)
#pragma unroll
  for (int gq = 0; gq < 4; ++gq) {
    f32x4 w;
    w[0] = v[gq * 4 + 0]; w[1] = v[gq * 4 + 1]; w[2] = v[gq * 4 + 2]; w[3] = v[gq * 4 + 3];
    *(f32x4*)(T + q * TP + 8 * gq + 4 * g) = w;
  }
  __syncthreads();
  const int c = kv0 + q;                            // this lane's column: 32 lanes write 128 consecutive bytes of a row
  if (c < Lkv) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int r = 2 * i + g;
      if (q0 + r < Lq) out[(long)(q0 + r) * ldp + c] = T[r * TP + q];
    }
  }
}

template <int NT>   // NT = ceil(launch Lkv / 32)
__global__ __launch_bounds__(64) void attn_probs_kernel(MapP p) {
  __shared__ __attribute__((aligned(16))) float mb[NT * 32];
  __shared__ __attribute__((aligned(16))) float T[32 * TP];
  const int lane = threadIdx.x, g = lane >> 5;
  const int seq = blockIdx.y, q0 = blockIdx.x * 32;
  const long kvs = p.kv_seq ? (long)p.kv_seq[seq] : (long)seq;
  const int Lq = min(p.q_len ? p.q_len[seq] : p.Lq, p.Lq);
  const int Lsrc = min(p.kv_len ? p.kv_len[kvs] : p.Lkv, p.Lkv);
  if (q0 >= Lq) return;                             // workgroup-uniform, before any barrier
  const long qrow = p.q_row0 ? (long)p.q_row0[seq] : (long)seq * p.Lq;
  const long kvrow = p.kv_row0 ? (long)p.kv_row0[kvs] : kvs * p.Lkv;
  for (int j = lane; j < NT * 32; j += 64)
    mb[j] = (j < Lsrc && (p.kmask == nullptr || p.kmask[(long)seq * p.Lkv + j])) ? 0.f : -INFINITY;
  __syncthreads();
  const int qc = min(q0 + (lane & 31), Lq - 1);     // rows past the sequence re-read its last row and are never stored
  const bf16* Qg = p.Q + (qrow + qc) * p.ldq + g * 8;
  const bf16* Kg = p.K + kvrow * p.ldk;
  float* Pm = p.Pm ? p.Pm + qrow * p.ldp : nullptr;
  f32x16 mean[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) mean[t] = zero16();

  for (int h = 0; h < p.nH; ++h) {
    bf16x8 qf[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) qf[kk] = *(const bf16x8*)(Qg + h * HD + kk * 16);
    const bf16* Kh = Kg + h * HD;
    float m = -INFINITY, l = 0.f;                   // running maximum (both halves of the wave agree on it) and this half's sum
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      if (t * 32 < Lsrc) {                          // wave-uniform
        const f32x16 s = score_tile(Kh, p.ldk, Lsrc, t, qf, mb, lane);
        float tm = s[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) tm = fmaxf(tm, s[r]);
        tm = fmaxf(tm, __shfl_xor(tm, 32, 64));
        const float mn = fmaxf(m, tm), ms = mn == -INFINITY ? 0.f : mn;
        float a = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) a += __builtin_amdgcn_exp2f(s[r] - ms);
        l = l * __builtin_amdgcn_exp2f(m - ms) + a;
        m = mn;
      }
    }
    l += __shfl_xor(l, 32, 64);
    const float ms = m == -INFINITY ? 0.f : m;
    const float inv = l > 0.f ? 1.f / l : 0.f;      // every key masked: the row is zeros
    float* Ph = p.Ph ? p.Ph + (long)h * p.head_stride + qrow * p.ldp : nullptr;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      f32x16 pr = zero16();
      if (t * 32 < Lsrc) {
        const f32x16 s = score_tile(Kh, p.ldk, Lsrc, t, qf, mb, lane);
#pragma unroll
        for (int r = 0; r < 16; ++r) pr[r] = __builtin_amdgcn_exp2f(s[r] - ms) * inv;
      }
      if (Pm) {
#pragma unroll
        for (int r = 0; r < 16; ++r) mean[t][r] += pr[r];
      }
      if (Ph) store_tile(T, pr, Ph, p.ldp, q0, Lq, t * 32, p.Lkv, lane);
    }
  }
  if (Pm) {
    const float invH = 1.f / (float)p.nH;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      f32x16 v;
#pragma unroll
      for (int r = 0; r < 16; ++r) v[r] = mean[t][r] * invH;
      store_tile(T, v, Pm, p.ldp, q0, Lq, t * 32, p.Lkv, lane);
    }
  }
}

}  // namespace

extern "C" int spmm_attn_probs(const void* Q, long ldq, const void* K, long ldk, const int* kmask, const int* kv_seq, const int* q_row0,
                               const int* q_len, const int* kv_row0, const int* kv_len, float* P_mean, float* P_heads, long ldp,
                               long head_stride, int nseq, int nH, int Lq, int Lkv, hipStream_t stream) {
  SPMM_CHECK_SHAPE(Q != nullptr && K != nullptr, "spmm_attn_probs: Q and K are required");
  SPMM_CHECK_SHAPE(P_mean != nullptr || P_heads != nullptr, "spmm_attn_probs: P_mean or P_heads is required");
  SPMM_CHECK_SHAPE((((uintptr_t)Q | (uintptr_t)K) & 15) == 0, "spmm_attn_probs: misaligned Q / K (16 bytes)");
  SPMM_CHECK_SHAPE((((uintptr_t)P_mean | (uintptr_t)P_heads | (uintptr_t)kmask | (uintptr_t)kv_seq | (uintptr_t)q_row0 | (uintptr_t)q_len |
                     (uintptr_t)kv_row0 | (uintptr_t)kv_len) & 3) == 0,
                   "spmm_attn_probs: misaligned P_mean / P_heads / kmask / kv_seq / q_row0 / q_len / kv_row0 / kv_len (4 bytes)");
  SPMM_CHECK_SHAPE(nH >= 1 && nH <= 16, "spmm_attn_probs: nH=%d (1 <= nH <= 16)", nH);
  SPMM_CHECK_SHAPE(ldq >= (long)nH * 64 && ldk >= (long)nH * 64, "spmm_attn_probs: ldq=%ld ldk=%ld must be >= nH*64=%d", ldq, ldk, nH * 64);
  SPMM_CHECK_SHAPE(ldq % 8 == 0 && ldk % 8 == 0, "spmm_attn_probs: ldq=%ld ldk=%ld must be multiples of 8 (16-byte rows)", ldq, ldk);
  SPMM_CHECK_SHAPE(Lq >= 1 && Lq <= 256 && Lkv >= 1 && Lkv <= 256, "spmm_attn_probs: Lq=%d Lkv=%d (1 <= Lq, Lkv <= 256)", Lq, Lkv);
  SPMM_CHECK_SHAPE(ldp >= (long)Lkv, "spmm_attn_probs: ldp=%ld must be >= Lkv=%d", ldp, Lkv);
  SPMM_CHECK_SHAPE(nseq >= 0, "spmm_attn_probs: nseq=%d (nseq >= 0)", nseq);
  SPMM_CHECK_SHAPE((q_row0 == nullptr) == (q_len == nullptr) && (kv_row0 == nullptr) == (kv_len == nullptr),
                   "spmm_attn_probs: q_row0/q_len and kv_row0/kv_len must be given in pairs");
  SPMM_CHECK_SHAPE(P_heads == nullptr || nH == 1 || head_stride >= ldp,
                   "spmm_attn_probs: head_stride=%ld must be positive and >= ldp=%ld", head_stride, ldp);
  if (nseq == 0) return SPMM_OK;
  MapP p = {(const bf16*)Q, ldq, (const bf16*)K, ldk, kmask, kv_seq, q_row0, q_len, kv_row0, kv_len, P_mean, P_heads, ldp, head_stride,
            nseq, nH, Lq, Lkv};
  const dim3 grid((unsigned)((Lq + 31) / 32), (unsigned)nseq), block(64);
  switch ((Lkv + 31) / 32) {
    case 1: hipLaunchKernelGGL(attn_probs_kernel<1>, grid, block, 0, stream, p); break;
    case 2: hipLaunchKernelGGL(attn_probs_kernel<2>, grid, block, 0, stream, p); break;
    case 3: hipLaunchKernelGGL(attn_probs_kernel<3>, grid, block, 0, stream, p); break;
    case 4: hipLaunchKernelGGL(attn_probs_kernel<4>, grid, block, 0, stream, p); break;
    case 5: hipLaunchKernelGGL(attn_probs_kernel<5>, grid, block, 0, stream, p); break;
    case 6: hipLaunchKernelGGL(attn_probs_kernel<6>, grid, block, 0, stream, p); break;
    case 7: hipLaunchKernelGGL(attn_probs_kernel<7>, grid, block, 0, stream, p); break;
    default: hipLaunchKernelGGL(attn_probs_kernel<8>, grid, block, 0, stream, p); break;
  }
  SPMM_LAUNCH_CHECK("spmm_attn_probs");
  return SPMM_OK;
}
