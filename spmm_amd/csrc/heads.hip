// Task head of the fine-tuning models for gfx950: the second Linear of reg_head plus its loss, forward and backward.
//
//   logits = A W2^T + b2        A = GELU(cls W1^T + b1) [B, W] bf16 (gemm_nt, EPI_GELU), W2 [C, W] / b2 [C] fp32 arena masters
//   kind 0  MSE   (d_regression.py:41-49)              C = 1, target float [B], mean over B
//   kind 1  CE    (d_classification.py:42-50)           target int32 class index [B], mean over B
//   kind 2  BCE   (d_classification_multilabel.py:42-47) target float [B, C], mean over B*C, in the logits form
//                 softplus(x) - x*y (BCELoss(sigmoid(x)) clamps log at -100: it differs once |x| > ~15)
//   backward: dA = dlogits W2 (bf16), dW2 += dlogits^T A, db2 += sum_b dlogits, dlogits = gscale * dloss/dlogits
//
// Two launches, no floating-point atomics: task_head_rows (one workgroup per row: logits, dA) and task_head_cols (one workgroup per
// 64 columns of W2: dW2 over every row in a fixed order; workgroup 0 also forms db2 and the mean loss, again in a fixed order).
// So two launches on the same inputs agree bit for bit.  The shapes are tiny (B <= 1024, C <= 64, W <= 4096): launch count, not
// bandwidth or FLOPs, is what this costs.
//
// Also here: spmm_s2p_append, the launch that closes one step of the SMILES -> PV regression loop (d_smiles2pv.py:14-52) and opens the
// next: the last Linear(H, 1) of property_mtr_head on the last-position rows, then property_embed + BertEmbeddings (inputs_embeds
// branch) of the predicted value, written as the next row of the append-only cache of embedded prefix rows.
#include "common.h"
#include "../../include/spmm_hip.h"

namespace {

constexpr int TH_THREADS = 256;
constexpr int TH_MAXW = 4096;                 // W <= 4096: each thread of a row owns at most 16 columns
constexpr int TH_PER = TH_MAXW / TH_THREADS;
constexpr int TH_MAXC = 64;
constexpr int TH_CPER = TH_MAXC / 4;          // dW2 rows per thread in task_head_cols (four waves split the C rows)
constexpr int TH_CHUNK = 64;                  // rows of dlogits staged in LDS at a time by task_head_cols

// Loss of row b from its logits x[0..C) and d(loss_b)/d(x) * scale into dl[0..C) (dl may be null).  One thread.
__device__ float row_loss(int kind, const float* x, int C, const void* target, int b, float scale, float* dl) {
  if (kind == 0) {
    const float d = x[0] - ((const float*)target)[b];
    if (dl) dl[0] = scale * 2.f * d;
    return d * d;
  }
  if (kind == 1) {
    const int t = ((const int*)target)[b];
    float m = x[0];
    for (int c = 1; c < C; ++c) m = fmaxf(m, x[c]);
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += expf(x[c] - m);
    const float lse = m + logf(s);
    const bool ok = t >= 0 && t < C;          // (F.cross_entropy raises on such a label: here the loss turns NaN, the gradient stays 0)
    if (dl)
      for (int c = 0; c < C; ++c) dl[c] = ok ? scale * (expf(x[c] - lse) - (c == t ? 1.f : 0.f)) : 0.f;
    return ok ? lse - x[t] : __int_as_float(0x7fc00000);
  }
  const float* y = (const float*)target + (long)b * C;
  float l = 0.f;
  for (int c = 0; c < C; ++c) {
    const float v = x[c];
    l += fmaxf(v, 0.f) - v * y[c] + log1pf(expf(-fabsf(v)));
    if (dl) dl[c] = scale * (1.f / (1.f + expf(-v)) - y[c]);
  }
  return l;
}

__device__ __forceinline__ float loss_denom(int kind, int B, int C) { return kind == 2 ? (float)B * (float)C : (float)B; }

// One workgroup per row b: logits[b, :] (C dot products over W, reduced wave by wave in a fixed order) and, with do_bwd, dA[b, :].
__global__ __launch_bounds__(TH_THREADS) void task_head_rows_kernel(const bf16* __restrict__ A, long lda, int B, int W, const float* __restrict__ W2,
                                                                    const float* __restrict__ b2, int C, int kind, const void* __restrict__ target,
                                                                    const float* __restrict__ gscale, float* __restrict__ logits,
                                                                    bf16* __restrict__ dA, long ldda, int do_bwd) {
  __shared__ float part[4][TH_MAXC];
  __shared__ float x[TH_MAXC];
  __shared__ float dl[TH_MAXC];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float a[TH_PER];
#pragma unroll
  for (int j = 0; j < TH_PER; ++j) {
    const int k = tid + j * TH_THREADS;
    a[j] = k < W ? (float)A[(long)b * lda + k] : 0.f;
  }
  for (int c = 0; c < C; ++c) {
    const float* w = W2 + (long)c * W;
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < TH_PER; ++j) {
      const int k = tid + j * TH_THREADS;
      if (k < W) s += a[j] * w[k];
    }
    s = wave_sum(s);
    if (lane == 0) part[wave][c] = s;
  }
  __syncthreads();
  if (tid < C) {
    const float v = ((part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid])) + b2[tid];
    x[tid] = v;
    logits[(long)b * C + tid] = v;
  }
  if (!do_bwd) return;
  __syncthreads();
  if (tid == 0) row_loss(kind, x, C, target, b, (gscale ? *gscale : 1.f) / loss_denom(kind, B, C), dl);
  __syncthreads();
#pragma unroll
  for (int j = 0; j < TH_PER; ++j) {
    const int k = tid + j * TH_THREADS;
    if (k < W) {
      float s = 0.f;
      for (int c = 0; c < C; ++c) s += dl[c] * W2[(long)c * W + k];
      dA[(long)b * ldda + k] = (bf16)s;
    }
  }
}

// One workgroup per 64 columns of W2: dW2[c, w] += sum_b dl[b, c] A[b, w] with the rows in order (thread: one column, every 4th C row).
// Workgroup 0 also writes the mean loss and db2[c] += sum_b dl[b, c], both summed in row order.  do_bwd = 0: workgroup 0 forms the loss only.
__global__ __launch_bounds__(TH_THREADS) void task_head_cols_kernel(const bf16* __restrict__ A, long lda, int B, int W, int C, int kind,
                                                                    const void* __restrict__ target, const float* __restrict__ gscale,
                                                                    const float* __restrict__ logits, float* __restrict__ loss,
                                                                    float* __restrict__ dW2, float* __restrict__ db2, int do_bwd) {
  __shared__ float dls[TH_CHUNK][TH_MAXC];
  __shared__ float lrow[TH_CHUNK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = blockIdx.x * 64 + lane;
  const bool lead = blockIdx.x == 0;
  const float scale = (gscale ? *gscale : 1.f) / loss_denom(kind, B, C);
  float acc[TH_CPER];
#pragma unroll
  for (int j = 0; j < TH_CPER; ++j) acc[j] = 0.f;
  float lsum = 0.f, dbsum = 0.f;
  for (int r0 = 0; r0 < B; r0 += TH_CHUNK) {
    const int n = B - r0 < TH_CHUNK ? B - r0 : TH_CHUNK;
    __syncthreads();
    if (tid < n) {
      const float l = row_loss(kind, logits + (long)(r0 + tid) * C, C, target, r0 + tid, scale, dls[tid]);
      lrow[tid] = l;
    }
    __syncthreads();
    if (lead) {
      if (tid == 0)
        for (int r = 0; r < n; ++r) lsum += lrow[r];
      if (do_bwd && tid >= 64 && tid - 64 < C)
        for (int r = 0; r < n; ++r) dbsum += dls[r][tid - 64];
    }
    if (!do_bwd) continue;
    for (int r = 0; r < n; ++r) {
      const float av = (float)A[(long)(r0 + r) * lda + col];
#pragma unroll
      for (int j = 0; j < TH_CPER; ++j) {
        const int c = wave + 4 * j;
        if (c < C) acc[j] += dls[r][c] * av;
      }
    }
  }
  if (lead && tid == 0 && loss) loss[0] = lsum / loss_denom(kind, B, C);
  if (!do_bwd) return;
  if (lead && tid >= 64 && tid - 64 < C) db2[tid - 64] += dbsum;
#pragma unroll
  for (int j = 0; j < TH_CPER; ++j) {
    const int c = wave + 4 * j;
    if (c < C) dW2[(long)c * W + col] += acc[j];
  }
}

}  // namespace

extern "C" int spmm_task_head(const void* A, long lda, int B, int W, const float* W2, const float* b2, int C, int kind, const void* target,
                              const float* gscale, float* logits, float* loss, void* dA, long ldda, float* dW2, float* db2, int do_bwd,
                              hipStream_t stream) {
  SPMM_CHECK_SHAPE(B >= 1 && B <= 1024, "spmm_task_head: B=%d (1 <= B <= 1024)", B);
  SPMM_CHECK_SHAPE(C >= 1 && C <= TH_MAXC, "spmm_task_head: C=%d (1 <= C <= %d)", C, TH_MAXC);
  SPMM_CHECK_SHAPE(W >= 64 && W <= TH_MAXW && W % 64 == 0, "spmm_task_head: W=%d (a multiple of 64 up to %d)", W, TH_MAXW);
  SPMM_CHECK_SHAPE(kind >= 0 && kind <= 2, "spmm_task_head: kind %d (0 = MSE, 1 = cross entropy, 2 = BCE)", kind);
  SPMM_CHECK_SHAPE(kind != 0 || C == 1, "spmm_task_head: MSE needs C = 1 (C=%d)", C);
  SPMM_CHECK_SHAPE(A && W2 && b2 && logits && lda >= W, "spmm_task_head: A, W2, b2 and logits are required (lda=%ld W=%d)", lda, W);
  SPMM_CHECK_SHAPE(target || (!loss && !do_bwd), "spmm_task_head: the loss and the backward need targets");
  SPMM_CHECK_SHAPE(!do_bwd || (dA && dW2 && db2 && ldda >= W), "spmm_task_head: backward outputs missing (ldda=%ld)", ldda);
  hipLaunchKernelGGL(task_head_rows_kernel, dim3(B), dim3(TH_THREADS), 0, stream, (const bf16*)A, lda, B, W, W2, b2, C, kind, target, gscale,
                     logits, (bf16*)dA, ldda, do_bwd);
  SPMM_LAUNCH_CHECK("spmm_task_head");
  if (loss || do_bwd) {
    hipLaunchKernelGGL(task_head_cols_kernel, dim3(do_bwd ? W / 64 : 1), dim3(TH_THREADS), 0, stream, (const bf16*)A, lda, B, W, C, kind, target,
                       gscale, logits, loss, dW2, db2, do_bwd);
    SPMM_LAUNCH_CHECK("spmm_task_head");
  }
  return SPMM_OK;
}

namespace {

// ------------------------------------------------------------------------------------------------------------ spmm_s2p_append
// One wave per row r (four rows per workgroup): the row of H <= 1024 values stays in registers, S2P_MAXC chunks of four per lane
// (8-byte bf16 loads / stores, 16-byte fp32 loads).
//   p = b3 + sum_h y[r,h] w3[h]                          fp32, lane-local chunks then the wave butterfly      -> pred[r*ldp + i]
//   e[h] = p pe_w[h] + pe_b[h] + pos_j[h] (+ type0[h])   property_embed (SPMM_models.py:36), xbert.py:209-217
//   xrow[r*Lc*H + h] = LN(e)[h] gamma[h] + beta[h]        two-pass variance as in ln_apply (csrc/rowops.hip); xrow = xcache + j*H, null: no next step
constexpr int S2P_MAXC = 4;
__global__ __launch_bounds__(256) void s2p_append_kernel(const bf16* __restrict__ y, long ldy, const float* __restrict__ w3,
                                                         const float* __restrict__ b3, const float* __restrict__ pe_w,
                                                         const float* __restrict__ pe_b, const float* __restrict__ pos_j,
                                                         const float* __restrict__ type0, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, float eps, float* __restrict__ pred, long ldp,
                                                         int i, bf16* __restrict__ xrow, long seq_stride, long rows, int H) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const bf16* yr = y + r * ldy;
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < S2P_MAXC; ++k) {
    const int c = (lane + 64 * k) * 4;
    if (c < H) {
      const bf16x4 a = *(const bf16x4*)(yr + c);
      const f32x4 w = *(const f32x4*)(w3 + c);
      s += ((float)a[0] * w[0] + (float)a[1] * w[1]) + ((float)a[2] * w[2] + (float)a[3] * w[3]);
    }
  }
  const float p = wave_sum(s) + b3[0];                // (the butterfly leaves the same sum in every lane)
  if (lane == 0) pred[r * ldp + i] = p;
  if (!xrow) return;
  float e[S2P_MAXC][4];
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < S2P_MAXC; ++k) {
    const int c = (lane + 64 * k) * 4;
    if (c < H) {
      const f32x4 w = *(const f32x4*)(pe_w + c), b = *(const f32x4*)(pe_b + c), ps = *(const f32x4*)(pos_j + c);
      f32x4 t = {0.f, 0.f, 0.f, 0.f};
      if (type0) t = *(const f32x4*)(type0 + c);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        e[k][j] = (p * w[j] + b[j]) + (ps[j] + t[j]);
        sum += e[k][j];
      }
    } else {
      e[k][0] = e[k][1] = e[k][2] = e[k][3] = 0.f;
    }
  }
  const float mean = wave_sum(sum) / H;
  float ss = 0.f;
#pragma unroll
  for (int k = 0; k < S2P_MAXC; ++k) {
    const int c = (lane + 64 * k) * 4;
    if (c < H) {
#pragma unroll
      for (int j = 0; j < 4; ++j) { const float d = e[k][j] - mean; ss += d * d; }
    }
  }
  const float var = wave_sum(ss) / H;
  float rstd = rsqrtf(var + eps);
  if (!(var + eps > 0.f)) rstd = 0.f;                 // an all-equal row with an eps that underflows: zeros, not NaN (as ln_apply)
  bf16* out = xrow + r * seq_stride;
#pragma unroll
  for (int k = 0; k < S2P_MAXC; ++k) {
    const int c = (lane + 64 * k) * 4;
    if (c < H) {
      const f32x4 gm = *(const f32x4*)(gamma + c), bt = *(const f32x4*)(beta + c);
      *(bf16x4*)(out + c) = to_bf16x4((e[k][0] - mean) * rstd * gm[0] + bt[0], (e[k][1] - mean) * rstd * gm[1] + bt[1],
                                      (e[k][2] - mean) * rstd * gm[2] + bt[2], (e[k][3] - mean) * rstd * gm[3] + bt[3]);
    }
  }
}

}  // namespace

extern "C" int spmm_s2p_append(const void* y, long ldy, const float* w3, const float* b3, const float* pe_w, const float* pe_b,
                               const float* pos, const float* type0, const float* gamma, const float* beta, float eps, float* pred,
                               long ldp, void* xcache, long rows, int H, int n_props, int i, hipStream_t stream) {
  SPMM_CHECK_SHAPE(rows >= 1 && rows <= (1l << 24), "spmm_s2p_append: rows=%ld (1 <= rows <= 2^24)", rows);
  SPMM_CHECK_SHAPE(H >= 64 && H % 64 == 0 && H <= 256 * S2P_MAXC, "spmm_s2p_append: H=%d (a multiple of 64 up to %d)", H, 256 * S2P_MAXC);
  SPMM_CHECK_SHAPE(n_props >= 1 && i >= 0 && i < n_props, "spmm_s2p_append: step i=%d of n_props=%d (0 <= i < n_props)", i, n_props);
  SPMM_CHECK_SHAPE(ldy >= H && ldy % 4 == 0, "spmm_s2p_append: ldy=%ld (at least H=%d, a multiple of 4)", ldy, H);
  SPMM_CHECK_SHAPE(ldp >= n_props, "spmm_s2p_append: ldp=%ld (at least n_props=%d)", ldp, n_props);
  SPMM_CHECK_SHAPE(y && w3 && b3 && pred, "spmm_s2p_append: y, w3, b3 and pred are required");
  const auto mis = [](const void* q, uintptr_t n) { return ((uintptr_t)q & (n - 1)) != 0; };
  SPMM_CHECK_SHAPE(!mis(y, 8) && !mis(xcache, 8) && !mis(w3, 16) && !mis(pe_w, 16) && !mis(pe_b, 16) && !mis(pos, 16) && !mis(type0, 16) &&
                       !mis(gamma, 16) && !mis(beta, 16),
                   "spmm_s2p_append: misaligned pointer (y, xcache: 8 bytes; w3, pe_w, pe_b, pos, type0, gamma, beta: 16 bytes)");
  const bool next = i + 1 < n_props;                  // the last step opens no further one: the cache is not written
  SPMM_CHECK_SHAPE(!next || (pe_w && pe_b && pos && gamma && beta && xcache),
                   "spmm_s2p_append: step %d of %d appends a cache row: pe_w, pe_b, pos, gamma, beta and xcache are required", i, n_props);
  const long j = i + 1, Lc = (long)n_props + 1;
  hipLaunchKernelGGL(s2p_append_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, (const bf16*)y, ldy, w3, b3, pe_w, pe_b,
                     next ? pos + j * H : nullptr, type0, gamma, beta, eps, pred, ldp, i, next ? (bf16*)xcache + j * H : nullptr, Lc * H,
                     rows, H);
  SPMM_LAUNCH_CHECK("spmm_s2p_append");
  return SPMM_OK;
}
