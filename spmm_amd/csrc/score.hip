// Teacher-forced scoring: vocabulary projection of the tied LM head, log_softmax and the gather of the label's entry in one launch
// (spmm_lm_score, include/spmm_hip.h).  The [rows, V] logits never leave the registers.
//
// lm_score_rows: a workgroup of four waves owns a block of 128 rows, a wave 32 of them (two halves of 16).  The logits are computed
// TRANSPOSED on v_mfma_f32_16x16x32_bf16 -- a 16-token tile of Wd is the A operand, 16 rows of y are the B operand -- so a lane holds, for
// ITS row (lane & 15), the tokens 16 t + 4 (lane >> 4) + r of every tile t: the whole Vpad-wide strip of a row sits in the accumulators of
// four lanes (NT tiles per half: 4, 20 or 32 for V <= 64, 320, 512).  Wd streams through LDS in K-slices of 64 columns (whole 128-byte
// lines of a row), shared by the four waves: the slice after the current one is fetched into registers while the MFMAs of the current one
// run, then stored; eight fragment reads stay in flight ahead of their MFMAs.  The widest strip, V > 320, keeps one half per wave (64 rows
// a workgroup) and 32-column slices: two halves would not fit the registers, a 64-column slice not the 64 KiB of LDS.  Rows of Wd past V
// are zero-filled in LDS, never read; their logits are masked out of the softmax.
//
// Order.  The sum over H of a (row, token) pair is one accumulator's chain over the K-slices in ascending order, whatever lane, half, wave
// or workgroup the row falls in.  A row's maximum and its sum of exponentials run over the lane's tiles in ascending order, then over the
// four lanes of the row by two butterfly steps (commutative at each step: the four lanes hold the same bits).  lm_score_seqs sums a
// sequence's tok_lp in ascending row order, one thread per sequence.  No floating-point atomics: the same y row gives the same tok_lp bits
// in any batch, and two launches agree bit for bit.
#include "common.h"
#include "../../include/spmm_hip.h"

namespace {

constexpr int NTHR = 256;
constexpr int BROWS_MAX = 128;            // rows of a workgroup: four waves x NH halves of 16 (the MFMA's column block)
constexpr int GRID_MAX = 1024;            // workgroups of a launch; they stride over the row blocks

// the label rule of spmm_s2s_loss (csrc/losses.hip::s2s_label), verbatim
__device__ __forceinline__ int score_label(const int* __restrict__ ids, const long* __restrict__ row_of, long r, long nd, int L, int V) {
  const long d = row_of ? row_of[r] : r;
  if (d < 0 || d >= nd || (int)(d % L) == L - 1) return 0;
  const int label = ids[d + 1];
  return (label > 0 && label < V) ? label : 0;
}

template <int NT, int NH, int KS>
__global__ __launch_bounds__(NTHR) void lm_score_rows(const bf16* __restrict__ y, long ldy, const bf16* __restrict__ Wd, long ldw,
                                                      const float* __restrict__ bias, const int* __restrict__ ids,
                                                      const long* __restrict__ row_of, long rows, long nd, int L, int V, int H,
                                                      float* __restrict__ tok_lp) {
  constexpr int WROWS = 16 * NH, BROWS = 4 * WROWS;
  constexpr int LDW = KS + 8;             // LDS row stride in elements (KS = 32: 80 bytes, 64: 144; the 16-byte reads of 16 rows cover all banks once)
  constexpr int KP = KS / 8, KK = KS / 32;   // 16-byte pieces of a row's slice; MFMA steps of a slice
  constexpr int CH = NT * 16 * KP / NTHR;    // pieces of a K-slice per thread
  __shared__ __attribute__((aligned(16))) bf16 wl[NT * 16 * LDW];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const long nblocks = (rows + BROWS - 1) / BROWS;
  const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  for (long blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
    const long row0 = blk * BROWS + w * WROWS;
    const bf16* yp[NH];
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      long r = row0 + h * 16 + c;
      if (r > rows - 1) r = rows - 1;                                      // rows past the batch: a valid address, dropped at the end
      yp[h] = y + r * ldy + g * 8;
    }
    f32x4 acc[NH][NT];
#pragma unroll
    for (int h = 0; h < NH; ++h)
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[h][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    bf16x8 wreg[CH], yb[NH][KK], ynext[NH][KK];
    auto fetch = [&](int k0) {
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        const int piece = tid + NTHR * j, v = piece / KP, part = piece % KP;
        wreg[j] = v < V ? *reinterpret_cast<const bf16x8*>(Wd + (long)v * ldw + k0 + part * 8) : zero8;
      }
#pragma unroll
      for (int h = 0; h < NH; ++h)
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) ynext[h][kk] = *reinterpret_cast<const bf16x8*>(yp[h] + k0 + kk * 32);
    };
    fetch(0);
    for (int k0 = 0; k0 < H; k0 += KS) {
      __syncthreads();                                                     // every wave is done with the slice before
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        const int piece = tid + NTHR * j;
        *reinterpret_cast<bf16x8*>(wl + (piece / KP) * LDW + (piece % KP) * 8) = wreg[j];
      }
#pragma unroll
      for (int h = 0; h < NH; ++h)
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) yb[h][kk] = ynext[h][kk];
      __syncthreads();
      if (k0 + KS < H) fetch(k0 + KS);
      const bf16* wp = wl + c * LDW + g * 8;
      bf16x8 af[KK * NT];                                                  // fragments in flight ahead of their MFMAs
#pragma unroll
      for (int u = 0; u < KK * NT; ++u) af[u] = *reinterpret_cast<const bf16x8*>(wp + (u % NT) * 16 * LDW + (u / NT) * 32);
#pragma unroll
      for (int u = 0; u < KK * NT; ++u)
#pragma unroll
        for (int h = 0; h < NH; ++h) acc[h][u % NT] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[u], yb[h][u / NT], acc[h][u % NT], 0, 0, 0);
      // schedule: AHEAD fragment reads first, then one further read behind every tile's MFMAs, so the LDS latency hides under the MFMAs
      constexpr int AHEAD = KK * NT < 8 ? KK * NT : 8;
      __builtin_amdgcn_sched_group_barrier(0x100, AHEAD, 0);
#pragma unroll
      for (int u = 0; u < KK * NT - AHEAD; ++u) {
        __builtin_amdgcn_sched_group_barrier(0x008, NH, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      }
      __builtin_amdgcn_sched_group_barrier(0x008, AHEAD * NH, 0);
    }
    // D: column (lane & 15) = row of the half, row 4 g + r = token of the tile
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      const long r = row0 + h * 16 + c;
      const int label = r < rows ? score_label(ids, row_of, r, nd, L, V) : 0;
      float mx = -INFINITY, xl = -INFINITY;
      float xs[NT][4];
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int v = t * 16 + g * 4 + i;
          const float x = v < V ? acc[h][t][i] + bias[v] : -INFINITY;
          xs[t][i] = x;
          mx = fmaxf(mx, x);
          xl = v == label ? x : xl;
        }
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      xl = fmaxf(xl, __shfl_xor(xl, 16, 64));                              // (one lane of the four holds the label's logit)
      xl = fmaxf(xl, __shfl_xor(xl, 32, 64));
      float se = 0.f;
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) se += __expf(xs[t][i] - mx);           // (exp(-inf) = 0 on the columns past V)
      se += __shfl_xor(se, 16, 64);
      se += __shfl_xor(se, 32, 64);
      if (g == 0 && r < rows) tok_lp[r] = label ? (xl - mx) - __logf(se) : 0.f;
    }
  }
}

// sequence s: the sum of its rows' tok_lp in ascending row order, and the number of labelled rows among them
__global__ __launch_bounds__(NTHR) void lm_score_seqs(const float* __restrict__ tok_lp, const int* __restrict__ ids,
                                                      const long* __restrict__ row_of, long rows, long nseq, long nd, int L, int V,
                                                      const int* __restrict__ seq_row0, const int* __restrict__ seq_len,
                                                      float* __restrict__ seq_lp, int* __restrict__ seq_n) {
  const long s = (long)blockIdx.x * NTHR + threadIdx.x;
  if (s >= nseq) return;
  long r0 = seq_row0 ? (long)seq_row0[s] : s * L;
  long r1 = r0 + (seq_len ? (long)seq_len[s] : (long)L);
  if (r0 < 0) r0 = 0;
  if (r1 > rows) r1 = rows;
  float lp = 0.f;
  int n = 0;
  for (long r = r0; r < r1; ++r) {
    if (score_label(ids, row_of, r, nd, L, V) == 0) continue;
    lp += tok_lp[r];
    ++n;
  }
  seq_lp[s] = lp;
  seq_n[s] = n;
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

extern "C" int spmm_lm_score(const void* y, long ldy, const void* Wd, long ldw, const float* bias, const int* ids, const long* row_of,
                             long rows, long nseq, int L, int V, int H, const int* seq_row0, const int* seq_len, float* tok_lp,
                             float* seq_lp, int* seq_n, spmm_stream_t stream) {
  SPMM_CHECK_SHAPE(H >= 64 && H <= 1024 && H % 64 == 0, "spmm_lm_score: H=%d must be a multiple of 64 up to 1024", H);
  SPMM_CHECK_SHAPE(V >= 2 && V <= 512, "spmm_lm_score: V=%d must be in [2,512]", V);
  SPMM_CHECK_SHAPE(rows >= 1 && nseq >= 1 && L >= 2 && rows <= nseq * (long)L,
                   "spmm_lm_score: rows=%ld nseq=%ld L=%d (L >= 2, 1 <= rows <= nseq*L)", rows, nseq, L);
  SPMM_CHECK_SHAPE(nseq <= 0x7fffffffL / NTHR, "spmm_lm_score: nseq=%ld exceeds %ld sequences per call", nseq, 0x7fffffffL / NTHR);
  SPMM_CHECK_SHAPE(y && Wd && bias && ids && tok_lp && seq_lp && seq_n,
                   "spmm_lm_score: y, Wd, bias, ids, tok_lp, seq_lp and seq_n are required");
  SPMM_CHECK_SHAPE(ldy >= H && ldy % 8 == 0 && ldw >= H && ldw % 8 == 0,
                   "spmm_lm_score: ldy=%ld ldw=%ld must be multiples of 8, at least H=%d", ldy, ldw, H);
  SPMM_CHECK_SHAPE(aligned(y, 16) && aligned(Wd, 16), "spmm_lm_score: y / Wd must be 16-byte aligned");
  SPMM_CHECK_SHAPE(aligned(bias, 4) && aligned(ids, 4) && aligned(tok_lp, 4) && aligned(seq_lp, 4) && aligned(seq_n, 4) &&
                       aligned(row_of, 8) && aligned(seq_row0, 4) && aligned(seq_len, 4),
                   "spmm_lm_score: misaligned bias / ids / tok_lp / seq_lp / seq_n / seq_row0 / seq_len (4 bytes) or row_of (8 bytes)");
  SPMM_CHECK_SHAPE((seq_row0 == nullptr) == (seq_len == nullptr), "spmm_lm_score: seq_row0 and seq_len come together");
  SPMM_CHECK_SHAPE(seq_row0 || rows == nseq * (long)L, "spmm_lm_score: dense sequences (no seq_row0 / seq_len) need rows=%ld == nseq*L=%ld",
                   rows, nseq * (long)L);
  const int brows = V <= 320 ? BROWS_MAX : BROWS_MAX / 2;
  const long nblocks = (rows + brows - 1) / brows;
  const dim3 grid((unsigned)(nblocks < GRID_MAX ? nblocks : GRID_MAX));
  const bf16* yb = reinterpret_cast<const bf16*>(y);
  const bf16* wb = reinterpret_cast<const bf16*>(Wd);
  const long nd = nseq * (long)L;
  if (V <= 64)
    hipLaunchKernelGGL((lm_score_rows<4, 2, 64>), grid, dim3(NTHR), 0, stream, yb, ldy, wb, ldw, bias, ids, row_of, rows, nd, L, V, H, tok_lp);
  else if (V <= 320)
    hipLaunchKernelGGL((lm_score_rows<20, 2, 64>), grid, dim3(NTHR), 0, stream, yb, ldy, wb, ldw, bias, ids, row_of, rows, nd, L, V, H, tok_lp);
  else
    hipLaunchKernelGGL((lm_score_rows<32, 1, 32>), grid, dim3(NTHR), 0, stream, yb, ldy, wb, ldw, bias, ids, row_of, rows, nd, L, V, H, tok_lp);
  SPMM_LAUNCH_CHECK("spmm_lm_score (rows)");
  hipLaunchKernelGGL(lm_score_seqs, dim3((unsigned)((nseq + NTHR - 1) / NTHR)), dim3(NTHR), 0, stream, tok_lp, ids, row_of, rows, nseq, nd, L,
                     V, seq_row0, seq_len, seq_lp, seq_n);
  SPMM_LAUNCH_CHECK("spmm_lm_score (sequences)");
  return SPMM_OK;
}
