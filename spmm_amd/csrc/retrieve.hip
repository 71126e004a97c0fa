// Retrieval: streaming top-k of Q query features against a library of unit features, without the [Q, N] similarity matrix
// (spmm_sim_topk, include/spmm_hip.h).
//
// Two launches.  sim_topk_part: workgroup (s, qt) walks the 256-row tiles s, s + S, .. of the chunk for the 16 queries of tile qt.  A tile's
// 16 x 256 similarities come from the exact f32-input MFMA into LDS; each wave then owns four of the queries and keeps their k best
// candidates in registers, one per lane, sorted (best in lane 0): a score is compared with the list's k-th entry first, and the few that
// pass are inserted by one ballot and one lane shift.  The lists go to the workspace as [S, Q, k] keys.  sim_topk_merge: one workgroup per
// query folds the S partial lists (and, merge = 1, the state already there) into the state.
//
// The order of candidates and the order of the sum over E are csrc/sim_scan.h's: "the k best of a set" does not depend on how the set was
// cut into tiles, workgroups or chunks, and a pair's score is the same chain whatever tile, lane or chunk the row falls in.  Hence any
// chunking of a library gives the same bits.  No floating-point atomics anywhere.
#include "sim_scan.h"
#include "../../include/spmm_hip.h"

namespace {

using namespace sim_scan;

constexpr int QT = 16;            // queries of a workgroup (the MFMA's 16 output rows)
constexpr int TR = 256;           // library rows of a tile: 4 waves x 4 blocks of 16
constexpr int TRP = TR + 4;       // score tile row stride in LDS (the four lane groups of a store land in four bank groups)
constexpr int NT = 256;
constexpr long IDX_EMPTY = 0x7fffffffffffffffL;

// ---- first launch: candidates of a chunk as 64-bit keys (sim_scan.h's pack_key over the row within the chunk)
__device__ __forceinline__ void list_insert(uint64_t& mine, uint64_t cand, int lane) {
  const int pos = __popcll(__ballot(mine > cand));
  const uint64_t up = shfl_up64(mine);
  mine = lane < pos ? mine : (lane == pos ? cand : up);
}

__global__ __launch_bounds__(NT) void sim_topk_part(const float* __restrict__ q, long ldq, const float* __restrict__ f, long ldf, long base,
                                                    int Q, int n, int E, int k, const float* __restrict__ cut_scores,
                                                    const long* __restrict__ cut_index, uint64_t* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int EP = E + 4;
  float* ql = smem;                     // [QT][EP]
  float* sl = smem + QT * EP;           // [QT][TRP]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int q0 = blockIdx.y * QT;
  for (int i = tid; i < QT * (E / 4); i += NT) {
    const int r = i / (E / 4), e4 = i % (E / 4);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (q0 + r < Q) v = *reinterpret_cast<const f32x4*>(q + (long)(q0 + r) * ldq + e4 * 4);
    *reinterpret_cast<f32x4*>(ql + r * EP + e4 * 4) = v;
  }
  uint64_t mine[4] = {0, 0, 0, 0}, thr[4] = {0, 0, 0, 0};
  uint32_t kc[4];
  long ic[4];
  const bool has_cut = cut_scores != nullptr;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int qi = q0 + w * 4 + u;
    kc[u] = 0u; ic[u] = -1;
    if (has_cut && qi < Q) { kc[u] = score_key(cut_scores[qi]); ic[u] = cut_index[qi]; }
  }
  __syncthreads();
  const int tiles = (n + TR - 1) / TR;
  for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int tile0 = t * TR;
    f32x4 acc[4];
    const float* fp[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};
      const int row = min(tile0 + w * 64 + b * 16 + c, n - 1);          // rows past the chunk: a valid address, dropped in the scan
      fp[b] = f + (long)row * ldf + g * 4;
    }
    const float* qp = ql + c * EP + g * 4;
    for (int k0 = 0; k0 < E; k0 += 64) {                                  // (E is a multiple of 64: four 16-element steps per trip)
#pragma unroll
      for (int kk = 0; kk < 64; kk += 16) {
        const f32x4 qa = *reinterpret_cast<const f32x4*>(qp + k0 + kk);
        f32x4 fb[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) fb[b] = *reinterpret_cast<const f32x4*>(fp[b] + k0 + kk);
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
          for (int b = 0; b < 4; ++b) acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[m], fb[b][m], acc[b], 0, 0, 0);
      }
    }
    // D: column (lane & 15) = library row of the block, row 4 g + r = query
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) sl[(g * 4 + r) * TRP + w * 64 + b * 16 + c] = acc[b][r];
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int ql_i = w * 4 + u;
      if (q0 + ql_i >= Q) continue;                                       // (wave-uniform)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = tile0 + lane + 64 * j;
        const uint32_t sk = score_key(sl[ql_i * TRP + lane + 64 * j]);
        const uint64_t key = pack_key(sk, (uint32_t)row);
        bool ok = row < n && key > thr[u];
        if (has_cut) ok = ok && ic[u] >= 0 && (sk < kc[u] || (sk == kc[u] && base + row > ic[u]));
        uint64_t mask = __ballot(ok);
        while (mask) {
          const int src = __ffsll((unsigned long long)mask) - 1;
          mask &= mask - 1;
          const uint64_t cand = shfl64(key, src);
          if (cand > thr[u]) {
            list_insert(mine[u], cand, lane);
            thr[u] = shfl64(mine[u], k - 1);
          }
        }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int qi = q0 + w * 4 + u;
    if (qi < Q && lane < k) part[((long)blockIdx.x * Q + qi) * k + lane] = mine[u];
  }
}

// ---- second launch: candidates as (score image, global index); empty = (0, IDX_EMPTY)
__device__ __forceinline__ bool better(uint32_t ka, long ia, uint32_t kb, long ib) { return ka > kb || (ka == kb && ia < ib); }

struct List2 {
  uint32_t key;
  long idx;
  uint32_t tk;      // the k-th entry (wave-uniform)
  long ti;
};

__device__ __forceinline__ void list2_offer(List2& L, uint32_t ck, long ci, int k, int lane) {
  const bool ok = !(ck == 0u && ci == IDX_EMPTY) && better(ck, ci, L.tk, L.ti);
  uint64_t mask = __ballot(ok);
  while (mask) {
    const int src = __ffsll((unsigned long long)mask) - 1;
    mask &= mask - 1;
    const uint32_t k1 = __shfl(ck, src, 64);
    const long i1 = (long)shfl64((uint64_t)ci, src);
    if (better(k1, i1, L.tk, L.ti)) {
      const int pos = __popcll(__ballot(better(L.key, L.idx, k1, i1)));
      const uint32_t uk = __shfl_up(L.key, 1, 64);
      const long ui = (long)shfl_up64((uint64_t)L.idx);
      L.key = lane < pos ? L.key : (lane == pos ? k1 : uk);
      L.idx = lane < pos ? L.idx : (lane == pos ? i1 : ui);
      L.tk = __shfl(L.key, k - 1, 64);
      L.ti = (long)shfl64((uint64_t)L.idx, k - 1);
    }
  }
}

__global__ __launch_bounds__(NT) void sim_topk_merge(const uint64_t* __restrict__ part, int S, int Q, int k, long base, int merge,
                                                     float* __restrict__ scores, long* __restrict__ index) {
  __shared__ uint32_t lk[4][64];
  __shared__ long li[4][64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, qi = blockIdx.x;
  List2 L{0u, IDX_EMPTY, 0u, IDX_EMPTY};
  if (merge && w == 0) {
    uint32_t ck = 0u;
    long ci = IDX_EMPTY;
    if (lane < k) {
      const long i = index[(long)qi * k + lane];
      if (i >= 0) { ci = i; ck = score_key(scores[(long)qi * k + lane]); }
    }
    list2_offer(L, ck, ci, k, lane);
  }
  const long total = (long)S * k;
  for (long e0 = (long)w * 256; e0 < total; e0 += 4 * 256) {
    uint64_t v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long e = e0 + j * 64 + lane;
      v[j] = 0;
      if (e < total) v[j] = part[((e / k) * Q + qi) * k + e % k];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool real = v[j] != EMPTY_KEY;
      list2_offer(L, real ? key_image(v[j]) : 0u, real ? base + (long)key_index(v[j]) : IDX_EMPTY, k, lane);
    }
  }
  lk[w][lane] = L.key;
  li[w][lane] = L.idx;
  __syncthreads();
  if (w != 0) return;
  for (int o = 1; o < 4; ++o) list2_offer(L, lane < k ? lk[o][lane] : 0u, lane < k ? li[o][lane] : IDX_EMPTY, k, lane);
  if (lane < k) {
    const bool empty = L.key == 0u && L.idx == IDX_EMPTY;
    scores[(long)qi * k + lane] = empty ? -__builtin_huge_valf() : key_score(L.key);
    index[(long)qi * k + lane] = empty ? -1 : L.idx;
  }
}

// row splits of a chunk: enough workgroups to fill the chip at any Q, few enough that the merge stays small beside the scan
inline int splits_of(int Q, long n) {
  const long tiles = (n + TR - 1) / TR;
  const int qt = (Q + QT - 1) / QT;
  long s = 512 / qt;
  if (s < 32) s = 32;
  if (s > tiles) s = tiles;
  return (int)s;
}

}  // namespace

extern "C" long spmm_sim_topk_workspace_bytes(int Q, long n, int k) {
  if (Q < 1 || n < 0 || k < 1) return 0;
  const long b = (long)splits_of(Q, n) * Q * k * 8;
  return b < 16 ? 16 : b;
}

extern "C" int spmm_sim_topk(const float* q, long ldq, const float* f, long ldf, long base, int Q, long n, int E, int k, float* scores,
                             long* index, int merge, const float* cut_scores, const long* cut_index, void* workspace, long workspace_bytes,
                             spmm_stream_t stream) {
  SPMM_CHECK_SHAPE(k >= 1 && k <= 64, "spmm_sim_topk: k=%d must be in [1,64]", k);
  if (int e = check_width("spmm_sim_topk", E)) return e;
  SPMM_CHECK_SHAPE(Q >= 1, "spmm_sim_topk: Q=%d must be at least 1", Q);
  SPMM_CHECK_SHAPE(Q <= 65535 * QT, "spmm_sim_topk: Q=%d exceeds %d queries per call", Q, 65535 * QT);
  SPMM_CHECK_SHAPE(n >= 0 && n <= 0x7fffff00L, "spmm_sim_topk: n=%ld must be in [0, 2^31 - 256] rows per chunk", n);   // (row numbers of the last, partial tile stay in int)
  SPMM_CHECK_SHAPE(merge == 0 || merge == 1, "spmm_sim_topk: merge=%d must be 0 or 1", merge);
  SPMM_CHECK_SHAPE(scores && index, "spmm_sim_topk: null scores / index (the state)");
  SPMM_CHECK_SHAPE(aligned(scores, 4) && aligned(index, 8), "spmm_sim_topk: misaligned scores / index (4 / 8 bytes)");
  SPMM_CHECK_SHAPE((cut_scores == nullptr) == (cut_index == nullptr), "spmm_sim_topk: cut_scores and cut_index come together");
  SPMM_CHECK_SHAPE(base >= 0 && base <= IDX_EMPTY - 0x80000000L, "spmm_sim_topk: base=%ld out of range", base);
  if (n == 0 && merge == 1) return SPMM_OK;                                 // nothing seen: the state stays as it is
  int S = 0;
  if (n > 0) {
    SPMM_CHECK_SHAPE(q && f, "spmm_sim_topk: null q / f");
    SPMM_CHECK_SHAPE(aligned(q, 16) && aligned(f, 16), "spmm_sim_topk: q / f must be 16-byte aligned");
    SPMM_CHECK_SHAPE(ldq >= E && ldq % 4 == 0 && ldf >= E && ldf % 4 == 0,
                     "spmm_sim_topk: ldq=%ld ldf=%ld must be multiples of 4, at least E=%d", ldq, ldf, E);
    S = splits_of(Q, n);
    const long need = (long)S * Q * k * 8;
    SPMM_CHECK_SHAPE(workspace && aligned(workspace, 16) && workspace_bytes >= need,
                     "spmm_sim_topk: workspace of %ld bytes (16-byte aligned) needed, %ld given (spmm_sim_topk_workspace_bytes)", need,
                     workspace ? workspace_bytes : 0L);
    const size_t lds = (size_t)(QT * (E + 4) + QT * TRP) * sizeof(float);     // at most 49 664 bytes (E = 512)
    hipLaunchKernelGGL(sim_topk_part, dim3(S, (Q + QT - 1) / QT), dim3(NT), lds, stream, q, ldq, f, ldf, base, Q, (int)n, E, k, cut_scores,
                       cut_index, reinterpret_cast<uint64_t*>(workspace));
    SPMM_LAUNCH_CHECK("spmm_sim_topk (scan)");
  }
  hipLaunchKernelGGL(sim_topk_merge, dim3(Q), dim3(NT), 0, stream, reinterpret_cast<const uint64_t*>(workspace), S, Q, k, base, merge, scores,
                     index);
  SPMM_LAUNCH_CHECK("spmm_sim_topk (merge)");
  return SPMM_OK;
}
