// Library clustering: nearest centre of every row (spmm_centroid_assign), members of every cluster (spmm_cluster_group) and the clusters'
// centres, norms and medoids (spmm_cluster_centroids); include/spmm_hip.h.
//
// centroid_assign.  The arithmetic of retrieval (csrc/retrieve.hip) with the roles swapped: many rows, few centres -- the row-stationary
// scan of csrc/sim_scan.h with the centres as its column side.  A tile's scores never leave the accumulators: every lane folds its four
// scores of a (centre block, row block) into a running best of its own -- one 64-bit key per row block -- and the four lane groups of a
// row are combined once, after the last tile.  No score tile, no per-row list, no workspace.  The chain and the candidate order are that
// header's, so the result has the bits of spmm_sim_topk(q = rows, f = centres, k = 1), however the centre list is cut into chunks.
//
// cluster_group.  A stable counting sort of the rows by cluster.  The rows are cut into nb blocks; launch 1 counts every block's rows per
// cluster (integer atomics into the block's own line of the [nb, K] table), launch 2 turns each column into running starts and the column
// totals into counts, launch 3 scans the counts into offsets, launch 4 lets block b walk its rows in ascending tiles of 256 and place row i
// at offsets[c] + start[b][c] + (rows of c earlier in the tile): members of a cluster ascend, whatever the grid.
//
// cluster_centroids.  A cluster's members are cut into pieces of PIECE = 256 consecutive members; one workgroup sums a piece's rows in
// member order (a sequential fp32 chain per component) and finds its medoid candidate; a second launch, one workgroup per cluster, adds the
// piece sums in ascending order, takes the norm on a fixed tree and writes the centre.  The order is a function of the member list alone.
// No floating-point atomics.
#include "sim_scan.h"
#include "../../include/spmm_hip.h"

namespace {

using namespace sim_scan;

constexpr int NT = 256;
constexpr int PIECE = 256;       // members of one partial centroid sum
constexpr long GROUP_TABLE = 1L << 24;      // entries of cluster_group's [nb, K] table at the most

// ------------------------------------------------------------------------------------------------------------------ assign
template <int E64>
__global__ __launch_bounds__(Shape<E64>::NT) void centroid_assign(const float* __restrict__ f, long ldf, const float* __restrict__ cen, long ldc,
                                                                  int c0, int n, int Kc, int merge, float* __restrict__ best,
                                                                  int* __restrict__ assign, const int* __restrict__ prev,
                                                                  int* __restrict__ changed) {
  using S = Shape<E64>;
  constexpr int AR = S::AR, NB = S::NB, CB = S::CB, CT = S::CT;
  __shared__ __attribute__((aligned(16))) float cl[CT * S::EP];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const long row0 = (long)blockIdx.x * AR + w * (NB * 16);
  f32x4 rows[NB][S::KB];
#pragma unroll
  for (int b = 0; b < NB; ++b) load_row_block<E64>(f, ldf, row0 + b * 16 + c, n, g, rows[b]);
  uint64_t mine[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) mine[b] = EMPTY_KEY;
  RowScan<E64> scan(cen, ldc, Kc, cl);
  for (int t = 0; t < scan.tiles; ++t) {
    f32x4 acc[CB][NB];
    scan.scores(t, rows, acc);
    // the key carries the index, so `>` keeps the lowest of equals; centres past the chunk are dropped
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = t * CT + cb * 16 + g * 4 + r;
        if (j < Kc) {
#pragma unroll
          for (int b = 0; b < NB; ++b) {
            const uint64_t key = cand_key(acc[cb][b][r], (uint32_t)(c0 + j));
            mine[b] = key > mine[b] ? key : mine[b];
          }
        }
      }
    scan.next(t);
  }
  int diff = 0;
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    uint64_t m = mine[b];
    uint64_t o = shfl_xor64(m, 16);
    m = o > m ? o : m;
    o = shfl_xor64(m, 32);
    m = o > m ? o : m;
    const long row = row0 + b * 16 + c;
    if (g == 0 && row < n) {
      if (merge) {
        const int ia = assign[row];
        if (ia >= 0) {
          const uint64_t s = cand_key(best[row], (uint32_t)ia);
          m = s > m ? s : m;
        }
      }
      const int ia = m == EMPTY_KEY ? -1 : (int)key_index(m);
      best[row] = m == EMPTY_KEY ? -__builtin_huge_valf() : key_score(key_image(m));
      assign[row] = ia;
      if (prev != nullptr && prev[row] != ia) ++diff;
    }
  }
  if (prev != nullptr) {                                                    // (wave-uniform)
    const int cnt = __popcll(__ballot(diff & 1)) + 2 * __popcll(__ballot(diff & 2));
    if (lane == 0 && cnt) atomicAdd(changed, cnt);
  }
}

// ------------------------------------------------------------------------------------------------------------------ group
// rows of block b: [b * rb, min(n, (b + 1) * rb)), rb a multiple of 256
__global__ __launch_bounds__(NT) void group_count(const int* __restrict__ assign, long n, int K, long rb, int* __restrict__ table,
                                                  int* __restrict__ outside) {
  const long lo = (long)blockIdx.x * rb, hi = min(n, lo + rb);
  int* line = table + (long)blockIdx.x * K;
  int out = 0;
  for (long i = lo + threadIdx.x; i < hi; i += NT) {
    const int a = assign[i];
    if (a >= 0 && a < K) atomicAdd(line + a, 1);
    else ++out;
  }
  if (out) atomicAdd(outside, out);
}

__global__ __launch_bounds__(NT) void group_starts(int* __restrict__ table, int nb, int K, int* __restrict__ counts) {
  const long c = (long)blockIdx.x * NT + threadIdx.x;
  if (c >= K) return;
  int run = 0;
  for (int b = 0; b < nb; ++b) {
    const int t = table[(long)b * K + c];
    table[(long)b * K + c] = run;
    run += t;
  }
  counts[c] = run;
}

// out[0 .. K] = exclusive scan of (counts[c] + add) / div, one workgroup: offsets (add 0, div 1) and piece starts (add PIECE - 1, div PIECE)
__global__ __launch_bounds__(1024) void scan_counts(const int* __restrict__ counts, int K, int add, int div, long* __restrict__ out) {
  __shared__ long part[1024];
  const int tid = threadIdx.x;
  const long per = ((long)K + 1023) / 1024, lo = min((long)K, tid * per), hi = min((long)K, lo + per);
  long s = 0;
  for (long c = lo; c < hi; ++c) s += (counts[c] + add) / div;
  part[tid] = s;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const long v = tid >= o ? part[tid - o] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  long run = part[tid] - s;
  for (long c = lo; c < hi; ++c) {
    out[c] = run;
    run += (counts[c] + add) / div;
  }
  if (tid == 1023) out[K] = part[1023];
}

__global__ __launch_bounds__(NT) void group_place(const int* __restrict__ assign, long n, int K, long rb, int* table,
                                                  const long* __restrict__ offsets, int* __restrict__ members) {
  __shared__ int al[NT];
  const int tid = threadIdx.x;
  const long lo = (long)blockIdx.x * rb, hi = min(n, lo + rb);
  int* line = table + (long)blockIdx.x * K;
  for (long t0 = lo; t0 < hi; t0 += NT) {
    const long i = t0 + tid;
    int a = -1;
    if (i < hi) {
      a = assign[i];
      if (a < 0 || a >= K) a = -1;
    }
    al[tid] = a;
    const int start = a >= 0 ? line[a] : 0;                                 // read by every row of the cluster before the barrier, moved on after it
    __syncthreads();
    int before = 0, all = 0;
    if (a >= 0) {
      for (int j = 0; j < NT; ++j) {
        const int same = al[j] == a;
        all += same;
        before += same & (j < tid);
      }
      members[offsets[a] + start + before] = (int)i;
      if (before == all - 1) line[a] = start + all;                         // (the cluster's last row of the tile)
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------------------------ centroids
// workgroup j: piece j of the piece list (pstart[c] <= j < pstart[c + 1] -> cluster c); sums[j] = its rows' sum, pmed[j] = its medoid key
__global__ __launch_bounds__(NT) void centroid_pieces(const float* __restrict__ f, long ldf, int E, const int* __restrict__ members,
                                                      const long* __restrict__ offsets, const long* __restrict__ pstart, int K,
                                                      const float* __restrict__ best, float* __restrict__ sums,
                                                      uint64_t* __restrict__ pmed) {
  __shared__ int ml[PIECE];
  __shared__ uint64_t kl[NT];
  const long j = blockIdx.x;
  if (j >= pstart[K]) return;                                               // (uniform)
  int lo = 0, hi = K;                                                       // the last c with pstart[c] <= j
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    if (pstart[mid] <= j) lo = mid; else hi = mid;
  }
  const int cl = lo, tid = threadIdx.x;
  const long m0 = offsets[cl] + (j - pstart[cl]) * PIECE;
  const int cnt = (int)min((long)PIECE, offsets[cl + 1] - m0);
  uint64_t key = 0;
  if (tid < cnt) {
    const int row = members[m0 + tid];
    ml[tid] = row;
    key = (((uint64_t)score_key(best[row]) + 1) << 31) | (0x7fffffffu - (uint32_t)row);   // (+ 1: a NaN member still beats "no member")
  }
  kl[tid] = key;
  __syncthreads();
  for (int o = NT / 2; o > 0; o >>= 1) {
    if (tid < o) kl[tid] = kl[tid + o] > kl[tid] ? kl[tid + o] : kl[tid];
    __syncthreads();
  }
  if (tid == 0) pmed[j] = kl[0];
  for (int e = tid; e < E; e += NT) {
    float s = 0.f;
    int i = 0;
    for (; i + 4 <= cnt; i += 4) {
      const float v0 = f[(long)ml[i] * ldf + e], v1 = f[(long)ml[i + 1] * ldf + e], v2 = f[(long)ml[i + 2] * ldf + e],
                  v3 = f[(long)ml[i + 3] * ldf + e];
      s = ((s + v0) + v1) + v2;
      s += v3;
    }
    for (; i < cnt; ++i) s += f[(long)ml[i] * ldf + e];
    sums[j * E + e] = s;
  }
}

__global__ __launch_bounds__(NT) void centroid_finish(const float* __restrict__ sums, const uint64_t* __restrict__ pmed,
                                                      const long* __restrict__ pstart, const int* __restrict__ counts, int E,
                                                      float* __restrict__ centres, long ldc, float* __restrict__ norm,
                                                      int* __restrict__ medoid) {
  __shared__ float sq[512];
  const int cl = blockIdx.x, tid = threadIdx.x;
  const long p0 = pstart[cl], p1 = pstart[cl + 1];
  float s[2] = {0.f, 0.f};
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int e = tid + u * NT;
    if (e < E)
      for (long p = p0; p < p1; ++p) s[u] += sums[p * E + e];
    sq[e] = e < E ? s[u] * s[u] : 0.f;
  }
  __syncthreads();
  for (int o = 256; o > 0; o >>= 1) {                                       // a fixed tree over 512 slots, whatever E is
    if (tid < o) sq[tid] += sq[tid + o];
    __syncthreads();
  }
  const float nr = sqrtf(sq[0]);
  if (tid == 0) {
    norm[cl] = nr;
    uint64_t m = 0;
    for (long p = p0; p < p1; ++p) m = pmed[p] > m ? pmed[p] : m;
    medoid[cl] = m == 0 ? -1 : (int)(0x7fffffffu - (uint32_t)(m & 0x7fffffffu));
  }
  if (counts[cl] > 0 && nr >= 1e-12f) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int e = tid + u * NT;
      if (e < E) centres[(long)cl * ldc + e] = s[u] / nr;
    }
  }
}

inline int group_blocks(long n, int K) {
  long nb = (n + 1023) / 1024, cap = GROUP_TABLE / K;
  if (nb > cap) nb = cap;
  return nb < 1 ? 1 : (int)nb;
}
inline long pieces_max(long n, int K) { return n / PIECE + K; }            // sum over clusters of ceil(count / PIECE), at the most
inline long align16(long b) { return (b + 15) & ~15L; }

}  // namespace

extern "C" int spmm_centroid_assign(const float* f, long ldf, const float* c, long ldc, long c0, long n, int Kc, int E, float* best, int* assign,
                                    int merge, const int* prev, int* changed, spmm_stream_t stream) {
  if (int e = check_width("spmm_centroid_assign", E)) return e;
  SPMM_CHECK_SHAPE(Kc >= 1, "spmm_centroid_assign: Kc=%d must be at least 1", Kc);
  SPMM_CHECK_SHAPE(c0 >= 0 && c0 + Kc <= 0x7fffffffL, "spmm_centroid_assign: c0=%ld with Kc=%d must keep centre indices in [0, 2^31 - 1)", c0, Kc);
  if (int e = check_rows("spmm_centroid_assign", n)) return e;
  SPMM_CHECK_SHAPE(merge == 0 || merge == 1, "spmm_centroid_assign: merge=%d must be 0 or 1", merge);
  SPMM_CHECK_SHAPE((prev == nullptr) == (changed == nullptr), "spmm_centroid_assign: prev and changed come together");
  SPMM_CHECK_SHAPE(aligned(prev, 4) && aligned(changed, 4), "spmm_centroid_assign: misaligned prev / changed (4 bytes)");
  if (n == 0) return SPMM_OK;
  SPMM_CHECK_SHAPE(best && assign, "spmm_centroid_assign: null best / assign (the state)");
  SPMM_CHECK_SHAPE(aligned(best, 4) && aligned(assign, 4), "spmm_centroid_assign: misaligned best / assign (4 bytes)");
  if (int e = check_operands("spmm_centroid_assign", f, ldf, c, ldc, E)) return e;
  dispatch_width(E, [&](auto e64) {
    constexpr int E64 = decltype(e64)::value, AR = Shape<E64>::AR;
    hipLaunchKernelGGL(centroid_assign<E64>, dim3((unsigned)((n + AR - 1) / AR)), dim3(Shape<E64>::NT), 0, stream, f, ldf, c, ldc, (int)c0, (int)n,
                       Kc, merge, best, assign, prev, changed);
  });
  SPMM_LAUNCH_CHECK("spmm_centroid_assign");
  return SPMM_OK;
}

extern "C" long spmm_cluster_group_workspace_bytes(long n, int K) {
  if (n < 0 || K < 1 || K > GROUP_TABLE) return 0;
  return align16((long)group_blocks(n, K) * K * 4);
}

extern "C" int spmm_cluster_group(const int* assign, long n, int K, int* counts, long* offsets, int* members, int* outside, void* workspace,
                                  long workspace_bytes, spmm_stream_t stream) {
  SPMM_CHECK_SHAPE(K >= 1 && K <= GROUP_TABLE, "spmm_cluster_group: K=%d must be in [1, 2^24]", K);
  SPMM_CHECK_SHAPE(n >= 0 && n <= 0x7fffff00L, "spmm_cluster_group: n=%ld must be in [0, 2^31 - 256] rows", n);
  SPMM_CHECK_SHAPE(counts && offsets && outside, "spmm_cluster_group: null counts / offsets / outside");
  SPMM_CHECK_SHAPE(aligned(counts, 4) && aligned(offsets, 8) && aligned(outside, 4),
                   "spmm_cluster_group: misaligned counts / offsets / outside (4 / 8 / 4 bytes)");
  SPMM_CHECK_SHAPE(n == 0 || (assign && members), "spmm_cluster_group: null assign / members");
  SPMM_CHECK_SHAPE(aligned(assign, 4) && aligned(members, 4), "spmm_cluster_group: misaligned assign / members (4 bytes)");
  const int nb = group_blocks(n, K);
  const long need = align16((long)nb * K * 4);
  SPMM_CHECK_SHAPE(workspace && aligned(workspace, 16) && workspace_bytes >= need,
                   "spmm_cluster_group: workspace of %ld bytes (16-byte aligned) needed, %ld given (spmm_cluster_group_workspace_bytes)", need,
                   workspace ? workspace_bytes : 0L);
  int* table = reinterpret_cast<int*>(workspace);
  long rb = (n + nb - 1) / nb;
  rb = (rb + NT - 1) / NT * NT;
  if (rb < NT) rb = NT;
  if (hipMemsetAsync(table, 0, (size_t)nb * K * 4, stream) != hipSuccess || hipMemsetAsync(outside, 0, 4, stream) != hipSuccess) {
    spmm_set_error("spmm_cluster_group: launch failed: clearing the workspace");
    return SPMM_ERR_LAUNCH;
  }
  if (n > 0) {
    hipLaunchKernelGGL(group_count, dim3(nb), dim3(NT), 0, stream, assign, n, K, rb, table, outside);
    SPMM_LAUNCH_CHECK("spmm_cluster_group (count)");
  }
  hipLaunchKernelGGL(group_starts, dim3((K + NT - 1) / NT), dim3(NT), 0, stream, table, nb, K, counts);
  SPMM_LAUNCH_CHECK("spmm_cluster_group (starts)");
  hipLaunchKernelGGL(scan_counts, dim3(1), dim3(1024), 0, stream, counts, K, 0, 1, offsets);
  SPMM_LAUNCH_CHECK("spmm_cluster_group (offsets)");
  if (n > 0) {
    hipLaunchKernelGGL(group_place, dim3(nb), dim3(NT), 0, stream, assign, n, K, rb, table, offsets, members);
    SPMM_LAUNCH_CHECK("spmm_cluster_group (place)");
  }
  return SPMM_OK;
}

extern "C" long spmm_cluster_centroids_workspace_bytes(long n, int K, int E) {
  if (n < 0 || K < 1 || E < 1) return 0;
  const long p = pieces_max(n, K);
  return align16(((long)K + 1) * 8) + align16(p * 8) + align16(p * E * 4);
}

extern "C" int spmm_cluster_centroids(const float* f, long ldf, long n, int E, const float* best, const int* counts, const long* offsets,
                                      const int* members, int K, float* centres, long ldc, float* norm, int* medoid, void* workspace,
                                      long workspace_bytes, spmm_stream_t stream) {
  SPMM_CHECK_SHAPE(E >= 1 && E <= 512, "spmm_cluster_centroids: E=%d must be in [1, 512]", E);
  SPMM_CHECK_SHAPE(K >= 1 && K <= GROUP_TABLE, "spmm_cluster_centroids: K=%d must be in [1, 2^24]", K);
  SPMM_CHECK_SHAPE(n >= 0 && n <= 0x7fffff00L, "spmm_cluster_centroids: n=%ld must be in [0, 2^31 - 256] rows", n);
  SPMM_CHECK_SHAPE(counts && offsets && centres && norm && medoid, "spmm_cluster_centroids: null counts / offsets / centres / norm / medoid");
  SPMM_CHECK_SHAPE(n == 0 || (f && best && members), "spmm_cluster_centroids: null f / best / members");
  SPMM_CHECK_SHAPE(ldc >= E && (n == 0 || ldf >= E), "spmm_cluster_centroids: ldf=%ld ldc=%ld must be at least E=%d", ldf, ldc, E);
  SPMM_CHECK_SHAPE(aligned(f, 4) && aligned(best, 4) && aligned(counts, 4) && aligned(offsets, 8) && aligned(members, 4) && aligned(centres, 4) &&
                       aligned(norm, 4) && aligned(medoid, 4),
                   "spmm_cluster_centroids: misaligned pointer (offsets 8 bytes, the others 4)");
  const long p = pieces_max(n, K);
  const long need = align16(((long)K + 1) * 8) + align16(p * 8) + align16(p * E * 4);
  SPMM_CHECK_SHAPE(workspace && aligned(workspace, 16) && workspace_bytes >= need,
                   "spmm_cluster_centroids: workspace of %ld bytes (16-byte aligned) needed, %ld given (spmm_cluster_centroids_workspace_bytes)",
                   need, workspace ? workspace_bytes : 0L);
  char* ws = reinterpret_cast<char*>(workspace);
  long* pstart = reinterpret_cast<long*>(ws);
  uint64_t* pmed = reinterpret_cast<uint64_t*>(ws + align16(((long)K + 1) * 8));
  float* sums = reinterpret_cast<float*>(ws + align16(((long)K + 1) * 8) + align16(p * 8));
  hipLaunchKernelGGL(scan_counts, dim3(1), dim3(1024), 0, stream, counts, K, PIECE - 1, PIECE, pstart);
  SPMM_LAUNCH_CHECK("spmm_cluster_centroids (pieces)");
  if (n > 0) {
    hipLaunchKernelGGL(centroid_pieces, dim3((unsigned)p), dim3(NT), 0, stream, f, ldf, E, members, offsets, pstart, K, best, sums, pmed);
    SPMM_LAUNCH_CHECK("spmm_cluster_centroids (sums)");
  }
  hipLaunchKernelGGL(centroid_finish, dim3(K), dim3(NT), 0, stream, sums, pmed, pstart, counts, E, centres, ldc, norm, medoid);
  SPMM_LAUNCH_CHECK("spmm_cluster_centroids (finish)");
  return SPMM_OK;
}
