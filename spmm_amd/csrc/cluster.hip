// Library clustering: nearest centre of every row (spmm_centroid_assign), members of every cluster (spmm_cluster_group) and the clusters'
// centres, norms and medoids (spmm_cluster_centroids); include/spmm_hip.h.
//
// centroid_assign.  The arithmetic of retrieval (csrc/retrieve.hip) with the roles swapped: many rows, few centres.  A workgroup owns
// AR = 128 rows -- each of its four waves two MFMA blocks of 16 -- and keeps them in REGISTERS for the whole launch (2 x E / 4 per lane); the
// centres go through LDS once per workgroup in tiles of 32 (E = 512: 16), the next tile's global loads in flight under the current tile's MFMAs.
// The 16 x 16 scores of (centre block, row block) never leave the accumulators: D's column (lane & 15) is the row, its rows 4 g + r the
// centres, so every lane folds its four scores into a running best of its own -- one 64-bit key per row block -- and the four lane groups
// of a row are combined once, after the last tile.  No score tile, no per-row list, no workspace.
//
// Same bits as spmm_sim_topk(q = rows, f = centres, k = 1).  The score of (row, centre) is one accumulator's chain of
// v_mfma_f32_16x16x4_f32: lane (c, g) feeds elements 16 kb + 4 g .. + 3 of its centre (A, from LDS) and of its row (B, registers), component
// m to the m-th of four MFMAs -- kb ascending, then m, then the k slot g, retrieve.hip's order; a product does not know which factor was A.
// Candidates are (score, centre index) under that kernel's total order (larger score, then lower index; NaN below every number; -0 = +0;
// an empty state below everything), as one integer key: the best of a set does not depend on how the set was cut into lanes, tiles or
// chunks.
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
#include "common.h"
#include "../../include/spmm_hip.h"

namespace {

constexpr int NT = 256;
constexpr int AR = 128;          // rows of an assign workgroup: 4 waves x NB blocks of 16
constexpr int NB = 2;            // row blocks of a wave
constexpr int PIECE = 256;       // members of one partial centroid sum
constexpr long GROUP_TABLE = 1L << 24;      // entries of cluster_group's [nb, K] table at the most

// Monotonic image of a score (retrieve.hip): larger float <-> larger key; -0 = +0; NaN -> 0, below -inf's image.
__device__ __forceinline__ uint32_t score_key(float s) {
  if (s != s) return 0u;
  if (s == 0.0f) s = 0.0f;
  const uint32_t u = __float_as_uint(s);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_score(uint32_t k) {
  if (k == 0u) return __uint_as_float(0x7fc00000u);
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}
// candidate (score, centre index < 2^31) as one key: a larger key is a better candidate, 0 is the empty slot
__device__ __forceinline__ uint64_t cand_key(float s, uint32_t idx) { return ((uint64_t)score_key(s) << 32) | (0xffffffffu - idx); }
__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int m) {
  const uint32_t lo = __shfl_xor((uint32_t)v, m, 64), hi = __shfl_xor((uint32_t)(v >> 32), m, 64);
  return ((uint64_t)hi << 32) | lo;
}

// ------------------------------------------------------------------------------------------------------------------ assign
template <int E64>
__global__ __launch_bounds__(NT) void centroid_assign(const float* __restrict__ f, long ldf, const float* __restrict__ cen, long ldc, int c0,
                                                      int n, int Kc, int merge, float* __restrict__ best, int* __restrict__ assign,
                                                      const int* __restrict__ prev, int* __restrict__ changed) {
  constexpr int E = 64 * E64, EP = E + 4, KB = E / 16;
  constexpr int CB = E64 < 8 ? 2 : 1, CT = 16 * CB;                        // centre blocks of an LDS tile (E = 512: one, the tile stays under 64 KiB)
  constexpr int LD4 = CT * (E / 4) / NT;                                   // 16-byte loads of a thread per centre tile
  __shared__ __attribute__((aligned(16))) float cl[CT * EP];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const long row0 = (long)blockIdx.x * AR + w * (NB * 16);
  f32x4 rows[NB][KB];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const long row = min(row0 + b * 16 + c, (long)n - 1);                   // rows past the end: a valid address, never written back
    const float* fp = f + row * ldf + g * 4;
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) rows[b][kb] = *reinterpret_cast<const f32x4*>(fp + kb * 16);
  }
  uint64_t mine[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) mine[b] = 0;
  f32x4 pre[LD4];
  auto fetch = [&](int t) {
#pragma unroll
    for (int i = 0; i < LD4; ++i) {
      const int e = tid + i * NT, r = e / (E / 4), e4 = e % (E / 4);
      const int j = min(t * CT + r, Kc - 1);                                // centres past the chunk: a valid address, dropped below
      pre[i] = *reinterpret_cast<const f32x4*>(cen + (long)j * ldc + e4 * 4);
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int i = 0; i < LD4; ++i) {
      const int e = tid + i * NT, r = e / (E / 4), e4 = e % (E / 4);
      *reinterpret_cast<f32x4*>(cl + r * EP + e4 * 4) = pre[i];
    }
  };
  const int tiles = (Kc + CT - 1) / CT;
  fetch(0);
  stage();
  __syncthreads();
  for (int t = 0; t < tiles; ++t) {
    if (t + 1 < tiles) fetch(t + 1);
    f32x4 acc[CB][NB];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
      for (int b = 0; b < NB; ++b) acc[cb][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* ap = cl + c * EP + g * 4;
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
      f32x4 a[CB];
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) a[cb] = *reinterpret_cast<const f32x4*>(ap + cb * 16 * EP + kb * 16);
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
#pragma unroll
          for (int b = 0; b < NB; ++b) acc[cb][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[cb][m], rows[b][kb][m], acc[cb][b], 0, 0, 0);
    }
    // D: column (lane & 15) = row of the block, row 4 g + r = centre of the block; the key carries the index, so `>` keeps the lowest of equals
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
    __syncthreads();
    if (t + 1 < tiles) {
      stage();
      __syncthreads();
    }
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
      const int ia = m == 0 ? -1 : (int)(0xffffffffu - (uint32_t)m);
      best[row] = m == 0 ? -__builtin_huge_valf() : key_score((uint32_t)(m >> 32));
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

template <int E64>
void launch_assign(const float* f, long ldf, const float* c, long ldc, int c0, long n, int Kc, int merge, float* best, int* assign,
                   const int* prev, int* changed, hipStream_t stream) {
  hipLaunchKernelGGL(centroid_assign<E64>, dim3((unsigned)((n + AR - 1) / AR)), dim3(NT), 0, stream, f, ldf, c, ldc, c0, (int)n, Kc, merge, best,
                     assign, prev, changed);
}

}  // namespace

extern "C" int spmm_centroid_assign(const float* f, long ldf, const float* c, long ldc, long c0, long n, int Kc, int E, float* best, int* assign,
                                    int merge, const int* prev, int* changed, spmm_stream_t stream) {
  SPMM_CHECK_SHAPE(E >= 64 && E <= 512 && E % 64 == 0, "spmm_centroid_assign: E=%d must be a multiple of 64 up to 512", E);
  SPMM_CHECK_SHAPE(Kc >= 1, "spmm_centroid_assign: Kc=%d must be at least 1", Kc);
  SPMM_CHECK_SHAPE(c0 >= 0 && c0 + Kc <= 0x7fffffffL, "spmm_centroid_assign: c0=%ld with Kc=%d must keep centre indices in [0, 2^31 - 1)", c0, Kc);
  SPMM_CHECK_SHAPE(n >= 0 && n <= 0x7fffff00L, "spmm_centroid_assign: n=%ld must be in [0, 2^31 - 256] rows", n);
  SPMM_CHECK_SHAPE(merge == 0 || merge == 1, "spmm_centroid_assign: merge=%d must be 0 or 1", merge);
  SPMM_CHECK_SHAPE((prev == nullptr) == (changed == nullptr), "spmm_centroid_assign: prev and changed come together");
  SPMM_CHECK_SHAPE((reinterpret_cast<uintptr_t>(prev) & 3) == 0 && (reinterpret_cast<uintptr_t>(changed) & 3) == 0,
                   "spmm_centroid_assign: misaligned prev / changed (4 bytes)");
  if (n == 0) return SPMM_OK;
  SPMM_CHECK_SHAPE(best && assign, "spmm_centroid_assign: null best / assign (the state)");
  SPMM_CHECK_SHAPE((reinterpret_cast<uintptr_t>(best) & 3) == 0 && (reinterpret_cast<uintptr_t>(assign) & 3) == 0,
                   "spmm_centroid_assign: misaligned best / assign (4 bytes)");
  SPMM_CHECK_SHAPE(f && c, "spmm_centroid_assign: null f / c");
  SPMM_CHECK_SHAPE((reinterpret_cast<uintptr_t>(f) & 15) == 0 && (reinterpret_cast<uintptr_t>(c) & 15) == 0,
                   "spmm_centroid_assign: f / c must be 16-byte aligned");
  SPMM_CHECK_SHAPE(ldf >= E && ldf % 4 == 0 && ldc >= E && ldc % 4 == 0,
                   "spmm_centroid_assign: ldf=%ld ldc=%ld must be multiples of 4, at least E=%d", ldf, ldc, E);
  switch (E / 64) {
    case 1: launch_assign<1>(f, ldf, c, ldc, (int)c0, n, Kc, merge, best, assign, prev, changed, stream); break;
    case 2: launch_assign<2>(f, ldf, c, ldc, (int)c0, n, Kc, merge, best, assign, prev, changed, stream); break;
    case 3: launch_assign<3>(f, ldf, c, ldc, (int)c0, n, Kc, merge, best, assign, prev, changed, stream); break;
    case 4: launch_assign<4>(f, ldf, c, ldc, (int)c0, n, Kc, merge, best, assign, prev, changed, stream); break;
    case 5: launch_assign<5>(f, ldf, c, ldc, (int)c0, n, Kc, merge, best, assign, prev, changed, stream); break;
    case 6: launch_assign<6>(f, ldf, c, ldc, (int)c0, n, Kc, merge, best, assign, prev, changed, stream); break;
    case 7: launch_assign<7>(f, ldf, c, ldc, (int)c0, n, Kc, merge, best, assign, prev, changed, stream); break;
    default: launch_assign<8>(f, ldf, c, ldc, (int)c0, n, Kc, merge, best, assign, prev, changed, stream); break;
  }
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
  SPMM_CHECK_SHAPE((reinterpret_cast<uintptr_t>(counts) & 3) == 0 && (reinterpret_cast<uintptr_t>(offsets) & 7) == 0 &&
                       (reinterpret_cast<uintptr_t>(outside) & 3) == 0,
                   "spmm_cluster_group: misaligned counts / offsets / outside (4 / 8 / 4 bytes)");
  SPMM_CHECK_SHAPE(n == 0 || (assign && members), "spmm_cluster_group: null assign / members");
  SPMM_CHECK_SHAPE((reinterpret_cast<uintptr_t>(assign) & 3) == 0 && (reinterpret_cast<uintptr_t>(members) & 3) == 0,
                   "spmm_cluster_group: misaligned assign / members (4 bytes)");
  const int nb = group_blocks(n, K);
  const long need = align16((long)nb * K * 4);
  SPMM_CHECK_SHAPE(workspace && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0 && workspace_bytes >= need,
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
  SPMM_CHECK_SHAPE((reinterpret_cast<uintptr_t>(f) & 3) == 0 && (reinterpret_cast<uintptr_t>(best) & 3) == 0 &&
                       (reinterpret_cast<uintptr_t>(counts) & 3) == 0 && (reinterpret_cast<uintptr_t>(offsets) & 7) == 0 &&
                       (reinterpret_cast<uintptr_t>(members) & 3) == 0 && (reinterpret_cast<uintptr_t>(centres) & 3) == 0 &&
                       (reinterpret_cast<uintptr_t>(norm) & 3) == 0 && (reinterpret_cast<uintptr_t>(medoid) & 3) == 0,
                   "spmm_cluster_centroids: misaligned pointer (offsets 8 bytes, the others 4)");
  const long p = pieces_max(n, K);
  const long need = align16(((long)K + 1) * 8) + align16(p * 8) + align16(p * E * 4);
  SPMM_CHECK_SHAPE(workspace && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0 && workspace_bytes >= need,
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
