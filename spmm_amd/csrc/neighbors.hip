// Threshold clustering: every row's neighbours above a similarity threshold (spmm_sim_range) and the leaders of a neighbour list -- Taylor-
// Butina / first-come sphere exclusion (spmm_leader_round, spmm_leader_finish); include/spmm_hip.h.
//
// sim_range.  csrc/cluster.hip's centroid_assign with the library on both sides: the row-stationary scan of csrc/sim_scan.h, whose chain
// gives a pair spmm_sim_topk's bits and score(i, j) score(j, i)'s.
//
// Ordered emission without atomics or a sort.  A row of a wave's block lives in the four lanes (c, g = 0 .. 3); nobody else writes its
// list.  Within a tile the column index ascends with (column block cb, lane group g, accumulator row r), so a lane's hits of one (cb, row
// block) are four bits, and the whole tile's are CB x NB x 4 <= 16 bits of one register.  Three shuffles (xor 16, 32, 48) hand every lane
// the other three groups' bits; a hit's place in the row's list is the row's running count + the hits of the lower groups of the same cb +
// the lower bits of its own four -- popcounts.  Every lane of a row advances the same running count by the same total, so the count is
// never exchanged again.  Tiles ascend, chunks are offered in ascending c0: the list ascends, whatever the chunking.
//
// leader_round / leader_finish.  One wave64 per row, its lanes striding the row's list (a row with 10^5 neighbours is 1 600 steps of a
// wave, not one thread's loop).  A round reads state_in only and writes state_out only; the open rows are counted with one integer atomic
// per wave.  No floating-point atomics anywhere.
#include "sim_scan.h"
#include "../../include/spmm_hip.h"

namespace {

using namespace sim_scan;

constexpr int NT = 256;
constexpr int WR = 4;            // rows (waves) of a leader workgroup

// ------------------------------------------------------------------------------------------------------------------ sim_range
template <int E64, bool EMIT>
__global__ __launch_bounds__(Shape<E64>::NT) void sim_range(const float* __restrict__ f, long ldf, int r0, int n, const float* __restrict__ col,
                                                            long ldc, int c0, int nc, float threshold, int* __restrict__ counts,
                                                            const long* __restrict__ offsets, int* __restrict__ nbr, long nbr_len) {
  using S = Shape<E64>;
  constexpr int AR = S::AR, NB = S::NB, CB = S::CB, CT = S::CT;
  __shared__ __attribute__((aligned(16))) float cl[CT * S::EP];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const long row0 = (long)blockIdx.x * AR + w * (NB * 16);
  f32x4 rows[NB][S::KB];
  int run[NB], self[NB];                                                    // hits so far (state included); the row's own library index, -1 past the end
  long at[NB];                                                              // where the row's list starts in nbr
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const long rr = row0 + b * 16 + c;
    const long row = load_row_block<E64>(f, ldf, rr, n, g, rows[b]);        // (rows past the end are never counted or written)
    run[b] = counts[row];
    self[b] = rr < n ? r0 + (int)rr : -1;
    at[b] = EMIT ? offsets[row] : 0;
  }
  RowScan<E64> scan(col, ldc, nc, cl);
  for (int t = 0; t < scan.tiles; ++t) {
    f32x4 acc[CB][NB];
    scan.scores(t, rows, acc);
    // Bit (b * CB + cb) * 4 + r of `mine`: that pair is a hit.
    uint32_t mine = 0;
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = t * CT + cb * 16 + g * 4 + r;
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          const bool hit = acc[cb][b][r] >= threshold && j < nc && self[b] >= 0 && (uint32_t)self[b] != (uint32_t)c0 + (uint32_t)j;      // (NaN >= t is false)
          mine |= (uint32_t)hit << ((b * CB + cb) * 4 + r);
        }
      }
    if (__ballot(mine != 0)) {                                              // (wave-uniform: most tiles of a sparse relation have no hit)
      uint32_t grp[4];                                                      // grp[x]: the bits of lane group g ^ x
      grp[0] = mine;
#pragma unroll
      for (int x = 1; x < 4; ++x) grp[x] = __shfl_xor(mine, 16 * x, 64);
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) {
          const int sh = (b * CB + cb) * 4;
          int below = 0, all = 0;
#pragma unroll
          for (int x = 0; x < 4; ++x) {
            const int p = __popc((grp[x] >> sh) & 15u);
            all += p;
            below += (g ^ x) < g ? p : 0;
          }
          if (EMIT) {
            const uint32_t h = (mine >> sh) & 15u;
            const int j0 = c0 + t * CT + cb * 16 + g * 4;
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (h & (1u << r)) {
                const long pos = at[b] + run[b] + below + __popc(h & ((1u << r) - 1u));
                if (pos >= 0 && pos < nbr_len) nbr[pos] = j0 + r;
              }
          }
          run[b] += all;
        }
    }
    scan.next(t);
  }
#pragma unroll
  for (int b = 0; b < NB; ++b)
    if (g == 0 && self[b] >= 0) counts[row0 + b * 16 + c] = run[b];
}

// ------------------------------------------------------------------------------------------------------------------ leaders
// Does row j come before row i?  by_count: more neighbours first, equal counts to the lower row; else the lower row first.
__device__ __forceinline__ bool before(int j, int cj, int i, int ci) { return cj > ci || (cj == ci && j < i); }

__global__ __launch_bounds__(NT) void leader_round(const int* __restrict__ counts, const long* __restrict__ offsets, const int* __restrict__ nbr,
                                                   long nbr_len, long n, int by_count, const int* __restrict__ state_in, int* __restrict__ state_out,
                                                   int* __restrict__ open_out) {
  const int lane = threadIdx.x & 63;
  const long i = (long)blockIdx.x * WR + (threadIdx.x >> 6);
  if (i >= n) return;                                                       // (wave-uniform)
  const int s = state_in[i];
  if (s != 0) {
    if (lane == 0) state_out[i] = s;
    return;
  }
  const int ci = by_count ? counts[i] : 0;
  const long lo = max(offsets[i], 0L), hi = min(offsets[i + 1], nbr_len);      // (a wrong offsets never reads outside nbr)
  int leader = 0, open = 0;
  for (long p = lo + lane; p < hi; p += 64) {
    const int j = nbr[p];
    if (j < 0 || j >= n) continue;                                          // (not a row: never followed)
    const int cj = by_count ? counts[j] : 0;
    if (!before(j, cj, (int)i, ci)) continue;
    const int sj = state_in[j];
    leader |= sj == 1;
    open |= sj == 0;
  }
  const bool any_leader = __ballot(leader) != 0, any_open = __ballot(open) != 0;
  const int out = any_leader ? 2 : (any_open ? 0 : 1);
  if (lane == 0) {
    state_out[i] = out;
    if (out == 0) atomicAdd(open_out, 1);
  }
}

__global__ __launch_bounds__(NT) void leader_finish(const int* __restrict__ counts, const long* __restrict__ offsets, const int* __restrict__ nbr,
                                                    long nbr_len, long n, int by_count, const int* __restrict__ state,
                                                    int* __restrict__ leader) {
  const int lane = threadIdx.x & 63;
  const long i = (long)blockIdx.x * WR + (threadIdx.x >> 6);
  if (i >= n) return;                                                       // (wave-uniform)
  if (state[i] == 1) {
    if (lane == 0) leader[i] = (int)i;
    return;
  }
  // the first leader of the list in priority order as the largest key: (count, -row); a row index keeps the low word above 0
  uint64_t best = 0;
  const long lo = max(offsets[i], 0L), hi = min(offsets[i + 1], nbr_len);
  for (long p = lo + lane; p < hi; p += 64) {
    const int j = nbr[p];
    if (j < 0 || j >= n || state[j] != 1) continue;
    const uint64_t key = ((uint64_t)(uint32_t)(by_count ? counts[j] : 0) << 32) | (0xffffffffu - (uint32_t)j);
    best = key > best ? key : best;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t other = shfl_xor64(best, o);
    best = other > best ? other : best;
  }
  if (lane == 0) leader[i] = best == 0 ? -1 : (int)(0xffffffffu - (uint32_t)best);
}

}  // namespace

extern "C" int spmm_sim_range(const float* f, long ldf, long r0, long n, const float* c, long ldc, long c0, long nc, int E, float threshold,
                              int* counts, const long* offsets, int* nbr, long nbr_len, spmm_stream_t stream) {
  if (int e = check_width("spmm_sim_range", E)) return e;
  if (int e = check_rows("spmm_sim_range", n)) return e;
  SPMM_CHECK_SHAPE(nc >= 0 && nc <= 0x7fffff00L, "spmm_sim_range: nc=%ld must be in [0, 2^31 - 256] columns per chunk", nc);
  SPMM_CHECK_SHAPE(r0 >= 0 && r0 + n <= 0x7fffffffL, "spmm_sim_range: r0=%ld with n=%ld must keep row indices in [0, 2^31 - 1)", r0, n);
  SPMM_CHECK_SHAPE(c0 >= 0 && c0 + nc <= 0x7fffffffL, "spmm_sim_range: c0=%ld with nc=%ld must keep column indices in [0, 2^31 - 1)", c0, nc);
  SPMM_CHECK_SHAPE(threshold == threshold, "spmm_sim_range: threshold is NaN");
  SPMM_CHECK_SHAPE(nbr_len >= 0, "spmm_sim_range: nbr_len=%ld must be at least 0", nbr_len);
  SPMM_CHECK_SHAPE((offsets == nullptr) == (nbr == nullptr) && (nbr != nullptr || nbr_len == 0),
                   "spmm_sim_range: offsets, nbr and nbr_len come together (all three to emit, none to count)");
  SPMM_CHECK_SHAPE(aligned(offsets, 8) && aligned(nbr, 4), "spmm_sim_range: misaligned offsets / nbr (8 / 4 bytes)");
  if (n == 0 || nc == 0) return SPMM_OK;
  SPMM_CHECK_SHAPE(counts, "spmm_sim_range: null counts (the state)");
  SPMM_CHECK_SHAPE(aligned(counts, 4), "spmm_sim_range: misaligned counts (4 bytes)");
  if (int e = check_operands("spmm_sim_range", f, ldf, c, ldc, E)) return e;
  dispatch_width(E, [&](auto e64) {
    constexpr int E64 = decltype(e64)::value, AR = Shape<E64>::AR;
    const dim3 grid((unsigned)((n + AR - 1) / AR)), block(Shape<E64>::NT);
    if (nbr != nullptr)
      hipLaunchKernelGGL((sim_range<E64, true>), grid, block, 0, stream, f, ldf, (int)r0, (int)n, c, ldc, (int)c0, (int)nc, threshold, counts,
                         offsets, nbr, nbr_len);
    else
      hipLaunchKernelGGL((sim_range<E64, false>), grid, block, 0, stream, f, ldf, (int)r0, (int)n, c, ldc, (int)c0, (int)nc, threshold, counts,
                         offsets, nbr, nbr_len);
  });
  SPMM_LAUNCH_CHECK("spmm_sim_range");
  return SPMM_OK;
}

extern "C" int spmm_leader_round(const int* counts, const long* offsets, const int* nbr, long nbr_len, long n, int by_count, const int* state_in,
                                 int* state_out, int* open_out, spmm_stream_t stream) {
  SPMM_CHECK_SHAPE(n >= 0 && n <= 0x7fffff00L, "spmm_leader_round: n=%ld must be in [0, 2^31 - 256] rows", n);
  SPMM_CHECK_SHAPE(nbr_len >= 0, "spmm_leader_round: nbr_len=%ld must be at least 0", nbr_len);
  SPMM_CHECK_SHAPE(by_count == 0 || by_count == 1, "spmm_leader_round: by_count=%d must be 0 or 1", by_count);
  SPMM_CHECK_SHAPE(by_count == 0 || counts, "spmm_leader_round: null counts with by_count=1");
  SPMM_CHECK_SHAPE(offsets && nbr && state_in && state_out && open_out, "spmm_leader_round: null offsets / nbr / state_in / state_out / open_out");
  SPMM_CHECK_SHAPE(state_in != state_out, "spmm_leader_round: state_in and state_out must be two buffers (a round reads the one, writes the other)");
  SPMM_CHECK_SHAPE(aligned(counts, 4) && aligned(offsets, 8) && aligned(nbr, 4) && aligned(state_in, 4) && aligned(state_out, 4) &&
                       aligned(open_out, 4),
                   "spmm_leader_round: misaligned pointer (offsets 8 bytes, the others 4)");
  if (n == 0) return SPMM_OK;
  hipLaunchKernelGGL(leader_round, dim3((unsigned)((n + WR - 1) / WR)), dim3(NT), 0, stream, counts, offsets, nbr, nbr_len, n, by_count, state_in,
                     state_out,
                     open_out);
  SPMM_LAUNCH_CHECK("spmm_leader_round");
  return SPMM_OK;
}

extern "C" int spmm_leader_finish(const int* counts, const long* offsets, const int* nbr, long nbr_len, long n, int by_count, const int* state, int* leader,
                                  spmm_stream_t stream) {
  SPMM_CHECK_SHAPE(n >= 0 && n <= 0x7fffff00L, "spmm_leader_finish: n=%ld must be in [0, 2^31 - 256] rows", n);
  SPMM_CHECK_SHAPE(nbr_len >= 0, "spmm_leader_finish: nbr_len=%ld must be at least 0", nbr_len);
  SPMM_CHECK_SHAPE(by_count == 0 || by_count == 1, "spmm_leader_finish: by_count=%d must be 0 or 1", by_count);
  SPMM_CHECK_SHAPE(by_count == 0 || counts, "spmm_leader_finish: null counts with by_count=1");
  SPMM_CHECK_SHAPE(offsets && nbr && state && leader, "spmm_leader_finish: null offsets / nbr / state / leader");
  SPMM_CHECK_SHAPE(aligned(counts, 4) && aligned(offsets, 8) && aligned(nbr, 4) && aligned(state, 4) && aligned(leader, 4),
                   "spmm_leader_finish: misaligned pointer (offsets 8 bytes, the others 4)");
  if (n == 0) return SPMM_OK;
  hipLaunchKernelGGL(leader_finish, dim3((unsigned)((n + WR - 1) / WR)), dim3(NT), 0, stream, counts, offsets, nbr, nbr_len, n, by_count, state,
                     leader);
  SPMM_LAUNCH_CHECK("spmm_leader_finish");
  return SPMM_OK;
}
