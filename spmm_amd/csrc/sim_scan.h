// Similarity of unit fp32 features on the exact-f32 MFMA: the one definition of the candidate order, of the accumulator chain and of the
// row-stationary scan that csrc/retrieve.hip (spmm_sim_topk), csrc/cluster.hip (spmm_centroid_assign) and csrc/neighbors.hip
// (spmm_sim_range) share.  Their bit-for-bit guarantees -- any chunking of a library gives the same bytes, assign = sim_topk(k = 1), the
// neighbour relation is exactly symmetric -- rest on what is written here and nowhere else.
//
// The chain.  The score of a pair is one accumulator's chain of v_mfma_f32_16x16x4_f32 (a k-ordered fmaf chain per output element):
// lane (c, g) of a wave (c = lane & 15, g = lane >> 4) holds 16 bytes -- elements 16 kb + 4 g .. + 3 -- of its A row and of its B row and
// feeds component m to the m-th of four MFMAs, whose k slot is g.  The sum over E runs kb ascending, then m, then g, whatever tile, lane,
// workgroup or chunk the pair falls in, and a product does not know which factor was A: score(i, j) has score(j, i)'s bits.
// sim_topk_part (query-stationary, a score tile in LDS) and RowScan below are the two loops that run this chain.
//
// The order.  A candidate is (score, index).  Larger score first, equal scores to the lower index, NaN below every number, -0 = +0, the
// empty slot below everything -- a total order, so the best (or the k best) of a set does not depend on how the set was cut into lanes,
// tiles, workgroups or chunks.  As integers: score_key is a monotonic image of the score, cand_key packs (image, ~index) so that a larger
// key is a better candidate and 0 is the empty slot.  spmm_amd/cluster.py::_score_key mirrors score_key on the host.
#pragma once
#include <type_traits>
#include "common.h"

namespace sim_scan {

// ---------------------------------------------------------------------------------------------------------------- the candidate order
// larger float <-> larger key; -0 = +0; NaN -> 0, below -inf's image (0x007fffff)
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
constexpr uint64_t EMPTY_KEY = 0;
// candidate (score image, index < 2^31) as one key; key_image / key_index take it apart again
__device__ __forceinline__ uint64_t pack_key(uint32_t image, uint32_t idx) { return ((uint64_t)image << 32) | (0xffffffffu - idx); }
__device__ __forceinline__ uint64_t cand_key(float s, uint32_t idx) { return pack_key(score_key(s), idx); }
__device__ __forceinline__ uint32_t key_image(uint64_t k) { return (uint32_t)(k >> 32); }
__device__ __forceinline__ uint32_t key_index(uint64_t k) { return 0xffffffffu - (uint32_t)k; }

__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src) {
  const uint32_t lo = __shfl((uint32_t)v, src, 64), hi = __shfl((uint32_t)(v >> 32), src, 64);
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t shfl_up64(uint64_t v) {
  const uint32_t lo = __shfl_up((uint32_t)v, 1, 64), hi = __shfl_up((uint32_t)(v >> 32), 1, 64);
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int m) {
  const uint32_t lo = __shfl_xor((uint32_t)v, m, 64), hi = __shfl_xor((uint32_t)(v >> 32), m, 64);
  return ((uint64_t)hi << 32) | lo;
}

// ---------------------------------------------------------------------------------------------------------------- the row-stationary scan
// Many rows against a column side that is walked once.  A workgroup of NT = 256 threads owns AR = 128 rows -- each of its four waves NB = 2
// MFMA blocks of 16 -- and keeps them in REGISTERS for the whole launch (NB x E / 4 floats per lane); the column side goes through LDS once
// per workgroup in tiles of CT = 32 (E = 512: 16), the next tile's global loads in flight under the current tile's MFMAs.  The 16 x 16
// scores of (column block cb, row block b) never leave the accumulators: D's column (lane & 15) is the row of the block, its rows
// 4 g + r the columns, so acc[cb][b][r] of lane (c, g) in tile t is the score of row block b's row c and column t CT + 16 cb + 4 g + r.
template <int E64>
struct Shape {
  static constexpr int E = 64 * E64, EP = E + 4, KB = E / 16;
  static constexpr int NT = 256, AR = 128, NB = 2;
  static constexpr int CB = E64 < 8 ? 2 : 1, CT = 16 * CB;                   // column blocks of an LDS tile (E = 512: one, the tile stays under 64 KiB)
  static constexpr int LD4 = CT * (E / 4) / NT;                              // 16-byte loads of a thread per column tile
};

// Lane (c, g)'s share of row min(rr, n - 1) (rows past the end: a valid address, the caller never writes them back) -> that row.
template <int E64>
__device__ __forceinline__ long load_row_block(const float* f, long ldf, long rr, int n, int g, f32x4 (&dst)[Shape<E64>::KB]) {
  const long row = min(rr, (long)n - 1);
  const float* fp = f + row * ldf + g * 4;
#pragma unroll
  for (int kb = 0; kb < Shape<E64>::KB; ++kb) dst[kb] = *reinterpret_cast<const f32x4*>(fp + kb * 16);
  return row;
}

// The walk over columns 0 .. nc - 1 (nc >= 1) of `col` in tiles; columns past nc are clamped copies of the last one, to be dropped by the
// caller.  cl: CT * EP floats of LDS, 16-byte aligned.  Every thread of the workgroup runs
//     RowScan<E64> scan(col, ldc, nc, cl);
//     for (int t = 0; t < scan.tiles; ++t) { f32x4 acc[CB][NB]; scan.scores(t, rows, acc); <consume acc>; scan.next(t); }
// so the consumer runs between the tile's MFMAs and the barrier that frees the LDS tile.  (The consumer stays in the kernel's own loop
// body: handed over as a functor, sim_range's emission costs two more VGPRs and E = 128 an occupancy step.)
template <int E64>
struct RowScan {
  using S = Shape<E64>;
  static constexpr int E = S::E, EP = S::EP, KB = S::KB, NT = S::NT, NB = S::NB, CB = S::CB, CT = S::CT, LD4 = S::LD4;
  const float* col;
  const long ldc;
  const int nc, tiles, tid;
  float* cl;
  f32x4 pre[LD4];

  __device__ __forceinline__ void fetch(int t) {
#pragma unroll
    for (int i = 0; i < LD4; ++i) {
      const int e = tid + i * NT, r = e / (E / 4), e4 = e % (E / 4);
      const int j = min(t * CT + r, nc - 1);
      pre[i] = *reinterpret_cast<const f32x4*>(col + (long)j * ldc + e4 * 4);
    }
  }
  __device__ __forceinline__ void stage() {
#pragma unroll
    for (int i = 0; i < LD4; ++i) {
      const int e = tid + i * NT, r = e / (E / 4), e4 = e % (E / 4);
      *reinterpret_cast<f32x4*>(cl + r * EP + e4 * 4) = pre[i];
    }
  }
  __device__ __forceinline__ RowScan(const float* col, long ldc, int nc, float* cl)
      : col(col), ldc(ldc), nc(nc), tiles((nc + CT - 1) / CT), tid(threadIdx.x), cl(cl) {
    fetch(0);
    stage();
    __syncthreads();
  }
  // acc = tile t's scores; the next tile's loads are in flight under the MFMAs
  __device__ __forceinline__ void scores(int t, const f32x4 (&rows)[NB][KB], f32x4 (&acc)[CB][NB]) {
    if (t + 1 < tiles) fetch(t + 1);
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
      for (int b = 0; b < NB; ++b) acc[cb][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int lane = tid & 63, c = lane & 15, g = lane >> 4;
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
  }
  __device__ __forceinline__ void next(int t) {
    __syncthreads();
    if (t + 1 < tiles) {
      stage();
      __syncthreads();
    }
  }
};

// ---------------------------------------------------------------------------------------------------------------- host side
// fn(std::integral_constant<int, E / 64>{}) for the E the contract admits (check_width)
template <class Fn>
inline void dispatch_width(int E, Fn&& fn) {
  switch (E / 64) {
    case 1: fn(std::integral_constant<int, 1>{}); break;
    case 2: fn(std::integral_constant<int, 2>{}); break;
    case 3: fn(std::integral_constant<int, 3>{}); break;
    case 4: fn(std::integral_constant<int, 4>{}); break;
    case 5: fn(std::integral_constant<int, 5>{}); break;
    case 6: fn(std::integral_constant<int, 6>{}); break;
    case 7: fn(std::integral_constant<int, 7>{}); break;
    default: fn(std::integral_constant<int, 8>{}); break;
  }
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// The operand contract of an entry point `name` with rows f and a column side c, in two steps because an empty call returns between them:
// the width and the row count (row numbers of the last, partial workgroup stay in int), then the operands themselves.
inline int check_width(const char* name, int E) {
  SPMM_CHECK_SHAPE(E >= 64 && E <= 512 && E % 64 == 0, "%s: E=%d must be a multiple of 64 up to 512", name, E);
  return SPMM_OK;
}
inline int check_rows(const char* name, long n) {
  SPMM_CHECK_SHAPE(n >= 0 && n <= 0x7fffff00L, "%s: n=%ld must be in [0, 2^31 - 256] rows", name, n);
  return SPMM_OK;
}
inline int check_operands(const char* name, const float* f, long ldf, const float* c, long ldc, int E) {
  SPMM_CHECK_SHAPE(f && c, "%s: null f / c", name);
  SPMM_CHECK_SHAPE(aligned(f, 16) && aligned(c, 16), "%s: f / c must be 16-byte aligned", name);
  SPMM_CHECK_SHAPE(ldf >= E && ldf % 4 == 0 && ldc >= E && ldc % 4 == 0, "%s: ldf=%ld ldc=%ld must be multiples of 4, at least E=%d", name, ldf,
                   ldc, E);
  return SPMM_OK;
}

}  // namespace sim_scan
