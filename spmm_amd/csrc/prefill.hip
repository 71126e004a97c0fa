// Prefill of the decoder's self-attention cache (spmm_kv_prefill, include/spmm_hip.h): the keys and values of whole prefixes, as the
// fused Q|K|V projection of a packed pass leaves them (token-major rows, head h at column h*64), moved into the head-major cache
// [R, nH, Lmax, 64] that csrc/decode.hip reads.  A pure permutation of 128-byte (token, head) cells: 16 bytes per lane, 8 lanes per cell,
// the lanes of a wave walk the token-major row (coalesced reads of nH*128 contiguous bytes per token), every store is a whole cell.
// No LDS, no atomics, nothing converted: the bits of the source arrive unchanged.
#include "common.h"
#include "../../include/spmm_hip.h"

namespace {

constexpr int PF_TOK = 16;           // positions per workgroup
constexpr int PF_THR = 256;

struct PrefillP {
  const uint4* K; const uint4* V; long ld8; long src_rows;      // ld8: source row stride in 16-byte chunks
  const int* row0; const int* len; const int* dst_row;
  uint4* Kc; uint4* Vc; int R, nH, Lmax;
};

__global__ __launch_bounds__(PF_THR) void kv_prefill_kernel(PrefillP p) {
  const int e = blockIdx.x, j0 = blockIdx.y * PF_TOK;
  const int n = min(p.len[e], p.Lmax);                           // (len <= 0: nothing)
  const int dst = p.dst_row[e];
  if (j0 >= n || dst < 0 || dst >= p.R) return;                  // workgroup-uniform
  const long r0 = p.row0[e];
  const int cpt = p.nH * 8;                                      // 16-byte chunks per token
  const int work = min(PF_TOK, n - j0) * cpt;
  const long cache0 = (long)dst * p.nH * p.Lmax * 8;             // chunk index of cell (dst, 0, 0)
  for (int i = threadIdx.x; i < work; i += PF_THR) {
    const int dj = i / cpt, c = i - dj * cpt;                    // position within the tile, chunk within the token's nH*64 columns
    const int j = j0 + dj;
    const long row = r0 + j;
    if (row < 0 || row >= p.src_rows) continue;                  // a position outside the source is neither read nor written
    const long s = row * p.ld8 + c;
    const uint4 kv = p.K[s], vv = p.V[s];
    const long d = cache0 + ((long)(c >> 3) * p.Lmax + j) * 8 + (c & 7);
    p.Kc[d] = kv;
    p.Vc[d] = vv;
  }
}

}  // namespace

extern "C" int spmm_kv_prefill(const void* K, const void* V, long ld, long src_rows, const int* row0, const int* len, const int* dst_row,
                               int E, void* Kc, void* Vc, int R, int nH, int Lmax, hipStream_t stream) {
  SPMM_CHECK_SHAPE(E >= 0 && R >= 1 && src_rows >= 1, "spmm_kv_prefill: E=%d R=%d src_rows=%ld (E >= 0, R >= 1, src_rows >= 1)", E, R, src_rows);
  SPMM_CHECK_SHAPE(Lmax >= 1 && Lmax <= 256, "spmm_kv_prefill: Lmax=%d outside [1, 256]", Lmax);
  SPMM_CHECK_SHAPE(nH >= 1 && (long)nH * 64 <= ld, "spmm_kv_prefill: nH=%d ld=%ld (nH >= 1, nH*64 <= ld)", nH, ld);
  SPMM_CHECK_SHAPE(ld % 8 == 0, "spmm_kv_prefill: ld=%ld must be a multiple of 8 (rows are read 16 bytes at a time)", ld);
  if (E == 0) return SPMM_OK;
  SPMM_CHECK_SHAPE(K != nullptr && V != nullptr && Kc != nullptr && Vc != nullptr && row0 != nullptr && len != nullptr && dst_row != nullptr,
                   "spmm_kv_prefill: K, V, Kc, Vc, row0, len and dst_row are required");
  SPMM_CHECK_SHAPE((((uintptr_t)K | (uintptr_t)V | (uintptr_t)Kc | (uintptr_t)Vc) & 15) == 0,
                   "spmm_kv_prefill: K, V, Kc and Vc must be 16-byte aligned");
  SPMM_CHECK_SHAPE((((uintptr_t)row0 | (uintptr_t)len | (uintptr_t)dst_row) & 3) == 0, "spmm_kv_prefill: misaligned row0 / len / dst_row (4 bytes)");
  PrefillP p = {(const uint4*)K, (const uint4*)V, ld / 8, src_rows, row0, len, dst_row, (uint4*)Kc, (uint4*)Vc, R, nH, Lmax};
  const dim3 grid((unsigned)E, (unsigned)((Lmax + PF_TOK - 1) / PF_TOK));
  hipLaunchKernelGGL(kv_prefill_kernel, grid, dim3(PF_THR), 0, stream, p);
  SPMM_LAUNCH_CHECK("spmm_kv_prefill");
  return SPMM_OK;
}
