// Logit warp of the PV -> SMILES search (spmm_logit_warp, include/spmm_hip.h): classifier-free guidance between the conditioned and the
// all-masked next-token logits, temperature, top-k and nucleus (top-p) truncation -- one launch between the LM head and the unchanged beam
// step (csrc/decode.hip::beam_step_kernel), which already turns a -inf logit into probability 0 and a -inf key.
//
// Shape of the work: R beam rows x V <= 512 logits.  One wave64 per row, four rows per workgroup, V/64 values per lane in registers as the
// beam step holds them.  Nothing is sorted: a row's z and exp(z - max) go to LDS as (z, e) pairs, and every lane walks ALL V pairs in
// ascending index -- every lane reads the same address, an LDS broadcast, no bank conflict -- counting for each of its own tokens how many
// entries rank above it (z larger, or equal with a lower index: wave_argmax's tie rule) and adding up their e.  That is the token's rank and
// the unnormalised mass of everything ranked above it: ~V^2/64 compare-and-add steps per lane.  The order of every sum is the index order
// (the normaliser: a fixed butterfly), so a row's result does not depend on what else is in the launch.
#include <cmath>

#include "common.h"
#include "../../include/spmm_hip.h"

namespace {

constexpr int WARP_VMAX = 512, WARP_KMAX = 8;

struct WarpP {
  const float* lc; const float* lu; long ld; int R, V;
  float w, temperature; int K; float top_p; int min_keep;   // K: tokens the top-k cut keeps (V: none)
  float* out; long ldo;
};

template <int VJ>
__global__ __launch_bounds__(256) void logit_warp_kernel(WarpP p) {
  __shared__ __attribute__((aligned(16))) float2 sze[4][WARP_VMAX];                        // (z, exp(z - max)) of the wave's row
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // (a scalar: the loop bounds below are)
  const long row = (long)blockIdx.x * 4 + wave;
  const bool active = row < p.R;                              // wave-uniform; no early return: the barriers below are the workgroup's
  const float NEG = -__builtin_inff();
  const int V = active ? p.V : 0;
  // ---- guidance and temperature: every input of the row is in registers before anything is written (out may be lc)
  float z[VJ];
#pragma unroll
  for (int i = 0; i < VJ; ++i) {
    const int j = lane + 64 * i;
    z[i] = NEG;
    if (j < V) {
      float g = p.lc[row * p.ld + j];
      if (p.lu) {
        const float u = p.lu[row * p.ld + j];
        g = __fadd_rn(u, __fmul_rn(p.w, __fsub_rn(g, u)));     // four roundings with the division: the bound the tests hold it to
      }
      z[i] = p.temperature == 1.f ? g : __fdiv_rn(g, p.temperature);
    }
  }
  const bool truncates = p.K < p.V || p.top_p < 1.f;          // launch-uniform
  bool keep[VJ];
#pragma unroll
  for (int i = 0; i < VJ; ++i) keep[i] = true;
  if (truncates) {
    float m = z[0];
#pragma unroll
    for (int i = 1; i < VJ; ++i) m = fmaxf(m, z[i]);
    m = wave_max(m);
    if (m == NEG) m = 0.f;                                    // (a row of -inf: every e is 0, nothing is NaN)
    float e[VJ];
#pragma unroll
    for (int i = 0; i < VJ; ++i) {
      const int j = lane + 64 * i;
      e[i] = j < V ? expf(z[i] - m) : 0.f;
      if (j < WARP_VMAX) sze[wave][j] = make_float2(z[i], e[i]);      // entries in [V, 64 * VJ) hold (-inf, 0): they rank above nothing
    }
    __syncthreads();
    int rank[VJ];
    float above[VJ];
#pragma unroll
    for (int i = 0; i < VJ; ++i) { rank[i] = 0; above[i] = 0.f; }
    const int V2 = (V + 1) & ~1;                              // (<= 64 * VJ: the pad entry exists)
    // The walk in blocks of 64 entries, block b being the entries the lanes hold in register b: every entry of a block b < i lies before
    // every token of register i (an equal value there ranks above: >=), every entry of a block b > i behind it (>), and only the
    // token's own block needs the index compare -- one compare per (entry, token) for all but 64 of the V entries.
#pragma unroll
    for (int b = 0; b < VJ; ++b) {
      const int c1 = min(64 * b + 64, V2);                    // (wave-uniform; an empty block past V runs no trip)
      for (int c = 64 * b; c < c1; c += 2) {
        const float4 pr = *(const float4*)&sze[wave][c];      // two (z, e) pairs, the same address in every lane
#pragma unroll
        for (int i = 0; i < VJ; ++i) {
          bool a0, a1;
          if (b < i) {
            a0 = pr.x >= z[i]; a1 = pr.z >= z[i];
          } else if (b > i) {
            a0 = pr.x > z[i]; a1 = pr.z > z[i];
          } else {
            const int j = lane + 64 * i;
            a0 = (pr.x > z[i]) | ((pr.x == z[i]) & (c < j));        // (| and &: no branch around the second compare)
            a1 = (pr.z > z[i]) | ((pr.z == z[i]) & (c + 1 < j));
          }
          rank[i] += (int)a0;
          above[i] += a0 ? pr.y : 0.f;
          rank[i] += (int)a1;
          above[i] += a1 ? pr.w : 0.f;
        }
      }
    }
    // the normaliser: the mass of the K best-ranked tokens
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < VJ; ++i) s += (lane + 64 * i < V && rank[i] < p.K) ? e[i] : 0.f;
    s = wave_sum(s);
    const float cut = p.top_p * s;
#pragma unroll
    for (int i = 0; i < VJ; ++i)
      keep[i] = rank[i] < p.min_keep || (rank[i] < p.K && (p.top_p >= 1.f || above[i] < cut));
  }
#pragma unroll
  for (int i = 0; i < VJ; ++i) {
    const int j = lane + 64 * i;
    if (j < V) p.out[row * p.ldo + j] = keep[i] ? z[i] : NEG;
  }
}

}  // namespace

extern "C" int spmm_logit_warp(const float* lc, const float* lu, long ld, int R, int V, float w, float temperature, int top_k, float top_p,
                               int min_keep, float* out, long ldo, hipStream_t stream) {
  SPMM_CHECK_SHAPE(R >= 0, "spmm_logit_warp: R=%d (R >= 0)", R);
  SPMM_CHECK_SHAPE(min_keep >= 1 && min_keep <= WARP_KMAX && V >= min_keep && V <= WARP_VMAX,
                   "spmm_logit_warp: min_keep=%d V=%d (1 <= min_keep <= 8, min_keep <= V <= 512)", min_keep, V);
  SPMM_CHECK_SHAPE(ld >= V && ldo >= V, "spmm_logit_warp: ld=%ld ldo=%ld must be >= V=%d", ld, ldo, V);
  SPMM_CHECK_SHAPE(std::isfinite(temperature) && temperature > 0.f, "spmm_logit_warp: temperature=%g must be finite and > 0", (double)temperature);
  SPMM_CHECK_SHAPE(top_p > 0.f && top_p <= 1.f, "spmm_logit_warp: top_p=%g outside (0, 1]", (double)top_p);
  SPMM_CHECK_SHAPE(top_k >= 0, "spmm_logit_warp: top_k=%d (>= 0; 0 or >= V: no top-k cut)", top_k);
  SPMM_CHECK_SHAPE(std::isfinite(w), "spmm_logit_warp: w=%g must be finite", (double)w);
  if (R == 0) return SPMM_OK;
  SPMM_CHECK_SHAPE(lc != nullptr && out != nullptr, "spmm_logit_warp: lc and out are required");
  SPMM_CHECK_SHAPE((((uintptr_t)lc | (uintptr_t)lu | (uintptr_t)out) & 3) == 0, "spmm_logit_warp: misaligned lc / lu / out (4 bytes)");
  WarpP p = {lc, lu, ld, R, V, w, temperature, (top_k > 0 && top_k < V) ? top_k : V, top_p, min_keep, out, ldo};
  const dim3 grid((unsigned)(((long)R + 3) / 4));
  if (V <= 320) hipLaunchKernelGGL(logit_warp_kernel<5>, grid, dim3(256), 0, stream, p);
  else hipLaunchKernelGGL(logit_warp_kernel<8>, grid, dim3(256), 0, stream, p);
  SPMM_LAUNCH_CHECK("spmm_logit_warp");
  return SPMM_OK;
}
