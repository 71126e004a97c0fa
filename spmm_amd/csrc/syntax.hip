// Grammar mask of the syntax-constrained PV -> SMILES search (spmm_smiles_mask, include/spmm_hip.h): one launch between the LM head and
// whatever reads the next-token logits (the logit warp, the beam step) that strikes, per beam row, every token that cannot follow the
// row's own token history in a well-formed SMILES string that still ends inside the position budget.  The grammar, the cost function and
// the packed per-token table are those of spmm_amd/smiles_syntax.py, which is normative; this file is its device form.
//
// Shape of the work: R beam rows, each a fold over < 256 history tokens and then V <= 512 independent decisions.  One wave64 per row, four
// rows per workgroup (logit_warp_kernel's shape).  The table ([V] x 16 bytes) is staged in LDS once per workgroup.  Every lane then looks
// up the table words of its share of the row's history and parks them in the wave's LDS strip, so the fold itself -- all 64 lanes walk the
// same strip in step, a broadcast read whose address does not depend on the state -- is a chain of integer ALU steps only: the loads ahead
// of it pipeline.  Afterwards each lane decides its V/64 tokens from the state every lane already holds.  Integer state only: a row's
// result cannot depend on the rest of the launch.  Plain vector stores, no atomics, no inline assembly.
#include "common.h"
#include "../../include/spmm_hip.h"

namespace {

constexpr int SYN_VMAX = 512, SYN_KMAX = 8, SYN_LMAX = 256;
constexpr int Q_BRK0 = 8, Q_REJECT = 10, Q_ACCEPT = 11;
// cost of the finite state, two bits per state: START, OPEN, BOND_A, BOND_B, DOT, BRK = 1, BRK0 = 2
constexpr unsigned Q_COST2 = 1u | (1u << 6) | (1u << 10) | (1u << 12) | (1u << 14) | (2u << 16) | (1u << 18);

struct SynP {
  float* logits; float* logits2; long ld; int R, V;
  const int* tokens; long tok_ld; int hist_rows, k; const int* mol;
  int t; const int* t_ptr; int t_off, t_last;
  const int4* table; int* state_out;
};

struct SynState { int q, depth, rings; };

// One token (its four table words) on a state that does not reject; q = Q_REJECT / Q_ACCEPT come back as they are in the table.
__device__ __forceinline__ SynState syn_step(SynState s, int4 w) {
  const bool inside = s.q >= Q_BRK0;
  const unsigned ends = inside ? (unsigned)w.y : (unsigned)w.x;
  const int nq = (ends >> (4 * (s.q & 7))) & 15;
  const unsigned cnt = inside ? (unsigned)w.w : (unsigned)w.z;
  const int need = (cnt >> 10) & 255, delta = (int)((cnt >> 18) & 255) - 128;
  SynState o;
  o.q = (nq >= Q_REJECT && nq != Q_ACCEPT) || s.depth < need ? Q_REJECT : nq;
  o.depth = s.depth + delta;
  o.rings = s.rings ^ (int)(cnt & 1023);
  return o;
}

__device__ __forceinline__ int syn_cost(SynState s) { return s.depth + __popc((unsigned)s.rings) + (int)((Q_COST2 >> (2 * s.q)) & 3); }

__global__ __launch_bounds__(256) void smiles_mask_kernel(SynP p) {
  __shared__ __attribute__((aligned(16))) int4 tab[SYN_VMAX];                 // the packed table
  __shared__ __attribute__((aligned(16))) int4 strip[4][SYN_LMAX];            // table words of the wave's history, in position order
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int v = threadIdx.x; v < p.V; v += 256) tab[v] = p.table[v];
  __syncthreads();
  const long row = (long)blockIdx.x * 4 + wave;
  const bool active = row < p.R;                            // wave-uniform; no early return: the barrier below is the workgroup's
  int t = p.t_ptr ? *p.t_ptr + p.t_off : p.t;
  t = min(max(t, 1), p.t_last);                             // (t_last < 256 was checked on the host: the strip holds every position)
  long hrow = -1;
  if (active) {
    const long g = row / p.k, b = row % p.k;
    hrow = (p.mol ? (long)p.mol[g] : g) * p.k + b;
    if (hrow < 0 || hrow >= p.hist_rows) hrow = -1;         // (a bad mol entry: the row rejects, nothing outside the histories is read)
  }
  if (hrow >= 0) {
    const int* h = p.tokens + hrow * p.tok_ld;
    for (int j = 1 + lane; j < t; j += 64) {                // position 0 is [CLS]
      const int tok = h[j];
      const bool outside = tok < 0 || tok >= p.V;           // a token outside the vocabulary: REJECT from every state
      int4 w = tab[outside ? 0 : tok];
      if (outside) { w.x = (int)0xAAAAAAAAu; w.y = 0xAA; w.z = 128 << 18; w.w = 128 << 18; }
      strip[wave][j] = w;
    }
  }
  __syncthreads();
  SynState s = {hrow >= 0 ? 0 : Q_REJECT, 0, 0};
  if (hrow >= 0) {
    for (int j = 1; j < t; ++j) {                           // every lane the same walk: the state ends up in all of them
      const SynState n = syn_step(s, strip[wave][j]);
      if (s.q < Q_REJECT) s = n;                            // REJECT is final; ACCEPT ([SEP] inside a history) rejects what follows
      if (s.q == Q_ACCEPT) s.q = Q_REJECT;
    }
  }
  if (!active) return;
  const bool dead = s.q >= Q_REJECT;
  if (p.state_out && lane == 0) {
    int* o = p.state_out + row * 4;
    o[0] = dead ? Q_REJECT : s.q;
    o[1] = dead ? 0 : s.depth;
    o[2] = dead ? 0 : s.rings;
    o[3] = dead ? -1 : syn_cost(s);
  }
  const int budget = p.t_last - t - 1;                      // non-[SEP] tokens that may still follow the one chosen now
  for (int v = lane; v < p.V; v += 64) {
    bool ok = false;
    if (!dead) {
      const SynState n = syn_step(s, tab[v]);
      if (n.q == Q_ACCEPT) ok = s.depth == 0 && s.rings == 0;
      else if (n.q < Q_REJECT) ok = syn_cost(n) <= budget;
    }
    if (!ok) {
      p.logits[row * p.ld + v] = SPMM_SYNTAX_MASKED;
      if (p.logits2) p.logits2[row * p.ld + v] = SPMM_SYNTAX_MASKED;
    }
  }
}

}  // namespace

extern "C" int spmm_smiles_mask(float* logits, float* logits2, long ld, int R, int V, const int* tokens, long tok_ld, int hist_rows, int k,
                                const int* mol, int Lmax, int t, const int* t_ptr, int t_off, int t_last, const int* table, int* state_out,
                                hipStream_t stream) {
  SPMM_CHECK_SHAPE(R >= 0, "spmm_smiles_mask: R=%d (R >= 0)", R);
  SPMM_CHECK_SHAPE(V >= 1 && V <= SYN_VMAX, "spmm_smiles_mask: V=%d (1 <= V <= 512)", V);
  SPMM_CHECK_SHAPE(k >= 1 && k <= SYN_KMAX && R % k == 0, "spmm_smiles_mask: k=%d R=%d (1 <= k <= 8, R a multiple of k)", k, R);
  SPMM_CHECK_SHAPE(Lmax >= 2 && Lmax <= SYN_LMAX, "spmm_smiles_mask: Lmax=%d (2 <= Lmax <= 256)", Lmax);
  SPMM_CHECK_SHAPE(t_last >= 1 && t_last < Lmax, "spmm_smiles_mask: t_last=%d Lmax=%d (0 < t_last < Lmax)", t_last, Lmax);
  SPMM_CHECK_SHAPE(t_ptr != nullptr || (t >= 1 && t <= t_last), "spmm_smiles_mask: t=%d t_last=%d (0 < t <= t_last)", t, t_last);
  SPMM_CHECK_SHAPE(ld >= V, "spmm_smiles_mask: ld=%ld must be >= V=%d", ld, V);
  SPMM_CHECK_SHAPE(tok_ld >= 1 && hist_rows >= 1, "spmm_smiles_mask: tok_ld=%ld hist_rows=%d (both >= 1)", tok_ld, hist_rows);
  SPMM_CHECK_SHAPE(mol != nullptr || (long)hist_rows >= (long)R, "spmm_smiles_mask: hist_rows=%d < R=%d without mol", hist_rows, R);
  if (R == 0) return SPMM_OK;
  SPMM_CHECK_SHAPE(logits != nullptr && tokens != nullptr && table != nullptr, "spmm_smiles_mask: logits, tokens and table are required");
  SPMM_CHECK_SHAPE((((uintptr_t)logits | (uintptr_t)logits2 | (uintptr_t)tokens | (uintptr_t)mol | (uintptr_t)t_ptr | (uintptr_t)state_out) & 3) == 0,
                   "spmm_smiles_mask: misaligned logits / logits2 / tokens / mol / t_ptr / state_out (4 bytes)");
  SPMM_CHECK_SHAPE(((uintptr_t)table & 15) == 0, "spmm_smiles_mask: misaligned table (16 bytes)");
  SynP p = {logits, logits2, ld, R, V, tokens, tok_ld, hist_rows, k, mol, t, t_ptr, t_off, t_last, (const int4*)table, state_out};
  hipLaunchKernelGGL(smiles_mask_kernel, dim3((unsigned)(((long)R + 3) / 4)), dim3(256), 0, stream, p);
  SPMM_LAUNCH_CHECK("spmm_smiles_mask");
  return SPMM_OK;
}
