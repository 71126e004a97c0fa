// One position of stochastic beam search (Kool, van Hoof, Welling 2019) for G property vectors ("groups") of W slots each: spmm_sbs_step
// (include/spmm_hip.h holds the contract).  The W sequences the search returns are a sample WITHOUT replacement from the model's sequence
// distribution: candidates are ranked by Gumbel-perturbed log-probabilities, a child's perturbation conditioned on its parent's
// (appendix B of the paper: the children's maximum is the parent's key).
//
// Shape of the work: per group W rows of V <= 512 logits, then the W best of up to W*V candidate keys, then W small gathers.  ONE launch,
// one workgroup per group (nothing a group computes depends on G or on the other groups), phases separated by workgroup barriers:
//   A  keys      one wave per row, V/64 logits per lane: log-sum-exp over the allowed tokens, the conditioned keys.  Only candidates that
//                can still be selected are kept: every used slot offers a candidate with its own key T (its arg-max child, or itself), so
//                with all W slots in use the W-th best key is >= the smallest T, and a key below that bound is dropped on the spot.  The
//                survivors -- about W of them, whatever V is -- go as (key image, token) pairs into the row's own segment of the caller's
//                workspace ws (2*V words per row: W*V pairs do not fit the LDS), compacted by the wave that owns the row: no atomics.
//                If fewer than min(W, finite candidates) survive (a live row with nothing allowed breaks the argument), the phase runs
//                again without the bound;
//   B  select    8-bit radix select over the survivors of the n-th largest COMPOSITE (key image << 32 | ~flat index), n = min(W, finite
//                candidates): the composites are pairwise distinct, so ties between equal keys go to the lower flat index with no code of
//                their own.  The walk stops at the first digit whose bin is taken whole;
//   C  sort      the n selected into LDS, bitonic sort, descending: slot order;
//   D  gather    one wave per new slot: scores, flags, token history, ancestry row, next token.
// Selection and gather share the launch because every *_out array is a twin of its *_in: no slot's input is overwritten before another
// slot has read it.  Integer histograms (LDS atomics on counts), per-row sums in a fixed order (a lane's elements in index order, then a
// xor butterfly): two launches give the same bytes.  Plain vector stores to global memory, no inline assembly.
// Measured at W = 1000, V = 300, every row live (tools/bench_distinct.py, profiles/distinct_bench.json): the first version -- every key
// to the workspace, the select over all W*V of them, libm's expf / log1pf -- took 1 045 us, 48 % of a decoder position: 300 000 LDS
// atomics per digit on the two or three bins that the sign and exponent of similar keys share.  With the bound, the LDS list and the
// hardware exp / log (the same 5.6e-6 against float64 as libm's: the error is the rounding of the fp32 sums at magnitude 64; exp(0) = 1
// and log(0) = -inf exactly, which is all the arg-max rule needs) it is 296 us: A 238, B 2, C 16, D 41 -- phase A is arithmetic (two exp
// and two log per (slot, token) pair on one compute unit), not latency.  Not tuned further.
#include "common.h"
#include "../../include/spmm_hip.h"

namespace {

constexpr int SBS_WMAX = 1024, SBS_VMAX = 512, SBS_LMAX = 256, SBS_VJ = SBS_VMAX / 64, SBS_SEP = 3;
constexpr int SBS_LCAP = 3072;                    // survivors the LDS copy holds (about W are expected); more are read back from the workspace
constexpr float SBS_ALLOWED_ABOVE = -1e29f;       // a logit at or below this (-inf, SPMM_SYNTAX_MASKED) is no candidate

struct SbsP {
  const float* logits; long ldl; const float* noise; long ldn;
  int G, W, V, Lmax; int t; const int* t_ptr; int t_off;
  const float* phi_in; const float* gum_in; const unsigned char* fin_in; const int* len_in; const int* tokens_in; const int* anc_in;
  float* phi_out; float* gum_out; unsigned char* fin_out; int* len_out; int* tokens_out; int* anc_out; int anc_ld;
  int* ids_out; int* parent_out; int* open_out; uint32_t* ws;
  int phases;                  // 4: the whole step; 1 .. 3: stop after phase A, B, C (SPMM_SBS_PHASES: what tools/bench_distinct.py times the phases with)
};

// order-preserving image of a float: a > b  <=>  img(a) > img(b) as unsigned integers (-inf is the smallest image of all that occur)
__device__ __forceinline__ uint32_t key_img(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float img_key(uint32_t i) { return __uint_as_float((i & 0x80000000u) ? (i & 0x7fffffffu) : ~i); }

__global__ __launch_bounds__(1024) void sbs_step_kernel(SbsP p) {
  __shared__ float s_lse[SBS_WMAX];                          // log-sum-exp of every live row (phase D forms phi with it again)
  __shared__ unsigned long long s_sel[SBS_WMAX];             // the selected composites
  __shared__ int s_cnt[SBS_WMAX];                            // survivors of every row; phase D: (parent, flags) of every new slot
  __shared__ int s_ptok[SBS_WMAX];                           // phase D: token of every new slot
  __shared__ unsigned long long s_list[SBS_LCAP];            // the survivors' composites, in arrival order (any order: they are counted and sorted)
  __shared__ int s_hist[256];
  __shared__ unsigned int s_minimg;
  __shared__ int s_used, s_nfin, s_kept, s_nsel, s_open, s_bin, s_rem, s_whole;
  const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, wave = tid >> 6, nwave = nthr >> 6;
  const int g = blockIdx.x, W = p.W, V = p.V, L = p.Lmax;
  const float NEG = -__builtin_inff();
  const uint32_t NEG_IMG = key_img(NEG);
  int t = p.t_ptr ? *p.t_ptr + p.t_off : p.t;
  t = min(max(t, 0), L - 2);                                 // (read from device memory: clamped; the host checked a t of its own)
  uint2* ws = (uint2*)p.ws + (long)g * W * V;              // the group's W segments of V (key image, token) pairs
  if (tid == 0) { s_minimg = 0xffffffffu; s_used = 0; s_nfin = 0; s_kept = 0; s_nsel = 0; s_open = 0; }
  __syncthreads();
  for (int i = tid; i < W; i += nthr) {
    const float T = p.gum_in[(long)g * W + i];
    if (T > NEG) { atomicMin(&s_minimg, key_img(T)); atomicAdd(&s_used, 1); }
  }
  __syncthreads();
  // every used slot offers a candidate with key T: with W of them the W-th best key is >= the smallest T
  uint32_t lb_img = s_used == W ? s_minimg : NEG_IMG + 1u;
  int n = 0;

  // ---- A: the keys of every row; the survivors (image >= lb_img) into the row's segment
  // A wave walks its rows one after the other; a row's inputs are requested one row ahead, unconditionally (every row of logits and noise
  // exists, whatever its slot holds), so that their latency -- all a row would otherwise wait for -- lies under the row before.
  struct RowIn { float T, phi; int fin; float l[SBS_VJ], nz[SBS_VJ]; };
  auto load_row = [&](int i, RowIn& r) {
    const long row = (long)g * W + i;
    r.T = p.gum_in[row]; r.phi = p.phi_in[row]; r.fin = p.fin_in[row];
    const float* lrow = p.logits + row * p.ldl;
    const float* nrow = p.noise + row * p.ldn;
#pragma unroll
    for (int q = 0; q < SBS_VJ; ++q) {
      const int j = lane + 64 * q;
      r.l[q] = j < V ? lrow[j] : NEG;
      r.nz[q] = j < V ? nrow[j] : 0.f;
    }
  };
  int M = 0;                                                 // survivors
  for (int attempt = 0; attempt < 2; ++attempt) {
    RowIn cur, nxt;
    if (wave < W) load_row(wave, cur);
    for (int i = wave; i < W; i += nwave) {
      nxt = cur;
      if (i + nwave < W) load_row(i + nwave, nxt);
      const float T = cur.T, phi = cur.phi;
      const bool used = T > NEG, fin = used && cur.fin != 0;             // (a NaN key is an empty slot)
      uint32_t img[SBS_VJ];
#pragma unroll
      for (int q = 0; q < SBS_VJ; ++q) img[q] = NEG_IMG;
      float lse = 0.f;
      if (fin) {
        if (lane == SBS_SEP) img[0] = key_img(T);            // exactly one candidate: itself
      } else if (used) {
        const float* l = cur.l;
        const float* nz = cur.nz;
        bool ok[SBS_VJ];
        float m = NEG;
#pragma unroll
        for (int q = 0; q < SBS_VJ; ++q) {
          ok[q] = l[q] > SBS_ALLOWED_ABOVE;
          if (ok[q]) m = fmaxf(m, l[q]);
        }
        m = wave_max(m);
        if (m > NEG) {                                       // (wave-uniform) a live row with nothing allowed contributes nothing
          float s = 0.f;
#pragma unroll
          for (int q = 0; q < SBS_VJ; ++q)
            if (64 * q < V) s += ok[q] ? __expf(l[q] - m) : 0.f;
          s = wave_sum(s);
          lse = m + __logf(s);
          float gk[SBS_VJ], Z = NEG;
#pragma unroll
          for (int q = 0; q < SBS_VJ; ++q) {
            gk[q] = ok[q] ? __fadd_rn(__fadd_rn(phi, __fsub_rn(l[q], lse)), nz[q]) : NEG;
            Z = fmaxf(Z, gk[q]);
          }
          Z = wave_max(Z);
#pragma unroll
          for (int q = 0; q < SBS_VJ; ++q) {
            if (64 * q >= V || !ok[q]) continue;
            const float v = __fadd_rn(__fsub_rn(T, gk[q]), __logf(__fsub_rn(1.0f, __expf(__fsub_rn(gk[q], Z)))));      // log1p(-exp(g - Z))
            const float key = __fsub_rn(__fsub_rn(T, fmaxf(0.f, v)), __logf(__fadd_rn(1.0f, __expf(-fabsf(v)))));      // log1p(exp(-|v|))
            if (key > NEG) img[q] = key_img(key);            // (NaN, from noise that is not finite, is no candidate)
          }
        }
      }
      int nf = 0, base = 0;
      uint2* seg = ws + (long)i * V;
#pragma unroll
      for (int q = 0; q < SBS_VJ; ++q) {
        if (64 * q >= V) continue;                           // (wave-uniform)
        const unsigned long long fm = __ballot(img[q] != NEG_IMG);
        const bool keep = img[q] >= lb_img;                  // (lb_img > NEG_IMG: never a -inf)
        const unsigned long long km = __ballot(keep);
        const int rank = __popcll(km & ((1ull << lane) - 1ull)), nk = __popcll(km);
        if (nk) {                                            // (wave-uniform) one LDS atomic per 64 tokens that hold a survivor
          int at = 0;
          if (lane == 0) at = atomicAdd(&s_kept, nk);
          at = __shfl(at, 0, 64) + rank;
          if (keep) {
            seg[base + rank] = make_uint2(img[q], (uint32_t)(lane + 64 * q));
            if (at < SBS_LCAP) s_list[at] = ((unsigned long long)img[q] << 32) | (uint32_t)~(uint32_t)(i * V + lane + 64 * q);
          }
        }
        nf += __popcll(fm);
        base += nk;                                          // (<= the row's V tokens: inside the segment)
      }
      if (lane == 0) {
        s_lse[i] = lse;
        s_cnt[i] = base;
        if (nf) atomicAdd(&s_nfin, nf);
      }
      cur = nxt;
    }
    __syncthreads();                                         // (the workspace stores of this workgroup are visible to it from here on)
    n = min(W, s_nfin);
    M = s_kept;
    const bool enough = M >= n;
    __syncthreads();
    if (enough) break;                                       // (workgroup-uniform)
    lb_img = NEG_IMG + 1u;                                   // the bound did not hold (a live row without a candidate): keep every finite key
    if (tid == 0) { s_nfin = 0; s_kept = 0; }
    __syncthreads();
  }

  if (p.phases < 2) return;                                  // (workgroup-uniform, as the two below)
  // the survivors: the LDS copy, or -- more of them than it holds -- the rows' segments, a wave per row
  const bool in_lds = M <= SBS_LCAP;
  auto each_survivor = [&](auto&& f) {
    if (in_lds) {
      for (int e = tid; e < M; e += nthr) f(s_list[e]);
    } else {
      for (int i = wave; i < W; i += nwave) {
        const uint2* seg = ws + (long)i * V;
        for (int e = lane; e < s_cnt[i]; e += 64) {
          const uint2 kv = seg[e];
          f(((unsigned long long)kv.x << 32) | (uint32_t)~(uint32_t)(i * V + (int)kv.y));
        }
      }
    }
  };

  // ---- B: the n-th largest composite among the survivors
  unsigned long long thr = ~0ull;                            // n == 0: nothing is selected
  if (n > 0) {
    unsigned long long prefix = 0ull;
    int rem = n;
    for (int pass = 0; pass < 8; ++pass) {
      const int shift = 56 - 8 * pass;
      for (int b = tid; b < 256; b += nthr) s_hist[b] = 0;
      __syncthreads();
      each_survivor([&](unsigned long long c) {
        const bool mine = pass == 0 ? true : ((c ^ prefix) >> (shift + 8)) == 0ull;        // (pass 0: no digit fixed yet; a shift by 64 is undefined)
        if (mine) atomicAdd(&s_hist[(int)((c >> shift) & 255)], 1);
      });
      __syncthreads();
      if (wave == 0) {                                       // bins from 255 down, four per lane: the bin in which the rem-th largest lies
        const int b0 = 255 - 4 * lane;
        int c4[4], tot = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) { c4[q] = s_hist[b0 - q]; tot += c4[q]; }
        int incl = tot;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const int up = __shfl_up(incl, o, 64);
          if (lane >= o) incl += up;
        }
        int run = incl - tot;
        if (run < rem && rem <= incl) {                      // exactly one lane
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            if (run < rem && rem <= run + c4[q]) { s_bin = b0 - q; s_rem = rem - run; s_whole = (rem - run == c4[q]); }
            run += c4[q];
          }
        }
      }
      __syncthreads();
      prefix |= (unsigned long long)s_bin << shift;
      rem = s_rem;
      const bool whole = s_whole != 0;
      __syncthreads();                                       // (s_bin / s_hist are rewritten by the next pass)
      if (whole) break;                                      // every composite with this prefix is taken: the digits below are zero
    }
    thr = prefix;
  }

  if (p.phases < 3) return;
  // ---- C: the selected, sorted
  int P2 = 1;
  while (P2 < W) P2 <<= 1;
  for (int e = tid; e < P2; e += nthr) s_sel[e] = 0ull;
  __syncthreads();
  if (n > 0) {
    each_survivor([&](unsigned long long c) {
      if (c >= thr) {
        const int pos = atomicAdd(&s_nsel, 1);
        if (pos < P2) s_sel[pos] = c;                        // (exactly n <= W of them)
      }
    });
  }
  __syncthreads();
  for (int k = 2; k <= P2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < P2; i += nthr) {
        const int x = i ^ j;
        if (x > i) {
          const unsigned long long a = s_sel[i], b = s_sel[x];
          if (((i & k) == 0) ? a < b : a > b) { s_sel[i] = b; s_sel[x] = a; }
        }
      }
      __syncthreads();
    }

  if (p.phases < 4) return;
  // ---- D: the new slots.  First a thread per slot: its parent, token, scores and flags (every load of a slot independent of the other
  // slots'); then histories and ancestry rows as one flat copy, four elements per thread in flight.
  const long rows_all = (long)p.G * W;
  for (int s = tid; s < W; s += nthr) {
    const long row = (long)g * W + s;
    const bool have = s < n;
    int par = s, tok = 0;
    float key = NEG, phi = NEG;
    bool pfin = false, fin = false;
    if (have) {
      const unsigned long long c = s_sel[s];
      const uint32_t e = ~(uint32_t)c;
      par = min((int)(e / (uint32_t)V), W - 1);
      tok = (int)(e - (uint32_t)par * (uint32_t)V);
      key = img_key((uint32_t)(c >> 32));
      const long prow = (long)g * W + par;
      pfin = p.fin_in[prow] != 0;
      phi = p.phi_in[prow];
      if (!pfin) phi = __fadd_rn(phi, __fsub_rn(p.logits[prow * p.ldl + tok], s_lse[par]));
      fin = pfin || tok == SBS_SEP;
    }
    p.phi_out[row] = phi;
    p.gum_out[row] = key;
    p.fin_out[row] = fin ? 1 : 0;
    p.len_out[row] = have ? (pfin ? p.len_in[(long)g * W + par] : t + 1) : 0;
    p.ids_out[row] = (have && !fin) ? tok : 0;
    if (p.parent_out) p.parent_out[row] = par;
    s_ptok[s] = tok;
    const unsigned long long om = __ballot(have && !fin);
    if (om != 0ull && (int)__builtin_ctzll(__ballot(true)) == lane) atomicAdd(&s_open, __popcll(om));
  }
  __syncthreads();                                           // (s_cnt has been read for the last time: it now takes the slots' codes)
  for (int s = tid; s < W; s += nthr) {
    const bool have = s < n;
    int par = s, pfin = 0;
    if (have) {
      const uint32_t e = ~(uint32_t)s_sel[s];
      par = min((int)(e / (uint32_t)V), W - 1);
      pfin = p.fin_in[(long)g * W + par] != 0;
    }
    s_cnt[s] = par | (pfin ? 1024 : 0) | (have ? 2048 : 0);
  }
  __syncthreads();
  const int total = W * L;
  for (int b0 = 0; b0 < total; b0 += 4 * nthr) {
    int tk[4], an[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = b0 + u * nthr + tid;
      tk[u] = 0; an[u] = 0;
      if (e < total) {
        const int s = e / L, pos = e - s * L, code = s_cnt[s];
        const long prow = (long)g * W + (code & 1023);
        an[u] = (int)((long)g * W + s);
        if (code & 2048) {
          tk[u] = (!(code & 1024) && pos == t) ? s_ptok[s] : p.tokens_in[prow * L + pos];
          if (pos < t) an[u] = (int)min(max((long)p.anc_in[prow * p.anc_ld + pos], 0L), rows_all - 1);      // (an index read from device memory)
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = b0 + u * nthr + tid;
      if (e < total) {
        const int s = e / L, pos = e - s * L;
        p.tokens_out[((long)g * W + s) * L + pos] = tk[u];
        p.anc_out[((long)g * W + s) * p.anc_ld + pos] = an[u];
      }
    }
  }
  __syncthreads();
  if (tid == 0) p.open_out[g] = s_open;
}

}  // namespace

extern "C" int spmm_sbs_step(const float* logits, long ldl, const float* noise, long ldn, int G, int W, int V, int Lmax, int t, const int* t_ptr,
                             int t_off, const float* phi_in, const float* gum_in, const unsigned char* fin_in, const int* len_in,
                             const int* tokens_in, const int* anc_in, float* phi_out, float* gum_out, unsigned char* fin_out, int* len_out,
                             int* tokens_out, int* anc_out, int anc_ld, int* ids_out, int* parent_out, int* open_out, unsigned int* ws,
                             hipStream_t stream) {
  SPMM_CHECK_SHAPE(G >= 0, "spmm_sbs_step: G=%d (G >= 0)", G);
  SPMM_CHECK_SHAPE(W >= 1 && W <= SBS_WMAX, "spmm_sbs_step: W=%d (1 <= W <= 1024)", W);
  SPMM_CHECK_SHAPE(V >= 4 && V <= SBS_VMAX, "spmm_sbs_step: V=%d (4 <= V <= 512)", V);
  SPMM_CHECK_SHAPE(Lmax >= 2 && Lmax <= SBS_LMAX, "spmm_sbs_step: Lmax=%d (2 <= Lmax <= 256)", Lmax);
  SPMM_CHECK_SHAPE(t_ptr != nullptr || (t >= 0 && t < Lmax - 1), "spmm_sbs_step: t=%d Lmax=%d (0 <= t < Lmax - 1)", t, Lmax);
  SPMM_CHECK_SHAPE(ldl >= V && ldn >= V, "spmm_sbs_step: ldl=%ld ldn=%ld must be >= V=%d", ldl, ldn, V);
  SPMM_CHECK_SHAPE(anc_ld >= Lmax, "spmm_sbs_step: anc_ld=%d < Lmax=%d", anc_ld, Lmax);
  SPMM_CHECK_SHAPE((long)G * W < (1L << 31) / SBS_VMAX, "spmm_sbs_step: G*W=%ld rows (G*W*512 must fit 31 bits)", (long)G * W);
  if (G == 0) return SPMM_OK;
  SPMM_CHECK_SHAPE(logits != nullptr && noise != nullptr && ws != nullptr, "spmm_sbs_step: logits, noise and ws are required");
  SPMM_CHECK_SHAPE(phi_in != nullptr && gum_in != nullptr && fin_in != nullptr && len_in != nullptr && tokens_in != nullptr && anc_in != nullptr,
                   "spmm_sbs_step: every state array (phi, gum, fin, len, tokens, anc) _in is required");
  SPMM_CHECK_SHAPE(phi_out != nullptr && gum_out != nullptr && fin_out != nullptr && len_out != nullptr && tokens_out != nullptr && anc_out != nullptr &&
                       ids_out != nullptr && open_out != nullptr,
                   "spmm_sbs_step: every state array _out, ids_out and open_out are required");
  SPMM_CHECK_SHAPE((((uintptr_t)logits | (uintptr_t)noise | (uintptr_t)t_ptr | (uintptr_t)phi_in | (uintptr_t)gum_in | (uintptr_t)len_in | (uintptr_t)tokens_in |
                     (uintptr_t)anc_in | (uintptr_t)phi_out | (uintptr_t)gum_out | (uintptr_t)len_out | (uintptr_t)tokens_out | (uintptr_t)anc_out |
                     (uintptr_t)ids_out | (uintptr_t)parent_out | (uintptr_t)open_out) & 3) == 0 && ((uintptr_t)ws & 7) == 0,
                   "spmm_sbs_step: misaligned pointer (4 bytes: everything but fin_in / fin_out; ws: 8)");
  SPMM_CHECK_SHAPE((const void*)phi_in != (const void*)phi_out && (const void*)gum_in != (const void*)gum_out && (const void*)fin_in != (const void*)fin_out &&
                       (const void*)len_in != (const void*)len_out && (const void*)tokens_in != (const void*)tokens_out &&
                       (const void*)anc_in != (const void*)anc_out,
                   "spmm_sbs_step: an _out array aliases its _in twin (the step is not in place)");
  SbsP p = {logits, ldl, noise, ldn, G, W, V, Lmax, t, t_ptr, t_off, phi_in, gum_in, fin_in, len_in, tokens_in, anc_in,
            phi_out, gum_out, fin_out, len_out, tokens_out, anc_out, anc_ld, ids_out, parent_out, open_out, (uint32_t*)ws, 4};
  if (const char* ph = getenv("SPMM_SBS_PHASES")) p.phases = ph[0] >= '1' && ph[0] <= '3' ? ph[0] - '0' : 4;      // (timing aid: the outputs are then not written)
  const int threads = W >= 16 ? 1024 : 64 * W;              // a wave per row up to the workgroup's 16
  hipLaunchKernelGGL(sbs_step_kernel, dim3((unsigned)G), dim3((unsigned)threads), 0, stream, p);
  SPMM_LAUNCH_CHECK("spmm_sbs_step");
  return SPMM_OK;
}
