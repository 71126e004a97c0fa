/* spmm_hip.h -- C ABI of libspmm_hip.so: the MI355X (gfx950) kernels behind the SPMM pretraining step.
 *
 * The reference (jinhojsk515/spmm) is pure Python on stock torch ops and has no FFI layer of its own; this ABI is
 * the boundary introduced beneath its Python class API.  Each entry point names the
 * reference code it replaces (file:line under /root/reference).  INTEGRATION.md shows the ctypes stub a
 * maintainer of the reference would add to call these from SPMM_models.py / xbert.py.
 *
 * Conventions
 *  - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller (PyTorch allocates; the
 *    library never allocates, frees or retains device memory).
 *  - "bf16" tensors are raw 16-bit bfloat16, passed as void*.  Token-major activations: row = seq * L + pos.
 *  - every call is asynchronous on `stream` (a hipStream_t); no call synchronises or reads device data on the host.
 *  - return value: 0 ok, 1 bad shape/argument, 2 HIP launch failure, 3 unsupported; message via spmm_last_error()
 *    (thread local).  No C++ exception crosses the boundary.
 *  - scalars that change from step to step (alpha, temp, lr, dropout seed, queue pointer, loss-gradient scales)
 *    are read from device memory so that a whole training step can be captured once into a hipGraph and replayed.
 */
#ifndef SPMM_HIP_H
#define SPMM_HIP_H

#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
typedef hipStream_t spmm_stream_t;
#else
typedef void* spmm_stream_t;
#endif

#ifdef __cplusplus
extern "C" {
#endif

int spmm_version(void);
const char* spmm_last_error(void);

/* epilogues of spmm_gemm_nt */
#define SPMM_EPI_BF16 0        /* C(bf16) = alpha*acc/(*div) + bias + R                                  */
#define SPMM_EPI_GELU 1        /* C2(bf16) = pre = acc + bias ; C(bf16) = gelu_erf(pre)                  */
#define SPMM_EPI_F32 2         /* C(f32)  = alpha*acc/(*div) + bias + R                                  */
#define SPMM_EPI_F32_ATOMIC 3  /* C(f32) += alpha*acc/(*div) + bias + R  with atomicAdd (split-K allowed) */
#define SPMM_EPI_GELU_GRAD 4   /* C(bf16) = acc * gelu_erf'(G)                                           */
#define SPMM_EPI_F32_ACC 5     /* C(f32) += alpha*acc/(*div) + bias + R   (plain read-modify-write, single owner) */
#define SPMM_EPI_GELU_DERIV 6  /* pre = acc + bias ; C(bf16) = gelu_erf(pre) ; C2(bf16) = gelu_erf'(pre): the FFN forward keeps  */
                               /* the derivative (one shared exp) so that the backward epilogue is SPMM_EPI_MUL                  */
#define SPMM_EPI_MUL 7         /* C(bf16) = (alpha*acc/(*div) + bias) * G   (G bf16, e.g. the stored gelu'; colsum allowed)      */
/* The five bf16-output epilogues (BF16, GELU, GELU_GRAD, GELU_DERIV, MUL) share pre = alpha*acc/(*div) + bias, in fp32: bias, alpha and *div
 * apply under every one of them -- SPMM_EPI_MUL stores (pre) * G and SPMM_EPI_GELU_GRAD (pre) * gelu_erf'(G), so a bias is added BEFORE the
 * multiplication (the step passes none there).  Rounding: gelu_erf(pre), gelu_erf'(pre) and pre of the two GELU forms are computed from the
 * fp32 pre and rounded to bf16 once.  An epilogue with a second operand rounds TWICE: pre is rounded to bf16 (the tile image the stores are
 * read from), then R is added (SPMM_EPI_BF16), or G / gelu_erf'(G) multiplied, in fp32 and the result is rounded to bf16 again -- on every
 * kernel alike.  colsum[n] += the sum, over the rows computed (*M_dev of them under a device-side row count), of the bf16 values stored
 * to C, in fp32 with atomics: it adds to what colsum holds.  C2 of SPMM_EPI_GELU / _GELU_DERIV is optional (null = not kept).
 * tests/gemm_bf16_reference.py holds the float64 reference and the error bound that follows from these rounding points. */
/* The three fp32-output epilogues take bias (fp32 [N]) and R (bf16 [M, ldr], ldr % 4 == 0, 8-B aligned) like SPMM_EPI_BF16; acc is the
 * whole K reduction: under split-K (SPMM_EPI_F32_ATOMIC, splits > 1) every K-slice adds alpha/(*div) times its partial sum and bias and
 * R are added exactly ONCE per element (by the first slice), whatever `splits` is. */

/* C[M,N] = A[M,K] . W[N,K]^T on MFMA (bf16 in, fp32 accumulate).  Replaces every nn.Linear on the path
 * (xbert.py:280-300 query/key/value, :370 attention output.dense, :435 intermediate.dense + erf GELU :436,
 * :448 output.dense, :673 transform.dense, :695 tied decoder; SPMM_models.py:31-42 heads) and, with transposed
 * operands, their dgrad/wgrad GEMMs; also the similarity GEMMs SPMM_models.py:108-111,121-124 (split-bf16 K=3E).
 * colsum (optional, bf16 / GELU-grad epilogues): colsum[n] += sum_m C[m][n] -- the bias gradient when C is a dY.
 * kernel (per call, no process state): 0 = chosen from the shape; SPMM_GEMM_K128 = 128x128 tile (every epilogue, split-K);
 * SPMM_GEMM_K128PC = the 128x128 tile with four loader waves beside the four compute waves (LDS-DMA issue and a four-stage ring off the
 * computing waves' instruction stream; holds a CU alone: chosen where the tiling gives at most one workgroup per CU -- the decoder's
 * 5 000-row launches);
 * SPMM_GEMM_K256x128 = 256x128 three-stage ring (no atomic epilogue); SPMM_GEMM_K256 = 256x256 tile, one barrier per k-step;
 * SPMM_GEMM_K256P8 = 256x256 tile on the 8-phase schedule (bf16-output epilogues, K % 128 == 0) -- the default for the
 * training step's large GEMMs: one persistent workgroup per CU walking its XCD's tile range.  SPMM_GEMM_K256P8_TILES = the same
 * kernel with one workgroup per tile, SPMM_GEMM_AUTO_TILES = the automatic choice with that variant wherever the 8-phase kernel
 * is chosen: for launches that share the GPU with a long-running kernel on another stream (a collective): the hardware dispatcher
 * then places tiles on whatever CUs are free instead of 1/256th of the work waiting for an occupied CU (tools/gemm_bench contend). */
#define SPMM_GEMM_AUTO 0
#define SPMM_GEMM_K128 1
#define SPMM_GEMM_K256x128 2
#define SPMM_GEMM_K256 3
#define SPMM_GEMM_K128PC 5
#define SPMM_GEMM_K256P8 8
#define SPMM_GEMM_K256P8_TILES 9
#define SPMM_GEMM_AUTO_TILES 16
int spmm_gemm_nt(const void* A, long lda, const void* W, long ldw, int M, int N, int K, int splits, const float* bias,
                 const float* div_ptr, float alpha, const void* R, long ldr, const void* G, long ldg, void* C, long ldc,
                 void* C2, long ldc2, int epi, float* colsum, int kernel, const int* M_dev, spmm_stream_t stream);
/* Device-side row counts (`M_dev` / `R_dev` / `rows_dev`, optional, null = none): spmm_gemm_nt (every kernel -- SPMM_GEMM_K128,
 * SPMM_GEMM_K128PC, SPMM_GEMM_K256x128, SPMM_GEMM_K256, SPMM_GEMM_K256P8 / _TILES, chosen or forced -- and every epilogue, split-K too),
 * spmm_gemm_tn (8-phase kernel, split launch), spmm_colsum_bf16, spmm_ln_fwd and spmm_ln_bwd take a pointer to an int in device memory
 * holding the number of rows to process, <= the host-side row count the launch and the buffers are sized for.  Rows past it are neither
 * read nor written.  For batches whose tail length only the device knows -- here the text hard negatives drawn on the device
 * (SPMM_models.py:166-178) that re-enter the fusion layers as packed query rows: no host read sizes the step. */
/* Weight-gradient GEMM C[N,K] += alpha * A[M,N]^T . B[M,K] straight from the token-major activations (LDS transpose reads,
 * no transposed copies); `splits` > 1 reduces partial slabs from `workspace` (spmm_gemm_tn_workspace_bytes) without atomics.
 * Replaces autograd's weight-gradient matmuls of every nn.Linear on the path.  spmm_colsum_bf16: bias gradients. */
long spmm_gemm_tn_workspace_bytes(int M, int N, int K, int splits);
/* kernel (per call): 0 = chosen from the shape; 1 = 128x128 tiles; 8 = 256x256 tiles on the 8-phase schedule (N, K % 8 == 0).
 * spmm_gemm_tn_splits returns the split count that fills the chip for that choice (pass the same `kernel` to both). */
int spmm_gemm_tn_splits(int M, int N, int K, int kernel);
/* Refused before any launch (SPMM_ERR_SHAPE): a null A, B or C; ldc < K (as spmm_gemm_tn_reduce refuses it); the alignment rules (N, K,
 * ldc multiples of 4; lda, ldb multiples of 8 that cover the 8-column chunks of N / K; A, B 16-byte aligned).
 * Row slicing of the 8-phase kernel (M >= 128; below that the 128x128 kernel runs): slices of rs = ceil(ceil(M / 128) / splits) * 128 rows,
 * ns = ceil(M / rs) of them (ns <= splits).  With over = ns * rs - M, the LAST slice is the rlast = rs - (over / 128) * 128 rows that end at
 * row M, and its first ndup = over % 128 rows, which the slice before also holds, are masked.  A single slice (ns == 1) takes the
 * rlast = (M / 128) * 128 rows that end at row M, and the 128x128 kernel adds the first M % 128 rows in a pass of its own.
 * With a device-side row count M_dev, a single slice or M < 256 runs on the 128x128 kernel at any `splits` (the device-side re-cut of the
 * slices runs over no fewer than 256 rows, so it needs operands of at least 256 rows); otherwise the slices are re-cut on the device by
 * the same rule, and slices left without rows contribute zero. */
int spmm_gemm_tn(const void* A, long lda, const void* B, long ldb, int M, int N, int K, int splits, float alpha, float* C,
                 long ldc, float* workspace, int kernel, const int* M_dev, spmm_stream_t stream);
/* C[n*ldc + k] += sum over ns slabs of N*K floats in `ws`: the split reduction spmm_gemm_tn runs itself, as an entry of its own. */
int spmm_gemm_tn_reduce(const float* ws, int ns, int N, int K, float* C, long ldc, spmm_stream_t stream);
int spmm_colsum_bf16(const void* x, long ld, int R, int C, float* out, const int* R_dev, spmm_stream_t stream);

/* Attention core softmax(QK^T/8 + mask) -> dropout -> .V for head_dim 64, Lq,Lkv <= 256 (one workgroup holds the K/V
 * panel of a head in LDS; the forward runs one workgroup per 128-query chunk, the backward one launch per 128-query chunk).
 * Replaces BertSelfAttention.forward xbert.py:305-354 incl. the additive masks of :889-948 (self: 0/-10000, causal
 * for sequences >= causal_from) and invert_attention_mask :1038-1043 (cross: 0/finfo.min, is_cross=1).
 * kv_seq (optional, [nseq]): query sequence s reads the keys/values of sequence kv_seq[s] -- the passes of SPMM.forward
 * that cross-attend to the same encoder_hidden_states (SPMM_models.py:139-150,181-199,224-231,245-250) share one K/V
 * projection instead of four.  kmask stays per query sequence; dK/dV are written per query sequence.
 * q_row0/q_len ([nseq]) and kv_row0/kv_len ([number of key/value sources]), optional pairs: packed variable-length
 * layouts -- sequence s owns q_len[s] <= Lq rows from row q_row0[s] of Q/O/dO/dQ, source u owns kv_len[u] <= Lkv rows from
 * row kv_row0[u] of K/V (and of dK/dV unless kv_seq is given).  Rows of padding tokens whose outputs never reach a loss
 * (SPMM_models.py:139-206 read only position 0 of those passes) are then simply not computed.
 * Sequences longer than 256 run as <= 128-long query / key chunks over several launches (spmm_amd/ops.py::attn_fwd_long):
 * q_off / kv_off give the chunk's position for the causal mask; backward d_mode 1 writes only D[q] = sum_kv P dP of this key
 * chunk to Dbuf [nseq, nH, Lq], d_mode 2 reads the D summed over all key chunks from Dbuf (0: computed in-kernel; d_mode != 0
 * takes Lq, Lkv <= 128). */
int spmm_attn_fwd(const void* Q, long ldq, const void* K, long ldk, const void* V, long ldv, const int* kmask,
                  const int* kv_seq, const int* q_row0, const int* q_len, const int* kv_row0, const int* kv_len, void* O,
                  long ldo, float* LSE, int nseq, int nH, int Lq, int Lkv, int causal_from, int is_cross, float dropout_p,
                  const uint64_t* seed_ptr, uint64_t seed_salt, int q_off, int kv_off, spmm_stream_t stream);
int spmm_attn_bwd(const void* Q, long ldq, const void* K, long ldk, const void* V, long ldv, const int* kmask,
                  const int* kv_seq, const int* q_row0, const int* q_len, const int* kv_row0, const int* kv_len,
                  const void* O, long ldo, const float* LSE, const void* dO, long lddo, void* dQ,
                  long lddq, void* dK, long lddk, void* dV, long lddv, int nseq, int nH, int Lq, int Lkv, int causal_from,
                  int is_cross, float dropout_p, const uint64_t* seed_ptr, uint64_t seed_salt, int q_off, int kv_off, int d_mode,
                  float* Dbuf, spmm_stream_t stream);

/* Fused cross-attention block, forward (csrc/xattn.hip) -- the unit BASELINE.json's metric names, one launch:
 *   Y = LayerNorm(dropout_h(dropout_a(softmax(Q K^T / 8 + mask)) V . Wo^T + bo) + R)
 * Replaces BertSelfAttention.forward xbert.py:305-354 (cross instantiation :285-290, encoder mask 0/finfo.min from
 * invert_attention_mask :1038-1043) followed by BertSelfOutput.forward xbert.py:369-373.  Q (already projected, xbert.py:280)
 * and K / V (:286-287, projected once per unique source) come from GEMM launches.  Layout arguments as spmm_attn_fwd
 * (kv_seq, packed q_row0/q_len, kv_row0/kv_len); R / Y / Z / mean / rstd / CTX are indexed by query row like Q.
 * WoF = spmm_xattn_pack_wo(attention.output.dense.weight).  Optional outputs (null = not kept): Z (pre-LayerNorm sum, what
 * spmm_ln_bwd reads), mean/rstd, CTX (attention context: weight gradient of Wo, spmm_attn_bwd), LSE.  The two dropouts draw the
 * masks spmm_attn_fwd (salt_a) and spmm_ln_fwd (salt_h, row counter row_base + row) would draw, so the existing backward kernels
 * regenerate them.  H = nH*64 in {128, 256, 768}, Lkv <= 128 (spmm_xattn_supported). */
int spmm_xattn_supported(int H, int nH, int Lq, int Lkv);
int spmm_xattn_pack_wo(const void* W, long ldw, void* out, int H, spmm_stream_t stream);
int spmm_xattn_fwd(const void* Q, long ldq, const void* K, long ldk, const void* V, long ldv, const int* kmask,
                   const int* kv_seq, const int* q_row0, const int* q_len, const int* kv_row0, const int* kv_len,
                   const void* WoF, const float* bo, const void* R, long ldr, const float* gamma, const float* beta, float eps,
                   void* Y, long ldy, void* Z, long ldz, float* mean, float* rstd, void* CTX, long ldc, float* LSE,
                   int nseq, int nH, int Lq, int Lkv, float attn_dropout_p, uint64_t salt_a, float hidden_dropout_p,
                   uint64_t salt_h, const uint64_t* seed_ptr, long row_base, spmm_stream_t stream);
/* Cross-attention probabilities as an output (csrc/attnmap.hip), one launch:
 *   P[s, h, q, j] = softmax_j(Q_h[q] . K_h[j] / 8 + mask),   P_mean[row(s, q), j] = (1 / nH) sum_h P[s, h, q, j]
 * Replaces BertSelfAttention.forward xbert.py:305-340 up to `attention_probs` (cross instantiation :285-290, encoder mask of
 * invert_attention_mask :1038-1043), without the dropout of :344: the probabilities themselves, which spmm_attn_fwd and spmm_xattn_fwd
 * never hold outside registers.  The mask is the cross mask of spmm_attn_fwd(is_cross=1): key j is masked if kmask[s, j] == 0 (kmask:
 * [nseq, Lkv], null = all ones) or j >= kv_len[source].  Q, K: the bf16 projections (head h at column h*64, head_dim 64, any nH in 1..16),
 * row strides ldq, ldk in elements (multiples of 8).  kv_seq, q_row0/q_len, kv_row0/kv_len: exactly as for spmm_attn_fwd; Lq, Lkv <= 256.
 * P_mean, P_heads (either may be null, not both): fp32, indexed by QUERY ROW like Q, row stride ldp >= Lkv, columns 0 .. Lkv-1; head h of
 * P_heads starts at P_heads + h * head_stride.  Columns of masked keys are written as exactly 0.0f; columns [Lkv, ldp) and rows that
 * belong to no sequence are not written; a query row whose keys are all masked gets zeros.  Scores on MFMAs from the bf16 inputs with fp32
 * accumulation; maximum, exponential, row sum and division in fp32; nothing is rounded to bf16.  The heads are summed in ascending order
 * in registers by the workgroup that owns the row (no atomics).  A sequence's rows of both outputs have the same bits wherever it sits in
 * the launch, whatever the other sequences are, for any launch Lkv >= its source length, and whether its source is reached through kv_seq
 * or a private copy.
 * Refused before a launch (rc = 1): a null Q or K; both outputs null; Q or K not 16-byte aligned (outputs and int arrays: 4 bytes); nH
 * outside [1, 16]; ldq or ldk < nH*64 or not a multiple of 8; Lq or Lkv outside [1, 256]; ldp < Lkv; nseq < 0; q_row0/q_len or
 * kv_row0/kv_len not given together; with P_heads and nH > 1 a head_stride < ldp.  nseq == 0 returns 0 without a launch. */
int spmm_attn_probs(const void* Q, long ldq, const void* K, long ldk, const int* kmask, const int* kv_seq,
                    const int* q_row0, const int* q_len, const int* kv_row0, const int* kv_len,
                    float* P_mean, float* P_heads, long ldp, long head_stride,
                    int nseq, int nH, int Lq, int Lkv, spmm_stream_t stream);
/* out[u] = sum over k in [start[u], start[u+1]) of src[list[k]]  (rows of W bf16 elements, fp32 accumulation, fixed order).
 * Folds the per-query-sequence dK/dV of a cross-attention whose sequences share key/value sources (kv_seq) back onto the
 * unique sources before the K/V weight- and data-gradient GEMMs. */
int spmm_segment_sum_bf16(const void* src, const int* start, const int* list, void* out, int U, long W, spmm_stream_t stream);

/* y = LayerNorm(dropout(x) + res): BertSelfOutput xbert.py:369-373, BertOutput :447-451, transform LN :675,
 * property_mtr_head LN SPMM_models.py:41.  zout (may alias x) keeps the pre-norm sum for backward. */
int spmm_ln_fwd(const void* x, const void* res, const float* gamma, const float* beta, void* y, void* zout, float* mean,
                float* rstd, long rows, int H, float eps, float dropout_p, const uint64_t* seed_ptr, uint64_t salt,
                const int* rows_dev, spmm_stream_t stream);
/* The same with the fp32 residual stream (EngineOptions.resid_fp32): res32 is read in fp32, the normalised row is
 * written as bf16 (y: the MFMA operand of the next GEMM) AND fp32 (y32: the next residual / the loss heads' input; may be null). */
int spmm_ln_fwd_r32(const void* x, const float* res32, const float* gamma, const float* beta, void* y, float* y32, void* zout,
                    float* mean, float* rstd, long rows, int H, float eps, float dropout_p, const uint64_t* seed_ptr,
                    uint64_t salt, spmm_stream_t stream);
/* dz = dLN(dy + dy2); dx = dropout-mask(dz) when drop_on_dy == 0; drop_on_dy == 1 masks dy instead (embeddings);
 * dgamma/dbeta accumulate with atomics (may be null for frozen parameters); dxsum (optional) += column sums of dx,
 * i.e. the bias gradient of the dense layer whose output was normalised.
 * beta_from_y (optional, [H]): `z` then holds the LayerNorm's OUTPUT y (what spmm_ln_fwd wrote, no dropout behind it) and the normalised
 * values are recovered as (y - beta) / gamma (0 where gamma == 0); `mean` may be null and spmm_ln_fwd need not keep its pre-norm sum. */
int spmm_ln_bwd(const void* dy, const void* dy2, const void* z, const float* mean, const float* rstd, const float* gamma,
                void* dz, void* dx, float* dgamma, float* dbeta, long rows, int H, float dropout_p,
                const uint64_t* seed_ptr, uint64_t salt, int drop_on_dy, float* dxsum, const int* rows_dev,
                const float* beta_from_y, spmm_stream_t stream);

/* One decode step of BertEmbeddings.forward (xbert.py:193-220) at inference: y[r] = LN(word[ids[r]] + pos[pos_index] +
 * type[0]) for `rows` single-token rows (every beam is at the same position).  pos_ptr (optional) overrides pos_index
 * with a device-resident step counter so that a captured hipGraph of the decode step can be replayed. */
int spmm_embed_step_ln_fwd(const int* ids, int pos_index, const int* pos_ptr, const float* word, const float* pos, const float* type0,
                           const float* gamma, const float* beta, void* y, long rows, int H, float eps, spmm_stream_t stream);

/* Single-query attention over a key/value cache (xbert.py:305-354 for the newest position only; the cache slots the
 * reference sketches at xbert.py:291-295,480,1344-1348).  Row r, head h: softmax_j(q_r,h . K[s(r,j), j, h] * scale) V[...],
 * j < Lkv <= 256, head_dim 64.  Key/value (s, j) of head h lives at element offset s*seq_stride + j*tok_stride + h*head_stride from K / V (token-major rows:
 * tok_stride = row width, head_stride = 64; head-major caches [S, nH, L, 64]: tok_stride = 64, head_stride = L*64).
 * s(r,j) = anc[r*anc_ld + j] (self-attention: beam ancestry table, cache rows are never moved) or r / kv_div when anc is
 * null (cross-attention: the k beams of a molecule share its PV keys/values).  `group` (R % group == 0): rows
 * n*group .. n*group+group-1 are the beams of one molecule -- served by one wave per head (group 2..8), which loads a key row they share once.
 * No mask: beams carry no padding (a masked, variable-length memory: spmm_decode_xattn).  t_ptr (optional, device int): the number of valid keys is *t_ptr + 1 (<= Lkv) instead of
 * Lkv -- the step counter of a replayed hipGraph.  knew / vnew (optional, with anc; row stride ldn): key and value of the newest
 * position (the last valid one) of every row, straight from the projection output: every row attends ITS OWN newest key / value
 * there (the table's entry for that position must name the row's own cache row: s(r, last) = r, or rowmap[r]), and the launch copies
 * them into that cache row for the positions to come, so the caller needs no cache-update copies of its own.  rowmap (optional, [R]):
 * the cache row row r's newest position goes to (s = rowmap[r]) -- after the caller dropped finished molecules from its batch, the
 * rows it still decodes keep writing to the cache rows their ancestry tables name.
 * Refused before a launch: strides that are no multiples of 8; 255 * tok_stride >= 2^31 (the kernels form j * tok_stride in 32 bits); q, K,
 * V, knew or vnew not 16-byte aligned, out not 8-byte aligned; a null q, K, V or out. */
int spmm_decode_attn(const void* q, long ldq, const void* K, const void* V, long seq_stride, long tok_stride, long head_stride, const int* anc,
                     int anc_ld, int kv_div, int group, void* out, long ldo, int R, int nH, int Lkv, float scale,
                     const int* t_ptr, const void* knew, const void* vnew, long ldn, const int* rowmap, spmm_stream_t stream);

/* Single-query CROSS-attention over a masked, variable-length memory: the decoder of reaction prediction attends to the encoded reactant
 * SMILES (SPMM_models_rxn.py `generate`: encoder_hidden_states = text_embeds, encoder_attention_mask = text_mask; xbert.py:305-354 for the
 * newest position), 1..149 tokens per reaction and different for every reaction of a batch.  Row r (of R) belongs to molecule
 * n = r / group -- rows n*group .. n*group+group-1 are its beams, served by one wave per head -- whose source is u = kv_seq ? kv_seq[n] : n.
 * Row r, head h: softmax_j(q_r,h . K[kv_row0[u] + j, h] * scale) V[kv_row0[u] + j, h], j < kv_len[u], head_dim 64.  K / V rows are
 * token-major with row stride ldkv elements, head h at column h*64: the two halves of the [M, 2H] output of the fused key|value
 * projection of PACKED text rows (padding rows dropped); a padded [U, L, 2H] buffer is the same call with kv_row0[u] = u*L.
 * kv_seq (optional, [R/group]), kv_row0, kv_len: device int32.  1 <= kv_len[u] <= Lkv_max <= 256: what the kernel reads from memory is
 * clamped into that range, so a bad length cannot address outside Lkv_max rows of the source, and no row at or beyond
 * kv_row0[u] + kv_len[u] is ever read (keys past the end are masked to -inf and not fetched: the last row may end the allocation).
 * After the caller dropped finished molecules from its batch only kv_seq is gathered; the memory never moves.
 * 1 <= group <= 8, R % group == 0; ldq, ldo, ldkv multiples of 8, >= nH*64; q, K, V 16-byte aligned, out 8-byte.  Arithmetic and
 * result layout as spmm_decode_attn (equal lengths give its cross-attention result bit for bit). */
int spmm_decode_xattn(const void* q, long ldq, const void* K, const void* V, long ldkv, const int* kv_seq, const int* kv_row0,
                      const int* kv_len, int group, void* out, long ldo, int R, int nH, int Lkv_max, float scale, spmm_stream_t stream);

/* One position of the k-beam PV -> SMILES search for N molecules (d_pv2smiles_batched.py:36-50; the top-k branch of
 * `generate`, d_pv2smiles_single.py:41-44) in one launch.  logits [N*k, V] fp32 (row stride ldl): next-token logits of every beam.
 * Per molecule: log softmax of the k most probable successors of every beam on top of the beam's score cur_p -> k*k candidates;
 * candidates whose token is [SEP] (id 3) are appended to the molecule's finals in row-major order (fin_p / fin_len / fin_tok,
 * F + 1 slots per molecule, slot F a dump; fin_n counts) and struck out with -1e5; a molecule holding >= k finals is done (done[n] = 1,
 * *n_done counts them) and keeps its state; otherwise the k best candidates become the new beams: tokens [N, k, Lmax] (int32
 * histories; position t receives the new token), cur_p, ids_out [N*k] (the token to feed next; 0 for finished molecules),
 * parent_out (optional) and the K/V ancestry table anc [N*k, anc_ld] of spmm_decode_attn (optional: positions < t inherited from
 * the parent row, positions >= t the row itself; the beams of a molecule that finishes at this position all take beam 0's row of the table --
 * nobody reads their outputs any more, and one shared row per position is the cheap case of spmm_decode_attn).  t = tokens held by every live beam = *t_ptr + t_off when t_ptr is given (a
 * replayed hipGraph), else the argument.  mol (optional, [N]): the batch is a compacted subset -- molecule i of logits / ids_out / anc is
 * molecule mol[i] of the state arrays; rowmap (optional, [N*k]): the K/V cache row of beam row i*k + b (what "the row itself" means in
 * anc).  k <= 8, k <= V <= 512, Lmax <= 256. */
int spmm_beam_step(const float* logits, long ldl, int N, int k, int V, int Lmax, int F, int t, const int* t_ptr, int t_off,
                   int* tokens, float* cur_p, float* fin_p, int* fin_len, int* fin_tok, int* fin_n, unsigned char* done,
                   int* anc, int anc_ld, int* ids_out, int* parent_out, int* n_done, const int* mol, const int* rowmap,
                   spmm_stream_t stream);

/* spmm_beam_step with the number of finals that ends a molecule's search as an argument: the arguments of spmm_beam_step, then `need`,
 * the stream last as everywhere.  A molecule is done once it holds >= need finals; need = k is spmm_beam_step bit for bit, need = k*k is
 * `evaluate_beam` of reaction prediction (d_rxn_prediction.py), which keeps searching until k*k hypotheses have ended and returns the k
 * best of them.  k <= need <= k*k and F >= need + k - 1: a position appends at most one [SEP] candidate per beam, so a molecule that is
 * not done holds < need finals and at most k are added -- slot F, the dump, is never reached. */
int spmm_beam_step_until(const float* logits, long ldl, int N, int k, int V, int Lmax, int F, int t, const int* t_ptr, int t_off,
                         int* tokens, float* cur_p, float* fin_p, int* fin_len, int* fin_tok, int* fin_n, unsigned char* done,
                         int* anc, int anc_ld, int* ids_out, int* parent_out, int* n_done, const int* mol, const int* rowmap,
                         int need, spmm_stream_t stream);

/* spmm_beam_step for the SAMPLED search (the stochastic branch of `generate`, d_pv2smiles_single.py:38-41): the arguments of spmm_beam_step,
 * then noise [N*k, V] fp32 (row stride ldn >= V), the stream last as everywhere.  The k candidates of a beam are the k largest of
 * key[j] = logits[j] + noise[j] (one fp32 add; ties to the lower index), in descending key order; their log-probabilities are those of the
 * UNPERTURBED logits.  With the Gumbel noise of spmm_gumbel_noise that is k draws without replacement from the next-token distribution,
 * in draw order (torch.multinomial(p, k, replacement=False)).  Finals, survivors, histories, ancestry, mol and rowmap as in spmm_beam_step. */
int spmm_beam_step_sampled(const float* logits, long ldl, int N, int k, int V, int Lmax, int F, int t, const int* t_ptr, int t_off,
                           int* tokens, float* cur_p, float* fin_p, int* fin_len, int* fin_tok, int* fin_n, unsigned char* done,
                           int* anc, int anc_ld, int* ids_out, int* parent_out, int* n_done, const int* mol, const int* rowmap,
                           const float* noise, long ldn, spmm_stream_t stream);

/* Counter-based Gumbel noise for spmm_beam_step_sampled: out[ci*k + b, j] (row stride ldo) for compact molecule ci < N, beam b < k, token
 * j < V is g = -log(-log(u)), u = ((h >> 8) + 0.5) * 2^-24 (never 0 or 1), h = rng_pair(seed_mix(*seed_ptr, salt), idx) (csrc/common.h) with the
 * 64-bit counter idx = (((mol_base + n) * Lmax + t) * k + b) * V + j, n = mol ? mol[ci] : ci (spmm_beam_step's convention), t = *t_ptr + t_off
 * when t_ptr is given.  A draw depends on (seed, salt, GLOBAL molecule index, position, beam, token) only -- not on the batch the molecule is
 * decoded in, the chunking of a run or compactions.  k <= 8, V <= 512, Lmax <= 256, 0 <= t < Lmax, N*k*V < 2^31. */
int spmm_gumbel_noise(const uint64_t* seed_ptr, uint64_t salt, int N, int k, int V, int Lmax, int t, const int* t_ptr, int t_off,
                      const int* mol, long mol_base, float* out, long ldo, spmm_stream_t stream);

/* Logit warp in front of the beam step (csrc/warp.hip): guidance, temperature, top-k and nucleus truncation of the next-token logits of R
 * beam rows, one launch.  lc, lu (may be null), out: fp32 rows of V logits, row strides ld (lc and lu) and ldo.  Per row:
 *   1. g_j = lu_j + w * (lc_j - lu_j) (classifier-free guidance: lc the conditioned, lu the all-masked logits; raw logits suffice, the
 *      per-row constants of the two log-softmaxes vanish in the next softmax); lu == null: g_j = lc_j exactly.
 *   2. z_j = g_j / temperature; temperature == 1: z_j = g_j exactly.
 *   3. Tokens are ranked by (z descending, j ascending): a tie goes to the lower index, as in spmm_beam_step.
 *   4. K = top_k if 0 < top_k < V, else V; q = softmax of z over the K best-ranked tokens.  The token of rank r is kept iff r < min_keep,
 *      or r < K and the sum of q over the ranks < r is < top_p.  top_p == 1 is "no nucleus cut": every partial sum of q is below 1.
 *   5. out_j = z_j if kept, else -inf.
 * min_keep is the search's k: the sampled beam step draws k tokens without replacement per row, so every row keeps >= k finite entries.
 * The columns [V, ld) of the inputs and [V, ldo) of out are neither read nor written; out may be lc (a row is read whole before it is
 * written).  fp32 throughout; every sum of a row has a fixed order, so a row's result does not depend on the rest of the launch.
 * Refused before a launch (rc = 1): R < 0; min_keep outside [1, 8]; V outside [min_keep, 512]; ld or ldo < V; temperature <= 0 or not
 * finite; top_p outside (0, 1]; top_k < 0; w not finite; with R > 0 a null lc or out.  R == 0 returns 0 without a launch. */
int spmm_logit_warp(const float* lc, const float* lu, long ld, int R, int V, float w, float temperature, int top_k, float top_p,
                    int min_keep, float* out, long ldo, spmm_stream_t stream);

/* Grammar mask of the syntax-constrained PV -> SMILES search (csrc/syntax.hip; grammar, cost and table layout: spmm_amd/smiles_syntax.py,
 * which is normative): one launch that strikes, in place, every next-token logit of R beam rows that cannot follow the row's own token
 * history in a well-formed SMILES string ending inside the position budget.  SYNTAX ONLY: parentheses, ring-bond digits, bracket atoms,
 * bond and dot placement, a non-empty molecule; not element symbols, valence, aromaticity, `%nn` ring labels ('%' rejects) or `C11`.
 * logits, logits2 (may be null; e.g. the guidance baseline): fp32 [R, V], row stride ld; logits2 receives the identical mask.
 * tokens: int32 histories, row stride tok_ld ELEMENTS, hist_rows rows; beam row i reads history row (mol ? mol[i / k] : i / k) * k + i % k
 * (spmm_beam_step's convention; a row index outside [0, hist_rows) makes the row reject and is not read).  Position 0 is [CLS] and is not
 * looked at; positions 1 .. t-1 are folded through the table; ids outside [0, V) reject.  t = tokens held by the row = the position the
 * next token lands at, = *t_ptr + t_off when t_ptr is given (clamped into [1, t_last]); t_last = the last position the search can write.
 * table: int32 [V, 4], 16-byte aligned (SyntaxTable.packed).  With the row's state (q, depth, rings) a token v other than [SEP] is allowed
 * iff it does not reject from q, depth >= need[v] and cost(state after v) <= t_last - t - 1; [SEP] iff the end rule holds; a history that
 * rejects allows nothing.  A masked entry becomes SPMM_SYNTAX_MASKED (finite: u + w (c - u) of two masked entries is the sentinel again,
 * not NaN); an allowed entry keeps its bits; columns [V, ld) are not touched.  state_out (optional): int32 [R, 4] = (q, depth, rings, cost)
 * of the history, (10, 0, 0, -1) for a history that rejects.  Integer state only: a row's result does not depend on the rest of the launch.
 * Refused before a launch (rc = 1): R < 0; V outside [1, 512]; k outside [1, 8] or R not a multiple of k; Lmax outside [2, 256]; t_last
 * outside [1, Lmax); without t_ptr a t outside [1, t_last]; ld < V; tok_ld or hist_rows < 1; hist_rows < R without mol; with R > 0 a null
 * logits, tokens or table, a pointer not 4-byte aligned or a table not 16-byte aligned.  R == 0 returns 0 without a launch. */
#define SPMM_SYNTAX_MASKED (-1e30f)
int spmm_smiles_mask(float* logits, float* logits2, long ld, int R, int V, const int* tokens, long tok_ld, int hist_rows, int k,
                     const int* mol, int Lmax, int t, const int* t_ptr, int t_off, int t_last, const int* table, int* state_out,
                     spmm_stream_t stream);

/* Device WordPiece (csrc/tokenize.hip; spmm_amd/tokenizer.py::SmilesWordPiece is normative, spmm_amd/wordpiece_device.py builds the table and
 * holds the host form of the walk): the token rows of N strings in ONE launch, as tokenizer.encode_smiles + pad_rows make them.
 * blob, offsets: string i is the bytes blob[offsets[i] : offsets[i+1] - gap); offsets int64 [N + 1], non-decreasing by at least gap and inside
 * the blob (the caller's contract: the kernel reads exactly those bytes); gap = 1 takes "\n".join(strings) as it is.
 * head [head_len]: the text every word starts with ("[CLS]"); the word of string s is s if s starts with the head, else head + s.
 * table [table_words]: WordPieceTable.words -- a trie as an open-addressed hash of (node, byte) -> child plus a terminal id per node; layout
 * in csrc/tokenize.hip.  A table whose header does not describe itself leaves every string to the host (status 2).
 * Per string, greedy longest-match-first over the word's character positions (position 0: the vocabulary entries as written; later
 * positions: the '##' entries by their content), followed to the END of the word before anything is cut:
 *     status 2, lens 0, the row all pad_id   a byte outside 0x21..0x7E anywhere in the string (whitespace splits words, UTF-8 characters
 *                                            are not bytes): the host tokenises these
 *     status 1, lens 2, [unk_id, sep_id]     the word is longer than max_chars bytes, or some position the chain reaches matches nothing
 *                                            (also beyond the max_pieces-th piece)
 *     status 0, lens c + 1                   the ids of the first c = min(pieces, max_pieces) pieces, then sep_id
 * ids int32 [N, ld]: every entry of a row is written, pad_id behind its lens[i] entries; lens, status int32 [N].  Nothing needs zeroing.
 * Integer state only; a row's result does not depend on the rest of the launch.
 * Refused before a launch (rc = 1): N < 0; gap outside {0, 1}; head_len outside [0, 16]; max_chars outside [1, 256]; max_pieces < 1;
 * ld < max_pieces + 1; table_words outside [8, 8192]; with N > 0 a null blob, offsets, table, ids, lens or status, a null head with
 * head_len > 0, a table / ids / lens / status not 4-byte aligned, offsets not 8-byte aligned.  N == 0 returns 0 without a launch. */
int spmm_wordpiece(const unsigned char* blob, const long* offsets, int N, int gap, const unsigned char* head, int head_len,
                   const int* table, int table_words, int max_chars, int max_pieces, int unk_id, int sep_id, int pad_id,
                   int* ids, long ld, int* lens, int* status, spmm_stream_t stream);

/* One position of stochastic beam search (Kool, van Hoof, Welling 2019; csrc/sbs.hip): sequences sampled WITHOUT replacement, for G
 * property vectors ("groups") of W slots each, in ONE launch (one workgroup per group; selection and gather share the launch because
 * every state array has an _out twin, so no input is overwritten before it is read).
 * logits, noise: fp32 [G*W, V], row strides ldl, ldn -- the next-token logits of every slot's row after any warp or mask, and the caller's
 * Gumbel noise (spmm_gumbel_noise).  t (*t_ptr + t_off when t_ptr is given, clamped into [0, Lmax - 2]): the tokens every live slot
 * holds = the position the new token lands at.
 * State in, row r = g*W + s: phi_in[r] log-probability of the slot's hypothesis; gum_in[r] its perturbed key T (-inf, or NaN: an EMPTY
 * slot); fin_in[r] (uchar) the hypothesis has ended; len_in[r]; tokens_in[r, Lmax] (int32); anc_in[r, anc_ld] (spmm_decode_attn's table).
 * Candidates of a group: an empty slot none; a finished slot i exactly one -- itself: key T_i, phi_i, token [SEP] (3); a live slot i one
 * per ALLOWED token j, allowed iff logits[i, j] > -1e29 (-inf and SPMM_SYNTAX_MASKED are not); a live slot with nothing allowed none.
 * Arithmetic, fp32, every operation rounded on its own, a row's sums in a fixed order:
 *     lse = log-sum-exp of l over the allowed tokens          phi_j = phi_i + (l_j - lse)          g_j = phi_j + noise[i, j]
 *     Z = max_j g_j          v_j = T_i - g_j + log1p(-exp(g_j - Z))          key_j = T_i - max(0, v_j) - log1p(exp(-|v_j|))
 * so the arg-max child has key = T_i exactly (log1p(-1) = -inf) and every other child a smaller one; a key that is NaN (noise that is not
 * finite) is no candidate.  A search starts with slot 0 at phi = 0, T = 0 and every other slot empty: position 0 has no mode of its own.
 * Selection: the W best candidates by (key descending, flat index i*V + j ascending) become slots 0 .. W-1 in that order; slots beyond the
 * number of finite candidates become empty (gum = phi = -inf, fin = 0, len = 0, tokens 0, ids_out = 0, their own ancestry row).
 * New slot s of parent p and token v: phi, gum = the candidate's; fin = fin_in[p] | (v == [SEP]); tokens_out[s] = tokens_in[p] with
 * position t <- v if p was live; len = len_in[p] if p was finished, else t + 1; anc_out[row(s), j] = anc_in[row(p), j] for j < t (clamped
 * into [0, G*W)) and row(s) for j >= t -- spmm_beam_step's convention without rowmap: cache rows never move.  ids_out[row(s)] = v, or 0
 * for a finished or empty slot: a finished slot's row keeps being stepped with token 0; nothing descends from it (its only candidate is
 * itself, and a child's ancestry below t is its parent's), so what that row writes into its own cache row is never read.
 * parent_out (optional) [G*W]: p (s for an empty slot).  open_out[g] (int32, plain store): live, unfinished slots after the step.
 * ws: 2*G*W*V 32-bit words of scratch, 8-byte aligned (per row up to V (key image, token) pairs; W*V of them do not fit the LDS).
 * A group's result does not depend on G or on the other groups of the launch; two launches give the same bytes.
 * (Timing aid: with SPMM_SBS_PHASES = 1, 2 or 3 in the environment the kernel stops after its first, second or third phase and writes
 * no output; tools/bench_distinct.py times the phases with it.)
 * Refused before a launch (rc = 1): G < 0; W outside [1, 1024]; V outside [4, 512]; Lmax outside [2, 256]; without t_ptr a t outside
 * [0, Lmax - 1); ldl or ldn < V; anc_ld < Lmax; G*W*512 >= 2^31; with G > 0 a null logits, noise, ws, state array (in or out), ids_out or
 * open_out, a pointer (other than fin_in / fin_out) not 4-byte aligned (ws: 8), an _out array equal to its _in twin.  G == 0 returns 0 without a
 * launch. */
int spmm_sbs_step(const float* logits, long ldl, const float* noise, long ldn, int G, int W, int V, int Lmax, int t, const int* t_ptr,
                  int t_off, const float* phi_in, const float* gum_in, const unsigned char* fin_in, const int* len_in,
                  const int* tokens_in, const int* anc_in, float* phi_out, float* gum_out, unsigned char* fin_out, int* len_out,
                  int* tokens_out, int* anc_out, int anc_ld, int* ids_out, int* parent_out, int* open_out, unsigned int* ws,
                  spmm_stream_t stream);

/* Prefill of the decoder's self-attention cache (csrc/prefill.hip): the keys and values of E whole prefixes, computed by one packed pass,
 * moved into the head-major caches of spmm_decode_attn -- keys and values of a layer in ONE launch.
 * Source: K, V bf16 token-major rows with row stride ld elements, head h at column h*64 -- the K and V column blocks of the fused Q|K|V
 * projection output [src_rows, 3H] of packed rows, passed as pointers into it (ld = 3H); src_rows = the rows the source has.
 * Destination: Kc, Vc bf16 [R, nH, Lmax, 64] contiguous (decode.CachedDecoder.kc[l] / vc[l]).
 * row0, len, dst_row: device int32 [E].  For entry e, head h < nH and position j < min(len[e], Lmax):
 *     Kc[dst_row[e], h, j, :] = K[row0[e] + j, h*64 : h*64 + 64],  and the same for V.
 * Several entries may read the same source rows; entries that name the same dst_row must not overlap in position (the order of their
 * stores is undefined).
 * Safety, part of the contract: everything read from device memory is clamped or skipped -- a position with row0[e] + j outside
 * [0, src_rows) is neither read nor written; an entry with dst_row[e] outside [0, R) is skipped; len[e] <= 0 writes nothing; positions at
 * or beyond Lmax are never written.  No byte of the caches outside the named (row, head, position) cells is written and nothing outside the
 * src_rows rows (nH*64 columns of each) is read.  A pure move: 16-byte loads and stores of the same bits, NaN payloads and -0 included.
 * No LDS, no atomics; any two launches give the same bytes.
 * Refused before a launch (rc = 1): a null K, V, Kc, Vc, row0, len or dst_row with E > 0; nH < 1 or nH*64 > ld; ld not a multiple of 8;
 * K, V, Kc or Vc not 16-byte aligned (row0, len, dst_row: 4 bytes); Lmax outside [1, 256]; R < 1, E < 0, src_rows < 1.  E == 0 returns 0
 * without a launch. */
int spmm_kv_prefill(const void* K, const void* V, long ld, long src_rows, const int* row0, const int* len, const int* dst_row, int E,
                    void* Kc, void* Vc, int R, int nH, int Lmax, spmm_stream_t stream);

/* mode 0: BertEmbeddings.forward xbert.py:193-220 from token ids.  mode 1: the PV path -- property_embed Linear(1,H),
 * bernoulli mask blend with property_mask, property_cls prepend (SPMM_models.py:82-88) fused with BertEmbeddings
 * (inputs_embeds branch).  Sequence s reads PV source row s % src_mod.  mode 2: generic inputs_embeds branch of
 * BertEmbeddings (pv_x = fp32 inputs_embeds [nseq*L, H]). */
int spmm_embed_ln_fwd(int mode, const int* ids, const float* word, const float* pos, const float* type0, const float* pv_x,
                      const float* pv_mask, const float* pv_w, const float* pv_b, const float* pv_cls,
                      const float* pv_masktok, int src_mod, const float* gamma, const float* beta, void* y, void* zout,
                      float* mean, float* rstd, long nseq, int L, int H, float eps, float dropout_p,
                      const uint64_t* seed_ptr, uint64_t salt, spmm_stream_t stream);
/* Backward of the embedding sum, modes 0 and 1 only (inputs_embeds takes no gradient here); every tensor of the mode is required. */
int spmm_embed_bwd(int mode, const void* dz, const int* ids, const float* pv_x, const float* pv_mask, int src_mod,
                   float* dword, float* dpos, float* dtype0, float* d_w, float* d_b, float* d_cls, float* d_masktok,
                   long nseq, int L, int H, spmm_stream_t stream);

/* layout helpers for the NT-only GEMM: activations^T for wgrad (+ fused bias-gradient column sums), fp32 master
 * weight -> bf16 shadow and transposed bf16 shadow for dgrad, casts, row gather / scatter-add
 * (SPMM_models.py:164-183 negatives; their backward). */
int spmm_transpose_bf16(const void* in, long ldi, void* out, long ldo, int R, int C, int Rpad, float* colsum,
                        spmm_stream_t stream);
int spmm_cast_transpose(const float* in, void* out, void* outT, int R, int C, spmm_stream_t stream);
/* all transposed bf16 weight shadows in one launch; descs_dev: device array of {const float* src; bf16* dstT; int R, C, tile0, ntc} */
long spmm_cast_transpose_desc_bytes(void);
int spmm_cast_transpose_multi(const void* descs_dev, int ndesc, int total_tiles, spmm_stream_t stream);
int spmm_cast_f32_bf16(const float* in, void* out, long n, spmm_stream_t stream);
int spmm_cast_bf16_f32(const void* in, float* out, long n, spmm_stream_t stream);
int spmm_acc_rows(float* dst, long ldd, const void* src, long lds, const long* idx, long rows, int H, int atomic,
                  spmm_stream_t stream);
int spmm_gather_rows(void* dst, const void* src, const long* idx, long rows, int H, spmm_stream_t stream);

/* Row bookkeeping of a step as device kernels (csrc/plan.hip) -- what SPMM.forward does with torch.cat / indexing on whole
 * tensors (SPMM_models.py:139-150,166-199: the ITM passes' query / key-value pairings and hard negatives; :95,105,201: only
 * position 0 of those passes is read), here on packed rows and without a tensor-library launch per index array.
 *  spmm_gather_rows2: dst[r] = idx[r] < 0 ? 0 : (idx[r] & 2^40 ? srcB : srcA)[idx[r] & (2^40 - 1)]  (rows of H bf16, H % 8 == 0).
 *  spmm_add_rows_bf16: dst[idx[r]] += src[r], every idx at most once.   spmm_zero_bytes / spmm_zero_rows: 16-byte granular fill with zeros
 *   (contiguous / `rows` pieces of row_bytes at a stride).
 *  spmm_gelu_bwd: out = dz * gelu'(pre), erf-GELU (the transform of BertLMPredictionHead xbert.py:673 and the GELU of
 *   property_mtr_head SPMM_models.py:39, backward).
 *  spmm_pack_plan: from the attention mask [B, Lt] and the host's count M of valid tokens: per sequence length / first packed row
 *   (lens32, row0_32, row0_64), rows[M] = dense row of every packed row, gidx2[M + B Lt] / gidx4[2M] = gather indices that build the
 *   [packed | dense] and [packed | packed] batches of the text encoders from their dense [2B Lt] embeddings, inv[2 B Lt] = packed row of
 *   every dense row (-1: padding) for the way back, idx_m[B + M] = rows the momentum text encoder's last layer keeps of its [packed | packed]
 *   batch (position 0 of the first copy, every row of the second); *bad |= 1 when the mask is not B non-empty prefixes with M tokens in all.
 *  spmm_fusion_plan: index arrays of the fusion batch (layout in csrc/plan.hip) from the sampled negatives neg[2B] (prop | text):
 *   idx6 (assembly gather over A = [prop_embeds ; prop_embeds_causal], B = [text_embeds ; hidden10]; the text negatives re-enter as PACKED
 *   query rows at the end of the batch, Mn = sum of their lengths known only on the device), neg_rows [B Lt] (row of text_embeds behind
 *   every packed negative row, -1 past Mn), idx_top (rows the top fusion layer keeps: position 0 of the 6B ITM sequences, every row of the
 *   LM and causal-PV passes), small32 [35 B + 2] (sequence -> key/value source maps, packed row tables, CSR inverse maps of the two shared
 *   key/value sources, and rows_dev = {rows of the batch, Mn}: the device-side row counts of the launches over it). */
int spmm_gather_rows2(void* dst, const void* srcA, const void* srcB, const long* idx, long rows, int H, spmm_stream_t stream);
int spmm_add_rows_bf16(void* dst, const long* idx, const void* src, long rows, int H, spmm_stream_t stream);
int spmm_zero_bytes(void* p, long nbytes, spmm_stream_t stream);
int spmm_zero_rows(void* p, long rows, long row_bytes, long stride_bytes, spmm_stream_t stream);
int spmm_gelu_bwd(const void* dz, const void* pre, void* out, long n, spmm_stream_t stream);
int spmm_pack_plan(const int* mask, int B, int Lt, int M, int* lens32, int* row0_32, long* row0_64, long* rows, long* gidx2,
                   long* gidx4, long* inv, long* idx_m, int* bad, spmm_stream_t stream);
int spmm_fusion_plan(const long* neg, const int* lens32, const int* row0_32, int B, int Lt, int Lp, int M,
                     long* idx6, long* neg_rows, long* idx_top, int* small32, spmm_stream_t stream);

/* F.normalize(proj(cls), dim=-1) SPMM_models.py:92,95,101,105; also emits split-bf16 GEMM operands. */
int spmm_l2norm_fwd(const float* x, long ldx, float* y, float* nrm, void* a3, void* w3, void* yT, long ldt, int rows, int E,
                    spmm_stream_t stream);
int spmm_l2norm_bwd(const float* dy, const float* y, const float* nrm, const float* gscale, void* dx, int rows, int E,
                    spmm_stream_t stream);
/* soft-target contrastive loss rows + gradient (SPMM_models.py:113-131). */
int spmm_ita_rows(const float* S, const float* SM, long ldj, int nrows, int B, int J, const float* alpha_ptr,
                  const float* temp_ptr, void* dS, long ldd, int Jpad, float* losses, int loss_slot, float* dtemp,
                  int* nan_flag, spmm_stream_t stream);
/* hard negatives SPMM_models.py:154-178: one multinomial draw per row, on device. */
int spmm_sample_neg(const float* S, long ldj, int B, const long* forced, const uint64_t* seed_ptr, uint64_t salt, long* out,
                    long out_offset, spmm_stream_t stream);
/* next-token CE + distillation SPMM_models.py:233-238 and its gradient w.r.t. the student logits.  n_nonpad_ws: 4 ints, 8-byte aligned
 * (the count of non-PAD labels, then the ticket and the 64-bit fixed-point sum of the order-independent loss accumulation). */
int spmm_lm_loss(const float* logits, const float* logits_m, long ldl, const int* ids, long nseq, int L, int V,
                 const float* alpha_ptr, int* n_nonpad_ws, const float* gscale, void* dlogits, long ldd, int Vpad,
                 float* losses, int loss_slot, spmm_stream_t stream);
/* seq2seq loss of the reaction model, CrossEntropyLoss(ignore_index=0) on the shifted product SPMM_models_rxn.py:31-46, on the decoder's
 * rows as the engine holds them: logits fp32 [rows, ldl] (V real columns); ids int32 [nseq*L], the dense product; row_of [rows] = dense row
 * of every packed row (the pack plan's `rows`; null: the rows are dense).  Row r with d = row_of ? row_of[r] : r predicts ids[d + 1] unless
 * d % L == L - 1; a label of 0 or outside [0, V) is ignored and never indexes memory.  loss = mean over the n labelled rows, n counted on
 * the device by the launch itself; n = 0 gives loss 0 and dlogits 0 (the reference divides 0 by 0).  dlogits (bf16 [rows, ldd], optional):
 * gscale / n * (softmax - onehot) on labelled rows, zero elsewhere and in columns V..Vpad-1; every element is written.  n_label_ws: 4 ints,
 * 8-byte aligned, as for spmm_lm_loss. */
int spmm_s2s_loss(const float* logits, long ldl, const int* ids, const long* row_of, long rows, long nseq, int L, int V,
                  int* n_label_ws, const float* gscale, void* dlogits, long ldd, int Vpad, float* losses, int loss_slot,
                  spmm_stream_t stream);
/* Teacher-forced scoring (csrc/score.hip): the vocabulary projection of the tied LM head, log_softmax and the gather of the label's entry
 * in one launch -- the [rows, V] logits are never written.  y: bf16 [rows, H], row stride ldy, the output of cls.predictions.transform
 * (Linear, GELU, LayerNorm); Wd: bf16 [V, H], row stride ldw, the decoder weight (= the word-embedding shadow); bias: fp32 [V].
 * logit[r, v] = bias[v] + sum_h y[r,h] Wd[v,h]: bf16 operands, fp32 accumulation on v_mfma_f32_16x16x32_bf16 (the operand rounding of
 * spmm_gemm_nt with SPMM_EPI_F32); log p = logit[label] - max - log sum exp(logit - max) in fp32, the row maximum subtracted first.
 * Labels: the rule of spmm_s2s_loss -- ids int32 [nseq*L], the dense sequences; row r is dense row d = row_of ? row_of[r] : r and predicts
 * ids[d + 1] unless d % L == L - 1; a label of 0 or outside [0, V) is ignored and never indexes memory.  A scored sequence
 * [CLS] t1 .. tn [SEP] PAD.. therefore sums over t1 .. tn and [SEP], which is what the beam searches accumulate.
 * Sequences: seq_row0 / seq_len int32 [nseq] = first row and row count of every sequence (packed rows); both null: dense, sequence s owns
 * the L rows from s * L (rows == nseq * L).  A sequence's rows are clamped to [0, rows).
 * Outputs, every element written: tok_lp fp32 [rows] = log p(label) of the row, 0 where the row has no label; seq_lp fp32 [nseq] = the sum
 * of the sequence's labelled rows; seq_n int32 [nseq] = their count ((0, 0) for a sequence without a label).
 * Determinism: no floating-point atomics.  The sum over H of a (row, token) pair is one MFMA accumulator chain over ascending K-slices; it
 * does not depend on the row's place in a tile, the grid or the batch.  Each row's softmax reduction has one fixed order.  seq_lp is summed
 * in ascending row order by a second small launch.  So the same y row gives bit-identical tok_lp in any batch, seq_lp[s] is the fp32
 * left-to-right sum of its tok_lp, and two launches agree bit for bit.
 * Limits, reported as bad arguments before anything is launched: H a multiple of 64 up to 1024; 2 <= V <= 512; rows >= 1, nseq >= 1, L >= 2,
 * rows <= nseq * L; ldy, ldw multiples of 8, at least H; y, Wd 16-byte aligned (they are read 16 bytes at a time), the fp32 / int32 arrays
 * 4-byte and row_of 8-byte aligned; y, Wd, bias, ids, tok_lp, seq_lp, seq_n not null; seq_row0 and seq_len both null or both given. */
int spmm_lm_score(const void* y, long ldy, const void* Wd, long ldw, const float* bias, const int* ids, const long* row_of, long rows,
                  long nseq, int L, int V, int H, const int* seq_row0, const int* seq_len, float* tok_lp, float* seq_lp, int* seq_n,
                  spmm_stream_t stream);
/* itm_head + cross entropy SPMM_models.py:201-206 (forward and backward in one pass). */
int spmm_itm_head(const void* xa, long stride_a, const void* xb, long stride_b, int H, const float* W, const float* bias,
                  int n, int B, const float* gscale, float* losses, int loss_slot, float* logits_out, void* dxa, void* dxb,
                  float* dW, float* db, int do_bwd, int x_is_f32, spmm_stream_t stream);
/* Task head of the fine-tuning models (d_regression.py / d_classification.py / d_classification_multilabel.py): logits[B,C] =
 * A W2^T + b2 in fp32 from the GELU activations A [B,W] (bf16, row stride lda) and the fp32 masters W2 [C,W], b2 [C]; kind 0 = MSE
 * (C = 1, target float [B]), 1 = cross entropy (target int32 [B]), 2 = BCE on logits (target float [B,C]).  `loss` (optional) is
 * WRITTEN with the mean loss.  do_bwd: dA = dlogits W2 (bf16, row stride ldda), dW2 += dlogits^T A, db2 += column sums of dlogits,
 * dlogits scaled by *gscale (null: 1).  No floating-point atomics: bit-identical results launch to launch.
 * 1 <= B <= 1024, 1 <= C <= 64, W a multiple of 64 up to 4096. */
int spmm_task_head(const void* A, long lda, int B, int W, const float* W2, const float* b2, int C, int kind, const void* target,
                   const float* gscale, float* logits, float* loss, void* dA, long ldda, float* dW2, float* db2, int do_bwd,
                   spmm_stream_t stream);
/* One launch that closes step i of the SMILES -> PV regression loop (d_smiles2pv.py:14-52) and opens step i + 1, for `rows` molecules.
 * y [rows, H] bf16 (row stride ldy): the transform part of property_mtr_head (Linear, GELU, LayerNorm; SPMM_models.py:39-41) on the
 * last-position rows.  Per row r:  p = b3[0] + sum_h y[r,h] w3[h] in fp32 (property_mtr_head.3, :42) -> pred[r*ldp + i];  then, unless
 * i == n_props - 1 (no next step: the cache is not touched), the embedded prefix row of position j = i + 1,
 *   LayerNorm(p pe_w + pe_b + pos[j] + type0) gamma + beta   (property_embed :36; BertEmbeddings, inputs_embeds branch xbert.py:209-218:
 *   the zero token type's row IS added there -- type0 null leaves it out), as bf16 -> xcache[(r*Lc + j)*H ..], Lc = n_props + 1.
 * xcache [rows, Lc, H] is the append-only cache of embedded prefix rows (row 0: the embedded property_cls, written by the caller);
 * w3, pe_w, pe_b, type0, gamma, beta: fp32 [H]; b3: fp32 [1]; pos: the PV encoder's position table [>= Lc, H]; all device memory.
 * One wave per row.  H a multiple of 64 up to 1024, 0 <= i < n_props, ldy >= H (a multiple of 4), ldp >= n_props.
 * Alignment: the fp32 vectors (w3, pe_w, pe_b, pos, type0, gamma, beta) are read 16 bytes at a time and y / xcache 8 bytes at a time, so
 * their base pointers must be 16-byte (y, xcache: 8-byte) aligned; violations are reported as a bad argument. */
int spmm_s2p_append(const void* y, long ldy, const float* w3, const float* b3, const float* pe_w, const float* pe_b, const float* pos,
                    const float* type0, const float* gamma, const float* beta, float eps, float* pred, long ldp, void* xcache,
                    long rows, int H, int n_props, int i, spmm_stream_t stream);
/* property_mtr_head final Linear(H,1) + masked MSE * 5 SPMM_models.py:251-256.  n_keep_ws: 4 ints, 8-byte aligned (as n_nonpad_ws). */
int spmm_mpm_head(const void* h, int Lp, int H, const float* w, const float* bias, const float* target, const float* mask,
                  int B, int* n_keep_ws, const float* gscale, float* losses, int loss_slot, float* pred_out, void* dh,
                  float* dw, float* db, int do_bwd, int x_is_f32, spmm_stream_t stream);
/* Small dense heads of the inference tier: out[r,n] = act(bias[n] + sum_k x[r,k] W[n,k]) in fp32 (x fp32 or bf16; act 0 = none,
 * 1 = erf-GELU) -- property_embed / property_proj / text_proj / itm_head / property_mtr_head called as modules on a few rows
 * (SPMM_models.py:36-43; d_smiles2pv.py:15-25, d_pv2smiles_batched.py:25-27). */
int spmm_rows_linear(const void* x, int x_is_bf16, long ldx, const float* W, const float* bias, float* out, long ldo, long rows,
                     int N, int K, int act, spmm_stream_t stream);
/* Retrieval (csrc/retrieve.hip): the k most similar library rows of every query, streamed -- the [Q, n] similarity matrix of
 * SPMM_models.py:108-111 (feat @ feat_all) is never formed.  q: fp32 [Q, E], row stride ldq; f: fp32 [n, E], row stride ldf, ONE CHUNK of a
 * library whose row i has the library index base + i.  State (in/out): scores fp32 [Q, k] and index int64 [Q, k], contiguous.
 *   merge = 0: the state is overwritten with the chunk's k best;  merge = 1: the chunk's candidates are merged with the state already there
 *   (chunks of one library must not overlap: an index offered twice is kept twice).
 * Contract: row j of scores / index holds the k largest q_j . f_i over every row seen so far, largest first, equal scores by ascending
 * library index; slots beyond the number of rows seen hold (-inf, -1); a NaN similarity ranks below every number (and above an empty
 * slot, so it is returned only when fewer than k numbers exist).  -0 and +0 are equal scores (returned as +0).  The sum over E has one fixed order
 * per (query, row) pair -- one exact-f32 MFMA accumulator chain (v_mfma_f32_16x16x4_f32, a k-ordered fmaf chain: one rounding per product,
 * fp32-grade) that does not depend on the row's place in a tile, a chunk or the grid -- so streaming a library in ANY chunking gives
 * bit-identical scores and identical indices to one call over the whole library, and two launches on the same inputs agree bit for bit.
 * No floating-point atomics.
 * cut_scores fp32 [Q] / cut_index int64 [Q] (optional, both or neither): only chunk rows that rank strictly BELOW the candidate
 * (cut_scores[j], cut_index[j]) are eligible for query j (none when cut_index[j] < 0) -- the next 64 of a ranking longer than 64: a second
 * pass over the library with the last entry of the first pass as the cut.  The state read by merge = 1 is not filtered.
 * workspace: spmm_sim_topk_workspace_bytes(Q, n, k) bytes, 16-byte aligned, private to the call until it completes on `stream` (the
 * per-workgroup partial lists between the scan launch and the merge launch); not needed when n = 0.
 * Limits, reported as bad arguments: 1 <= k <= 64; E a multiple of 64 up to 512; Q >= 1; 0 <= n <= 2^31 - 256 rows per chunk (n = 0 with
 * merge = 1 leaves the state as it is, with merge = 0 it empties the state); q, f 16-byte aligned; ldq, ldf multiples of 4, at least E;
 * base >= 0. */
long spmm_sim_topk_workspace_bytes(int Q, long n, int k);
int spmm_sim_topk(const float* q, long ldq, const float* f, long ldf, long base, int Q, long n, int E, int k, float* scores, long* index,
                  int merge, const float* cut_scores, const long* cut_index, void* workspace, long workspace_bytes, spmm_stream_t stream);
/* Library clustering (csrc/cluster.hip): spherical k-means and farthest-first picks on the features spmm_sim_topk searches.
 *
 * spmm_centroid_assign: the nearest centre of every row, streamed -- the [n, Kc] similarity matrix is never formed.  f: fp32 [n, E], row
 * stride ldf; c: fp32 [Kc, E], row stride ldc, ONE CHUNK of a centre list whose row j has the centre index c0 + j.  State (in/out): best
 * fp32 [n] and assign int32 [n].
 *   merge = 0: the state is overwritten with the chunk's best centre;  merge = 1: the state already there competes as one more candidate
 *   (centre lists processed in chunks; with Kc = 1, one step of farthest-first traversal: best becomes the similarity to the nearest pick).
 * Contract: candidates are ordered exactly as spmm_sim_topk orders them -- larger score first, equal scores by ascending centre index, NaN
 * below every number, -0 and +0 equal (returned as +0); with merge = 1 a state of (-inf, -1) is the empty slot (any assign < 0 is).  The
 * score of (row, centre) is that kernel's accumulator chain (v_mfma_f32_16x16x4_f32; 16-element step ascending, then component, then lane
 * group), so best / assign are bit-identical to spmm_sim_topk(q = f, f = c, k = 1, base = c0, merge), for any chunking of the centres; two
 * launches on the same inputs agree bit for bit.  No workspace, no floating-point atomics.
 * prev int32 [n] / changed (device int), optional, both or neither: *changed += the number of rows whose final assign differs from prev
 * (an integer atomic: the count is deterministic).  prev must not alias assign.
 * Limits, reported as bad arguments: E a multiple of 64 up to 512; Kc >= 1; c0 >= 0 and c0 + Kc <= 2^31 - 1; 0 <= n <= 2^31 - 256 (n = 0 is a
 * no-op); f, c 16-byte aligned; ldf, ldc multiples of 4, at least E; merge 0 or 1. */
int spmm_centroid_assign(const float* f, long ldf, const float* c, long ldc, long c0, long n, int Kc, int E, float* best, int* assign,
                         int merge, const int* prev, int* changed, spmm_stream_t stream);
/* spmm_cluster_group: the members of every cluster, a stable counting sort of the rows by assign int32 [n].  counts int32 [K]; offsets int64
 * [K + 1] (offsets[0] = 0, offsets[K] = the number of rows in a cluster); members int32 [n]: the rows of cluster c are
 * members[offsets[c] : offsets[c + 1]] in ASCENDING row order (entries past offsets[K] are not written).  A row whose assign is outside
 * [0, K) -- -1, the empty slot -- is in no cluster; *outside (device int, overwritten) counts those rows.  Integer atomics only: the result
 * does not depend on the grid.  workspace: spmm_cluster_group_workspace_bytes(n, K) bytes, 16-byte aligned, private to the call.
 * Limits, reported as bad arguments: 1 <= K <= 2^24; 0 <= n <= 2^31 - 256. */
long spmm_cluster_group_workspace_bytes(long n, int K);
int spmm_cluster_group(const int* assign, long n, int K, int* counts, long* offsets, int* members, int* outside, void* workspace,
                       long workspace_bytes, spmm_stream_t stream);
/* spmm_cluster_centroids: per cluster c of a grouping (counts / offsets / members of spmm_cluster_group over f fp32 [n, E], row stride ldf):
 *   the fp32 sum of its members' rows, in an order fixed by the member list alone -- pieces of 256 consecutive members summed in member
 *   order, the piece sums added in ascending order (a 500 000-member cluster is 1 954 workgroups and one combining pass, not one chain);
 *   norm[c] fp32 = the length of that sum (0 for an empty cluster);
 *   centres[c, :] (fp32, row stride ldc) = sum / norm, written ONLY when the cluster has members and norm >= 1e-12: otherwise the row is
 *   left as it was (spherical k-means keeps the old centre of an empty or cancelled cluster until the host re-seeds it);
 *   medoid[c] int32 = the member with the largest best[row] in spmm_sim_topk's score order (NaN lowest, -0 = +0), ties to the lowest row;
 *   -1 for an empty cluster.
 * No floating-point atomics; two launches on the same inputs agree bit for bit.  workspace: spmm_cluster_centroids_workspace_bytes(n, K, E)
 * bytes, 16-byte aligned, private to the call.  Limits, reported as bad arguments: 1 <= E <= 512; 1 <= K <= 2^24; 0 <= n <= 2^31 - 256;
 * ldf, ldc at least E. */
long spmm_cluster_centroids_workspace_bytes(long n, int K, int E);
int spmm_cluster_centroids(const float* f, long ldf, long n, int E, const float* best, const int* counts, const long* offsets,
                           const int* members, int K, float* centres, long ldc, float* norm, int* medoid, void* workspace,
                           long workspace_bytes, spmm_stream_t stream);
/* Threshold clustering (csrc/neighbors.hip): every pair of library rows more similar than a threshold, and Taylor-Butina / first-come
 * leaders on that list -- the number of clusters is a result, not an argument.
 *
 * spmm_sim_range: the neighbours of every row above `threshold`, streamed -- the [n, nc] similarity matrix is never formed.  f: fp32 [n, E],
 * row stride ldf, the rows with the library indices r0 .. r0 + n - 1; c: fp32 [nc, E], row stride ldc, ONE CHUNK of the column side whose
 * row j has the library index c0 + j (a self-join passes the same library on both sides).  State (in/out): counts int32 [n].
 *   count mode (offsets = nbr = NULL, nbr_len = 0): counts[i] += the hits of row i in this chunk;
 *   emit mode (offsets int64 [n], nbr int32 [nbr_len]): hit number p of row i in this chunk, p counted in ascending j, is written as c0 + j
 *   to nbr[offsets[i] + counts[i] + p]; after that counts[i] += the hits.  A position outside [0, nbr_len) is not written and the count
 *   still advances: a wrong offsets can lose entries but never writes outside nbr.
 * Contract: (i, j) is a hit when score(i, j) >= threshold -- a float compare, so a NaN score never hits -- and r0 + i != c0 + j: the
 * diagonal is never a neighbour, an exact copy elsewhere in the library is.  The score is the accumulator chain of spmm_sim_topk /
 * spmm_centroid_assign (v_mfma_f32_16x16x4_f32; 16-element step ascending, then component, then lane group): bit-identical to those
 * kernels', and score(i, j) has the bits of score(j, i), so the neighbour relation of a self-join is exactly symmetric.  Column chunks
 * offered in ascending c0 give every row's list in ascending library index, and ANY chunking of the columns (or of the rows, with r0 and
 * the matching slices of counts / offsets) gives the same bytes; two launches on the same inputs agree bit for bit.  A wave is the only
 * writer of its rows' lists and counts: no atomics on nbr, no floating-point atomics, no sort, no workspace.
 * Limits, reported as bad arguments: E a multiple of 64 up to 512; 0 <= n, nc <= 2^31 - 256 (either being 0 is a no-op); r0, c0 >= 0 and
 * r0 + n, c0 + nc <= 2^31 - 1; threshold not NaN; f, c 16-byte aligned; ldf, ldc multiples of 4, at least E; offsets, nbr and nbr_len all
 * given or none; nbr_len >= 0. */
int spmm_sim_range(const float* f, long ldf, long r0, long n, const float* c, long ldc, long c0, long nc, int E, float threshold,
                   int* counts, const long* offsets, int* nbr, long nbr_len, spmm_stream_t stream);
/* spmm_leader_round / spmm_leader_finish: the leaders of a SYMMETRIC neighbour list (offsets int64 [n + 1], nbr int32 [nbr_len]: the
 * neighbours of row i are nbr[offsets[i] : offsets[i + 1]]; entries outside [0, n) are ignored, positions outside [0, nbr_len) never read).
 * The sequential rule: visit the rows in priority order; a row not yet claimed becomes a leader and claims its unclaimed neighbours.
 * Priority: by_count = 1 (Taylor-Butina) more neighbours first -- counts int32 [n] -- equal counts to the LOWER row (RDKit's
 * Butina.ClusterData gives equal counts to the higher index); by_count = 0 (leader / sphere exclusion: keep the first occurrence) the
 * lower row first, counts may be NULL.  On a symmetric relation the leaders are the lexicographically first maximal independent set,
 * which one round computes in parallel: state int32 [n] is 0 (open), 1 (leader) or 2 (member); an open row with a leader among its
 * neighbours of higher priority becomes a member, one whose neighbours of higher priority are all members (or that has none) becomes a
 * leader, any other stays open.  A round reads state_in and writes every row of state_out (they must be two buffers); *open_out (device
 * int) += the rows still open, one integer atomic per wave.  Start from zeros and repeat until a round leaves no row open: every round
 * decides at least the best open row; a path under row priority needs n rounds, a typical similarity graph a handful.
 * spmm_leader_finish: leader[i] int32 = i for a leader, else the highest-priority leader among i's neighbours -- the one that claims it in
 * the sequential run (-1 for a row that is neither: an open row, a member without a leader).  One wave64 per row, its lanes striding the
 * list.  Integer-exact; two launches agree bit for bit.
 * Refused as bad arguments: null pointers (counts only with by_count = 1), n outside [0, 2^31 - 256] (n = 0 is a no-op), nbr_len < 0,
 * by_count other than 0 or 1, state_in == state_out. */
int spmm_leader_round(const int* counts, const long* offsets, const int* nbr, long nbr_len, long n, int by_count, const int* state_in,
                      int* state_out, int* open_out, spmm_stream_t stream);
int spmm_leader_finish(const int* counts, const long* offsets, const int* nbr, long nbr_len, long n, int by_count, const int* state,
                       int* leader, spmm_stream_t stream);
/* _dequeue_and_enqueue SPMM_models.py:272-286 (+ the bf16 GEMM shadows of the queue).  skip_flag (optional, device int): when
 * non-zero neither the queue nor the pointer is touched -- the reference's NaN guard returns before the enqueue
 * (SPMM_models.py:132-134 vs :208), so a non-finite momentum feature never enters the queue. */
int spmm_enqueue(const float* feats, int n, int E, float* queue, int Q, void* w3, void* qT, long ldt, int Bloc, long* ptr,
                 int advance, const int* skip_flag, spmm_stream_t stream);
int spmm_queue_shadow(const float* queue, int E, int Q, void* w3, void* qT, long ldt, int Bloc, spmm_stream_t stream);
/* temp.clamp_(0.01, 0.5) SPMM_models.py:80-81 */
int spmm_clamp_scalar(float* p, float lo, float hi, spmm_stream_t stream);

/* clip_grad_norm_(5.) + AdamW SPMM_models.py:340,361-362 and the EMA of the momentum encoders :266-269. */
long spmm_adam_scalars_bytes(void);
long spmm_grad_sqnorm_workspace_bytes(void);
/* deterministic (fixed-order) sum of squares: replicas with identical gradients get identical clip coefficients */
int spmm_grad_sqnorm(const float* g, long n, float* out_zeroed, float* workspace, spmm_stream_t stream);
int spmm_adamw_step(float* p, const float* g, float* m, float* v, void* bf16_shadow, long n, const float* lr_ptr,
                    float beta1, float beta2, float eps, float weight_decay, const float* normsq, float max_norm, int* step,
                    const int* nan_flag, void* scalars_ws, spmm_stream_t stream);
int spmm_ema_update(float* pm, const float* p, void* bf16_shadow, long n, float momentum, spmm_stream_t stream);
int spmm_axpy_scalar(float* dst, const float* src, const float* scale_ptr, float scale, int n, spmm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SPMM_HIP_H */
