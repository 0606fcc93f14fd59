/*
 * db1_hip.h -- C ABI of libdb1_hip.so: the MI355X (gfx950) kernels behind the DB1
 * hot path (Transformer-XL decoder fwd/bwd, image-patch embedder, masked CE,
 * fused Adam, mu-law tokenizer).
 *
 * The reference (Shanghai-Digital-Brain-Laboratory/BDM-DB1) has NO native boundary
 * on this path: it is eager PyTorch (src/model/transformer_xl.py) under DeepSpeed.
 * Each entry point below therefore cites the reference Python lines whose
 * arithmetic it replaces; bdm_db1_amd/ binds them with ctypes (INTEGRATION.md
 * shows the stub a reference maintainer would add).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch-ROCm tensors are
 *     only containers).  The library never allocates, frees or synchronises: there is no
 *     hipMalloc / hipFree / hipDeviceSynchronize behind any entry point.  An entry point
 *     that needs scratch takes (void* ws, int64_t ws_bytes) -- 16-byte aligned device memory
 *     the caller owns -- and has a query  int64_t db1_<op>_workspace_bytes(shape...)  that
 *     returns what that call needs (0 = none, ws may then be NULL); too little workspace is
 *     DB1_ERR_WORKSPACE_TOO_SMALL, except for the GEMMs, which then take a kernel that needs
 *     none.  The scratch is dead when the call's work on the stream is done: one buffer of the
 *     largest size serves every call of a stream;
 *   - every call is asynchronous on the given hipStream_t (passed as void*) and may be
 *     captured into a hipGraph;
 *   - return value: 0 = ok, negative = DB1_ERR_*; db1_last_error() gives a
 *     thread-local message; no C++ exception crosses the boundary;
 *   - dtype codes: DB1_F32 / DB1_BF16; "acc" outputs are float32 and are
 *     ACCUMULATED into (+=), so gradient accumulation and tied parameters are free;
 *   - no global mutable state: the library keeps one immutable per-device cache ("this kernel's
 *     dynamic-LDS attribute is set", std::call_once) and reads its A/B environment switches
 *     once; the kernel-steering hooks of the tests are thread-local and live in db1_hip_test.h.
 *     Any number of host threads / devices / streams may call concurrently;
 *   - no float atomics anywhere: every reduction across workgroups goes through partial sums (in the workspace) that are added in a fixed
 *     order, or has a single contributor per output -- the same inputs give the same bits, with or without a workspace.
 */
#ifndef DB1_HIP_H
#define DB1_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { DB1_F32 = 0, DB1_BF16 = 1 };
enum {
    DB1_OK = 0,
    DB1_ERR_BAD_SHAPE = -1,
    DB1_ERR_BAD_ALIGN = -2,
    DB1_ERR_UNSUPPORTED_DTYPE = -3,
    DB1_ERR_WORKSPACE_TOO_SMALL = -4,
    DB1_ERR_HIP = -5,
    DB1_ERR_UNSUPPORTED = -6
};
enum { DB1_ACT_GEGLU = 0, DB1_ACT_GELU = 1, DB1_ACT_RELU = 2 };

int db1_version(void);
const char* db1_last_error(void);
/* 1 if the running device is gfx950; product code refuses to run otherwise. */
int db1_device_is_gfx950(void);

/* ------------------------------------------------------------------ GEMM
 * C[z][m,n] = alpha * sum_k A[z][m,k] * B[z][k,n] + beta * C[z][m,n] + bias[n]
 * Fully strided (element (m,k) of A at A + m*a_rs + k*a_cs, etc.), two-level batch
 * z = z0*batch1 + z1 with per-level strides.  fp32 accumulation always.  Replaces
 * nn.Linear / torch.einsum (transformer_xl.py:136-141,163-170,220,228,264-268,595).
 * Dispatch: bf16 operands whose strides form a K-major/M-major pattern with the
 * alignment the MFMA tile kernels need go to the 128x128x64 bf16 MFMA kernels
 * (NT / NN / TN); everything else (fp32 parity gate, odd shapes, tiny models) goes to
 * a strided kernel on the exact-fp32 MFMA (v_mfma_f32_16x16x4_f32).
 */
int db1_gemm_strided(const void* A, const void* B, void* C, const void* bias,
                     int M, int N, int K, int dtA, int dtB, int dtC, int dtBias,
                     int64_t a_rs, int64_t a_cs, int64_t b_rs, int64_t b_cs, int64_t c_rs, int64_t c_cs,
                     int batch0, int batch1,
                     int64_t a_bs0, int64_t a_bs1, int64_t b_bs0, int64_t b_bs1, int64_t c_bs0, int64_t c_bs1,
                     float alpha, float beta, void* ws, int64_t ws_bytes, void* stream);
/* Scratch of the deterministic split-K path (fp32 partial sums of outputs too small to fill the chip, added in a fixed order).
 * Without it (ws NULL / smaller) the same product runs on a kernel that needs none: results are equally valid, large-K weight
 * gradients are slower. */
int64_t db1_gemm_workspace_bytes(int M, int N, int K, int dtA, int dtB, int dtC,
                                 int64_t a_rs, int64_t a_cs, int64_t b_rs, int64_t b_cs, int64_t c_rs, int64_t c_cs,
                                 int batch0, int batch1);
/* which kernel db1_gemm_strided takes for this product given ws_bytes of workspace (-1: as much as it wants):
 * 0 strided fp32-MFMA, 1 128x128 tile, 2 256x128 tile, 3 / 4 256x256 8-wave (k64 x 2 / k32 x 4), 5 256x256 4-wave hand-scheduled,
 * 6 skinny W-streaming, 7 256x128 4-wave hand-scheduled; +16 split-K through the workspace; +32 the last partial wave of tile rows runs as a second call */
int db1_gemm_kernel_choice(int M, int N, int K, int dtA, int dtB, int dtC,
                           int64_t a_rs, int64_t a_cs, int64_t b_rs, int64_t b_cs, int64_t c_rs, int64_t c_cs,
                           int batch0, int batch1, float beta, int64_t ws_bytes);
/* Row-major 2-D conveniences.  nt: C = A[M,K] * B[N,K]^T (y = x W^T);
 * nn: C = A[M,K] * B[K,N] (dx = dy W);  tn: C = A[K,M]^T * B[K,N] (dW = dy^T x). */
/* db1_gemm_strided with a structural-zero hint for A (an optimisation only: results are those of the plain call):
 *   tri_mode 1: A[m, k] == 0 for k > m;   tri_mode 2: A[m, k] == 0 for (k mod tri_period) < m.
 * Used for the two contractions over dT (dS re-indexed by distance, zero above the causal diagonal): dq_r = dT.R (mode 1) and
 * dR = dT^T.(q+v) over k = (batch, query) (mode 2, period = L): the k-tiles that are zero by construction are never read. */
int db1_gemm_strided_tri(const void* A, const void* B, void* C, const void* bias, int M, int N, int K, int dtA, int dtB, int dtC, int dtBias,
                         int64_t a_rs, int64_t a_cs, int64_t b_rs, int64_t b_cs, int64_t c_rs, int64_t c_cs, int batch0, int batch1,
                         int64_t a_bs0, int64_t a_bs1, int64_t b_bs0, int64_t b_bs1, int64_t c_bs0, int64_t c_bs1, float alpha, float beta,
                         int tri_mode, int tri_period, void* ws, int64_t ws_bytes, void* stream);
int db1_gemm_nt(const void* A, const void* B, void* C, const void* bias, int M, int N, int K,
                int64_t lda, int64_t ldb, int64_t ldc, int dtAB, int dtC, float alpha, float beta, void* ws, int64_t ws_bytes, void* stream);
/* The attention input projection (transformer_xl.py:136-141,160-175): C[M,N] = A[M,K] * W[N,K]^T in bf16, except that the columns n < split_n
 * (the query block) are written as acc + bias_u[n] to Cu and acc + bias_v[n] to Cv (row stride ld_uv) instead of to C: q + r_w_bias and
 * q + r_r_bias leave the GEMM's accumulators directly (no separate pass, one rounding).  Large shapes only (see _supported). */
int db1_gemm_nt_headbias_supported(int M, int N, int K, int split_n);
int db1_gemm_nt_headbias(const void* A, const void* W, void* C, void* Cu, void* Cv, const void* bias_u, const void* bias_v, int M, int N, int K,
                         int split_n, int64_t lda, int64_t ldw, int64_t ldc, int64_t ld_uv, void* stream);
int db1_gemm_nn(const void* A, const void* B, void* C, const void* bias, int M, int N, int K,
                int64_t lda, int64_t ldb, int64_t ldc, int dtAB, int dtC, float alpha, float beta, void* ws, int64_t ws_bytes, void* stream);
int db1_gemm_tn(const void* A, const void* B, void* C, const void* bias, int M, int N, int K,
                int64_t lda, int64_t ldb, int64_t ldc, int dtAB, int dtC, float alpha, float beta, void* ws, int64_t ws_bytes, void* stream);
/* The "bias + GEGLU" epilogue of the feed-forward GEMMs (PositionwiseFF, transformer_xl.py:246-292; GEGLU = a * gelu_erf(b),
 * activations.py:19-32).  Forward: Z[M, 2 dff] = A[M, K] * W1[2 dff, K]^T + bias AND ACT[M, dff] = Z[:, :dff] * gelu(Z[:, dff:]) from the
 * same accumulators (ACT is computed from the ROUNDED Z, i.e. it equals db1_ffn_act_fwd on the stored Z bit for bit).  Backward:
 * dact = dY[M, K] * W2[K, dff] is never stored; the epilogue reads Z and writes dZ[M, 2 dff] = (dact * gelu(g), dact * v * gelu'(g)) and
 * dbias_acc[2 dff] (fp32) += the column sums of the stored dZ, added in a fixed order (the same arithmetic per element as db1_gemm_nn +
 * db1_ffn_act_bwd_bias).  Large bf16 shapes run fused inside the 4-wave tile GEMM (..._fused() says which: 1 = fused, the separate
 * activation passes over Z disappear); every other shape / dtype runs the equivalent separate launches.  dt: operands, Z, ACT, bias. */
int db1_gemm_nt_geglu_fused(int M, int dff, int K, int dt, int64_t lda, int64_t ldw, int64_t ldz, int64_t ldact);
int db1_gemm_nt_geglu(const void* A, const void* W1, const void* bias, void* Z, void* ACT, int M, int dff, int K,
                      int64_t lda, int64_t ldw, int64_t ldz, int64_t ldact, int dt, void* ws, int64_t ws_bytes, void* stream);
int db1_gemm_nn_geglu_bwd_fused(int M, int dff, int K, int dt, int64_t lddy, int64_t ldw, int64_t ldz, int64_t lddz);
int64_t db1_gemm_nn_geglu_bwd_workspace_bytes(int M, int dff, int K, int dt, int64_t lddy, int64_t ldw, int64_t ldz, int64_t lddz);
int db1_gemm_nn_geglu_bwd(const void* dY, const void* W2, const void* Z, void* dZ, float* dbias_acc, int M, int dff, int K,
                          int64_t lddy, int64_t ldw, int64_t ldz, int64_t lddz, int dt, void* ws, int64_t ws_bytes, void* stream);
/* ... WITHOUT the bias reduce (fused shapes only): parts [M / 128][2 dff] float32 = the column sums of dZ per 128-row block */
int db1_gemm_nn_geglu_bwd_parts(const void* dY, const void* W2, const void* Z, void* dZ, float* parts, int M, int dff, int K,
                                int64_t lddy, int64_t ldw, int64_t ldz, int64_t lddz, int dt, void* stream);
/* which kernel db1_gemm_strided would pick: 0 = strided fp32-MFMA, 1 = bf16 MFMA tile kernel */
int db1_gemm_would_use_fast(int M, int N, int K, int dtA, int dtB, int dtC,
                            int64_t a_rs, int64_t a_cs, int64_t b_rs, int64_t b_cs, int64_t c_rs, int64_t c_cs);

/* ------------------------------------------------------------------ residual + LayerNorm
 * s = alpha * x + r ; y = LayerNorm(s) * gamma + beta   (transformer_xl.py:231-238, 288-290;
 * alpha = DeepNorm alpha or 1).  r may be NULL (plain LN, pre-LN models).  s_out (may alias r,
 * may be NULL) receives s for the backward.  mean/rstd: float32 [rows]. */
/* Dropout (transformer_xl.py:229,262-269: on the attention / feed-forward output before the residual sum) is part of this kernel:
 * with drop_p > 0, s = alpha * x + dropout(r).  No mask is stored: keep decisions are a counter-based function (Philox4x32-10) of
 * (drop_seed, drop_step, drop_site, element index) -- see db1_dropout -- and the backward regenerates them.
 * drop_step_dev (nullable, device): the step used is drop_step + *drop_step_dev, read when the kernel RUNS -- a captured hipGraph of a
 * training micro-step (bdm_db1_amd.GraphedTrainStep) draws new masks at every replay by bumping that counter. */
int db1_layernorm_residual_fwd(const void* x, const void* r, float alpha, const void* gamma, const void* beta,
                               void* y, void* s_out, float* mean, float* rstd,
                               int64_t rows, int d, float eps,
                               float drop_p, uint64_t drop_seed, uint32_t drop_site, uint32_t drop_step, const uint32_t* drop_step_dev,
                               int dt, int dtParam, void* stream);
/* ds = dL/ds (dtype dt); dr_out (nullable) = dL/dr = ds under the forward's keep decisions (== ds when drop_p = 0);
 * dgamma_acc / dbeta_acc: float32 [d], accumulated.
 * drop_rows_per_step (0: off): the rows are SEVERAL micro-steps' rows, drop_rows_per_step each, run through one backward (a whole gradient-
 * accumulation window, TransformerXL's deferred backward): row r takes the keep decisions of step drop_step + r / drop_rows_per_step, its
 * elements counted from the first row of its block -- what that micro-step's own forward drew. */
int64_t db1_layernorm_residual_bwd_workspace_bytes(int64_t rows, int d, int dt);   /* per-block parameter-gradient partials */
int db1_layernorm_residual_bwd(const void* dy, const void* s, const void* gamma, const float* mean, const float* rstd,
                               void* ds, void* dr_out, float* dgamma_acc, float* dbeta_acc,
                               int64_t rows, int d,
                               float drop_p, uint64_t drop_seed, uint32_t drop_site, uint32_t drop_step, const uint32_t* drop_step_dev,
                               int64_t drop_rows_per_step, int dt, int dtParam, void* ws, int64_t ws_bytes, void* stream);
/* the same launch WITHOUT the parameter reduce: the per-block partial sums [blocks][2][d] float32 (parts_bytes >=
 * db1_layernorm_residual_bwd_workspace_bytes; bf16 rows of the register-resident widths only, else DB1_ERR_UNSUPPORTED) stay in `parts`;
 * db1_colsum_acc over that [blocks, 2 d] matrix yields (dgamma | dbeta).  For gradient accumulation: one reduce per optimizer step. */
int db1_layernorm_residual_bwd_parts(const void* dy, const void* s, const void* gamma, const float* mean, const float* rstd,
                                     void* ds, void* dr_out, float* parts, int64_t parts_bytes, int64_t rows, int d,
                                     float drop_p, uint64_t drop_seed, uint32_t drop_site, uint32_t drop_step, const uint32_t* drop_step_dev,
                                     int64_t drop_rows_per_step, int dt, int dtParam, void* stream);

/* ------------------------------------------------------------------ dropout
 * y[e] = x[e] * keep(e) * 65536 / (65536 - thr),  thr = round(p * 65536)   (nn.Dropout, transformer_xl.py:409,545,575; y may alias x).
 * keep(e) = [ u16(e) >= thr ] where the eight 16-bit uniforms of elements 8b .. 8b+7 are the 128 output bits of Philox4x32-10 on
 * counter (b lo, b hi, site, step) under key (seed lo, seed hi), low half-word first.  The same call is its own backward
 * (dx = dropout(dy) with the same seed / site / step).  n: a multiple of 8. */
int db1_dropout(const void* x, void* y, int64_t n, float p, uint64_t seed, uint32_t site, uint32_t step, const uint32_t* step_dev, int dt, void* stream);

/* ------------------------------------------------------------------ feed-forward activation
 * GEGLU: out[r, j] = z[r, j] * gelu_erf(z[r, n + j]) (activations.py:19-32); GELU/RELU: elementwise. */
int db1_ffn_act_fwd(const void* z, void* out, int64_t rows, int n_out, int act, int dt, void* stream);
int db1_ffn_act_bwd(const void* z, const void* dout, void* dz, int64_t rows, int n_out, int act, int dt, void* stream);
/* same, and dbias_acc[c] += sum_r dz[r, c] over all columns of dz (float32 [2*n_out] for GEGLU, [n_out] otherwise): the
 * gradient of the first feed-forward bias (transformer_xl.py:264) from the same pass; fixed summation order. */
int64_t db1_ffn_act_bwd_bias_workspace_bytes(int64_t rows, int n_out, int act);
int db1_ffn_act_bwd_bias(const void* z, const void* dout, void* dz, float* dbias_acc, int64_t rows, int n_out, int act, int dt,
                         void* ws, int64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ inference with memory: the linear maps between two attention launches
 * ONE new token (batch 1) through o_net (fed by the merge of the decode attention's chunk partials, as db1_linear_decode_attn) -> LayerNorm
 * -> ff1 + GEGLU -> ff2 -> LayerNorm -> the NEXT layer's qkv projection, as one launch of 256 persistent workgroups whose weight stream never
 * stops (csrc/decode_chain.hip; transformer_xl.py:227-243,246-292,136; evaluate_rl.py:157-266).  w_qkv_next NULL = the last layer: the launch
 * ends with ff2 and hands back h1_out (LN1's row) and f_out (ff2's row) for the head's own input LayerNorm.  All rows bf16.
 * The workgroups hand the stage vectors over through scratch rows of tagged 32-bit words ({bf16, tag = slot + 1}; polled until every word
 * carries the launch's tag): scratch = db1_decode_chain_scratch_bytes() bytes, ZEROED ONCE when allocated and then left alone; consecutive
 * launches on one scratch must use DIFFERENT slots (0 .. 65534; the layer index, so n_layer >= 2) and run one after the other (one stream).
 * w_o_next (or NULL): the w_o of the launch that follows; its lines are touched so that they wait in L2 / the memory-side cache.
 * The int at db1_decode_chain_error_offset() is set to 1 when a poll ran into its limit (all 256 workgroups must be resident at once;
 * results invalid).  Built for d = 2048, dff = 4096, d_head = 128 on a device with >= 256 CUs (db1_decode_chain_supported checks both). */
int db1_decode_chain_supported(int d, int dff, int H, int D, int nunit);
int64_t db1_decode_chain_scratch_bytes(void);
int64_t db1_decode_chain_error_offset(void);
int db1_decode_chain(const float* att_part, int nunit, int H, const void* x_res, const void* w_o, const void* w1, const void* b1, const void* w2,
                     const void* b2, const void* w_qkv_next, const void* w_o_next, const void* g1, const void* be1, const void* g2, const void* be2,
                     float alpha, float eps, void* h1_out, void* f_out, void* x_next, void* qkv_next, void* scratch, int slot, int d, int dff, void* stream);

/* out_acc[c] += sum_r x[r, c]  (bias / u / v gradients). ldx = row stride in elements. */
int64_t db1_colsum_acc_workspace_bytes(int64_t rows, int cols);   /* per-chunk partials, added in a fixed order */
int db1_colsum_acc(const void* x, float* out_acc, int64_t rows, int cols, int64_t ldx, int dt, void* ws, int64_t ws_bytes, void* stream);
/* y = a + b (elementwise), used by pre-LN residuals and dq = dq_k + dq_r */
int db1_add(const void* a, const void* b, void* y, int64_t n, int dt, void* stream);
/* y = a + b and, from the same pass, sum_a_acc[c] += sum_r a[r, c], sum_b_acc[c] += sum_r b[r, c] (float32, fixed order; y may alias b).
 * The attention backward's dq = dq_k + dq_r with the r_w_bias / r_r_bias gradients (transformer_xl.py:160-209): one pass instead of three. */
int64_t db1_add2d_colsums_workspace_bytes(int64_t rows, int cols);
int db1_add2d_colsums(const void* a, int64_t lda, const void* b, int64_t ldb, void* y, int64_t ldy, float* sum_a_acc, float* sum_b_acc,
                      int64_t rows, int cols, int dt, void* ws, int64_t ws_bytes, void* stream);
/* y[r, c] = a[r, c] + b[r, c] with row strides (a may have a different dtype; y may alias b) */
int db1_add2d(const void* a, int64_t lda, const void* b, int64_t ldb, void* y, int64_t ldy, int64_t rows, int cols,
              int dtA, int dt, void* stream);
/* base[segments[2i] .. + segments[2i+1]) = 0 for i < n_segments (offsets / lengths in elements, a device table of int64 pairs): one
 * launch clears the scattered small float32 accumulators of the gradient arena after an optimizer step. */
int db1_zero_segments(float* base, const int64_t* segments, int n_segments, void* stream);
/* y[i] = (dtOut) x[i] */
int db1_cast(const void* x, void* y, int64_t n, int dtIn, int dtOut, void* stream);

/* ------------------------------------------------------------------ embeddings
 * out[t, :] = table[ids[t], :] (zeros where ids[t] < 0)   (transformer_xl.py:627-629, 665, 677, 686) */
int db1_embed_gather_fwd(const void* table, const int64_t* ids, void* out, int64_t n_tokens, int d,
                         int64_t ld_out, int64_t n_table_rows, int dtTable, int dtOut, void* stream);
/* out[t, :] += row_table[row_ids[t], :] + col_table[col_ids[t], :]  (VisionEmbedding's position term, vision_embedding.py:117-180, added
 * onto the patch embeddings in one pass; (out + row) + col in fp32, one rounding; ids outside the tables add nothing) */
int db1_vision_pos_add(void* out, const void* row_table, const void* col_table, const int64_t* row_ids, const int64_t* col_ids, int64_t n,
                       int d, int64_t n_table_rows, int dtTable, int dt, void* stream);
/* dtable_acc[ids[t], :] += dout[t, :]; ids outside [0, n_table_rows) are skipped, as they read zeros in the forward.  Deterministic: no
 * float atomics -- the tokens are ordered by table row with a stable device radix sort (csrc/scatter.hip: the library's own LSD passes,
 * no vendor primitive) and every table row is written by the one wave that adds its tokens in token order.  d and ld_dout: multiples of
 * 16 bytes. */
int64_t db1_embed_scatter_add_workspace_bytes(int64_t n_tokens);   /* sort keys / values + the sort's own scratch + partial rows of long runs (d <= 8192) */
int db1_embed_scatter_add_bwd(const void* dout, const int64_t* ids, float* dtable_acc, int64_t n_tokens, int d,
                              int64_t ld_dout, int64_t n_table_rows, int dt, void* ws, int64_t ws_bytes, void* stream);
/* RL sequence assembly (transformer_xl.py:621-660): rows with ids >= 0 take word_table[ids];
 * the k-th "-1" placeholder of row b takes vis[b, k, :]; then + pos_table[position_id].
 * labels (may be NULL): label == -1 -> 0 in place (:644-645).  Token ids >= n_word_rows / position ids outside [0, n_pos_rows)
 * contribute nothing (no out-of-table access). */
int db1_rl_assemble_fwd(const void* word_table, const void* pos_table, const void* vis, const int64_t* ids,
                        const int64_t* position_id, int64_t* labels, void* out,
                        int B, int L, int d, int n_vis_per_row, int64_t n_word_rows, int64_t n_pos_rows, int dtTable, int dt, void* stream);
int64_t db1_rl_assemble_bwd_workspace_bytes(int B, int L);   /* the two table gradients are sorted-run scatters (db1_embed_scatter_add_bwd) */
int db1_rl_assemble_bwd(const void* dout, const int64_t* ids, const int64_t* position_id,
                        float* dword_acc, float* dpos_acc, void* dvis,
                        int B, int L, int d, int n_vis_per_row, int64_t n_word_rows, int64_t n_pos_rows, int dt,
                        void* ws, int64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ masked cross-entropy on materialised logits
 * (transformer_xl.py:602-609). logits [T, ld] (columns >= V are padding); a label outside [0, V) adds no loss and gets no gradient
 * (torch's ignore_index).  fwd: lse[t], and
 * sums[0] += sum_t mask*nll, sums[1] += sum_t mask.  bwd: dlogits = mask/sums[1] * gscale * (softmax - onehot)
 * (zeros in the padding), may be in place. */
int64_t db1_masked_ce_fwd_workspace_bytes(int64_t T);   /* per-token losses, summed in a fixed order */
int db1_masked_ce_fwd(const void* logits, const int64_t* labels, const float* mask, float* lse, float* sums,
                      int64_t T, int V, int64_t ld, int dt, void* ws, int64_t ws_bytes, void* stream);
int db1_masked_ce_bwd(const void* logits, const int64_t* labels, const float* mask, const float* lse, const float* sums,
                      void* dlogits, int64_t T, int V, int64_t ld, float gscale, int dt, void* stream);
/* both in ONE pass over the rows (each row stays in the registers of its workgroup: ld <= 34 816 elements in bf16, 17 408 in fp32): lse,
 * sums[0] += sum(mask * nll), sums[1] += sum(mask), and logits overwritten by dlogits = mask / norm[1] * gscale * (softmax - onehot);
 * norm[1] = the loss normaliser (a device float pair like `sums`).  Bit-equal to db1_masked_ce_fwd followed by db1_masked_ce_bwd.
 * ws: db1_masked_ce_fwd_workspace_bytes(T). */
int db1_masked_ce_fwd_bwd_supported(int V, int64_t ld, int dt);
int db1_masked_ce_fwd_bwd(void* logits, const int64_t* labels, const float* mask, float* lse, float* sums, const float* norm,
                          int64_t T, int V, int64_t ld, float gscale, int dt, void* ws, int64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ tied LM head + masked cross-entropy, chunked over the token rows
 * (transformer_xl.py:593-613).  The (T x vocabulary) logits tensor is never materialised: chunk_rows rows of logits at a time
 * live in the workspace (chunk_rows <= 0: 16 384).  h [T, d], W [n_w_rows, d] (rows >= V are zero padding, n_w_rows a multiple of
 * 256 keeps the tile GEMMs on their fast path), both of dtype dt.  Same loss / lse / gradient arithmetic as db1_gemm_* +
 * db1_masked_ce_* on a materialised tensor (the reductions inside a chunk and across chunks run in a fixed order).
 *   _fwd     : lse [T]; sums[0] += sum(mask * nll), sums[1] += sum(mask)                     (evaluation, logits-free forward)
 *   _fwd_bwd : additionally dh [T, d] (dtype dt) and dW_acc [n_w_rows, d] float32 = beta_dw * dW_acc + dW, both for
 *              loss * gscale -- one sweep, no recomputation: the normaliser sum(mask) is known before the first chunk. */
int64_t db1_lmhead_ce_workspace_bytes(int64_t T, int n_w_rows, int d, int chunk_rows, int dt, int train);
int db1_lmhead_ce_fwd(const void* h, const void* W, const int64_t* labels, const float* mask, float* lse, float* sums,
                      int64_t T, int V, int n_w_rows, int d, int chunk_rows, int dt, void* ws, int64_t ws_bytes, void* stream);
int db1_lmhead_ce_fwd_bwd(const void* h, const void* W, const int64_t* labels, const float* mask, float* lse, float* sums,
                          void* dh, float* dW_acc, float beta_dw, float gscale,
                          int64_t T, int V, int n_w_rows, int d, int chunk_rows, int dt, void* ws, int64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ relative-position attention for inference with memory
 * (evaluate_rl.py:157-266; transformer_xl.py:124-133,160-225).  q = 1..64 new queries per sequence against klen = mlen + q cached
 * keys / values (bf16, d_head 128).  qu, qv: [B, q, H, D]; k, v: row j of sequence b at k + b*kv_batch_stride + j*kv_row_stride
 * (+ h*D); R: [nd, H*D] rows indexed by distance mlen + i - j; out: [B, q, H, D].  Same visibility predicate as the
 * materialised path: i - shift < j <= i + mlen. */
int db1_relattn_decode_supported(int B, int q, int klen, int H, int D, int dt);
int64_t db1_relattn_decode_workspace_bytes(int B, int q, int klen, int H);   /* per-key-chunk partial outputs of the flash-decoding merge */
int db1_relattn_decode_fwd(const void* qu, const void* qv, const void* k, const void* v, int64_t kv_row_stride,
                           int64_t kv_batch_stride, const void* R, int nd, void* out, int B, int q, int klen, int mlen, int H,
                           int D, int shift, float scale, void* ws, int64_t ws_bytes, void* stream);

/* The same attention for ANY number of new queries (prompt prefill over a memory, long-text scoring), in ONE launch without partials, merge,
 * workspace or atomics (two launches on the same inputs give the same bits): operands, layout and visibility rule of db1_relattn_decode_fwd;
 * lse [B, H, q] float32 (NULL: not written) = log of the sum of exp(score) over the visible keys.
 * Supported: bf16, D == 128, 1 <= q <= 8192, mlen >= 0, klen == mlen + q <= 16384, shift >= 0 with shift + mlen >= 1 (every row sees a
 * key; shift == 0 is same_length over a full memory), nd >= 1, strides multiples of 8 elements, 16-byte aligned operands. */
int db1_relattn_mem_supported(int B, int q, int klen, int mlen, int H, int D, int shift, int dt);
int64_t db1_relattn_mem_workspace_bytes(int B, int q, int klen, int H);      /* 0 */
int db1_relattn_mem_fwd(const void* qu, const void* qv, const void* k, const void* v, int64_t kv_row_stride, int64_t kv_batch_stride,
                        const void* R, int nd, void* out, float* lse, int B, int q, int klen, int mlen, int H, int D, int shift,
                        float scale, void* ws, int64_t ws_bytes, void* stream);
/* db1_relattn_mem_fwd with the keys / values in TWO places (a prefill that projects only its own tokens): logical key j < mlen is row j of the
 * memory, k_mem / v_mem + b*mem_batch_stride + j*mem_row_stride (+ h*D); key j >= mlen is row j - mlen of the call's own q rows, k_new /
 * v_new + b*new_batch_stride + (j - mlen)*new_row_stride (e.g. views of qkv_new [B, q, 3, H, D]).  EITHER memory stride may be 0: one row
 * for every position, one memory for every sequence.  Everything else is db1_relattn_mem_fwd's rule with klen = mlen + q, and the result is
 * bit for bit that of db1_relattn_mem_fwd over the concatenation: the same kernel, steps, order and rounding points -- only the addresses of
 * the staged rows differ; no atomics, no workspace (_workspace_bytes is 0).
 * Supported: what db1_relattn_mem_supported supports at klen = mlen + q, with mlen >= 1 (DB1_ERR_UNSUPPORTED otherwise); the new rows'
 * stride >= H*D, the memory's 0 or >= H*D, nd >= 1, no NULL operand but lse (DB1_ERR_BAD_SHAPE); strides multiples of 8 elements, operands
 * 16-byte aligned (DB1_ERR_BAD_ALIGN).  Refused before anything is launched. */
int db1_relattn_mem_kv_supported(int B, int q, int mlen, int H, int D, int shift, int dt);
int64_t db1_relattn_mem_kv_workspace_bytes(int B, int q, int mlen, int H);     /* 0 */
int db1_relattn_mem_kv_fwd(const void* qu, const void* qv, const void* k_new, const void* v_new, int64_t new_row_stride,
                           int64_t new_batch_stride, const void* k_mem, const void* v_mem, int64_t mem_row_stride, int64_t mem_batch_stride,
                           const void* R, int nd, void* out, float* lse, int B, int q, int mlen, int H, int D, int shift, float scale,
                           void* ws, int64_t ws_bytes, void* stream);
/* db1_relattn_mem_kv_fwd with the memory in the SLOTS OF A K/V RING (a prefix cache's row continued by a call; tests/ring_fork_rule.py restates
 * the rule in NumPy).  `base` is the base ring's layer buffer, [M_base, cap_base, 2, H, D] bf16 (fp8 == 0) or [M_base, cap_base, 264 H] bytes
 * (fp8 != 0, the fp8 K/V ring's slot); state_base[0], its origin, is read on the device; base_rows (int32 [B]; NULL: the identity, B <=
 * M_base) names the ring row call row b continues -- repeats are allowed, call rows may share one memory row.
 * Logical key j < mlen of call row b is slot (state_base[0] + j) % cap_base of ring row base_rows[b]: on a bf16 ring the slot's [2, H, D] pair
 * as it is, on an fp8 ring payload * scale per (K | V, head) block (ops.kv8_unpack's value, exact in bf16).  Key j >= mlen is row j - mlen of
 * the call's own k_new / v_new.  Everything else is db1_relattn_mem_fwd's rule at klen = mlen + q, and the result is bit for bit that of
 * db1_relattn_mem_kv_fwd over the unpacked, linearised memory (the fp8 kernel's caveat: dequantised values that are subnormal in bf16 are not
 * covered; a NaN byte yields NaN, not particular NaN bits).  No workspace (_workspace_bytes is 0).
 * Guard (a launch cannot validate device data): a base_rows[b] outside [0, M_base) is read as row 0, an origin outside [0, cap_base) as 0 --
 * every read stays in bounds --, one thread ORs bit 3 (value 8) into *status (int32 [1]), and the output of those call rows is what the rule
 * gives for the clamped values: the bit says not to trust it.
 * Supported: what db1_relattn_mem_kv_supported supports, with 1 <= mlen < cap_base and an even H on an fp8 ring (DB1_ERR_UNSUPPORTED
 * otherwise); no NULL operand but lse and base_rows, the new rows' stride >= H*D, nd >= 1, M_base >= 1 (DB1_ERR_BAD_SHAPE); alignment as
 * db1_relattn_mem_kv_fwd, the int32 vectors 4-byte aligned (DB1_ERR_BAD_ALIGN).  Refused before anything is launched. */
int db1_relattn_mem_ring_supported(int B, int q, int mlen, int cap_base, int fp8, int H, int D, int shift, int dt);
int64_t db1_relattn_mem_ring_workspace_bytes(int B, int q, int mlen, int H);   /* 0 */
int db1_relattn_mem_ring_fwd(const void* qu, const void* qv, const void* k_new, const void* v_new, int64_t new_row_stride,
                             int64_t new_batch_stride, const void* base, int fp8, int M_base, int cap_base, const int32_t* state_base,
                             const int32_t* base_rows, int32_t* status, const void* R, int nd, void* out, float* lse, int B, int q, int mlen,
                             int H, int D, int shift, float scale, void* ws, int64_t ws_bytes, void* stream);

/* The same attention over a RING of cached keys / values (hipGraph-friendly inference: nothing is concatenated or copied per call):
 * kv_ring [B, cap, 2, H, D] bf16, cap >= mlen + q; logical key j < mlen is ring row (ring_state[0] + j) % cap; the q new keys / values come
 * from this call's packed projections qkv_new [B, q, 3, H, D] and are appended at rows (ring_state[0] + mlen + i) % cap by the same
 * launch; q + r_w_bias / q + r_r_bias are formed inside (u, vb [H, D]).  ring_state is a DEVICE int (the row of logical key 0), advanced
 * by db1_ring_advance(state, q, cap) after the last layer of a call -- so one captured graph serves every call.  klen <= 2048. */
int64_t db1_relattn_decode_ring_workspace_bytes(int B, int q, int klen, int H);
int db1_relattn_decode_ring_fwd(const void* qkv_new, const void* u, const void* vb, void* kv_ring, const int* ring_state, int cap, const void* R,
                                int nd, void* out, int B, int q, int mlen, int H, int D, int shift, float scale, void* ws, int64_t ws_bytes,
                                void* tickets, void* stream);
int db1_ring_advance(int* state, int q, int cap, void* stream);
/* `tickets` (optional): db1_linear_decode_tickets_bytes() bytes, ZERO before the first launch and left zero by every launch that uses them.
 * With it (and q <= 16) the key chunk that finishes last for a (batch, head) merges the partial results inside the attention launch.
 * out == NULL (q <= 16): no merge at all, the per-chunk partial results stay in ws for db1_linear_decode_attn. */

/* ------------------------------------------------------------------ grouped K/V ring (tests/group_ring_rule.py restates the rule in NumPy).
 * Beam search and best-of-n sampling decode M = G W rows whose W rows per group share one prompt.  Per layer the memory is
 *   a BASE ring  [G, cap_b, 2, H, D] bf16, origin state_b[0], cap_b >= mlen: the prompt's mlen keys / values, one row per group, only read;
 *   a TAIL ring  [M, cap_t, 2, H, D] bf16, origin state_t[0], window Lt, cap_t >= Lt + 1: the keys / values every row generated itself, and
 *   n_tail[0], the number of valid tail keys, 0 <= n_tail <= min(Lt, mlen).
 * Row r belongs to group g = r / W.  Its logical memory is the last mlen positions of cat(base window of g, its n_tail tail keys):
 *   logical key j <  mlen - n_tail          base slot (state_b[0] + n_tail + j) % cap_b of base row g
 *   mlen - n_tail <= j < mlen               tail slot (state_t[0] + Lt - mlen + j) % cap_t of tail row r
 *   j == mlen                               the call's own key / value from qkv_new [M, 1, 3, H, D]; the same launch appends it at tail slot
 *                                           (state_t[0] + Lt) % cap_t of row r.  No other byte of either ring changes.
 * Scores, distances (mlen - j for the one query), visibility (j > -shift), u / vb, scale and the rounding points are those of
 * db1_relattn_decode_ring_fwd at q = 1: fp32 scores from bf16 MFMA, P rounded to bf16 before P.V, one normalisation, one bf16 store.  Only the
 * grouping of the partial sums differs (chunks of 128 base POSITIONS read once per group, then chunks of 128 tail positions per row), so
 * the result is not bit-equal to the per-row ring kernel's; it is deterministic: the partials are merged in that fixed order, without
 * atomics, and two launches give the same bits.  out [M, 1, H, D] bf16.
 * Guard: an n_tail outside [0, min(Lt, mlen)] or an origin outside its ring is clamped into range (every access stays in bounds) and one
 * thread ORs bit 0 into *status (int32 [1]; the launch's only atomic).
 * Supported (_supported; DB1_ERR_UNSUPPORTED otherwise): bf16, D == 128, 1 <= W <= 64, 1 <= mlen <= 2047, 1 <= Lt <= 4096, cap_b >= mlen,
 * cap_t >= Lt + 1.  DB1_ERR_BAD_SHAPE: a NULL buffer, nd < 1, shift < 0; DB1_ERR_BAD_ALIGN: an operand that is not 16-byte aligned;
 * DB1_ERR_WORKSPACE_TOO_SMALL: fewer than _workspace_bytes.  db1_group_ring_advance, after the last layer of a call: state_t[0] = (state_t[0] + 1) %
 * cap_t and n_tail[0] = min(n_tail[0] + 1, Lt, mlen).  db1_ring_reorder serves the tail as it is: rings = the tail rings, mlen = Lt. */
int db1_relattn_decode_group_supported(int G, int W, int mlen, int Lt, int cap_b, int cap_t, int H, int D, int dt);
int64_t db1_relattn_decode_group_workspace_bytes(int G, int W, int mlen, int Lt, int H);
int db1_relattn_decode_group_fwd(const void* qkv_new, const void* u, const void* vb, const void* base, const int32_t* state_b, int cap_b, void* tail,
                                 const int32_t* state_t, int cap_t, const int32_t* n_tail, int Lt, const void* R, int nd, void* out, int G, int W,
                                 int mlen, int H, int D, int shift, float scale, int32_t* status, void* ws, int64_t ws_bytes, void* stream);
int db1_group_ring_advance(int32_t* state_t, int32_t* n_tail, int cap_t, int Lt, int mlen, void* stream);

/* ------------------------------------------------------------------ fp8 K/V ring (tests/kv8_rule.py restates the format in NumPy).
 * The same ring with half the bytes per key: kv_ring is [B, cap, slot] BYTES, one slot = one key position of one batch row:
 *     H * 128 bytes of K payload, H * 128 bytes of V payload, H fp32 K scales, H fp32 V scales     (264 H bytes; D == 128, H even)
 * Payload: OCP e4m3fn (1-4-3, bias 7, largest finite 448, no infinity, NaN = 0x7f / 0xff) -- the gfx950 conversion format.
 * Scale, per (row, position, K or V, head) over its 128 bf16 elements: amax = the largest magnitude among the FINITE elements; s = the
 *     smallest power of two with amax <= 448 s; amax == 0 gives s = 1; the exponent of s is at least -126 (s stays a normal fp32).
 * Payload = rne_e4m3(x / s): the division is exact and |x / s| <= 448, so the e4m3 rounding is the only rounding and nothing saturates.
 * Dequantised value = payload * s, exact in bf16 (where it is not subnormal).
 * Non-finite elements: an infinity or NaN takes no part in amax and is stored as the byte 0x7f (NaN, dequantised NaN) whatever its sign; the
 *     scale and every other byte of its block are what they would be without it, so it reaches only its own (row, position, K or V, head).
 * db1_relattn_decode_ring_kv8_fwd: operands and the three forms (out; out == NULL with the partials in ws; tickets) of
 * db1_relattn_decode_ring_fwd.  Memory keys come from the ring; the call's own keys are read from qkv_new (bf16) and appended to the ring
 * quantised by the rule above; every other byte of the ring stays.  The result is bit for bit that of db1_relattn_decode_ring_fwd over the
 * dequantised ring (same chunks, steps, merge order and rounding points; the scales are applied where a power of two is exact: K's to the
 * fp32 score before the relative term, V's to the probability before its bf16 rounding) as long as no dequantised value is subnormal.
 * DB1_ERR_UNSUPPORTED: D != 128, odd H, q outside 1 .. 64, klen > 2048; DB1_ERR_BAD_SHAPE: cap < klen or a NULL operand; DB1_ERR_BAD_ALIGN. */
int64_t db1_kv8_slot_bytes(int H, int D);                                   /* 264 H, or 0 where the format is not defined */
int db1_relattn_decode_ring_kv8_supported(int B, int q, int klen, int H, int D);
int64_t db1_relattn_decode_ring_kv8_workspace_bytes(int B, int q, int klen, int H);
int db1_relattn_decode_ring_kv8_fwd(const void* qkv_new, const void* u, const void* vb, void* kv_ring, const int* ring_state, int cap, const void* R,
                                    int nd, void* out, int B, int q, int mlen, int H, int D, int shift, float scale, void* ws, int64_t ws_bytes,
                                    void* tickets, void* stream);
/* src bf16 [n, mlen, 2, H, D] (projected keys / values) -> slots: position j of row i at dst + i * dst_row_stride + j * slot (bytes; the
 * stride a multiple of 16 and at least mlen slots, e.g. cap * slot to write into ring[:, :mlen]).  One pass, no workspace. */
int db1_kv8_quantize_supported(int H, int D);
int db1_kv8_quantize(const void* src, void* dst, int n, int mlen, int H, int D, int64_t dst_row_stride, void* stream);

/* ------------------------------------------------------------------ the inference layer's linear maps (M <= 64 new tokens), fused
 * y[M, N] = x[M, K] . W^T + bias (bf16, W K-major like nn.Linear.weight, leading dimension K) as a stream over W, finishing the layer's
 * small follow-up work inside the same launch:
 *   geglu != 0: W is [2 N, K] (value rows, then gate rows), bias [2 N]; y = (x W_v^T + b_v) * gelu_erf(x W_g^T + b_g), both halves rounded
 *               to bf16 first like the reference's z tensor (transformer_xl.py:262-269 with activations.py:19-32);
 *   pre_out != NULL (M <= 16, K <= 2048, K % 256 == 0): the INPUT rows are normalised on the way in, x_eff = LayerNorm(pre_alpha * pre_res + x)
 *               * pre_gamma + pre_beta (two passes in fp32 over the sum rounded to bf16, like db1_layernorm_residual_fwd; the row sums are
 *               grouped differently, so the bf16 result can differ from that launch in the last place), stored to pre_out [M, K] as well --
 *               the residual LayerNorm that closes the PREVIOUS sub-layer costs no launch and no inter-workgroup hand-off;
 *   ln_out != NULL: after the last column group has stored y, ln_out[M, N] = LayerNorm(alpha * res + y) * gamma + beta (N = 512, 1024 or
 *               2048; the arithmetic of db1_layernorm_residual_fwd on the stored bf16 y: equal results) -- for M > 16.
 * K is split over workgroups when N alone gives too few of them; the partial tiles are added in split order by the last arrival
 * (deterministic).  `tickets`: db1_linear_decode_tickets_bytes() bytes, zero before the first launch, left zero.
 * db1_linear_decode_supported(..., ln): bit 0 = with ln_out, bit 1 = with pre_out. */
int64_t db1_linear_decode_tickets_bytes(void);
/* ... and the attention output projection fed by the attention's per-chunk partial results: db1_relattn_decode_ring_fwd with out == NULL
 * (q <= 16) leaves [B*H][chunks = ceil(klen / 128)][64][D + 2] floats (unnormalised output, maximum, sum per query) in ITS workspace; this
 * launch merges them on the way in (the arithmetic of the attention's own merge) and multiplies by W [N, H D].  B q <= 2 rows, <= 12 chunks. */
int db1_linear_decode_attn_supported(int B, int q, int H, int D, int nunit, int N);
int db1_linear_decode_attn(const float* attn_part, int nunit, int B, int q, int H, int D, const void* w, void* y, int64_t ldy, int N, void* stream);
int64_t db1_linear_decode_workspace_bytes(int M, int N, int K, int geglu);
int db1_linear_decode_supported(int M, int N, int K, int geglu, int ln);
int db1_linear_decode(const void* x, int64_t ldx, const void* w, const void* bias, int dtBias, void* y, int64_t ldy, int M, int N, int K,
                      int geglu, const void* pre_res, int64_t ld_pre_res, float pre_alpha, const void* pre_gamma, const void* pre_beta,
                      float pre_eps, void* pre_out, int64_t ld_pre_out, const void* res, int64_t ld_res, float alpha, const void* gamma,
                      const void* beta, float eps, void* ln_out, int64_t ld_out, int dtParam, void* tickets, void* ws, int64_t ws_bytes,
                      void* stream);

/* ------------------------------------------------------------------ fp8 decode weights (tests/w8_rule.py restates the format in NumPy).
 * The same linear maps with about half the bytes of W to stream.  A weight W [N, K] (bf16, K-major, K % 128 == 0) becomes ONE buffer of
 * db1_w8_bytes(N, K) = N K + 4 N (K / 128) bytes:
 *     N * K bytes of e4m3 payload, row-major; then N * (K / 128) fp32 scales, row-major      (0.516 of the bf16 bytes)
 * A block is the 128 consecutive k of one row.  Scale, payload, NaN byte and exponent floor of a block are exactly the fp8 K/V ring's rule
 * above (tests/kv8_rule.py: quantize): the scale is the smallest power of two s with amax <= 448 s over the block's FINITE elements (1 for a
 * block of zeros, at least 2^-126), x / s is exact, the e4m3 rounding is the only rounding, payload * s is exact in bf16 (where it is not
 * subnormal there), a non-finite element is stored as the byte 0x7f and takes no part in amax.
 * db1_w8_quantize: w [N, K] with leading dimension ldw >= K (elements, a multiple of 8) -> out; one pass, no workspace.
 * db1_linear_decode_w8 / db1_linear_decode_attn_w8: the operands of db1_linear_decode / db1_linear_decode_attn with the packed buffer in place
 * of w (geglu: the buffer of the whole [2 N, K] weight); workspace and tickets are db1_linear_decode's.  Only the kernel's W load sites differ
 * (16 payload bytes + one scale per lane and 64-wide k-step, widened to the bf16 operands in registers): the k partition, MFMA order, LDS
 * reduction, split-K, epilogues, LayerNorm prologue and tail are the bf16 kernel's, so the result is BIT FOR BIT that of db1_linear_decode /
 * db1_linear_decode_attn over the dequantised weight (ops.w8_unpack), as long as no dequantised value is subnormal in bf16.
 * _supported: the bf16 entry point's, and K % 128 == 0.  Refused before anything is launched, with the bf16 entry points' codes: NULL operands
 * (DB1_ERR_BAD_SHAPE), a buffer that is not 16-byte aligned (DB1_ERR_BAD_ALIGN), K % 128 != 0 (DB1_ERR_UNSUPPORTED), and -- the fp8 form is
 * instantiated for what a bf16 model produces -- an fp32 bias or fp32 LayerNorm parameters (DB1_ERR_UNSUPPORTED). */
int64_t db1_w8_bytes(int N, int K);                                         /* 0 where the format is not defined */
int db1_w8_quantize(const void* w, int64_t ldw, int N, int K, void* out, void* stream);
int db1_linear_decode_w8_supported(int M, int N, int K, int geglu, int ln);
int db1_linear_decode_w8(const void* x, int64_t ldx, const void* w8, const void* bias, int dtBias, void* y, int64_t ldy, int M, int N, int K,
                         int geglu, const void* pre_res, int64_t ld_pre_res, float pre_alpha, const void* pre_gamma, const void* pre_beta,
                         float pre_eps, void* pre_out, int64_t ld_pre_out, const void* res, int64_t ld_res, float alpha, const void* gamma,
                         const void* beta, float eps, void* ln_out, int64_t ld_out, int dtParam, void* tickets, void* ws, int64_t ws_bytes,
                         void* stream);
int db1_linear_decode_attn_w8_supported(int B, int q, int H, int D, int nunit, int N);
int db1_linear_decode_attn_w8(const float* attn_part, int nunit, int B, int q, int H, int D, const void* w8, void* y, int64_t ldy, int N, void* stream);
/* fp8 weights in the persistent chain (csrc/decode_chain.hip; tests/w8_chain_rule.py restates the map in NumPy).
 * db1_decode_chain_w8: the argument list of db1_decode_chain with w_o, w1, w2, w_qkv_next and w_o_next as packed buffers of the format above
 * ([d, d], [2 dff, d], [d, dff], [3 d, d], [d, d]; the same copies the launches above read).  Biases and LayerNorm parameters stay bf16.  Same
 * scratch (db1_decode_chain_scratch_bytes / _error_offset), same slot rule: a bf16 launch and an fp8 launch may follow each other on one
 * scratch with different slots.  Only the weight load sites and the widening differ from the bf16 kernel.  The lane-to-column map is kept:
 *     piece j of a row (K columns) for lane l (0 .. 63) = columns (64 j + l) 8 .. + 7 = the 8 payload bytes at row K + (64 j + l) 8,
 *     all in scale block (64 j + l) >> 4 = 4 j + l / 16 of the row (K / 128 blocks: 16 for o_net, ff1 and qkv rows, 32 for ff2 rows).
 * A value is v_cvt_pk_f32_fp8 of the payload times the block's scale in fp32 (exact) and enters the bf16 kernel's fmaf chain in its order
 * (elements 0 .. 7 of piece 0, then piece 1, ...) and its wave sum: a launch is BIT FOR BIT db1_decode_chain over the dequantised weights
 * (ops.w8_unpack), as long as no dequantised value is subnormal in bf16.
 * _w8_supported: what db1_decode_chain_supported accepts.  Refused before anything is launched, with db1_decode_chain's codes: a geometry the
 * query refuses (DB1_ERR_UNSUPPORTED), a slot out of range or a NULL operand (DB1_ERR_BAD_SHAPE), a buffer that is not 16-byte aligned
 * (DB1_ERR_BAD_ALIGN; here w_o_next too: its payload is read as the launch's own rows are). */
int db1_decode_chain_w8_supported(int d, int dff, int H, int D, int nunit);
int db1_decode_chain_w8(const float* att_part, int nunit, int H, const void* x_res, const void* w_o8, const void* w1_8, const void* b1, const void* w2_8,
                        const void* b2, const void* w_qkv_next8, const void* w_o_next8, const void* g1, const void* be1, const void* g2, const void* be2,
                        float alpha, float eps, void* h1_out, void* f_out, void* x_next, void* qkv_next, void* scratch, int slot, int d, int dff, void* stream);

/* ------------------------------------------------------------------ relative-position attention, materialised path
 * (fp32 parity gate, any head size).  Buffers S,T are float32 in [H][B][Lq][*] layout.
 * qu = q + u, qv = q + v_bias from the packed qkv activations [B, L, 3, H, D]  (transformer_xl.py:161,167). */
int db1_relattn_add_head_bias(const void* qkv, const void* u, const void* vb, void* qu, void* qv,
                              int B, int Lq, int Lk, int H, int D, int dt, int dtParam, void* stream);
/* P[h,b,i,j] = softmax_j( (AC[h,b,i,j] + T[h,b,i, mlen+i-j]) * scale ) over visible keys
 * i - shift < j <= i + mlen  (closed form of _rel_shift + mask, transformer_xl.py:98-110,171-209,551-567);
 * written in place over AC.  lse (nullable) [H,B,Lq].  A row with NO visible key gets the uniform distribution over all Lk keys,
 * as the reference's masked_fill(-1e30) + softmax does (and no gradient flows into its scores). */
int db1_relattn_softmax_fwd(float* AC, const float* T, float* lse, int H, int B, int Lq, int Lk, int nd,
                            int mlen, int shift, float scale, void* stream);
/* dS = P * (dP - rowsum(P*dP)) * scale, in place over dP; dT[h,b,i,mlen+i-j] = dS[h,b,i,j] (zero elsewhere). */
int db1_relattn_softmax_bwd(const float* P, float* dP, float* dT, int H, int B, int Lq, int Lk, int nd,
                            int mlen, int shift, float scale, void* stream);

/* ------------------------------------------------------------------ relative-position flash attention (bf16, D = 128)
 * Fused QK^T + skewed Q~R^T + online softmax + PV; never materialises (L x L).
 * R [L,H,D] bf16 indexed by distance; out [B,L,H,D] bf16, lse [B,H,L] f32.
 * Training shape only: Lq == Lk, causal window i - shift < j <= i (shift >= L means plain causal). */
int db1_relattn_flash_supported(int B, int L, int H, int D, int dt);
/* qu = q + u, qv = q + v_bias: [B,L,H,D] contiguous (db1_relattn_add_head_bias); k, v: pointers INTO the packed
 * qkv activations with their row / batch strides in elements.
 * probs / mblk (optional, both or neither): keep the unnormalised probabilities p~ = exp2((s - m_blk) c2), c2 = scale log2 e, as bf16 MFMA
 * fragment images [64 lanes][8] per (key block jb of 32, 16-query tile qt) and the running maxima m_blk c2 they refer to [B*H][L/32][L] f32,
 * for db1_relattn_flash_bwd.  Only tiles on or below the causal diagonal exist (qt >= 2 jb); per (batch, head) they are stored as a triangle,
 * key block major: tile index qt + jb (L/16 - 1 - jb) -- db1_relattn_flash_probs_bytes(B, L, H) bytes in all (round 6: 25 instead of 49 GiB
 * for DB1-1.3B at 64 x 1024 tokens).  Tiles of blocks outside a sliding window are not written. */
int64_t db1_relattn_flash_probs_bytes(int B, int L, int H);
int db1_relattn_flash_fwd(const void* qu, const void* qv, const void* k, const void* v, int64_t kv_row_stride,
                          int64_t kv_batch_stride, const void* R, void* out, float* lse,
                          int B, int L, int H, int D, int shift, float scale, void* probs, float* mblk, void* stream);
/* dq (the (q+u).k branch only), dk, dv are written with their own row / batch strides (they live inside dqkv);
 * dT [H,B,L,L] bf16 = dS re-indexed by distance (input of the dq_r / dR GEMMs, zero where nothing is visible);
 * delta [B,H,L] f32 scratch (rowsum(dout * out): written by the query-side kernel, read by the key-side kernel).
 * Three ways to run it, by what the caller provides (all valid backward passes; P enters dV as bf16 in each):
 *   probs + mblk (what db1_relattn_flash_fwd stored) and db1_relattn_flash_bwd_workspace_bytes(B, L, H, 1) bytes of scratch:
 *       no score is recomputed -- P = p~ exp2(m_blk c2 - lse log2 e) on both sides, the factors go from the query side to the key side
 *       through the scratch (B*H*L*L/32 floats), and each side forms its own dS = P (dP - delta) scale from its own dP = dO.V^T
 *       (memory for time: B*H*L*L bf16 + B*H*L*L/32 floats per LAYER kept from the forward);
 *   no probs, db1_relattn_flash_bwd_workspace_bytes(B, L, H, 0) bytes of scratch (2 x B*H*L*L bf16): the query side recomputes scores,
 *       relative term and softmax and leaves P and dS in the scratch for the key side;
 *   neither (ws NULL / smaller): both sides recompute. */
int64_t db1_relattn_flash_bwd_workspace_bytes(int B, int L, int H, int have_probs);
int db1_relattn_flash_bwd(const void* qu, const void* qv, const void* k, const void* v, int64_t kv_row_stride,
                          int64_t kv_batch_stride, const void* R, const void* out, const void* dout, const float* lse,
                          float* delta, void* dq, void* dk, void* dv, int64_t dqkv_row_stride, int64_t dqkv_batch_stride,
                          void* dT, int B, int L, int H, int D, int shift, float scale, const void* probs, const float* mblk,
                          void* ws, int64_t ws_bytes, void* stream);

/* dq_r[b, i, h, :] = sum_{dist} dT[h, b, i, dist] * R[dist, h, :] (the (q+v).R branch of the query gradient, transformer_xl.py:160-209) as a
 * stream over dT with R stationary in registers: dT [H,B,L,L] bf16 (zero for dist > i), R [L, H*128] bf16 with row stride r_row_stride,
 * out [B,L,H,128] bf16 with row / batch strides in elements.  Same result as db1_gemm_strided_tri on the same operands. */
int db1_relattn_dqr_supported(int B, int L, int H, int D, int dt);
int64_t db1_relattn_dqr_workspace_bytes(int L, int H);   /* the transposed copy of R the stream kernel keeps in registers (+ the fused entry point's column-sum partials) */
int db1_relattn_dqr(const void* dT, const void* R, int64_t r_row_stride, void* out, int64_t out_row_stride, int64_t out_batch_stride,
                    int B, int L, int H, int D, void* ws, int64_t ws_bytes, void* stream);

/* The same stream with the rest of the query gradient in its epilogue (one pass less over two [B, L, H, 128] tensors):
 *   dq[b,i,h,:] = dq[b,i,h,:] + dq_r          (dq holds the (q+u).k branch from db1_relattn_flash_bwd on entry; one rounding)
 *   du_acc[h*128 + c] += sum_{b,i} dq_k[b,i,h,c]   (r_w_bias gradient),   dv_acc[h*128 + c] += sum_{b,i} dq_r[b,i,h,c]   (r_r_bias gradient)
 * float32 accumulators; the per-workgroup partial sums are added in a fixed order (deterministic). */
int db1_relattn_dqr_fused(const void* dT, const void* R, int64_t r_row_stride, void* dq, int64_t dq_row_stride, int64_t dq_batch_stride,
                          float* du_acc, float* dv_acc, int B, int L, int H, int D, void* ws, int64_t ws_bytes, void* stream);
/* ... WITHOUT its two reduces: parts [2][db1_relattn_dqr_parts_rows(H)][H * 128] float32 receives the per-workgroup column sums (dq_k -> du
 * half, dq_r -> dv half) for the caller to add up later (db1_colsum_acc per half) */
int db1_relattn_dqr_parts_rows(int H);
int db1_relattn_dqr_fused_parts(const void* dT, const void* R, int64_t r_row_stride, void* dq, int64_t dq_row_stride, int64_t dq_batch_stride,
                                float* parts, int B, int L, int H, int D, void* ws, int64_t ws_bytes, void* stream);
/* ... over a batch made of `ngroups` blocks of B / ngroups sequences, block g with its OWN R at R + g * r_group_stride elements: a whole
 * gradient-accumulation window run through ONE backward (TransformerXL's deferred backward; every micro-step drew its own position-table
 * dropout, transformer_xl.py:575, hence its own R = r_net(table), :138).  ngroups must divide B and the 256 / H workgroups of a head. */
int db1_relattn_dqr_groups_supported(int B, int L, int H, int D, int dt, int ngroups);
int64_t db1_relattn_dqr_groups_workspace_bytes(int L, int H, int ngroups);
int db1_relattn_dqr_fused_groups(const void* dT, const void* R, int64_t r_row_stride, int64_t r_group_stride, int ngroups, void* dq,
                                 int64_t dq_row_stride, int64_t dq_batch_stride, float* du_acc, float* dv_acc, int B, int L, int H, int D,
                                 void* ws, int64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ image-patch embedder pieces
 * (src/tokenizer/vision_embedding.py:65-86).  pixels [N_img, C, Himg, Wimg] -> normalised patches
 * [(n h w), C, p, p]: (x-mean)/(1e-6+std_unbiased)/sqrt(p) per (patch, channel). */
int db1_patch_normalize(const void* pixels, void* patches, int n_img, int C, int Himg, int Wimg, int p,
                        int dtIn, int dtOut, void* stream);
/* im2col for 3x3/pad 1 on p x p patches: x [N, C, p, p] -> cols [N*p*p, kpad] (kpad >= C*9 is the row stride; padding
 * columns are zero-filled so that K is a multiple of 8 for the MFMA tile GEMM); col2im gathers the reverse. */
int db1_im2col3x3(const void* x, void* cols, int64_t N, int C, int p, int kpad, int dt, void* stream);
int db1_col2im3x3(const void* dcols, void* dx, int64_t N, int C, int p, int kpad, int dt, void* stream);
/* Channels-last variants (the bf16 path): activations [N, p*p, C], column matrix tap-major cols[(n,y,x)][(ky*3+kx)*C + c], so every
 * access is a 16-byte vector of consecutive channels.  db1_conv_weight_permute builds the matching GEMM operand [Cout, kpad] from
 * the reference's [Cout, Cin, 3, 3] weight (vision_embedding.py:44-63), db1_conv_wgrad_unpermute adds a gradient computed in that
 * order back to the parameter layout.  The GroupNorm+GELU pair is specialised to the embedder's C = 64, hw = 256. */
int db1_patch_normalize_nhwc(const void* pixels, void* patches, int n_img, int C, int Himg, int Wimg, int p,
                             int dtIn, int dtOut, void* stream);
int db1_im2col3x3_nhwc(const void* x, void* cols, int64_t N, int C, int p, int kpad, int dt, void* stream);
int db1_col2im3x3_nhwc(const void* dcols, void* dx, int64_t N, int C, int p, int kpad, int dt, void* stream);
int db1_conv_weight_permute(const void* w, void* wp, int Cout, int Cin, int kpad, int dtIn, int dtOut, void* stream);
int db1_conv_wgrad_unpermute(const float* gp, float* g_acc, int Cout, int Cin, int kpad, void* stream);
/* Implicit-GEMM 3x3 convolutions for the 64 -> 64 channel layers on 16x16 patches (channels-last bf16): no column matrix.
 *   fwd (sign = +1): y[pix, o] = sum_{tap,c} x[pix + s(tap), c] * w_op[o, tap*64 + c] + bias[o], w_op from db1_conv_weight_permute;
 *   data gradient (sign = -1): x := dy, w_op := db1_conv_weight_permute_t(weight)  ([c, tap*64 + o]), bias = NULL;
 *   wgrad: gp_acc[o, tap*64 + c] += sum_pix dy[pix, o] * x[pix + s(tap), c]   (float32 [64, 576]; the pixel ranges' partial sums are added
 *          in a fixed order through the workspace: db1_conv3x3_implicit_wgrad_workspace_bytes, required). */
int db1_conv_weight_permute_t(const void* w, void* wp, int Cout, int Cin, int dtIn, int dtOut, void* stream);
int db1_conv3x3_implicit_fwd(const void* x, const void* w_op, const void* bias, void* y, int64_t n_patches, int sign, int dtBias,
                             void* stream);
/* same with a residual [n_patches * 256, 64] (bf16) added in the epilogue: y = conv + bias + res (the residual block's closing sum) */
int db1_conv3x3_implicit_fwd_res(const void* x, const void* w_op, const void* bias, const void* res, void* y, int64_t n_patches, int sign,
                                 int dtBias, void* stream);
/* The 3 -> 64 channel convolution of 16x16 patches (channels-last bf16 [n_patches*256, 3]) in one streaming kernel: y [n_patches*256, 64] =
 * conv + bias and, beside it, the column matrix cols [n_patches*256, 32] (tap-major, k = tap*3 + c, zero for k >= 27) that the weight
 * gradient contracts over; w_op [64, 32] as db1_conv_weight_permute leaves it. */
int db1_conv1_fused_fwd(const void* x, const void* w_op, const void* bias, void* cols, void* y, int64_t n_patches, int dtBias, void* stream);
int64_t db1_conv3x3_implicit_wgrad_workspace_bytes(int64_t n_patches);   /* per-pixel-range partial sums: with them the result is bit-reproducible */
int db1_conv3x3_implicit_wgrad(const void* dy, const void* x, float* gp_acc, float* gbias_acc /* optional [64]: += column sums of dy (the bias gradient) */,
                               int64_t n_patches, void* ws, int64_t ws_bytes, void* stream);
int db1_groupnorm_gelu_nhwc_fwd(const void* x, const void* gamma, const void* beta, void* y, float* mean, float* rstd,
                                int64_t N, int C, int hw, int groups, float eps, int dt, int dtParam, void* stream);
int64_t db1_groupnorm_gelu_nhwc_bwd_workspace_bytes(int64_t N);   /* per-sample parameter-gradient rows, summed in a fixed order (required) */
/* res (nullable): a tensor of dx's shape added to dx in fp32 before its one rounding -- the gradient that reaches x past the block
   (PatchEmbeddings' residual sum, vision_embedding.py:65-86), so that no separate add pass runs; res must not overlap dx */
int db1_groupnorm_gelu_nhwc_bwd(const void* dy, const void* x, const void* gamma, const void* beta, const float* mean,
                                const float* rstd, void* dx, const void* res, float* dgamma_acc, float* dbeta_acc,
                                int64_t N, int C, int hw, int groups, int dt, int dtParam, void* ws, int64_t ws_bytes, void* stream);
/* layout shuffles between GEMM output [N*p*p, C] ("NHWC") and [N, C, p, p] ("NCHW") */
int db1_nhwc_to_nchw(const void* x, void* y, int64_t N, int C, int hw, int dt, void* stream);
int db1_nchw_to_nhwc(const void* x, void* y, int64_t N, int C, int hw, int dt, void* stream);
/* GroupNorm(groups) + erf-GELU on [N, C, hw]; saves mean/rstd [N*groups]. bwd returns dx and accumulates dgamma/dbeta. */
int db1_groupnorm_gelu_fwd(const void* x, const void* gamma, const void* beta, void* y, float* mean, float* rstd,
                           int64_t N, int C, int hw, int groups, float eps, int dt, int dtParam, void* stream);
int db1_groupnorm_gelu_bwd(const void* dy, const void* x, const void* gamma, const void* beta, const float* mean,
                           const float* rstd, void* dx, float* dgamma_acc, float* dbeta_acc,
                           int64_t N, int C, int hw, int groups, int dt, int dtParam, void* stream);

/* ------------------------------------------------------------------ optimizer
 * acc[0] += sum(x^2)  (global-norm clipping, train_config.py:211-215).  Workspace-free form: ONE workgroup, so the sum does not depend on
 * arrival order -- meant for small vectors (n <= 2^24, DB1_ERR_UNSUPPORTED above: one workgroup is 1 / 256 of the chip); the whole gradient
 * arena goes through db1_sumsq_det / db1_grad_norm_sq. */
int db1_sumsq_acc(const void* x, float* acc, int64_t n, int dt, void* stream);
/* the same sum over the whole chip (per-workgroup partials in the workspace, fixed-order final add); overwrite != 0: acc[0] = sum, else += */
int64_t db1_sumsq_det_workspace_bytes(int64_t n);
int db1_sumsq_det(const void* x, float* acc, int64_t n, int dt, int overwrite, void* ws, int64_t ws_bytes, void* stream);
/* One fused Adam/AdamW step over a flat segment (DeepSpeed FusedAdam stand-in; torch.optim semantics).
 * g: gradients, float32 or (dtGrad = DB1_BF16) the bf16 copy the data-parallel engine all-reduces (train.py:231-232);
 * p32/m/v: float32 state; p_work (nullable): bf16 working copy written alongside.
 * grad scale = gscale * min(1, clip / (sqrt(*norm_sq) * gscale + 1e-6)) when clip > 0 and norm_sq != NULL. */
int db1_adam_step(float* p32, const void* g, float* m, float* v, void* p_work, int64_t n,
                  double lr, double beta1, double beta2, double eps, double wd, int adamw, int step,
                  float gscale, float clip, const float* norm_sq, int dtGrad, int dtWork, void* stream);

/* ------------------------------------------------------------------ scalar tokenizer
 * ContinuousScalarTokenizer.discretize (src/tokenizer/scalar_tokenizer.py:28-45), bit-exact ids. */
int db1_mulaw_discretize(const float* x, int32_t* ids, int64_t n, int is_action, int num_bins, float mu, float M,
                         void* stream);
/* ContinuousScalarTokenizer.decode (scalar_tokenizer.py:47-63; caller evaluate_rl.py:263): ids (int32, or int64 when ids_are_int64)
 * clipped to [0, num_bins-1] -> x = id/num_bins*2 - 1; observations additionally sign(x) * ((1 + M*mu)^|x| - 1) / mu.
 * *oob_flag (device int, nullable) is OR-ed with 1 when an id was out of range (the reference warns and clips). */
int db1_mulaw_decode(const void* ids, float* out, int64_t n, int ids_are_int64, int is_action, int num_bins, float mu, float M,
                     int* oob_flag, void* stream);

/* ------------------------------------------------------------------ composite entry points: one call per block of the
 * reference's forward / backward, sequencing the launches above (csrc/composite.hip), so that a host in any language drives the hot
 * path without re-implementing the Python orchestration.  bf16 activations; same conventions (caller-owned device pointers, (ws, ws_bytes)
 * scratch with a size query, asynchronous on `stream`, int status). */
/* acc[0] = sum(g^2) over a flat gradient segment: the global-norm clip's reduction (train_config.py:211-215).  Deterministic: per-workgroup
 * partial sums through the workspace, added in a fixed order. */
int64_t db1_grad_norm_sq_workspace_bytes(int64_t n);
int db1_grad_norm_sq(const void* g, float* acc, int64_t n, int dt, void* ws, int64_t ws_bytes, void* stream);
/* backward of the tied head + masked CE (transformer_xl.py:593-613) from the (lse, sums) a previous db1_lmhead_ce_fwd left: the logits are
 * recomputed 16 384 rows at a time; dh [T, d] = d(loss * gscale) / dh, dW_acc [n_w_rows, d] (float32) = beta_dw * dW_acc + d(loss * gscale) / dW */
int64_t db1_lmhead_ce_bwd_workspace_bytes(int64_t T, int n_w_rows, int d, int chunk_rows, int dt);
int db1_lmhead_ce_bwd(const void* h, const void* W, const int64_t* labels, const float* mask, const float* lse, const float* sums, void* dh,
                      float* dW_acc, float beta_dw, float gscale, int64_t T, int V, int n_w_rows, int d, int chunk_rows, int dt, void* ws,
                      int64_t ws_bytes, void* stream);
/* RelPartialLearnableMultiHeadAttn score / softmax / P.V (transformer_xl.py:160-225, _rel_shift :98-110, mask :551-567) on the packed
 * projections qkv [B, L, 3, H, D] (bf16, D = 128, L % 128 == 0), u / vb [H, D], R [L, H, D] = r_net(position table):
 *   fwd: qu = q + u, qv = q + vb (outputs, [B, L, H, D], kept by the caller for the backward), out [B, L, H, D], lse [B, H, L];
 *        probs [B*H, L/32, L/16, 512] bf16 + mblk [B*H, L/32, L] float32 (both or neither): the forward keeps its probabilities;
 *   bwd: dqkv [B, L, 3, H, D] and dR [L, H, D] written, du_acc / dvb_acc [H, D] float32 += ; dT [H, B, L, L] bf16 is caller scratch that must
 *        be ZERO above the causal diagonal on entry (every other entry is rewritten: one zero-initialised buffer serves all calls);
 *        plain causal window only (shift >= L). */
int db1_relattn_fwd(const void* qkv, const void* u, const void* vb, const void* R, void* qu, void* qv, void* out, float* lse, void* probs,
                    float* mblk, int B, int L, int H, int D, int shift, float scale, void* stream);
int64_t db1_relattn_bwd_workspace_bytes(int B, int L, int H, int D, int have_probs);
int db1_relattn_bwd(const void* qkv, const void* qu, const void* qv, const void* R, const void* out, const void* dout, const float* lse,
                    const void* probs, const float* mblk, void* dqkv, void* dR, float* du_acc, float* dvb_acc, void* dT, int B, int L, int H,
                    int D, int shift, float scale, void* ws, int64_t ws_bytes, void* stream);
/* PatchEmbeddings.forward / its backward (vision_embedding.py:65-86) on 16 x 16 patches: pixels [n_img, C, Himg, Wimg] float32 ->
 * emb [N, d] bf16, N = n_img * (Himg / 16) * (Wimg / 16) (position embeddings are the caller's gather).  weights[12] (bf16, the reference's
 * layouts) / grads[12] (float32 accumulators, +=) in state-dict order: conv1.{weight,bias}, residual_path.0.{weight,bias},
 * residual_path.2.{weight,bias}, residual_path.3.{weight,bias}, residual_path.5.{weight,bias}, projection.{weight,bias}.
 * `save` (db1_patch_embed_save_bytes) carries the forward's activations to the backward. */
int64_t db1_patch_embed_save_bytes(int n_img, int C, int Himg, int Wimg, int p);
int64_t db1_patch_embed_workspace_bytes(int n_img, int C, int Himg, int Wimg, int p, int d, int backward);
int db1_patch_embed_fwd(const float* pixels, const void* const* weights, void* emb, void* save, int n_img, int C, int Himg, int Wimg, int p,
                        int d, void* ws, int64_t ws_bytes, void* stream);
int db1_patch_embed_bwd(const void* demb, const void* const* weights, const void* save, float* const* grads, int n_img, int C, int Himg,
                        int Wimg, int p, int d, void* ws, int64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ next-token selection (generation; the reference picks tokens with
 * logits.argmax(-1) in torch and a host copy per token, evaluate_rl.py:157-266; its caption / VQA evaluation keeps the tokens before the first EOS,
 * text_decoder.py:42-62).  ONE launch picks one token for each of the M rows of logits [M, ld] (fp32 / bf16; columns >= V are padding):
 *   - candidates: the FINITE logits of the columns in [vocab_lo, vocab_hi) (NaN and +-inf never chosen);
 *   - greedy (or top_k == 1): the largest logit, lowest column on ties (torch.argmax);
 *   - else top-k (0 = off): keep {l >= the k-th largest}; top-p (1 = off): p = softmax(l / T) in fp32 over what is left, keep {l >= tau},
 *     tau = the largest kept logit with mass{l >= tau} >= top_p (sort-free: every token tied at a threshold is kept); then Gumbel-max:
 *     argmax over the kept set of l / T - log(-log u), lowest column on ties, with u = ((x >> 8) + 0.5) * 2^-24 and x = output (col % 4) of
 *     Philox4x32-10 on the counter (col / 4, stream_id[row] (NULL: row), step_base + *t, 0xE0000100) under the key (seed_lo, seed_hi);
 *   - a row with finished[row] != 0 writes pad_id; a row that picks eos_id writes it and sets finished; a row with no candidate writes pad_id,
 *     sets finished and status bit 0; otherwise lengths[row] += 1 (the tokens before EOS).  The token goes to out[row * max_new + *t] (status bit 1
 *     and no write if *t is outside [0, max_new)) and to next_ids[row * ids_stride] (int64: the next call's input ids).  status[row] |= bits.
 * *t is a device int32 the launch only READS (the caller advances it, e.g. with a captured t += 1): the call can be replayed from a hipGraph.
 * V <= 36 864 (_supported); no workspace (the query returns 0). */
int db1_select_tokens_supported(int V, int64_t ld, int dt);
int64_t db1_select_tokens_workspace_bytes(int M, int V, int dt);
int db1_select_tokens(const void* logits, int M, int V, int64_t ld, int dt, int vocab_lo, int vocab_hi, float temperature, int top_k, float top_p,
                      int greedy, uint32_t seed_lo, uint32_t seed_hi, int eos_id, int pad_id, int step_base, const int32_t* t,
                      const int32_t* stream_id, int32_t* finished, int32_t* lengths, int32_t* out, int max_new, int64_t* next_ids,
                      int64_t ids_stride, int32_t* status, void* ws, int64_t ws_bytes, void* stream);
/* The _lp forms (db1_select_tokens_lp, db1_select_tokens_slots_lp) choose exactly as the forms above -- out, lengths, finished, status,
 * next_ids and t come out bit-identical on the same inputs -- and also say how likely the chosen token was (tests/logprob_rule.py restates
 * the rule in NumPy).  logprob [rows | n_slots, max_new] and sum_logprob [rows | n_slots] (float32, both required: a NULL one is
 * DB1_ERR_BAD_SHAPE before any launch):
 *   - lse = the fp32 log-sum-exp over the row's candidates, the FINITE logits of the columns in [vocab_lo, vocab_hi) as the launch reads them
 *     (a row edited by db1_constrain_logits is scored on the edited values); temperature, top-k and top-p are NOT applied: lp is the model's
 *     log-probability of the token over the window, the quantity of db1_score_rows' logprob and db1_beam_step's l - lse;
 *   - lp = (l[tok] - max) - log(sum exp(l - max)), the sum in a fixed order (the wave butterflies, then the 16 wave results in order): the
 *     same inputs give the same bits;
 *   - wherever the launch writes a chosen token to out[row, t] it writes lp to logprob[row, t] and does sum_logprob[row] += lp (one fp32 add
 *     per launch by the thread that owns the row; the EOS token is included, as in the beam rule);
 *   - a finished row of the lockstep form (out gets pad_id) writes 0.0f to logprob[row, t] and leaves the sum alone; so does a row with no
 *     candidate;
 *   - t out of range: neither is touched; a vacant slot, or a row_map entry outside [0, n_slots): neither is touched.
 * No atomics, no workspace; the _supported and _workspace_bytes queries of the forms above hold for these too. */
int db1_select_tokens_lp(const void* logits, int M, int V, int64_t ld, int dt, int vocab_lo, int vocab_hi, float temperature, int top_k,
                         float top_p, int greedy, uint32_t seed_lo, uint32_t seed_hi, int eos_id, int pad_id, int step_base, const int32_t* t,
                         const int32_t* stream_id, int32_t* finished, int32_t* lengths, int32_t* out, int max_new, int64_t* next_ids,
                         int64_t ids_stride, int32_t* status, float* logprob, float* sum_logprob, void* ws, int64_t ws_bytes, void* stream);
/* The _top forms (db1_select_tokens_top, db1_select_tokens_slots_top) are the _lp forms -- every output of those comes out bit-identical
 * on the same inputs -- and also say which tokens the model ranked highest at the step (tests/topn_rule.py restates the rule in NumPy).
 * 1 <= top_n <= 16; top_ids (int32) and top_logprob (float32) are [rows | n_slots, max_new, top_n] (both required: a NULL one, or a top_n
 * outside 1 .. 16, is DB1_ERR_BAD_SHAPE before any launch).  For a row that writes a token to out[row, t]:
 *   - the candidates are those of lse above: the FINITE logits of the columns in [vocab_lo, vocab_hi) as the launch reads them (after
 *     db1_constrain_logits: a banned token is never an alternative); temperature, top-k and top-p are NOT applied;
 *   - the alternatives are the candidates sorted by logit descending, ties by the lower column -- the order of the greedy arg-max, whose
 *     keys tell -0.0 (lower) from +0.0; entry i < k = min(top_n, #candidates) is top_ids[row, t, i] = the column c of the i-th and
 *     top_logprob[row, t, i] = (l[c] - max) - log(sum exp(l - max)), the expression of lp with the same max and sum: the chosen token, when it
 *     is among the alternatives, carries the bits of logprob[row, t]; top_logprob[row, t, 0 .. k) never increases; greedy: top_ids[row, t, 0]
 *     is the token;
 *   - the entries [k, top_n) are top_ids = -1 and top_logprob = -inf: fewer candidates than top_n, a row with no candidate (k = 0), and a
 *     finished row of the lockstep form (the write that puts pad_id into out and 0 into logprob);
 *   - t out of range, a vacant slot, a row_map entry outside [0, n_slots): neither buffer is touched, as for logprob.
 * top_n rounds of one block-wide maximum over (key, ~column) pairs strictly below the last winner, on the keys the selection already holds in
 * registers (round 0 is the arg-max the selection has reduced anyway); only the thread that held the last winner looks for its next pair.  No
 * LDS beyond the selection's, no workspace, no atomics; the _supported and _workspace_bytes queries of the plain forms hold for these too. */
int db1_select_tokens_top(const void* logits, int M, int V, int64_t ld, int dt, int vocab_lo, int vocab_hi, float temperature, int top_k,
                          float top_p, int greedy, uint32_t seed_lo, uint32_t seed_hi, int eos_id, int pad_id, int step_base, const int32_t* t,
                          const int32_t* stream_id, int32_t* finished, int32_t* lengths, int32_t* out, int max_new, int64_t* next_ids,
                          int64_t ids_stride, int32_t* status, float* logprob, float* sum_logprob, int top_n, int32_t* top_ids,
                          float* top_logprob, void* ws, int64_t ws_bytes, void* stream);
/* The slot form of db1_select_tokens (continuous batching: every row of a decode batch is a SLOT that requests pass through).  The
 * selection rule is db1_select_tokens' own, unchanged; the bookkeeping is per slot:
 *   - logits row i belongs to slot row_map[i] (int32 [M], distinct; NULL: slot i, and then n_slots == M).  t, limit, stream_id, finished,
 *     lengths, status ([n_slots]), out ([n_slots, max_new]) and next_ids are indexed by the SLOT; a row_map entry outside [0, n_slots) is skipped;
 *   - a slot with finished[slot] != 0 is vacant: pad_id goes to next_ids[slot * ids_stride] and nothing else is touched (not out, t, lengths);
 *   - a live slot needs 0 <= t[slot] < limit[slot] <= max_new; otherwise status bit 1, finished[slot] = 1, pad_id to next_ids, nothing else;
 *   - else the token is chosen as db1_select_tokens chooses it, the Philox counter being (col / 4, stream_id[slot] (NULL: slot),
 *     step_base + t[slot], 0xE0000100): a request's draws depend on its logits, its stream id, the seed and its own token index only, not on
 *     the slot it sits in or on when it was admitted.  The token goes to out[slot * max_new + t[slot]] and to next_ids[slot * ids_stride];
 *     EOS / no candidate / lengths as there; then t[slot] += 1, WRITTEN by the launch (one workgroup owns a slot: no atomics, and a graph
 *     replay needs no captured t += 1), and t[slot] == limit[slot] sets finished[slot].
 * Same V limit and logits formats as db1_select_tokens (_supported); no workspace (the query returns 0). */
int db1_select_tokens_slots_supported(int V, int64_t ld, int dt);
int64_t db1_select_tokens_slots_workspace_bytes(int M, int V, int dt);
int db1_select_tokens_slots(const void* logits, int M, int V, int64_t ld, int dt, int vocab_lo, int vocab_hi, float temperature, int top_k,
                            float top_p, int greedy, uint32_t seed_lo, uint32_t seed_hi, int eos_id, int pad_id, int step_base, int32_t* t,
                            const int32_t* limit, const int32_t* stream_id, int32_t* finished, int32_t* lengths, int32_t* out, int max_new,
                            int64_t* next_ids, int64_t ids_stride, int32_t* status, const int32_t* row_map, int n_slots, void* ws,
                            int64_t ws_bytes, void* stream);
/* db1_select_tokens_slots with the token log-probs of db1_select_tokens_lp (the rule is stated there): logprob [n_slots, max_new] at
 * column t[slot], sum_logprob [n_slots], both indexed by the SLOT. */
int db1_select_tokens_slots_lp(const void* logits, int M, int V, int64_t ld, int dt, int vocab_lo, int vocab_hi, float temperature, int top_k,
                               float top_p, int greedy, uint32_t seed_lo, uint32_t seed_hi, int eos_id, int pad_id, int step_base, int32_t* t,
                               const int32_t* limit, const int32_t* stream_id, int32_t* finished, int32_t* lengths, int32_t* out, int max_new,
                               int64_t* next_ids, int64_t ids_stride, int32_t* status, const int32_t* row_map, int n_slots, float* logprob,
                               float* sum_logprob, void* ws, int64_t ws_bytes, void* stream);
/* db1_select_tokens_slots_lp with the alternatives of db1_select_tokens_top (the rule is stated there): top_ids and top_logprob
 * [n_slots, max_new, top_n] at [slot, t[slot]], indexed by the SLOT. */
int db1_select_tokens_slots_top(const void* logits, int M, int V, int64_t ld, int dt, int vocab_lo, int vocab_hi, float temperature, int top_k,
                                float top_p, int greedy, uint32_t seed_lo, uint32_t seed_hi, int eos_id, int pad_id, int step_base, int32_t* t,
                                const int32_t* limit, const int32_t* stream_id, int32_t* finished, int32_t* lengths, int32_t* out, int max_new,
                                int64_t* next_ids, int64_t ids_stride, int32_t* status, const int32_t* row_map, int n_slots, float* logprob,
                                float* sum_logprob, int top_n, int32_t* top_ids, float* top_logprob, void* ws, int64_t ws_bytes, void* stream);
/* The per-slot form: db1_select_tokens_slots / _lp / _top with the sampling parameters of every SLOT read on the device instead of passed as
 * launch scalars, so ONE captured launch serves requests that are decoded differently (tests/slot_params_rule.py restates the rule in NumPy).
 * params is int32 [n_slots, 8], 32 bytes per slot, the base 32-byte aligned, indexed by the SLOT (not by the logits row); floats as their
 * fp32 bits:
 *     word 0  greedy (0 / 1)            word 4  seed, low 32 bits
 *     word 1  top_k                     word 5  seed, high 32 bits
 *     word 2  vocab_lo                  word 6  inv_temperature = fp32 1 / temperature (ONE fp32 division on the host, the one the scalar
 *     word 3  vocab_hi                          forms do at the launch; the kernel divides nothing, so no rounding can differ)
 *                                       word 7  top_p
 *   - a slot's record is read after the vacant-slot and counter checks of the slot form (a vacant slot's record, and that of a slot whose
 *     counter is out of range, is never looked at) and before its logits; all eight values are uniform over the slot's workgroup;
 *   - guard (the launch cannot check device data): a live slot's record is INVALID if not 0 <= vocab_lo < vocab_hi <= V, or if greedy == 0
 *     and any of: inv_temperature not finite and positive (NaN, 0, negative, inf), top_k < 0, top_p not in (0, 1].  An invalid slot gets
 *     status bit 2 (status[slot] |= 4), finished[slot] = 1 and pad_id in next_ids[slot * ids_stride]; nothing else of it is touched (out, t,
 *     lengths, logprob, sum_logprob, top_ids and top_logprob stay): the treatment of a counter out of range.  A greedy slot (word 0 != 0)
 *     ignores words 1 and 4 .. 7, as the scalar forms ignore those arguments when greedy;
 *   - otherwise the token, the bookkeeping, the Philox counter (col / 4, stream_id[slot] (NULL: slot), step_base + t[slot], 0xE0000100) under
 *     the slot's own key (word 4, word 5), the log-prob and the alternatives are exactly those of db1_select_tokens_slots / _lp / _top called
 *     with the slot's parameters as scalars; the candidates of lse and of the alternatives are the finite logits of the slot's OWN window;
 *   - eos_id, pad_id, step_base, max_new and the log-prob / top-n switches stay per launch (they fix buffer shapes, and
 *     db1_constrain_logits reads eos_id as a scalar).
 * One entry point for the three modes: logprob == sum_logprob == NULL, top_n == 0 and top_ids == top_logprob == NULL is the plain form; both
 * log-prob buffers (top_n 0, no top buffers) the _lp form; those, 1 <= top_n <= 16 and both top buffers the _top form.  Any other
 * combination, a NULL params or a params pointer that is not 32-byte aligned is DB1_ERR_BAD_SHAPE before any launch.  The _supported and
 * _workspace_bytes queries of db1_select_tokens_slots hold for it: no workspace, no atomics, no LDS beyond the selection's. */
int db1_select_tokens_slots_per(const void* logits, int M, int V, int64_t ld, int dt, const int32_t* params, int eos_id, int pad_id,
                                int step_base, int32_t* t, const int32_t* limit, const int32_t* stream_id, int32_t* finished, int32_t* lengths,
                                int32_t* out, int max_new, int64_t* next_ids, int64_t ids_stride, int32_t* status, const int32_t* row_map,
                                int n_slots, float* logprob, float* sum_logprob, int top_n, int32_t* top_ids, float* top_logprob, void* ws,
                                int64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ beam search (captions / answers / text; tests/beam_rule.py restates
 * the rule in NumPy).  G groups (prompts) of W beams (1 <= W <= 16), M = G * W rows, row b = g * W + j; step t = 0 .. max_new - 1 chooses
 * token t.  At every step (db1_beam_step, on logits [M, ld] of the step, fp32 / bf16 widened to fp32):
 *   1. row candidates: the columns c in [vocab_lo, vocab_hi) with a finite logit; lse_b = fp32 log-sum-exp over them;
 *      s(b, c) = beam_score[b] + (l[b, c] - lse_b);
 *   2. live beams: at t = 0 only j = 0 of each group (beam_score is not read); later the rows with beam_score > -inf.  A dead row offers
 *      nothing; a live row without a candidate sets status[g] bit 0;
 *   3. the group's candidates sorted by s descending, ties by the lower (j, c); the first 2W are walked in order:
 *   4. c == eos_id at rank < W: a finished hypothesis (the parent's tokens, then EOS; length n = t; score s / (t + 1)^length_penalty) is
 *      offered to the pool; EOS at rank >= W is dropped; any other candidate becomes the next beam j' (parent b, token c, beam_score s) until
 *      W beams are filled; unfilled beams get beam_score -inf (and parent = themselves).  The pool keeps the W best hypotheses sorted by
 *      score descending; on equal scores the one offered first stays ahead;
 *   5. the group is done when no beam was filled, or when the pool holds W hypotheses and its worst score >= (best new beam_score) /
 *      (t + 1)^length_penalty.  A done group's rows write pad_id to next_ids and change no other state;
 *   6. at t = max_new - 1, after the walk, every new beam is offered (in beam order) with n = t + 1 (no EOS) and score beam_score / (t + 1)^lp;
 *   7. output: the first R pool entries of each group.
 * State (device, int32 unless noted): beam_score float [M], parent [M], tokens [M, max_new] (the beams' histories, permuted in place),
 * pool_tokens [G, W, max_new] (W slots per group, EOS then pad_id after a hypothesis' n tokens), pool_len / pool_score (float) / pool_slot
 * [G, W] (sorted: entry k is slot pool_slot[g, k]), pool_count / done / switches / status [G].  Before step 0: pool_count, done, switches,
 * status zero.  switches[g] += the number of new beams (t > 0) whose parent is another row.  The new beams' tokens go to
 * next_ids[b * ids_stride] (int64).  status bit 1: *t outside [0, max_new) (nothing written but pad_id to next_ids).
 * Two launches (rows x vocabulary chunks; one workgroup per group), fixed-order reductions: the same inputs give the same bits.  *t is only
 * READ: the step can be captured into a graph.  V <= 65 536 (_supported). */
int db1_beam_step_supported(int V, int64_t ld, int W, int dt);
int64_t db1_beam_step_workspace_bytes(int M, int V, int W, int max_new, int dt);
int db1_beam_step(const void* logits, int G, int W, int V, int64_t ld, int dt, int vocab_lo, int vocab_hi, int eos_id, int pad_id,
                  float length_penalty, const int32_t* t, int max_new, float* beam_score, int32_t* parent, int32_t* tokens,
                  int32_t* pool_tokens, int32_t* pool_len, float* pool_score, int32_t* pool_slot, int32_t* pool_count, int32_t* done,
                  int32_t* switches, int64_t* next_ids, int64_t ids_stride, int32_t* status, void* ws, int64_t ws_bytes, void* stream);
/* Diverse (group) beam search (Vijayakumar et al., 2016; tests/diverse_beam_rule.py restates the rule in NumPy on tests/beam_rule.py).
 * The W beams of each of G prompts are split into D sub-groups of W' = W / D beams (D >= 1, D * W' <= 16); row b = (g * D + d) * W' + j for
 * prompt g, sub-group d, beam j, and EVERY state array has the layout of db1_beam_step for G * D groups of W' beams (beam_score / parent /
 * tokens [G * W, ...], the pool arrays [G * D, W', ...], pool_count / done / switches / status [G * D]).  At step t, for each prompt, the
 * sub-groups d = 0 .. D - 1 choose in turn over a list `chosen` that starts empty:
 *   1. a sub-group that is done, or a counter outside [0, max_new): as in the plain rule (pad_id to next_ids, status bit 1 for the counter);
 *      it adds nothing to `chosen`;
 *   2. candidates: steps 1-2 of the plain rule over the sub-group's W' rows, s = beam_score + (l - lse), lse in fp32; at t = 0 only beam
 *      j = 0 of EACH sub-group is live;
 *   3. n(c) = the number of entries of `chosen` equal to c; sel = s - fp32(n) * diversity_penalty in fp32 (no lower than -FLT_MAX); the
 *      sub-group's candidates sorted by sel descending, ties by the lower (j, c); the first 2W' are walked;
 *   4. the walk is step 4 of the plain rule with W' for W: EOS at rank < W' becomes a hypothesis, later EOS are dropped, other candidates
 *      fill the W' new beams in sel order.  Every STORED score is the unpenalised s (beam scores, pool scores s / (t + 1)^length_penalty):
 *      the penalty only ranks, the model's log-probability stays what the plain search and the scoring report;
 *   5. the sub-group is done when no beam was filled, or when its pool holds W' entries and the worst one >= (the LARGEST s among the new
 *      beams) / (t + 1)^length_penalty;
 *   6. at t = max_new - 1 the new beams are offered as in the plain rule;
 *   7. a sub-group that is not done after this step appends the tokens of its filled beams to `chosen`, in beam order (EOS never fills a
 *      beam and is never counted);
 *   8. output, on the host: a prompt's D pools merged, sorted by (score descending, d ascending, position in its pool ascending), the
 *      first R (1 <= R <= W).
 * A later sub-group sees at most W - W' distinct penalised tokens, so a row's raw top W' + W (by logit descending, column ascending)
 * holds its share of the penalised top 2W': launch 1 is db1_beam_step's rows kernel over G * D groups of W' with K = W' + W (<= 32), and
 * the workspace depends on that K.  Launch 2: one workgroup per PROMPT loops over its sub-groups, `chosen` in LDS.  Fixed order, no
 * atomics, no communication between workgroups: the same inputs give the same bits; at D = 1, diversity_penalty = 0 the bits of
 * db1_beam_step, at D > 1, diversity_penalty = 0 those of db1_beam_step over G * D groups of W'.  *t is only READ.  `W` below is W', the
 * beams of ONE sub-group.  Refused before a launch, with db1_beam_step's codes: a NULL buffer, D < 1, D * W' > 16, G * D * W' > 65535, an
 * empty window, a diversity_penalty that is negative or not finite, a short workspace. */
int db1_beam_step_diverse_supported(int V, int64_t ld, int W, int D, int dt);
int64_t db1_beam_step_diverse_workspace_bytes(int M, int V, int W, int D, int max_new, int dt);
int db1_beam_step_diverse(const void* logits, int G, int D, int W, float diversity_penalty, int V, int64_t ld, int dt, int vocab_lo,
                          int vocab_hi, int eos_id, int pad_id, float length_penalty, const int32_t* t, int max_new, float* beam_score,
                          int32_t* parent, int32_t* tokens, int32_t* pool_tokens, int32_t* pool_len, float* pool_score,
                          int32_t* pool_slot, int32_t* pool_count, int32_t* done, int32_t* switches, int64_t* next_ids,
                          int64_t ids_stride, int32_t* status, void* ws, int64_t ws_bytes, void* stream);
/* Beam K/V history of a RingMemory: rings = a DEVICE array of n_layers pointers to rings [M, cap, slot] (slot = 2 * H * D bf16 =
 * slot_bytes, a multiple of 16).  After the forward of step t (state = the ring origin after that call's advance) the last t logical keys
 * of every row, slots (state + mlen - t + i) % cap for i < t, are copied from row parent[b] to row b in every layer; rows with parent[b] == b
 * (or a parent outside b's group) and rows of groups with done[g] != 0 (done NULL: none) are left alone; *t outside [1, max_t] copies
 * nothing.  Two launches (gather into the workspace, write back): an in-place permutation with duplicates.  Requires max_t <= mlen < cap. */
int db1_ring_reorder_supported(int64_t slot_bytes);
int64_t db1_ring_reorder_workspace_bytes(int n_layers, int M, int max_t, int64_t slot_bytes);
int db1_ring_reorder(const void* const* rings, int n_layers, int M, int W, int cap, int64_t slot_bytes, const int32_t* state, int mlen,
                     const int32_t* t, int max_t, const int32_t* parent, const int32_t* done, void* ws, int64_t ws_bytes, void* stream);
/* A new request takes over rows of a RingMemory: rings as for db1_ring_reorder, src = a DEVICE array of n_layers pointers to the projected
 * keys / values [n, mlen, slot] of n requests, rows = int32 [n], distinct target rows in [0, M).  Logical key j < mlen of source row i goes to
 * slot (state[0] + j) % cap of row rows[i] in every layer (state = the ring origin, read on the device: no host synchronisation); nothing
 * else is written: the other rows and the cap - mlen slots outside the window of the loaded rows stay as they are.  ONE launch, a pure copy in
 * 16-byte words.  A rows[i] outside [0, M) is skipped and sets bit 0 of *status (int32 [1], |=); an origin outside [0, cap) copies nothing and
 * sets bit 1.  n == 0 is a no-op.  Requires slot_bytes % 16 == 0 and 0 < mlen < cap (_supported; DB1_ERR_UNSUPPORTED otherwise).  Every ring and
 * every source base pointer must be 16-byte aligned: they sit in device arrays the entry point cannot read, so this is the CALLER's to keep
 * (as for db1_ring_reorder; ops.ring_load_rows checks it). */
int db1_ring_load_rows_supported(int64_t slot_bytes, int mlen, int cap);
int db1_ring_load_rows(const void* const* rings, const void* const* src, int n_layers, int M, int n, int cap, int64_t slot_bytes,
                       const int32_t* state, int mlen, const int32_t* rows, int32_t* status, void* stream);
/* Prefill straight into the ring (tests/ring_prefill_rule.py restates the rule in NumPy): the slots of new tenants written from (a K/V memory
 * of mlen rows, a call's own q rows of K/V) of ONE layer -- operands and strides of db1_relattn_mem_kv_fwd, n_src sequences; `ring` is that
 * layer's ring, [M, cap, 2, H, D] bf16 (fp8 == 0) or [M, cap, 264 H] bytes (fp8 != 0, the fp8 K/V ring's slot).  For destination i in
 * [0, n_dst): row = rows[i], s = src[i] (src NULL: s = i); for logical position j in [0, mlen): position j of the LAST mlen rows of
 * cat(memory of s (mlen rows), new rows of s (q rows)) -- memory row j + q while j + q < mlen, else new row j + q - mlen; q >= mlen takes
 * everything from the call -- goes to slot (state[0] + j) % cap of ring row `row`.  state[0] is read on the device and not changed.  bf16
 * ring: the K row and the V row are copied as they are; fp8 ring: quantised by the fp8 K/V ring's rule, bit for bit what db1_kv8_quantize
 * writes.  No other byte of the ring changes.  *status (int32 [1], |=; the launch's only atomic): bit 0 for a row outside [0, M) (skipped),
 * bit 1 for an origin outside [0, cap) (nothing written), bit 2 for an s outside [0, n_src) (skipped).  rows must be distinct.  ONE launch.
 * DB1_ERR_UNSUPPORTED: D != 128, an odd H on an fp8 ring, q < 1, mlen outside [1, cap); DB1_ERR_BAD_SHAPE: a NULL buffer (src may be
 * NULL), n_dst > M, a row stride below H*D (the memory's may be 0); DB1_ERR_BAD_ALIGN: as db1_relattn_mem_kv_fwd.  n_dst == 0 is a no-op. */
int db1_ring_prefill_rows_supported(int fp8, int q, int mlen, int cap, int H, int D);
int db1_ring_prefill_rows(void* ring, int fp8, int M, int cap, const void* k_new, const void* v_new, int64_t new_row_stride,
                          int64_t new_batch_stride, const void* k_mem, const void* v_mem, int64_t mem_row_stride, int64_t mem_batch_stride,
                          const int32_t* state, const int32_t* rows, const int32_t* src, int n_dst, int n_src, int q, int mlen, int H, int D,
                          int32_t* status, void* stream);
/* Fork ring rows (tests/ring_fork_rule.py): db1_ring_prefill_rows with a RING as the memory.  `base` [M_base, cap_base, slot], state_base and
 * base_rows (int32 [n_src]; NULL: the identity, n_src <= M_base) are db1_relattn_mem_ring_fwd's; both rings have the same format (fp8) and
 * H, cap may differ.  Destination i takes ring row rows[i] of `ring` from call row s = src[i] (src NULL: i) over base row r = base_rows[s]:
 * logical position j in [0, mlen) is row c = j + q of cat(memory of r (mlen rows), new rows of s (q rows)).  For c < mlen the SLOT BYTES of
 * base slot (state_base[0] + c) % cap_base are copied as they are -- an fp8 slot keeps its payload and scales, a fork never requantises --,
 * otherwise it is new row c - mlen, copied (bf16) or quantised by the fp8 K/V ring's rule (fp8).  The position goes to slot
 * (state[0] + j) % cap of ring row rows[i].  *status |=: bits 0 / 1 / 2 as db1_ring_prefill_rows, bit 3 (value 8) for a base row outside
 * [0, M_base) or a base origin outside [0, cap_base) (that destination is skipped).  No other byte of either ring changes; the base ring is
 * never written.  ONE launch.
 * DB1_ERR_UNSUPPORTED: what db1_ring_prefill_rows refuses, or mlen >= cap_base; DB1_ERR_BAD_SHAPE: overlapping base and destination
 * buffers, a NULL buffer (src and base_rows may be NULL), n_dst > M, a row stride below H*D; DB1_ERR_BAD_ALIGN: as db1_ring_prefill_rows.
 * n_dst == 0 is a no-op. */
int db1_ring_fork_rows_supported(int fp8, int q, int mlen, int cap_base, int cap, int H, int D);
int db1_ring_fork_rows(void* ring, int fp8, int M, int cap, const void* base, int M_base, int cap_base, const int32_t* state_base,
                       const int32_t* base_rows, const void* k_new, const void* v_new, int64_t new_row_stride, int64_t new_batch_stride,
                       const int32_t* state, const int32_t* rows, const int32_t* src, int n_dst, int n_src, int q, int mlen, int H, int D,
                       int32_t* status, void* stream);

/* ------------------------------------------------------------------ decoding constraints (tests/constraint_rule.py restates the rule in
 * NumPy).  db1_constrain_logits edits the step's logits [M, ld] (fp32 / bf16; columns >= V are padding) IN PLACE, before
 * db1_select_tokens / db1_select_tokens_slots / db1_beam_step read them: those take only FINITE logits as candidates and keep NaN and
 * +-inf out of their log-sum-exp, so a banned column is a column set to -inf.  Logits row i belongs to slot row_map[i] (NULL: slot i, and
 * then n_slots == M); its history H = hist[slot * max_new + 0 .. t) holds the tokens it has generated so far (the prompt is not part of
 * it) and t = t[slot] (t_per_slot != 0) or t[0] is its token index.  For one row l[0 .. V):
 *   1. guard: nothing in the row is touched when t is outside [0, max_new), when finished[slot] != 0 (finished NULL: no such test), or when
 *      the row_map entry is outside [0, n_slots);
 *   2. repetition penalty theta (> 0; 1 = off): every DISTINCT token c of H with 0 <= c < V and l[c] finite, once however often it occurs:
 *      l[c] <- round(l32 * inv_theta) if l32 > 0 else round(l32 * theta), l32 = the stored value widened to fp32, inv_theta = the fp32
 *      nearest to 1 / theta (computed by the caller in double), each product ONE fp32 multiplication, round = identity (fp32) or round to
 *      nearest even (bf16).  History entries outside [0, V) (a pad_id) are skipped, non-finite logits are left as stored;
 *   3. no-repeat n-gram of size ngram (0 = off): for every i in [ngram - 1, t) with H[i - ngram + 1 .. i - 1] == H[t - ngram + 1 .. t - 1],
 *      column H[i] is banned (ngram = 1: every token of H; nothing while t < ngram - 1);
 *   4. banned ids: every id of the device list bad[0 .. n_bad) inside [0, V) is banned at every step;
 *   5. minimum length: eos_id (>= 0) is banned while t < min_new;
 *   6. a banned column is WRITTEN as -inf, after the penalty (a ban overrides it); a ban outside [0, V) is ignored;
 *   7. every other column of the row, the padding columns [V, ld) and every other row stay bit-identical.
 * One workgroup per row, the row's history staged in LDS: O(t + n_bad) columns are touched, the vocabulary is never swept.  No atomics: only
 * the first occurrence of a token computes and stores its penalised value, a workgroup barrier follows, then the bans store -inf
 * (duplicates write the same bits): the same inputs give the same bits.  t, hist, finished, row_map and bad are only READ: the launch can be
 * captured into a graph and replayed.  With nothing to do (theta == 1, ngram == 0, n_bad == 0, no minimum length) there is no launch.
 * The first-occurrence test scans the history before each position: O(t^2 / 256) LDS reads per thread in the worst case (all tokens
 * distinct), on top of the O(t + n_bad) columns touched.
 * max_new <= 4096 and n_bad <= 1024 (_supported; DB1_ERR_UNSUPPORTED otherwise); no workspace (the query returns 0). */
int db1_constrain_logits_supported(int V, int64_t ld, int max_new, int n_bad, int dt);
int64_t db1_constrain_logits_workspace_bytes(int M, int V, int max_new, int n_bad, int dt);
int db1_constrain_logits(void* logits, int M, int V, int64_t ld, int dt, const int32_t* t, int t_per_slot, const int32_t* hist, int max_new,
                         const int32_t* finished, const int32_t* row_map, int n_slots, float theta, float inv_theta, int ngram,
                         const int32_t* bad, int n_bad, int eos_id, int min_new, void* ws, int64_t ws_bytes, void* stream);
/* db1_constrain_logits_pen: db1_constrain_logits with a frequency penalty freq, a presence penalty pres (any finite value, negative ones
 * included; 0 = off) and an additive bias list bias_ids / bias_val [n_bias] (device, n_bias <= 1024; the ids DISTINCT: the caller's to keep,
 * a device list cannot be checked at the launch) -- tests/penalty_rule.py restates the rule in NumPy.  The guard (1) and the bans (3 .. 7)
 * are db1_constrain_logits' own and the bans still come last, so a ban overrides everything.  Step 2 becomes, for a row that passed the guard:
 *   2a. penalties: every DISTINCT token c of H with 0 <= c < V and l[c] finite is edited once; n_c = its number of occurrences in H (entries
 *       of H outside [0, V) are neither penalised nor counted):
 *         v = l32, the stored value widened to fp32;
 *         theta != 1:            v = l32 > 0 ? v * inv_theta : v * theta            (the multiplication of db1_constrain_logits)
 *         freq != 0 || pres != 0: p = fp32(n_c) * freq;  p = p + pres;  v = v - p    (three fp32 operations, each rounded, NONE fused: not
 *                                                                                   with each other and not with the multiplication above)
 *         l[c] <- round(v), ONE store: identity (fp32), round to nearest even (bf16);
 *   2b. after a workgroup barrier, the bias: for every (id, b) with 0 <= id < V whose STORED logit, as the penalties left it, is finite:
 *       l[id] <- round(widen(l[id]) + b), one fp32 addition.  A column that is in the history and in the bias list is therefore rounded
 *       twice in bf16: that is the rule (one writer per column per phase, no atomics).  Non-finite logits are left as stored;
 *   then a barrier, then the bans.
 * The thread that holds a token's first occurrence counts its later copies in the staged history: this count scan roughly doubles the
 * worst-case O(t^2 / 256) term of the first-occurrence test (all tokens distinct); O(t + n_bad + n_bias) columns are touched.  No atomics,
 * LDS the 16 KB of history; t, hist, finished, row_map and the three lists are only READ: capturable.  The new mode is a compile-time flag
 * of the kernel: db1_constrain_logits launches the instantiation it always did, and with freq == 0, pres == 0 and n_bias == 0 this entry
 * point launches that one too (the same bits; no launch when nothing else is set either).  _supported adds n_bias <= 1024; no workspace. */
int db1_constrain_logits_pen_supported(int V, int64_t ld, int max_new, int n_bad, int n_bias, int dt);
int64_t db1_constrain_logits_pen_workspace_bytes(int M, int V, int max_new, int n_bad, int n_bias, int dt);
int db1_constrain_logits_pen(void* logits, int M, int V, int64_t ld, int dt, const int32_t* t, int t_per_slot, const int32_t* hist, int max_new,
                             const int32_t* finished, const int32_t* row_map, int n_slots, float theta, float inv_theta, int ngram,
                             const int32_t* bad, int n_bad, int eos_id, int min_new, float freq, float pres, const int32_t* bias_ids,
                             const float* bias_val, int n_bias, void* ws, int64_t ws_bytes, void* stream);
/* db1_constrain_logits_slots_per: db1_constrain_logits_pen with the constraints of every SLOT read on the device instead of passed as launch
 * scalars and one shared list each, so ONE captured launch serves requests that are constrained differently (tests/slot_constraints_rule.py
 * restates the rule in NumPy on top of tests/penalty_rule.py).  t is int32 [n_slots] (always per slot), hist [n_slots, max_new]; cons is
 * int32 [n_slots, 8], 32 bytes per slot, the base 32-byte aligned, indexed by the SLOT (not by the logits row); floats as their fp32 bits:
 *     word 0  theta (the repetition penalty)        word 4  freq
 *     word 1  inv_theta = fp32 1 / theta (ONE fp32  word 5  pres
 *             division on the host, the one the     word 6  n_bad  (entries used of the slot's row of bad)
 *             scalar forms do; the kernel divides   word 7  n_bias (entries used of the slot's rows of bias_ids / bias_val)
 *             nothing)
 *     word 2  ngram
 *     word 3  min_new (already 0 when there is no eos_id)
 * bad is int32 [n_slots, bad_cap], bias_ids int32 and bias_val float [n_slots, bias_cap], row s the lists of slot s (the bias ids of a slot
 * DISTINCT); 0 <= bad_cap, bias_cap <= 1024, and a capacity of 0 allows NULL for its lists.  eos_id stays per launch.  For logits row i with
 * slot = row_map[i] (NULL: i, and then n_slots == M):
 *   1. guard, in this order: a slot outside [0, n_slots); finished[slot] != 0; t[slot] outside [0, max_new): the row is left alone and the
 *      record is never looked at;
 *   2. the eight words are read (uniform over the workgroup, before the history is staged).  The launch cannot check device data, so the
 *      kernel does: a record is INVALID if theta or inv_theta is not finite and positive, ngram < 0, min_new < 0, freq or pres is not finite,
 *      n_bad is outside [0, bad_cap] or n_bias outside [0, bias_cap].  An invalid slot gets status bit 3 (status[slot] |= 8) and
 *      finished[slot] = 1, written by one thread; no bit of its logits changes, and the selection that follows treats it as any finished slot
 *      (pad_id fed forward);
 *   3. a record that edits nothing (theta == 1, freq == pres == 0, ngram == 0, n_bad == n_bias == 0, and eos_id < 0 or min_new == 0) leaves
 *      before the history is staged: the row keeps its bits;
 *   4. otherwise the row's bits are exactly those of db1_constrain_logits_pen called with the slot's values as scalars and the slot's own
 *      list rows (with freq == pres == 0 and n_bias == 0 those of db1_constrain_logits): the same phases in the same order, the same
 *      unfused products.
 * A compile-time mode of the same kernel; the other two entry points launch the instantiations they always did.  Its queries are those of
 * the slot form, db1_constrain_logits_slots_supported / _workspace_bytes (as db1_select_tokens_slots' hold for its _per form): they take the
 * two capacities where db1_constrain_logits_pen's take n_bad and n_bias.  No atomics, no workspace (the query returns 0), LDS the 16 KB of history; only finished and status of an invalid slot are written besides the logits: capturable.
 * A NULL cons, finished or status, a cons that is not 32-byte aligned or a NULL list with a capacity above 0 is DB1_ERR_BAD_SHAPE, a
 * capacity above 1024 or max_new above 4096 DB1_ERR_UNSUPPORTED (_supported), before any launch. */
int db1_constrain_logits_slots_supported(int V, int64_t ld, int max_new, int bad_cap, int bias_cap, int dt);
int64_t db1_constrain_logits_slots_workspace_bytes(int M, int V, int max_new, int bad_cap, int bias_cap, int dt);
int db1_constrain_logits_slots_per(void* logits, int M, int V, int64_t ld, int dt, const int32_t* t, const int32_t* hist, int max_new,
                                   int32_t* finished, int32_t* status, const int32_t* row_map, int n_slots, const int32_t* cons,
                                   const int32_t* bad, int bad_cap, const int32_t* bias_ids, const float* bias_val, int bias_cap, int eos_id,
                                   void* ws, int64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ stop sequences (tests/stop_rule.py restates the rule in NumPy).
 * db1_stop_match runs AFTER the selection launch of a step (db1_select_tokens / _slots / _slots_per and their _lp / _top forms) on the state
 * that launch has just updated, and ends every row whose generated tokens now end in one of n_stop token sequences (1 <= n_stop <= 16):
 * stop_tok int32 [n_stop, 16] and stop_len int32 [n_stop] (each 1 .. 16; a length outside matches nothing), both on the device.  Two int32
 * vectors of state per slot next to the selection's: checked (the value of lengths at the last look) and stop_hit; both zero when a
 * generation starts or a request moves into a slot.  For logits row i with s = row_map[i] (NULL: s = i, and then n_slots == M; an s outside
 * [0, n_slots) is skipped):
 *   1. n = lengths[s]; n == checked[s]: nothing of the slot is touched.  The selection grows lengths exactly when it writes a token that is
 *      not EOS, so this skips vacant slots, rows that finished earlier, rows that just wrote EOS and rows without a candidate, and it does
 *      examine a slot that reached its limit on this very token; neither t nor the lockstep / slot distinction is needed;
 *   2. checked[s] = n; n < 1 or n > max_new: nothing else;
 *   3. sequence k of length L matches if L <= n and out[s, n - L + j] == stop_tok[k, j] for all j < L (nothing before column 0 is read: only
 *      generated tokens are matched, never the prompt); the longest match wins, the lowest k among equals; no match: done;
 *   4. on a match, m = n - L: out[s, m .. n) = pad_id, lengths[s] = checked[s] = m, finished[s] = 1, stop_hit[s] = k + 1,
 *      next_ids[s * ids_stride] = pad_id; with logprob / sum_logprob (both or neither): logprob[s, m .. n) = 0 and sum_logprob[s] = the fp32
 *      sum of logprob[s, 0 .. m) added one by one from 0.0f -- the bits the selection's running sum had after token m - 1; with top_n /
 *      top_ids / top_logprob (all or none, only with the log-prob pair; top_n 0 and NULL: none): [s, m .. n, :] = -1 / -inf.
 * One wave per row: lane k tests sequence k, one fixed-order wave maximum picks the winner, the lanes clear the range, lane 0 re-adds the
 * sum.  No atomics, no workspace, no LDS; nothing is read back: capturable and replayable.  A bad combination of the optional buffers, a
 * NULL required one or a shape out of range is DB1_ERR_BAD_SHAPE, n_stop > 16 DB1_ERR_UNSUPPORTED (_supported), before any launch. */
int db1_stop_match_supported(int n_stop, int max_new);
int db1_stop_match(const int32_t* stop_tok, const int32_t* stop_len, int n_stop, int pad_id, int32_t* lengths, int32_t* checked,
                   int32_t* finished, int32_t* stop_hit, int32_t* out, int max_new, int64_t* next_ids, int64_t ids_stride,
                   const int32_t* row_map, int M, int n_slots, float* logprob, float* sum_logprob, int top_n, int32_t* top_ids,
                   float* top_logprob, void* stream);
/* db1_stop_match_per: db1_stop_match with every SLOT's own list (tests/slot_constraints_rule.py): stop_tok is int32 [n_slots, 16, 16] and
 * stop_len int32 [n_slots, 16], both indexed by the slot s of step 1 above.  There is no n_stop: all 16 entries of the slot's list are
 * looked at, and an unused entry has length 0 (a length outside 1 .. 16 matches nothing, as above; a slot whose 16 lengths are 0 has no
 * stop sequence).  Everything else -- steps 1 .. 4, the longest match and then the lowest index, what is cleared, the sum rebuilt in token
 * order -- is bit for bit db1_stop_match called with the slot's own list.  A compile-time mode of the same kernel: one wave per row, no LDS,
 * no atomics, no workspace; capturable.  The same refusals before any launch. */
int db1_stop_match_per(const int32_t* stop_tok, const int32_t* stop_len, int pad_id, int32_t* lengths, int32_t* checked, int32_t* finished,
                       int32_t* stop_hit, int32_t* out, int max_new, int64_t* next_ids, int64_t ids_stride, const int32_t* row_map, int M,
                       int n_slots, float* logprob, float* sum_logprob, int top_n, int32_t* top_ids, float* top_logprob, void* stream);

/* ------------------------------------------------------------------ speculative decoding (tests/spec_rule.py restates the rule in NumPy).
 * A one-token call streams every weight once; a call of Q = 1 + k tokens costs little more.  So a step feeds every row its last emitted token
 * and k GUESSED next tokens, and keeps as many of the model's own choices as the guesses allow.  The choice at a position is a pure function
 * of (that position's logits, stream id, seed, token index) -- db1_select_tokens' rule -- and under same_length attention a q-token call
 * over the ring equals q one-token calls, so the tokens that come out are exactly those of the one-token loop, sampled or greedy: a guess
 * is kept only if it IS the token the selection picks.  No rejection sampling.
 * State: t [1], finished / lengths / status [M], out [M, max_new] and optionally logprob [M, max_new] / sum_logprob [M], as db1_select_tokens
 * has them; ids int64 [M, Q], the step's input (column 0: the last emitted token, not yet in the ring; column 1 + j: the guess for token
 * index t + j); scratch sel, hit int32 [M, Q], lp float [M, Q], n_acc int32 [1], hist int32 [Q + 1].  A step verifies q_in positions
 * (1 <= q_in <= Q) over logits [M * q_in, ld], row r's position i at logits row r * q_in + i, in three launches:
 *   1. db1_spec_pick, M * q_in workgroups.  Token index tau = *t + i.  sel[r, i] = SKIP (-2) if finished[r] or tau outside [0, max_new);
 *      NONE (-1) if the window holds no finite logit; else the token db1_select_tokens picks from that logits row with the Philox counter
 *      (col / 4, stream_id[r] (NULL: r), step_base + tau, 0xE0000100).  hit[r, i] = 1 iff i + 1 < q_in and ids[r, i + 1] == sel[r, i], else
 *      0.  With lp: lp[r, i] = the _lp rule's value for the pick, 0 for NONE and SKIP.  The launch writes nothing else and only reads ids.
 *   2. db1_spec_accept, one workgroup per row.  *t outside [0, max_new]: status[r] |= 2 on every row, n_acc = 0, nothing else.
 *      *t == max_new: n_acc = 0 and nothing else (no status bit: the host may replay past the end until its next look).  Otherwise a row
 *      is LIVE iff sel[r, 0] != SKIP.  A live row walks i = 0, 1, ...; it emits position i and stops after it if sel[r, i] is NONE or
 *      eos_id (the row ends), tau + 1 == max_new, i == q_in - 1, or hit[r, i] == 0; a_row = its emissions.  n_acc = the minimum of a_row
 *      over the live rows, 0 if there is none.  Every live row commits exactly its first n_acc emissions (there is one t and one ring
 *      origin, so the rows are cut to the shortest).  Per emission i: out[r, t + i] = sel[r, i] (pad_id for NONE); lengths[r] += 1 unless EOS
 *      or NONE; logprob[r, t + i] = lp[r, i] and sum_logprob[r] += lp[r, i], one fp32 add per token in token order (NONE: 0 and no add);
 *      finished[r] = 1 on EOS or NONE; status[r] |= 1 on NONE.  A row that was not live writes pad_id (and 0) at the n_acc positions.
 *      n_acc > 0: ids[r, 0] = the last committed token, pad_id if the row is finished by now.  Then the k guesses with t' = t + n_acc over
 *      the history h = cat(ctx[r, :ctx_len[r]], out[r, :t']) of n tokens (ctx int32 [M, ctx_cap], ctx_len clamped to [0, ctx_cap]; NULL: none;
 *      ctx_cap + max_new <= 4096):  a finished row, or n == 0: ids[r, 1 + j] = pad_id.  script (int32 [M, max_new]) non-NULL: d_j =
 *      script[r, t' + j] if t' + j < max_new and the value lies in [0, V), else h[n - 1].  Else the n-gram lookup: for g = ngram_max down to
 *      ngram_min with n > g, the largest p <= n - g - 1 with h[p .. p + g) == h[n - g .. n); the first g with such a p wins and d_j =
 *      h[p + g + (j mod L)], L = n - (p + g) (a loop goes on periodically); no match at any g: d_j = h[n - 1].  ids[r, 1 + j] = d_j, j < k.
 *   3. db1_spec_commit, one thread: *t += n_acc; *ring_state = (*ring_state + cap - (q_in - n_acc)) % cap where ring_state is given (the
 *      forward has advanced the origin by q_in with db1_ring_advance; the keys of the positions that were not kept fall outside the
 *      window and are overwritten by the next call); hist[n_acc] += 1 where hist is given.
 * The pick of token 0 after a prefill is the same three launches with q_in = 1 (nothing to verify, no ring_state, no hist).
 * Every workgroup of launch 2 derives n_acc from sel, hit and *t only, which no workgroup of that launch writes: no atomics, no
 * communication between workgroups, fixed-order reductions -- two runs give the same bits; nothing is read back: capturable.
 * DB1_ERR_BAD_SHAPE before any launch: a NULL required buffer, q_in outside 1 .. Q, Q outside 2 .. 16, M * Q > 65535, an empty window, lp /
 * logprob / sum_logprob not all or none, ctx without ctx_len, an n-gram range outside 1 <= min <= max <= 8, cap <= 0 with a ring_state;
 * DB1_ERR_UNSUPPORTED: V above db1_select_tokens' limit, ctx_cap + max_new > 4096. */
int db1_spec_pick_supported(int V, int64_t ld, int dt, int Q);
int db1_spec_pick(const void* logits, int M, int q_in, int Q, int V, int64_t ld, int dt, int vocab_lo, int vocab_hi, float temperature, int top_k,
                  float top_p, int greedy, uint32_t seed_lo, uint32_t seed_hi, int pad_id, int step_base, const int32_t* t,
                  const int32_t* stream_id, const int32_t* finished, int max_new, const int64_t* ids, int32_t* sel, int32_t* hit, float* lp,
                  void* stream);
int db1_spec_accept_supported(int Q, int ctx_cap, int max_new, int ngram_min, int ngram_max);
int db1_spec_accept(int M, int q_in, int Q, int eos_id, int pad_id, int V, int max_new, const int32_t* t, const int32_t* sel,
                    const int32_t* hit, const float* lp, int32_t* finished, int32_t* lengths, int32_t* out, int32_t* status, float* logprob,
                    float* sum_logprob, int64_t* ids, const int32_t* ctx, const int32_t* ctx_len, int ctx_cap, const int32_t* script,
                    int ngram_min, int ngram_max, int32_t* n_acc, void* stream);
int db1_spec_commit_supported(int Q, int cap);
int db1_spec_commit(int32_t* t, const int32_t* n_acc, int32_t* hist, int q_in, int Q, int32_t* ring_state, int cap, void* stream);

/* ------------------------------------------------------------------ scoring given text (tests/score_rule.py restates the rule in NumPy).
 * For a row of logits l[0 .. V) (fp32 / bf16 read as stored and widened to fp32; columns >= V are padding), a label y and a window
 * [vocab_lo, vocab_hi) with 0 <= vocab_lo < vocab_hi <= V:
 *   - candidates: the FINITE logits of the columns in the window (NaN and +-inf are never candidates: the rule of db1_select_tokens and
 *     db1_beam_step);
 *   - lse = fp32 log-sum-exp over the candidates, their maximum subtracted first (window [0, V), finite logits: the lse of db1_masked_ce_fwd);
 *     -inf when there is no candidate;
 *   - logprob = l[y] - lse when y is a candidate; y in [0, V) but not a candidate (outside the window or not finite): logprob = -inf,
 *     rank = -1 and status bit 0; y outside [0, V) (torch's ignore_index, as db1_masked_ce_fwd treats it): the row is IGNORED,
 *     logprob = 0, rank = -1, no status bit, and it counts as masked out in db1_score_segments;
 *   - top1 = the candidate with the largest logit, the lowest column on ties; -1 (and status bit 1) when there is no candidate;
 *   - rank = the number of candidates whose logit is strictly greater than l[y] (0: the label is the arg-max or tied with it).
 * db1_score_rows: logits [T, ld] -> lse, logprob (float [T]), top1, rank, status (int32 [T]; every entry WRITTEN, status included).  One
 * workgroup per row, the row stays in registers between the maximum and the sum / count pass (one read of the logits, nothing written to
 * them); fixed-order reductions: the same inputs give the same bits.  Rows of at most 34 816 elements, ld a multiple of 16 bytes, logits
 * 16-byte aligned (_supported).  No workspace, no device scalars written by the host: capturable.
 * db1_lmhead_score: the rows of h [T, d] times the tied head W [n_w_rows, d] (n_w_rows >= V: the padded vocabulary), chunk_rows rows of logits at
 * a time in the workspace (0: 16 384) with db1_score_rows on every chunk: the [T, n_w_rows] logits tensor never exists.
 * db1_score_segments: n_seg segments of seg_len consecutive rows -> out [n_seg, 3] (float) = {sum(mask * logprob), sum(mask),
 * sum(mask * (rank == 0))} over the rows with mask != 0 whose label lies in [0, V) (ignored rows count as mask 0), added in a fixed order.  A
 * counted row with logprob = -inf makes its segment's first sum -inf; nothing becomes NaN.
 * db1_score_rows_top / db1_lmhead_score_top: db1_score_rows / db1_lmhead_score -- lse, logprob, top1, rank and status come out bit-identical
 * -- and the row's top_n best candidates (1 <= top_n <= 16; tests/topn_rule.py): top_ids (int32) and top_logprob (float32) are [T, top_n], both
 * required.  The alternatives of a row are its candidates sorted by logit descending, ties by the lower column, -0.0 and +0.0 being one
 * value as they are for top1 and rank; entry i < k = min(top_n, #candidates) holds the column c and l[c] - lse, the expression of logprob
 * with the same lse; the entries [k, top_n) hold -1 and -inf (a row with no candidate: all of them).  They do not depend on the label: an
 * ignored row gets what its logits give.  So top_ids[., 0] == top1; a label that is among the alternatives carries the bits of logprob; for
 * a candidate label whose logit no other candidate shares, rank < top_n implies top_ids[., rank] == label; top_logprob[., 0 .. k) never
 * increases.  A separate instantiation of the row kernel: after the sum pass the row's registers are rewritten as order-preserving keys
 * and top_n rounds of one block-wide maximum each run over them (the rounds of db1_select_tokens_top); one launch per chunk as before, no
 * workspace beyond db1_lmhead_score's (its _workspace_bytes and _supported queries hold), no atomics. */
int db1_score_rows_supported(int V, int64_t ld, int dt);
int db1_score_rows(const void* logits, const int64_t* labels, float* lse, float* logprob, int32_t* top1, int32_t* rank, int32_t* status,
                   int64_t T, int V, int64_t ld, int dt, int vocab_lo, int vocab_hi, void* stream);
int db1_score_rows_top(const void* logits, const int64_t* labels, float* lse, float* logprob, int32_t* top1, int32_t* rank, int32_t* status,
                       int64_t T, int V, int64_t ld, int dt, int top_n, int32_t* top_ids, float* top_logprob, int vocab_lo, int vocab_hi,
                       void* stream);
int64_t db1_lmhead_score_workspace_bytes(int64_t T, int n_w_rows, int d, int chunk_rows, int dt);
int db1_lmhead_score(const void* h, const void* W, const int64_t* labels, float* lse, float* logprob, int32_t* top1, int32_t* rank,
                     int32_t* status, int64_t T, int V, int n_w_rows, int d, int vocab_lo, int vocab_hi, int chunk_rows, int dt, void* ws,
                     int64_t ws_bytes, void* stream);
int db1_lmhead_score_top(const void* h, const void* W, const int64_t* labels, float* lse, float* logprob, int32_t* top1, int32_t* rank,
                         int32_t* status, int64_t T, int V, int n_w_rows, int d, int vocab_lo, int vocab_hi, int chunk_rows, int dt, int top_n,
                         int32_t* top_ids, float* top_logprob, void* ws, int64_t ws_bytes, void* stream);
int db1_score_segments(const float* logprob, const int32_t* rank, const int64_t* labels, const float* mask, float* out, int64_t n_seg,
                       int64_t seg_len, int V, void* stream);

/* ------------------------------------------------------------------ action decoding for RL rollouts (tests/action_rule.py restates the rule
 * in NumPy).  The reference restricts the logits to the action vocabulary, subtracts the environment's action mask, takes the argmax, maps the
 * id back to a tokenizer bin and copies it to the host once per action token (evaluate_rl.py:96-138,157-266).  db1_select_actions: ONE launch
 * picks one action token for each of the M environments from logits [M, ld] (fp32 / bf16; columns >= V are padding):
 *   - candidates: the FINITE logits of the columns [act_lo, act_hi), 0 <= act_lo < act_hi <= V, at most 4096 columns; mask (uint8 [M, n_mask],
 *     1 = allowed; NULL with n_mask 0: none) covers the columns act_lo .. act_lo + n_mask, n_mask <= act_hi - act_lo: a column whose mask
 *     byte is 0 is not a candidate; NaN and +-inf are never chosen;
 *   - the choice is exactly db1_select_tokens' over the window [act_lo, act_hi) of a row in which every masked column holds -inf: greedy (or
 *     top_k == 1) the largest logit, lowest column on ties; else top-k, top-p and the Gumbel-max draw of that rule with its Philox layout
 *     (counter (col / 4, stream_id[row] (NULL: row), step, 0xE0000100), word col % 4, key (seed_lo, seed_hi)) and the fp32 sums of top-p added
 *     in that kernel's order: the same token, bit for bit.  step = step_base + ctr[0] * act_len + ctr[1];
 *   - ctr (device int32 [2]) = {env_step, i}, only READ (the caller advances it, e.g. with a captured ctr[1] += 1): capturable.
 *     i == act_len is the memorising call of the reference's protocol (the last action token enters the memory, nothing is chosen): NOTHING
 *     is written, no status bit.  i outside [0, act_len]: status[row] |= 2 and nothing else is written;
 *   - for 0 <= i < act_len: bins[row, i] = token - act_lo (int32 [M, act_len]); values[row, i] (float [M, act_len], nullable) = the action
 *     branch of db1_mulaw_decode on that bin with num_bins (bin / num_bins * 2 - 1, the same instructions); next_ids[row * ids_stride] =
 *     token (int64: the next call's input ids);
 *   - a row with no candidate writes token act_lo, bin 0 and status[row] |= 1.
 * One workgroup of 256 threads per row, which reads the window only; no atomics, no workspace (the query returns 0), no communication
 * between workgroups, fixed-order reductions: two launches give the same bits.  DB1_ERR_BAD_SHAPE before any launch: a NULL logits, ctr,
 * bins, next_ids or status, an empty window or one outside [0, V), n_mask outside [0, act_hi - act_lo] or not matching mask, act_len
 * outside 1 .. 64, num_bins < 1, M outside 1 .. 65535, and, when not greedy, a temperature that is not finite and positive, top_k < 0 or
 * top_p outside (0, 1]; DB1_ERR_UNSUPPORTED: a window wider than 4096 columns (_supported); DB1_ERR_UNSUPPORTED_DTYPE.
 * db1_obs_tokens: float observations x [M, obs_dim] -> ids[row * ids_stride + j] = bin_base + the observation branch of db1_mulaw_discretize
 * on x[row, j] (the same device function: the same ids) for j < obs_dim, and ids[row * ids_stride + obs_dim] = sep_id (int64; ids_stride >=
 * obs_dim + 1): the observation call's input ids of every environment in one launch.  Nothing else is written. */
int db1_select_actions_supported(int V, int64_t ld, int dt, int act_lo, int act_hi);
int64_t db1_select_actions_workspace_bytes(int M, int V, int dt);
int db1_select_actions(const void* logits, int M, int V, int64_t ld, int dt, int act_lo, int act_hi, const uint8_t* mask, int n_mask,
                       float temperature, int top_k, float top_p, int greedy, uint32_t seed_lo, uint32_t seed_hi, int step_base,
                       const int32_t* ctr, const int32_t* stream_id, int act_len, int num_bins, int32_t* bins, float* values,
                       int64_t* next_ids, int64_t ids_stride, int32_t* status, void* stream);
int db1_obs_tokens(const float* x, int M, int obs_dim, int64_t* ids, int64_t ids_stride, int bin_base, int sep_id, int num_bins, float mu,
                   float M_scale, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DB1_HIP_H */
