/*
 * itr_hip.h -- C ABI of libitr_hip.so: the MI355X (gfx950) encode -> score -> loss / rank
 * hot path of WangFei-2019/Image-text-Retrieval.
 *
 * The reference is 100 % Python and has no FFI layer; its seams for this path are the
 * Python callables listed in SURVEY.md section 8(b).  Each entry point below replaces the
 * arithmetic of one of them (reference file:line cited per function); the Python package
 * `itr_amd` keeps the reference's call signatures on top of this ABI (see INTEGRATION.md for
 * the ctypes binding a maintainer of the reference would add).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to contiguous row-major data unless the name ends in
 *     `_host`; fp32 unless stated; the caller owns all memory (no allocation inside);
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); every call only
 *     enqueues work on it and returns;
 *   - return value: ITR_OK (0) or a negative ITR_ERR_* code; `itr_last_error()` returns a
 *     thread-local message for the last failing call on this thread;
 *   - no exceptions cross the ABI, no global mutable state besides the error string.
 */
#ifndef ITR_HIP_H
#define ITR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ITR_OK 0
#define ITR_ERR_BADARG (-1)      /* -> Python ValueError */
#define ITR_ERR_UNSUPPORTED (-2) /* -> Python NotImplementedError */
#define ITR_ERR_HIP (-3)         /* -> Python RuntimeError */

typedef void *itr_stream_t;

const char *itr_last_error(void);
/* ABI version, bumped on any signature change. */
#define ITR_ABI_VERSION 35
int itr_abi_version(void);

/* ---- a1: l2norm / l1norm  (itr/modalmodule/utils.py:4-15) ----------------------------
 * y[r,:] = x[r,:] / (norm(x[r,:]) + eps), eps added AFTER the sqrt.  kind: 0 = L2, 1 = L1,
 * 2 = F.normalize semantics x / max(||x||_2, eps) (TextEncoder.py:151, ImgEncoder.py:349),
 * 3 = plain x / ||x||_2 without eps (pdist_cos, Objectives.py:318-319; 0/0 stays NaN).
 * take_abs != 0 additionally applies |.| (use_abs, ImgEncoder.py:144).  In place allowed. */
int itr_l2norm_rows(const float *x, float *y, int64_t rows, int dim, float eps, int kind,
                    int take_abs, itr_stream_t stream);

/* y[b,:] = mean_r x[b,r,:] for x [B,R,F]  (torch.mean(x, 1): Fusionmodule.py:412,422; TextEncoder.py:191;
 * ImgEncoder.py:348; the VSE++ region pooling of SURVEY Q3).  At most 65535 groups per call; x and y 16-byte aligned when F % 4 == 0
 * (the float4 path), any alignment otherwise. */
int itr_mean_mid(const float *x, float *y, int64_t B, int R, int F, itr_stream_t stream);

/* ---- measure='order' (config.py:74): order_sim, Objectives.py:24-30 ----------------------
 * out[i, c] = -sqrt( sum_d max(0, s[c, d] - im[i, d])^2 ), out [Ni, Nc] row-major.  D a multiple of 4. */
int itr_order_scores(const float *im, const float *s, float *out, int64_t Ni, int64_t Nc, int D, itr_stream_t stream);
/* Gradient of itr_order_scores for train_emb: S = its output, dS [Ni, Nc] -> d_im [Ni, D], d_s [Nc, D].  A pair with
 * S == 0 (no violated dimension) carries no gradient (torch propagates sqrt'(0) * 0 = NaN there). */
int itr_order_bwd(const float *im, const float *s, const float *S, const float *dS, float *d_im, float *d_s, int64_t Ni,
                  int64_t Nc, int D, itr_stream_t stream);
/* SAEM with measure='order' uses the euclidean distance `pdist` as its "similarity" (Objectives.py:54-56, :297-307):
 * S <- sqrt(n1[i] - 2 S[i, c] + n2[c] + 1e-4) in place on S = x1 x2^T (itr_gemm_nt), n1 / n2 = squared row norms
 * (itr_row_sqnorm: out[r] = sum_d x[r, d]^2). */
int itr_row_sqnorm(const float *x, float *out, int64_t rows, int D, itr_stream_t stream);
int itr_pdist_finish(float *S, const float *n1, const float *n2, int64_t Ni, int64_t Nc, itr_stream_t stream);

/* ---- VSRN region-relationship reasoning: Rs_GCN.forward between its 1x1 convolutions
 * (itr/modalmodule/vsrn_.py:50-71).  tpg [n_img*N, ld]: per region row the three convolution outputs side by side,
 * theta at columns [0, D), phi at [D, 2D), g at [2D, 3D) (one GEMM with the stacked weight).  For every image
 *   y[n, :] = sum_m (theta[n,:] . phi[m,:] / N) g[m, :]           (R = theta_v phi_v^T; R_div_C = R / N; y = R_div_C g_v)
 * y [n_img*N, ldy].  N <= 36 regions (more: ITR_ERR_UNSUPPORTED), D and ld multiples of 4. */
int itr_gcn_relation(const float *tpg, int64_t ld, float *y, int64_t ldy, int64_t n_img, int N, int D,
                     itr_stream_t stream);

/* ---- generic fp32 MFMA GEMM used by the towers ----------------------------------------
 * C[M,N] = act(A[M,K] * B[N,K]^T + bias[N]);  lda/ldb/ldc are row strides in elements.
 * bias may be NULL.  lda < K is allowed (overlapping A rows = a convolution over consecutive rows).  act: 0 none, 1 relu, 2 tanh, 3 sigmoid, 4 gelu(erf), 5 leaky_relu(0.1),
 * 6 NaN -> 0 (itr_gemm_nt only: pdist_cos' `res[res != res] = 0`, Objectives.py:321, without a second pass over the matrix).
 * Exact fp32 (v_mfma_f32_32x32x2_f32).  Replaces nn.Linear / torch.mm call sites on the path
 * (ImgEncoder.py:137, Objectives.py:21, Fusionmodule.py:427-431 ...). */
int itr_gemm_nt(const float *A, int64_t lda, const float *B, int64_t ldb, const float *bias,
                float *C, int64_t ldc, int64_t M, int64_t N, int64_t K, int act,
                itr_stream_t stream);
/* The same product with the kernel chosen by the CALLER (cross-checks and timing; results are bit-identical for every choice):
 * algo 0 = itr_gemm_nt's own selection rule, 1 = the 128 x 128 tile kernel, 2 / 3 = the streaming kernel (plain / XCD-aware tile
 * map) for every shape it admits (N % 128 == 0, K % 64 == 0, K >= 128, 16-byte rows, act in {none, relu, gelu}; other shapes
 * fall through to the tile kernel).  algo 4 = the skinny kernel for M <= 128 rows (N >= 64, K >= 128, 16-byte rows; csrc/gemm_skinny.hip:
 * 16-column strips over all rows, N / 16 workgroups): NOT bit-identical to the others (another k order) and therefore never the
 * library's own choice -- the training tape asks for it for decoder steps and per-caption vector layers. */
int itr_gemm_nt_algo(const float *A, int64_t lda, const float *B, int64_t ldb, const float *bias,
                     float *C, int64_t ldc, int64_t M, int64_t N, int64_t K, int act, int algo,
                     itr_stream_t stream);

/* ---- split-bf16 GEMM (study, opt-in; SURVEY.md 8d "bf16-in / fp32-acc variant reported separately") -------------
 * itr_split_bf16: x [rows, K] fp32 -> out [rows][K / 32][hi (32 bf16) | lo (32 bf16)], hi = bf16(x), lo = bf16(x - hi), both
 * round-to-nearest-even: x = hi + lo + O(2^-17 |x|).  K a multiple of 32; one 32-wide chunk of one row is one 128-byte line.
 * itr_gemm_nt_bf16: C[M,N] = act(A B^T + bias) on v_mfma_f32_32x32x16_bf16 with fp32 accumulation from such operands;
 * terms = 3: hi.hi + hi.lo + lo.hi ("bf16x3"), terms = 1: hi.hi (plain bf16).  lda / ldb count interleaved bf16 elements
 * (2 x the fp32 row stride; lda < 2 K = overlapping rows as in itr_gemm_nt).  No default path calls these: itr_gemm_nt
 * (exact fp32) is the product GEMM. */
int itr_split_bf16(const float *x, uint16_t *out, int64_t rows, int64_t K, itr_stream_t stream);
int itr_gemm_nt_bf16(const uint16_t *A, int64_t lda, const uint16_t *B, int64_t ldb, const float *bias, float *C, int64_t ldc,
                     int64_t M, int64_t N, int64_t K, int act, int terms, itr_stream_t stream);

/* "fp16x3" variant of the study GEMM: fp16 planes (11 + 11 mantissa bits) of x' = s x with s the power of two that puts the
 * tensor's absmax in [2^14, 2^15) (the matrix core flushes fp16 subnormals, so hi must stay normal), lo scaled by 2^11, cross
 * terms in a second accumulator set, everything folded back with exact powers of two: error at the fp32 rounding level for
 * ANY finite operands.  itr_split_f16 computes absmax and the planes; scale_state (2 floats, device) receives the absmax
 * bits and 1 / s and is handed to the GEMM.  Same operand layout as itr_split_bf16. */
int itr_split_f16(const float *x, uint16_t *out, float *scale_state, int64_t rows, int64_t K, itr_stream_t stream);
int itr_gemm_nt_f16x3(const uint16_t *A, int64_t lda, const float *scale_state_a, const uint16_t *B, int64_t ldb,
                      const float *scale_state_b, const float *bias, float *C, int64_t ldc, int64_t M, int64_t N, int64_t K, int act,
                      itr_stream_t stream);

/* ---- a2: EncoderImagePrecomp.forward (itr/modalmodule/ImgEncoder.py:133-147) -----------
 * out[rows, D] = l2norm(x[rows, F] * W[D, F]^T + b[D]) [abs]; rows = n_img * n_regions.
 * no_imgnorm / use_abs as in the reference constructor. */
int itr_proj_l2norm(const float *x, const float *W, const float *b, float *out, int64_t rows,
                    int F, int D, int no_imgnorm, int use_abs, itr_stream_t stream);

/* ---- a3: EncoderText.forward (itr/modalmodule/TextEncoder.py:38-70) --------------------
 * Embedding -> (bi)GRU with packed-sequence semantics -> (fwd+bwd)/2 -> [l2norm] [abs].
 * Captions are PACKED: caption c owns rows [tok_off[c], tok_off[c]+len[c]) of `tokens`
 * (int64 ids, device) and of `out` (fp32 [n_tok, D]).  Captions must be sorted by length
 * DESCENDING (collate_fn does this, data_loader.py:146).  Host arrays: len_host[B].
 * w_ih [3D,E], w_hh [3D,D], b_ih/b_hh [3D] with torch gate order (r,z,n); *_rev = NULL for a
 * uni-directional GRU.  gather_last is a flag word: bit 0 (ITR_GRU_GATHER_LAST) writes only the len-1 state of every
 * caption to out_last[B,D] (method_name in {VSE++,VSRN}, TextEncoder.py:57-60) -- `out` may be NULL then; bit 1
 * (ITR_GRU_BATCH_INVARIANT) makes a caption's result independent of the batch it is encoded in, bit for bit (the
 * recurrence GEMM of a small batch is otherwise split along K, which sums in another order): the sharded evaluation
 * sets it so that every partition of the caption axis gives the single-process rank vectors.
 * workspace: itr_gru_workspace_bytes(n_tok, B, E, D, bi) bytes.
 * Token ids must lie in [0, V): the CALLER validates them (nn.Embedding raises IndexError; itr_amd.ops.gru_encode does the same before
 * the call).  The library only keeps memory safe -- an id outside the range reads embedding row 0 -- and raises no flag: the call
 * enqueues work and returns, it cannot report what a kernel finds. */
#define ITR_GRU_GATHER_LAST 1
#define ITR_GRU_BATCH_INVARIANT 2
/* launch-order variants of the bi-GRU kept as cross-checks (bit-identical results; both measured slower than the default):
 * bit 2: ONE recurrence GEMM and ONE gate launch per time step for both directions; bit 3: each direction's input projection
 * on its own stream after the fork (the round-2 order). */
#define ITR_GRU_PAIRED_DIRECTIONS 4
#define ITR_GRU_INPUT_AFTER_FORK 8
/* The input projection W_ih emb[id] + b_ih depends on the token's id alone: a call with at least twice as many tokens as the
 * vocabulary has words (an evaluation) projects the V embedding rows once and the gate kernel reads the row of the token's id
 * (bit-identical: the same GEMM kernels on the same rows).  bit 4 forces the per-token projection (the cross-check). */
#define ITR_GRU_PER_TOKEN_INPUT 16
/* Last-state output: the batch runs as n interleaved caption chains (caption c in chain c mod n), each a GEMM -> gates sequence
 * on its own stream, so that one chain's launches fill the drains of the others (bit-identical for every n).  bits 5-7: n = 1..4;
 * 0 = the library's choice (2 chains from 4 096 captions on). */
#define ITR_GRU_CHAINS(n) (((n) & 7) << 5)
/* The first time step of a direction starts from h = 0: W_hh h + b_hh is b_hh itself (a product of zero rows sums to +0 exactly), so
 * the step's recurrence GEMM -- the largest of the direction, all captions are still running -- is not launched.  bit 8 launches it
 * anyway (the cross-check; bit-identical). */
#define ITR_GRU_FIRST_STEP_GEMM 256
size_t itr_gru_workspace_bytes(int64_t n_tok, int64_t B, int E, int D, int bidirectional);
int itr_gru_fwd(const int64_t *tokens, const int64_t *tok_off, const int32_t *len_dev,
                const int32_t *len_host, int64_t B, int64_t n_tok, const float *embed, int64_t V,
                int E, int D, const float *w_ih, const float *w_hh, const float *b_ih,
                const float *b_hh, const float *w_ih_rev, const float *w_hh_rev,
                const float *b_ih_rev, const float *b_hh_rev, int no_txtnorm, int use_abs,
                int gather_last, float *out, float *out_last, void *workspace,
                size_t workspace_bytes, itr_stream_t stream);

/* ---- a4: cosine_sim (itr/modalmodule/Objectives.py:18-21) ------------------------------
 * S[Ni,Nc] = im[Ni,D] * s[Nc,D]^T.  Also serves pdist_cos (a9, :310-323) after
 * itr_l2norm_rows(kind=3) and MultiViewMatching (a8) via itr_mvm_scores. */
int itr_cosine_scores(const float *im, const float *s, float *S, int64_t Ni, int64_t Nc, int D,
                      int64_t ldS, itr_stream_t stream);

/* ---- a8: MultiViewMatching.forward (itr/modalmodule/Fusionmodule.py:674-692) ------------
 * S[i,c] = max_v imgs[i,v,:] . caps[c,:]   (imgs [Ni,k,D], caps [Nc,D]). */
int itr_mvm_scores(const float *imgs, const float *caps, float *S, int64_t Ni, int64_t Nc, int k,
                   int D, int64_t ldS, itr_stream_t stream);

/* ---- a5/a10: ContrastiveLoss / TripletLoss (Objectives.py:76-115, :492-517) ------------
 * loss = sum_i red_{j!=i}[m + S_ij - S_ii]_+ + sum_j red_{i!=j}[m + S_ij - S_jj]_+,
 * red = max if max_violation else sum.  fwd writes loss[0] and, for the backward, the arg of
 * the row / column maxima (row_arg[B], col_arg[B]; unused for the sum form, may be NULL).
 * bwd writes dS[B,B] = grad_loss[0] * dloss/dS. */
int itr_hinge_maxviol_fwd(const float *S, int B, int64_t ldS, float margin, int max_violation,
                          float *loss, int32_t *row_arg, int32_t *col_arg, float *cost_ws /* [2B] */,
                          itr_stream_t stream);
int itr_hinge_maxviol_bwd(const float *S, int B, int64_t ldS, float margin, int max_violation,
                          const int32_t *row_arg, const int32_t *col_arg, const float *grad_loss,
                          float *dS, int64_t lddS, itr_stream_t stream);
/* The same loss (Objectives.py:93-115, :492-517) when several rows of a batch share their positive: group[B] (int32, device) names
 * the image of every pair, and an entry (i, j) with i != j and group[i] == group[j] is MASKED -- it is no negative:
 *   loss = sum_i red_{j != i, j unmasked}[m + S_ij - S_ii]_+ + sum_j red_{i != j, i unmasked}[m + S_ij - S_jj]_+.
 * A masked entry costs 0 like the diagonal, is never a row or column arg-max, gets dS = 0 and adds nothing to the diagonal's
 * gradient; the positive stays the diagonal.  The mask is symmetric, so one vector serves rows and columns; any int32 value is a
 * group.  Ties as above: the larger cost wins, on equal costs the lower index, chosen among the UNMASKED candidates (and the
 * diagonal, whose cost is 0).  The forward never writes a masked index into row_arg / col_arg, and the backward checks the mask
 * again.  With all groups distinct every output has the bits of the pair above.  Launches, determinism (no float atomics) and the
 * host checks are the pair's: null S / group / loss / cost_ws / dS / grad_loss, B < 1, ldS < B, lddS < B, missing args with
 * max_violation -> ITR_ERR_BADARG.
 * Purely additive: no existing signature changes, ITR_ABI_VERSION stays 35. */
int itr_hinge_groups_fwd(const float *S, const int32_t *group, int B, int64_t ldS, float margin, int max_violation,
                         float *loss, int32_t *row_arg, int32_t *col_arg, float *cost_ws /* [2B] */, itr_stream_t stream);
int itr_hinge_groups_bwd(const float *S, const int32_t *group, int B, int64_t ldS, float margin, int max_violation,
                         const int32_t *row_arg, const int32_t *col_arg, const float *grad_loss,
                         float *dS, int64_t lddS, itr_stream_t stream);

/* ---- InfoNCE (softmax contrastive) loss on the same B x B matrix: row i is image i, column j caption j, the positive is the
 * diagonal.  The entry stands next to ContrastiveLoss.forward (Objectives.py:93-115) and replaces no reference line.
 *   scale = float32(1 / temperature), z = scale * S (one fp32 product).
 *   group[B] (int32, device; any values) or NULL = no mask: an off-diagonal entry (i, j) with group[i] == group[j] is MASKED, the
 *   rule of itr_hinge_groups_*.  A(i) = {i} u {j : group[j] != group[i]}; the mask is symmetric, so A(i) serves row i and column i.
 *     row_lse[i] = log sum_{j in A(i)} exp(z[i,j])        col_lse[j] = log sum_{i in A(j)} exp(z[i,j])
 *     loss = ( sum_i (row_lse[i] - z[i,i]) + sum_j (col_lse[j] - z[j,j]) ) / (2 B)
 *     dS[i,j] = g * scale / (2 B) * ( exp(z[i,j] - row_lse[i]) + exp(z[i,j] - col_lse[j]) - 2 [i == j] )   for j in A(i)
 *     dS[i,j] = 0 exactly at masked entries;  g = grad_loss[0] (device scalar, as in the hinge).
 *   B = 1 gives loss 0 and dS 0; a row whose negatives are all masked contributes 0.
 * fwd writes loss[0], row_lse[B] and col_lse[B] (fp32, kept for the backward) and needs itr_infonce_workspace_bytes(B) bytes of
 * scratch; bwd makes one pass that writes every entry of dS once, zeros at masked entries included.  Every log-sum-exp subtracts
 * its running maximum; masked entries are skipped, not turned into -inf arithmetic.  Deterministic: no float atomics, the 2B terms
 * are summed in a fixed order, two runs give the same bits, and all-distinct groups give the bits of group == NULL.  S is read in
 * whole 256-byte row segments by the row pass and by the column pass alike.  B is not limited to a multiple of anything.
 * Host checks before anything touches the device (ITR_ERR_BADARG, "itr_infonce_fwd: ..." / "itr_infonce_bwd: ..."): null S /
 * loss / row_lse / col_lse / workspace / grad_loss / dS, B < 1, ldS < B, lddS < B, scale not finite or <= 0.
 * Purely additive: no existing signature changes, ITR_ABI_VERSION stays 35. */
size_t itr_infonce_workspace_bytes(int B);
int itr_infonce_fwd(const float *S, const int32_t *group /* or NULL */, int B, int64_t ldS, float scale, float *loss,
                    float *row_lse, float *col_lse, void *workspace, itr_stream_t stream);
int itr_infonce_bwd(const float *S, const int32_t *group /* or NULL */, int B, int64_t ldS, float scale, const float *row_lse,
                    const float *col_lse, const float *grad_loss, float *dS, int64_t lddS, itr_stream_t stream);

/* ---- Score distillation on the same B x B matrix: the student's scores S are pulled towards the ranking distribution of a teacher's
 * scores T [B, B] over the same batch (T carries no gradient), row-wise and column-wise.  The entry stands
 * next to ContrastiveLoss.forward (Objectives.py:93-115) and replaces no reference line.
 *   scale_s = float32(1 / distill_temperature), scale_t = float32(1 / distill_teacher_temperature),
 *   z_s = scale_s * S, z_t = scale_t * T (one fp32 product each).
 *     p_row[i,:] = softmax_j z_t[i,:]     q_row[i,:] = softmax_j z_s[i,:]
 *     p_col[:,j] = softmax_i z_t[:,j]     q_col[:,j] = softmax_i z_s[:,j]
 *     KL_row[i] = sum_j p_row[i,j] (z_t[i,j] - z_s[i,j]) - lse_t_row[i] + lse_s_row[i]
 *     KL_col[j] = sum_i p_col[i,j] (z_t[i,j] - z_s[i,j]) - lse_t_col[j] + lse_s_col[j]
 *     loss = ( sum_i KL_row[i] + sum_j KL_col[j] ) / (2 B)
 *     dS[i,j] = g scale_s / (2 B) ( (q_row - p_row)[i,j] + (q_col - p_col)[i,j] );   g = grad_loss[0] (device scalar, as in the hinge).
 *   There is no group mask: every row and column runs over the whole batch.  The teacher scores the other captions of an image highly,
 *   so they become soft positives and need no mask.
 *   The two log-sum-exps of a row or column are subtracted from each other first, then from the cross term.  With T bit-equal to S and
 *   scale_t == scale_s the loss is bit-zero and dS is bit-zero; B = 1 gives loss 0 and dS 0.
 * fwd is one pass over both matrices (a running (max, sum) pair for z_s and a (max, sum, weighted sum) triple for z_t per row and column)
 * plus a finishing workgroup; it writes loss[0] and the four log-sum-exp vectors row_lse_s[B], col_lse_s[B], row_lse_t[B], col_lse_t[B]
 * (fp32, kept for the backward) and needs itr_distill_workspace_bytes(B) bytes of scratch (0 for B <= 0; linear in B).  bwd is one
 * launch that writes every entry of dS once from the four saved vectors.  Deterministic: no float atomics, the 2B terms are summed in a
 * fixed order in float64, two runs give the same bits.  S and T are read in whole 256-byte row segments by the row pass and by the
 * column pass alike.  B is not limited to a multiple of anything; ldS, ldT and lddS may exceed B.
 * Host checks before anything touches the device (ITR_ERR_BADARG, "itr_distill_fwd: ..." / "itr_distill_bwd: ..."): a null pointer,
 * B < 1, ldS < B, ldT < B, lddS < B, scale_s or scale_t not finite or <= 0.
 * Purely additive: no existing signature changes, ITR_ABI_VERSION stays 35. */
size_t itr_distill_workspace_bytes(int B);
int itr_distill_fwd(const float *S, const float *T, int B, int64_t ldS, int64_t ldT, float scale_s, float scale_t, float *loss,
                    float *row_lse_s, float *col_lse_s, float *row_lse_t, float *col_lse_t, void *workspace, itr_stream_t stream);
int itr_distill_bwd(const float *S, const float *T, int B, int64_t ldS, int64_t ldT, float scale_s, float scale_t,
                    const float *row_lse_s, const float *col_lse_s, const float *row_lse_t, const float *col_lse_t,
                    const float *grad_loss, float *dS, int64_t lddS, itr_stream_t stream);

/* ---- Cross-batch memory (XBM): the two losses above on batch u memory.  S [B, B] is the step's matrix (image i vs caption j); R [B, n]
 * scores image i against memory caption k and C [n, B] memory image k against caption j, the memory being n detached (image, caption)
 * embeddings of earlier steps.  Row i's candidates are S[i, :] then R[i, :], column j's are S[:, j] then C[:, j]; a candidate index
 * t in [0, B + n) is in-batch for t < B and memory slot t - B otherwise.  The entries replace no reference line.
 *   group[B], bank_group[n] (int32, device; any values; never NULL -- bank_group may be NULL when n == 0).  Kept sets:
 *     S (i, j), i != j: dropped iff mask_batch && group[i] == group[j]   (the rule of itr_hinge_groups_*; the diagonal is the positive)
 *     R (i, k):         dropped iff group[i] == bank_group[k]            (always: a stored caption of the query's own image)
 *     C (k, j):         dropped iff bank_group[k] == group[j]
 *   A dropped entry is skipped, never fed into the arithmetic, and its gradient is bit-zero.
 * Hinge: cost = max(0, (margin + s) - d) in fp32, d = S[q,q]; the diagonal and dropped entries cost 0.
 *     sum form  loss = all row-side costs over S and R + all column-side costs over S and C
 *     max form  loss = sum_i max(row i's candidates) + sum_j max(column j's candidates)
 *   row_arg[B], col_arg[B] (required in both forms): max form -- the candidate index of the largest cost; the larger cost wins, on
 *   equal costs the earlier candidate (in-batch ascending, then slots ascending), chosen among kept candidates and the diagonal only.
 *   Sum form -- the number of violators of the row / column (the diagonal's gradient is -g (row_arg[i] + col_arg[i])).
 *   bwd checks range and mask of the saved args again; max form: at most one nonzero per row of dR and per column of dC.
 * InfoNCE: scale = float32(1 / temperature), z = scale * s (one fp32 product).
 *     row_lse[i] = log( sum_{j kept} exp zS[i,j] + sum_{k kept} exp zR[i,k] )
 *     col_lse[j] = log( sum_{i kept} exp zS[i,j] + sum_{k kept} exp zC[k,j] )
 *     loss = ( sum_i (row_lse[i] - zS[i,i]) + sum_j (col_lse[j] - zS[j,j]) ) / (2 B)
 *     dS[i,j] = g scale / (2 B) ( exp(zS[i,j] - row_lse[i]) + exp(zS[i,j] - col_lse[j]) - 2 [i == j] ),
 *     dR[i,k] = g scale / (2 B) exp(zR[i,k] - row_lse[i]),   dC[k,j] = g scale / (2 B) exp(zC[k,j] - col_lse[j])   on kept, 0 elsewhere
 *   Every log-sum-exp is a running (max, sum) pair; the empty set is the pair with sum 0.
 * fwd needs itr_xbm_workspace_bytes(B, n) bytes of scratch.  Rows are read by one wave each; for the columns a workgroup owns 64
 * adjacent columns and one slice of the B + n candidate rows, read in whole 256-byte row segments, and a finishing workgroup merges
 * the slices in slice order and sums the 2B terms in float64.  Deterministic: no float atomics, two runs give the same bits.
 * bwd writes every entry of dS [B,B], dR [B,n] and dC [n,B] once, zeros included; g = grad_loss[0] (device scalar).
 * Host checks before anything touches the device (ITR_ERR_BADARG, "<entry>: ..."): null pointers, B < 1, n < 0, ldS < B, ldR < n,
 * ldC < B (and lddS / lddR / lddC alike), B (B + 2 n) >= 2^31, scale not finite or <= 0.
 * itr_xbm_ring_write: table[(head + r) % capacity, :] = src[r, :] for r < count, rows of `width` 32-bit words -- one launch writes a
 * push of the memory's FIFO across the wrap (0 <= head < capacity, count <= capacity).
 * Purely additive: no existing signature changes, ITR_ABI_VERSION stays 35. */
size_t itr_xbm_workspace_bytes(int B, int n);
int itr_xbm_hinge_fwd(const float *S, int64_t ldS, const float *R, int64_t ldR, const float *C, int64_t ldC, const int32_t *group,
                      const int32_t *bank_group, int B, int n, int mask_batch, float margin, int max_violation, float *loss,
                      int32_t *row_arg, int32_t *col_arg, void *workspace, itr_stream_t stream);
int itr_xbm_hinge_bwd(const float *S, int64_t ldS, const float *R, int64_t ldR, const float *C, int64_t ldC, const int32_t *group,
                      const int32_t *bank_group, int B, int n, int mask_batch, float margin, int max_violation,
                      const int32_t *row_arg, const int32_t *col_arg, const float *grad_loss, float *dS, int64_t lddS, float *dR,
                      int64_t lddR, float *dC, int64_t lddC, itr_stream_t stream);
int itr_xbm_infonce_fwd(const float *S, int64_t ldS, const float *R, int64_t ldR, const float *C, int64_t ldC, const int32_t *group,
                        const int32_t *bank_group, int B, int n, int mask_batch, float scale, float *loss, float *row_lse,
                        float *col_lse, void *workspace, itr_stream_t stream);
int itr_xbm_infonce_bwd(const float *S, int64_t ldS, const float *R, int64_t ldR, const float *C, int64_t ldC, const int32_t *group,
                        const int32_t *bank_group, int B, int n, int mask_batch, float scale, const float *row_lse,
                        const float *col_lse, const float *grad_loss, float *dS, int64_t lddS, float *dR, int64_t lddR, float *dC,
                        int64_t lddC, itr_stream_t stream);
int itr_xbm_ring_write(const void *src, void *table, int64_t capacity, int64_t width, int64_t head, int64_t count,
                       itr_stream_t stream);

/* ---- a6: xattn_score_t2i / xattn_score_i2t (Objectives.py:329-476) ---------------------
 * img [Ni,R,D]; words [n_rows,D] with caption c owning rows cap_off[c] .. cap_off[c]+len[c]-1
 * (padded (Nc,L,D) input: cap_off[c] = c*L).  S[i,c] written with row stride ldS.
 * mode: 0 t2i, 1 i2t.  norm: 0 clipped_l2norm, 1 l2norm, 2 softmax, 3 no_norm, 4 clipped,
 * 5 l1norm, 6 clipped_l1norm.  agg: 0 LogSumExp, 1 Max, 2 Sum, 3 Mean.
 * Three steps:
 *  1. itr_scan_plan_tiles (pure CPU): whole captions are bin-packed (tiles filled exactly where the lengths allow it) into column
 *     tiles of <= ITR_SCAN_NT words: cap_order[Nc] lists the caption ids tile by tile and
 *     tile_begin[n_tiles+1] indexes it; the caller copies both to the device.
 *  2. itr_scan_prepare: once per (image block, caption set, mode) -- re-packs the word embeddings tile
 *     by tile into the workspace and precomputes region Gram matrices V_i V_i^T + word norms (t2i) or
 *     region norms + caption Gram matrices E_c E_c^T (i2t).
 *  3. itr_scan_xattn_scores: the fused MFMA kernel; needs only `img` and the prepared workspace and may
 *     be called repeatedly (other norm / agg / lambda) without preparing again.
 * workspace: itr_scan_workspace_bytes(Ni, R, n_rows, Nc, n_tiles, D) bytes. */
#define ITR_SCAN_NT 64
int itr_scan_plan_tiles(const int32_t *len_host, int64_t Nc, int nt, int32_t *tile_begin_host,
                        int32_t *cap_order_host, int64_t *n_tiles);
size_t itr_scan_workspace_bytes(int64_t Ni, int R, int64_t n_rows, int64_t Nc, int64_t n_tiles, int D);
int itr_scan_prepare(const float *img, const float *words, const int64_t *cap_off,
                     const int32_t *cap_len, const int32_t *tile_begin_dev,
                     const int32_t *cap_order_dev, int64_t n_tiles, int64_t Ni, int64_t Nc,
                     int64_t n_rows, int R, int D, int mode, void *workspace, size_t workspace_bytes,
                     itr_stream_t stream);
int itr_scan_xattn_scores(const float *img, int64_t n_tiles, int64_t Ni, int64_t Nc, int64_t n_rows,
                          int R, int D, int mode, int norm, int agg, float lambda_softmax,
                          float lambda_lse, float *S, int64_t ldS, void *workspace,
                          size_t workspace_bytes, itr_stream_t stream);

/* Opt-in study variant (SURVEY.md 8d "bf16-in / fp32-acc variant reported separately"): the same scores
 * with the region x word dot products on the bf16 matrix core from split operands, x = hi + lo, hi.hi + hi.lo + lo.hi,
 * fp32 accumulation ("bf16x3", ~1e-6 of the fp32 result on the unit-norm operands of this path); the epilogue is the
 * fp32 one.  bf16_workspace: itr_scan_bf16_workspace_bytes(Ni, R, n_tiles, D) bytes of scratch for the split planes.
 * split_format 0: bf16 planes (8 + 8 mantissa bits).  split_format 1 ("fp16x3"): fp16 planes (11 + 11 bits, lo scaled by 2^11,
 * cross terms in a second accumulator): ~1e-7 of the fp32 result, needs |x| <= 65504 (unit-norm rows on this path). */
size_t itr_scan_bf16_workspace_bytes(int64_t Ni, int R, int64_t n_tiles, int D);
int itr_scan_xattn_scores_bf16x3(const float *img, int64_t n_tiles, int64_t Ni, int64_t Nc, int64_t n_rows, int R, int D,
                                 int mode, int norm, int agg, float lambda_softmax, float lambda_lse, float *S,
                                 int64_t ldS, void *workspace, size_t workspace_bytes, void *bf16_workspace,
                                 size_t bf16_workspace_bytes, int split_format, itr_stream_t stream);

/* ---- a11: BERT building blocks (itr/modalmodule/bert.py:113-358); the dense layers use itr_gemm_nt (act 4 =
 * erf-GELU :29-34, act 2 = tanh pooler :299-302).
 * itr_bert_embed_ln : out[b,t,:] = LN(word[ids] + pos[t] + type[type_ids]) (:127-157); type_ids may be NULL (zeros).
 * itr_add_layernorm : out = LN(x + residual) with the TF-style epsilon inside the sqrt (:113-126); residual may be NULL.
 * itr_mha_small     : per (sequence, head): softmax(Q K^T * scale + (1 - mask) * -10000) V for L <= 64 (:185-207);
 *                     q/k/v are [B*L, ld*] views (heads contiguous, head h at column h*dk); mask [B*L] of 0/1 or NULL.
 * itr_relu_maxpool  : out[b,c] = max_{t<valid} relu(x[b,t,c])  (SAEM conv head, TextEncoder.py:148-149). */
int itr_bert_embed_ln(const int64_t *ids, const int64_t *type_ids, const float *word_emb, const float *pos_emb,
                      const float *type_emb, const float *gamma, const float *beta, float *out, int64_t B,
                      int L, int H, int64_t vocab, int max_pos, int type_vocab, float eps, itr_stream_t stream);
int itr_add_layernorm(const float *x, const float *residual, const float *gamma, const float *beta, float *out,
                      int64_t rows, int H, float eps, itr_stream_t stream);
int itr_mha_small(const float *q, const float *k, const float *v, int64_t ldq, int64_t ldk, int64_t ldv,
                  const float *mask, float *out, int64_t ldo, int64_t B, int L, int heads, int dk, float scale,
                  itr_stream_t stream);
int itr_relu_maxpool(const float *x, float *out, int64_t ldo, int64_t B, int L, int C, int valid,
                     itr_stream_t stream);

/* ---- a13: CAMERA helpers (itr/modalmodule/camera_.py; ImgEncoder.py:355-433; TextEncoder.py:162-197) ----
 * itr_gemm_nt_acc     : C = act(C + A B^T + bias)  -- sums the taps of the dilated Conv1d summarisation (:100-103)
 * itr_mul_rows        : out[r,c] = a[r,c] * b[r*ldb + c]   (position gating :75, query/key gates :38-40)
 * itr_affine_cols     : out = act(x*scale[c] + shift[c]) + residual  (eval BatchNorm1d folded; scale/shift/residual may be NULL)
 * itr_agsa_gate       : the query / key gate of GatedQueryAttLayer.forward (:36-44) in one kernel: rows = positions x heads, q / k
 *                       [rows, dk] (dk = 16 or 32; other head sizes: compose itr_gemm_nt + itr_mul_rows),  G = fc_q(q) * fc_k(k),
 *                       M = sigmoid(fc_g(G)) [rows, 2 dk],  q_out = q * M[:, :dk],  k_out = k * M[:, dk:]  (outputs may alias inputs)
 * itr_camera_posenc   : absoluteEncode(boxes, imgs_wh) -> [B*R, 6]   (:118-128)
 * itr_camera_summarize: softmax over regions of smry[B,R,k], L^T X, F.normalize -> [B,k,D]  (ImgEncoder.py:385-389); R <= 64
 *                       (more: ITR_ERR_UNSUPPORTED) */
int itr_gemm_nt_acc(const float *A, int64_t lda, const float *B, int64_t ldb, const float *bias, float *C,
                    int64_t ldc, int64_t M, int64_t N, int64_t K, int act, itr_stream_t stream);
/* C = act(R + A B^T + bias): itr_gemm_nt_acc with the summand read from its own matrix (Rs_GCN's `W(y) + v`, vsrn_.py:64-67: no
 * copy of v into the output first).  Same arithmetic order as itr_gemm_nt_acc on a copy: bit-identical. */
int itr_gemm_nt_residual(const float *A, int64_t lda, const float *B, int64_t ldb, const float *bias, const float *R, int64_t ldr,
                         float *C, int64_t ldc, int64_t M, int64_t N, int64_t K, int act, itr_stream_t stream);
int itr_mul_rows(const float *a, const float *b, int64_t ldb, float *out, int64_t R, int C, itr_stream_t stream);
int itr_affine_cols(const float *x, const float *scale, const float *shift, const float *residual, float *out,
                    int64_t R, int C, int act, itr_stream_t stream);
int itr_agsa_gate(const float *q, const float *k, int64_t rows, int dk, const float *Wq, const float *bq, const float *Wk,
                  const float *bk, const float *Wg, const float *bg, float *q_out, float *k_out, itr_stream_t stream);
int itr_camera_posenc(const float *boxes, const float *imgs_wh, float *out, int64_t B, int R, itr_stream_t stream);
int itr_camera_summarize(const float *smry, const float *X, float *out, int64_t B, int R, int k, int D,
                         itr_stream_t stream);

/* ---- a7: EncoderSimilarity.forward (SGRAF; itr/modalmodule/Fusionmodule.py:373-664), eval mode ----
 * img [Ni,36,D] (l2-normalised regions), words [n_rows,D] with the caption layout of the SCAN entry points
 * (cap_off / cap_len / tile plan from itr_scan_plan_tiles on the word lengths).  module: 0 = SAF, 1 = SGR.
 * weights: device pointers named after the reference's state_dict (row-major [out,in] like nn.Linear).
 * S[i,c] in (0,1).  max_len = longest caption (<= 63).  workspace: itr_sgraf_workspace_bytes(...).
 * node_group_*: optional plan for SGR's fused graph steps (GraphReasoning x sgr_step, Fusionmodule.py:564-597, in one
 * workgroup per group of captions): itr_sgr_plan_node_groups (pure CPU) bins whole captions by the node count of their
 * graph (cap_len[c] + 1) into groups of <= 16 captions and <= 64 node rows (small_rows = 64: one workgroup per CU, the
 * default) or, for captions of <= 31 words, <= 32 node rows (small_rows = 32: two workgroups per CU; same scores); pass
 * its group_begin / group_order arrays (device copies) and the group count.  Any plan with <= 16 captions and <= 64 node
 * rows per group is accepted; a group that breaks these bounds is not scored and its captions' columns of S are filled
 * with NaN.  NULL / 0: the steps run one kernel chain per step (also taken for sim_dim != 256). */
typedef struct {
    /* v_global_w (VisualSA :464-507) */
    const float *v_loc_w, *v_loc_b, *v_loc_bn_w, *v_loc_bn_b, *v_loc_bn_mean, *v_loc_bn_var; /* Linear[D,D], BN(36) */
    const float *v_glo_w, *v_glo_b, *v_glo_bn_w, *v_glo_bn_b, *v_glo_bn_mean, *v_glo_bn_var; /* Linear[D,D], BN(D)  */
    const float *v_com_w, *v_com_b;                                                          /* Linear[1,D]         */
    /* t_global_w (TextSA :519-559) */
    const float *t_loc_w, *t_loc_b, *t_glo_w, *t_glo_b, *t_com_w, *t_com_b;
    /* sim_tranloc_w / sim_tranglo_w [S,D], sim_eval_w [1,S] (:391-395) */
    const float *loc_w, *loc_b, *glo_w, *glo_b, *eval_w, *eval_b;
    /* SAF_module.attn_sim_w [1,S], SAF_module.bn (1 channel) (:608-611) */
    const float *saf_w, *saf_b, *saf_bn_w, *saf_bn_b, *saf_bn_mean, *saf_bn_var;
    /* SGR_module.sgr{k}.graph_query_w / graph_key_w / sim_graph_w [S,S] (:573-576) */
    const float *sgr_q_w[8], *sgr_q_b[8], *sgr_k_w[8], *sgr_k_b[8], *sgr_g_w[8], *sgr_g_b[8];
} itr_sgraf_weights;
int itr_sgr_plan_node_groups(const int32_t *cap_len_host, int64_t Nc, int small_rows /* 64 or 32 */,
                             int32_t *group_begin_host, int32_t *group_order_host, int64_t *n_groups);
/* image_block: images per block of the pair stage -- 0 = ITR_SGRAF_DEFAULT_IMAGE_BLOCK, else a multiple of 4 in [4, 64]; never more than
 * the call's image count rounded up to 4.  The workspace grows with it (5k x 25k: 64 -> SAF 38 GB, SGR 42 GB; 16 -> 13 / 14 GB) and
 * the scores do not depend on it: the caller picks it for the memory it has -- itr_sgraf_pick_image_block returns the largest of
 * 64 / 32 / 16 / 8 / 4 whose workspace fits max_workspace_bytes (and that size in *workspace_bytes), or ITR_ERR_UNSUPPORTED when even a
 * 4-image block does not fit (the reference's own loop is O(tile) in memory: Fusionmodule.py:406-451 scores one caption at a time).
 * flags: ITR_SGRAF_UNFUSED_STEPS = SGR's graph steps as the step-by-step kernel chain even when a node-group plan is given (the form
 * the fused kernel is cross-checked against; also what runs -- and what the workspace must be sized for -- when NO plan is passed);
 * ITR_SGRAF_NON_PERSISTENT = fused SGR with one workgroup per (image, group) instead of the persistent walk.  Same scores. */
#define ITR_SGRAF_DEFAULT_IMAGE_BLOCK 64
#define ITR_SGRAF_UNFUSED_STEPS 1
#define ITR_SGRAF_NON_PERSISTENT 2
size_t itr_sgraf_workspace_bytes(int64_t Ni, int64_t Nc, int64_t n_rows, int64_t n_tiles, int D, int S,
                                 int module, int image_block, int flags);
int itr_sgraf_pick_image_block(int64_t Ni, int64_t Nc, int64_t n_rows, int64_t n_tiles, int D, int S, int module, int flags,
                               size_t max_workspace_bytes, size_t *workspace_bytes /* host, may be NULL */);
int itr_sgraf_scores(const float *img, const float *words, const int64_t *cap_off, const int32_t *cap_len,
                     const int32_t *tile_begin_dev, const int32_t *cap_order_dev, int64_t n_tiles,
                     int64_t Ni, int64_t Nc, int64_t n_rows, int max_len, int R, int D, int S, int module,
                     int sgr_step, const itr_sgraf_weights *w, const int32_t *node_group_begin_dev,
                     const int32_t *node_group_order_dev, int64_t n_node_groups, int image_block, int flags, float *S_out,
                     int64_t ldS, void *workspace, size_t workspace_bytes, itr_stream_t stream);

/* diagnostics (bench.py's sustained-clock probe): one INSTRUMENTED launch of the SCAN kernel with the arguments of
 * itr_scan_xattn_scores.  `scratch` [Ni, ld_scratch >= Nc + 64] is not a score matrix afterwards: its first 64 bytes hold eight
 * uint64 counters summed over all workgroups -- [0..6] shader-clock cycles (s_memtime) per phase, [7] 100 MHz ticks
 * (s_memrealtime); the rest is undefined.  sustained clock [MHz] = 100 * sum(c[0..6]) / c[7]. */
int itr_debug_scan_clock_probe(const float *img, int64_t n_tiles, int64_t Ni, int64_t Nc, int64_t n_rows, int R, int D, int mode,
                               int norm, int agg, float lambda_softmax, float lambda_lse, float *scratch, int64_t ld_scratch,
                               void *workspace, size_t workspace_bytes, itr_stream_t stream);

/* ---- a17: i2t / t2i ranker (itr/metricmodule/evaluation.py:156-222) --------------------
 * Sort-free: rank(query, gt) = #{k: S_k > S_gt} + #{k > gt: S_k == S_gt}; i2t takes the min
 * over the im_div GT captions im_div*i .. im_div*i+im_div-1; t2i's GT image is j / im_div.
 * top1 = argmax (highest index on ties).  S is the LOCAL row block [n_rows_local, Nc] holding
 * global image rows row0 .. row0+n_rows_local-1 (row0 = 0 for a single GPU).
 *   i2t_rank/top1 [n_rows_local]  -- complete (rows are local).
 *   t2i needs the GT score of every caption: pass s_gt[Nc] (gathered over ranks); the kernel
 *   ACCUMULATES partial counts into t2i_rank[Nc] (int32, zero it first) and max-reduces
 *   t2i_best[Nc] (uint64 key = ordered(score) << 32 | row; zero it first), so a sum /
 *   max all-reduce over ranks completes them.  itr_rank_gather_gt fills s_gt for the GT
 *   rows this rank owns (others left untouched; buffer pre-filled with -inf + max-reduce).
 * ONE pass over S serves both directions (every element is read once: 4 bytes per pair), between a small preparation and a
 * small finishing kernel.  workspace: itr_rank_workspace_bytes(n_rows_local, Nc) bytes, 8-byte aligned (per-row GT keys and running
 * top-1 keys, the GT scores when the call gathers them itself).
 * s_gt may be NULL when the block holds EVERY ground-truth row (row0 = 0 and n_rows_local * im_div >= Nc: the single-GPU call):
 * the scores are then read from S itself -- no itr_rank_gather_gt launch.  flags: ITR_RANK_INIT_COLUMNS = zero t2i_rank / t2i_best
 * inside the call (single-call use; leave it out when several row blocks -- or several ranks -- accumulate into them).
 * Order of scores: -0.0 == +0.0; NaN sorts as the LARGEST value (np.argsort's order: NaN last ascending, first after
 * [::-1]), ties -- also among NaN / +inf -- go to the higher index; the float64 entry points use the same rule. */
#define ITR_RANK_INIT_COLUMNS 1
int itr_rank_gather_gt(const float *S, int64_t ldS, int64_t row0, int64_t n_rows_local, int64_t Nc,
                       int im_div, float *s_gt, itr_stream_t stream);
size_t itr_rank_workspace_bytes(int64_t n_rows_local, int64_t Nc);
int itr_rank_counts(const float *S, int64_t ldS, int64_t row0, int64_t n_rows_local, int64_t Nc,
                    int im_div, const float *s_gt, int32_t *i2t_rank, int32_t *i2t_top1,
                    int32_t *t2i_rank, uint64_t *t2i_best, int flags, void *workspace, size_t workspace_bytes, itr_stream_t stream);
/* float64 matrices.  The reference ranks the float64 array cal_sims returns (evaluation.py:169, :209), and
 * evalrank_ensemble averages two models' matrices in float64 before ranking (evaluation.py:380, :398): such
 * scores are not fp32-representable, so they are counted in float64 -- same counts, same tie rule, index-exact.
 * t2i_best_key[Nc] (zero it first) is max-reduced to the 64-bit ordered key of every column's best score;
 * itr_rank_t2i_top1_f64 then max-reduces t2i_top1[Nc] (int32, pre-filled with -1) to the highest global row
 * holding that key (second pass over S; with several ranks: max all-reduce the keys between the two calls and
 * t2i_top1 after). */
int itr_rank_gather_gt_f64(const double *S, int64_t ldS, int64_t row0, int64_t n_rows_local, int64_t Nc,
                           int im_div, double *s_gt, itr_stream_t stream);
int itr_rank_counts_f64(const double *S, int64_t ldS, int64_t row0, int64_t n_rows_local, int64_t Nc,
                        int im_div, const double *s_gt, int32_t *i2t_rank, int32_t *i2t_top1,
                        int32_t *t2i_rank, uint64_t *t2i_best_key, itr_stream_t stream);
int itr_rank_t2i_top1_f64(const double *S, int64_t ldS, int64_t row0, int64_t n_rows_local, int64_t Nc,
                          const uint64_t *t2i_best_key, int32_t *t2i_top1, itr_stream_t stream);
/* host-side summary (evaluation.py:181-185): out5 = r1, r5, r10, medr, meanr. */
int itr_recall_from_ranks(const int32_t *ranks_host, int64_t n, double *out5);

/* ---- positions under any ground-truth relation (csrc/rank_gt.hip) -------------------------
 * The ranker above knows one ground truth, caption j <-> image j / im_div.  These entry points take a sparse relation in both
 * CSR forms (int32, on the device): img_ptr [Ni + 1] / img_cap [nnz], the positive captions of every image, ascending within an
 * image, and cap_ptr [Nc + 1] / cap_img [nnz], the positive images of every caption, ascending.  They return, per pair,
 *   i2t_pos [nnz] (image-CSR order) / t2i_pos [nnz] (caption-CSR order): the 0-based position of that positive in its query's
 *   ranked list = #{k : key_k > key_positive} over the whole row / column, in the ranker's order (larger score first, the higher
 *   index on an exact tie, -0.0 == +0.0, NaN as +inf).  Any number of positives per query, from none to the whole gallery.
 * S [n_rows_local, Nc] is a row block holding global rows row0 .. row0 + n_rows_local - 1 of the Ni rows (ldS >= Nc, any alignment).
 *   itr_rank_gt_gather writes the keys of the positives whose ROW lies in the block into i2t_key / t2i_key [nnz] (uint64; other
 *     entries are left untouched): a column's positives may lie in rows of another block, so all blocks are gathered first;
 *   itr_rank_gt_count counts the block against the keys: i2t_pos of the block's rows is final (plain stores), t2i_pos is an
 *     integer sum over row blocks (other blocks, other ranks just add).  flags: ITR_RANK_GT_INIT = zero t2i_pos inside the call
 *     (the first block, or a whole matrix).  workspace: itr_rank_gt_workspace_bytes(nnz, 0) bytes, 8-byte aligned.
 * itr_rank_gt_positions_f64: a whole float64 matrix (cal_sims' output, ensemble averages) in float64 order (ordered double, then
 * the index), gather and count in one call; workspace: itr_rank_gt_workspace_bytes(nnz, 1) bytes.
 * The relation must be well formed (the Python layer validates it on the host); whatever it holds, no entry of it becomes an
 * address unchecked.  Null pointers, ldS < Nc, negative sizes, rows past Ni -> ITR_ERR_BADARG; nnz, Ni or Nc >= 2^31 ->
 * ITR_ERR_UNSUPPORTED; nnz == 0, n_rows_local == 0 or Nc == 0 -> ITR_OK, nothing written.
 * Purely additive: no existing signature changes, ITR_ABI_VERSION stays 35. */
#define ITR_RANK_GT_INIT 1
size_t itr_rank_gt_workspace_bytes(int64_t nnz, int f64);
int itr_rank_gt_gather(const float *S, int64_t ldS, int64_t row0, int64_t n_rows_local, int64_t Nc, int64_t Ni, int64_t nnz,
                       const int32_t *img_ptr, const int32_t *img_cap, const int32_t *cap_ptr, const int32_t *cap_img,
                       uint64_t *i2t_key, uint64_t *t2i_key, itr_stream_t stream);
int itr_rank_gt_count(const float *S, int64_t ldS, int64_t row0, int64_t n_rows_local, int64_t Nc, int64_t Ni, int64_t nnz,
                      const int32_t *img_ptr, const int32_t *cap_ptr, const uint64_t *i2t_key, const uint64_t *t2i_key,
                      int32_t *i2t_pos, int32_t *t2i_pos, int flags, void *workspace, size_t workspace_bytes, itr_stream_t stream);
int itr_rank_gt_positions_f64(const double *S, int64_t ldS, int64_t Ni, int64_t Nc, int64_t nnz, const int32_t *img_ptr,
                              const int32_t *img_cap, const int32_t *cap_ptr, const int32_t *cap_img, int32_t *i2t_pos,
                              int32_t *t2i_pos, void *workspace, size_t workspace_bytes, itr_stream_t stream);

/* ---- top-K retrieval lists (itr/metricmodule/evaluation.py:156-222) ----------------------
 * The reference builds the full ranked list of every query, inds = np.argsort(sims[index])[::-1] (evaluation.py:169 i2t,
 * :209 t2i), and keeps inds[0] and the ground truth's position.  These entry points return the first K entries of those
 * lists, selected on the GPU in the ranker's order (larger score first, the higher index on exact ties, -0.0 == +0.0, NaN
 * as +inf): column 0 is the ranker's top-1.  Returned scores are the ORIGINAL bits of S at the returned index (a -0.0
 * stays -0.0, a NaN stays NaN).  1 <= K <= ITR_TOPK_MAX (ITR_ERR_UNSUPPORTED above).
 * itr_topk: S is the LOCAL row block [n_rows_local, Nc] (leading dimension ldS >= Nc, any alignment) holding global rows
 * row0 .. row0 + n_rows_local - 1.  Either direction may be left out by passing NULL for both of its outputs.
 *   i2t: row_idx [n_rows_local, K] (column indices, best first), row_val [n_rows_local, K]; K > Nc -> ITR_ERR_BADARG.
 *   t2i: col_key [Nc, K] (uint64 key = ordered score << 32 | GLOBAL row, best first) and col_val [Nc, K]: a partial list of
 *        this block's rows.  A block with fewer than K rows leaves key 0 / score 0 in the entries past them.
 *        itr_topk_merge merges n_parts such lists, laid out [n_parts][Nc][K_in] (row blocks of one matrix, ranks), into the
 *        whole-matrix lists col_idx [Nc, K] (global rows; -1 where the parts hold fewer than K entries) / col_val [Nc, K];
 *        the result is the same for every partition of the rows.  n_parts <= ITR_TOPK_MAX_PARTS, K <= n_parts * K_in.
 *   workspace: itr_topk_workspace_bytes(n_rows_local, Nc, K) bytes, 8-byte aligned (0 bytes: may be NULL).
 * itr_topk_f64: a whole float64 matrix (cal_sims' output, ensemble averages); the key is the ordered double, then the index,
 * with the same tie, NaN and signed-zero rules.  col_idx [Nc, K] / col_val [Nc, K] are final; K larger than a requested
 * line -> ITR_ERR_BADARG.
 * n_rows == 0 or Nc == 0: ITR_OK, nothing written. */
#define ITR_TOPK_MAX 128
#define ITR_TOPK_MAX_PARTS 32
size_t itr_topk_workspace_bytes(int64_t n_rows_local, int64_t Nc, int K);
int itr_topk(const float *S, int64_t ldS, int64_t row0, int64_t n_rows_local, int64_t Nc, int K, int32_t *row_idx,
             float *row_val, uint64_t *col_key, float *col_val, void *workspace, size_t workspace_bytes, itr_stream_t stream);
int itr_topk_merge(const uint64_t *part_key, const float *part_val, int n_parts, int64_t Nc, int K_in, int K,
                   int32_t *col_idx, float *col_val, itr_stream_t stream);
int itr_topk_f64(const double *S, int64_t ldS, int64_t n_rows, int64_t Nc, int K, int32_t *row_idx, double *row_val,
                 int32_t *col_idx, double *col_val, itr_stream_t stream);

/* ---- running top-K column lists: a similarity matrix that is never stored (csrc/topk_fold.hip) ----
 * itr_topk_fold_cols folds ONE row block S [n_rows_local, Nc] (global rows row0 .. row0 + n_rows_local - 1, leading dimension
 * ldS >= Nc, any alignment) into running column lists col_key [Nc, K] / col_val [Nc, K], which the call reads AND writes.  Their
 * layout is exactly that of itr_topk's column part: keys = ordered score << 32 | GLOBAL row, best first, key 0 = empty entry;
 * col_val holds the ORIGINAL bits of the score (carried along with its key, never rebuilt from it: a -0.0 stays -0.0, a NaN
 * stays NaN).  After the call the lists hold the K largest keys of (the lists before) U (the entries of this block's columns).
 *   - All zeros is the empty starting state; a part written by itr_topk (same K) is a valid starting state too.
 *   - A state is a valid part for itr_topk_merge: itr_topk_merge(state, 1 part, K_in = K) turns it into col_idx / col_val.
 *   - The result is a function of the SET of keys alone: any partition of a matrix into row blocks, folded in any order, gives
 *     bit for bit the whole-matrix lists of itr_topk + itr_topk_merge, however the workgroups of a call are scheduled.
 *   - PRECONDITION (documented, not checked): the block's rows are not in the lists already (a row folded twice is listed twice).
 *   - No host read-back and no allocation inside the call.  workspace: itr_topk_fold_workspace_bytes(n_rows_local, Nc, K) bytes
 *     (currently 0 for every shape: a strip of columns is merged where it lies; NULL is accepted then).
 * Arguments as for itr_topk, except that K outside 1 .. ITR_TOPK_MAX is ITR_ERR_UNSUPPORTED on either side; null S or outputs,
 * ldS < Nc, negative sizes, rows beyond the key's 32-bit index -> ITR_ERR_BADARG; n_rows_local == 0 or Nc == 0 -> ITR_OK,
 * nothing written.
 * Purely additive: no existing signature changes, ITR_ABI_VERSION stays 35. */
size_t itr_topk_fold_workspace_bytes(int64_t n_rows_local, int64_t Nc, int K);
int itr_topk_fold_cols(const float *S, int64_t ldS, int64_t row0, int64_t n_rows_local, int64_t Nc, int K,
                       uint64_t *col_key, float *col_val, void *workspace, size_t workspace_bytes, itr_stream_t stream);

/* ---- query-time search: top-K of a few queries against a resident gallery (csrc/search.hip) ----
 * The reference ranks a query by scoring it against everything, cosine_sim (Objectives.py:18-21), and sorting the line,
 * inds = np.argsort(sims[index])[::-1] (evaluation.py:169 i2t, :209 t2i).  itr_search_topk does both for n_queries
 * (1 .. ITR_SEARCH_MAX_QUERIES) query vectors [n_queries, D] against gallery rows [n_gallery, D] (fp32, leading dimensions
 * ldq, ldg >= D, any alignment) in ONE pass over the gallery; the score matrix is never written.
 *   - Score: the bits of itr_cosine_scores(queries, gallery): ONE fp32 fmaf chain per pair from +0.0, acc = fmaf(q_k, g_k, acc),
 *     in the k order of the tile GEMM behind that entry (inside every block of 8: k = 0, 4, 1, 5, 2, 6, 3, 7; blocks ascending; D
 *     zero-padded to a multiple of 32).  No split over D, no other order.
 *   - Order: the ranker's key of (score, row0 + local row): larger score first, the higher index on exact ties, -0.0 == +0.0,
 *     NaN as +inf.
 *   - key [n_queries, K] (uint64) / val [n_queries, K] in exactly the layout of itr_topk's column part: best first, key =
 *     ordered score << 32 | GLOBAL row, val the score's own bits, key 0 / val 0 for an empty entry (K > n_gallery).  One call
 *     on a gallery shard is a valid part for itr_topk_merge ([n_parts][n_queries][K]) and a valid state for
 *     itr_topk_fold_cols.  idx (may be NULL): [n_queries, K] int32 global rows, -1 where empty.
 *   - The lists are the K largest keys of the query's n_gallery keys: a function of that set alone, independent of how the
 *     gallery is cut into slabs, of scheduling and of how the queries are grouped inside the launch.  n_slabs pins the number of
 *     gallery slabs that select partial lists independently before the final merge: 0 = the library's choice, else
 *     1 .. ITR_SEARCH_MAX_SLABS; every value gives the same bytes.
 *   - workspace: itr_search_topk_workspace_bytes(n_queries, n_gallery, K, n_slabs) bytes, 8-byte aligned, caller-owned.  No
 *     allocation, no host read-back, no atomics on floats.
 * Checked before any device call: null pointers, ldq / ldg < D, negative sizes, D < 1, n_slabs out of range, rows beyond the
 * key's 32-bit index -> ITR_ERR_BADARG; K outside 1 .. ITR_TOPK_MAX or n_queries > ITR_SEARCH_MAX_QUERIES ->
 * ITR_ERR_UNSUPPORTED; n_queries == 0 -> ITR_OK, nothing launched; n_gallery == 0 -> ITR_OK, all-empty lists written.
 * Purely additive: no existing signature changes, ITR_ABI_VERSION stays 35. */
#define ITR_SEARCH_MAX_QUERIES 64
#define ITR_SEARCH_MAX_SLABS 1024
size_t itr_search_topk_workspace_bytes(int64_t n_queries, int64_t n_gallery, int K, int n_slabs);
int itr_search_topk(const float *queries, int64_t ldq, int64_t n_queries, const float *gallery, int64_t ldg, int64_t row0,
                    int64_t n_gallery, int64_t D, int K, int n_slabs, uint64_t *key, float *val, int32_t *idx,
                    void *workspace, size_t workspace_bytes, itr_stream_t stream);

/* ---- hubness correction before ranking: CSLS and inverted softmax (csrc/hubness.hip) ----
 * Both corrections subtract a per-image and a per-caption vector, S'[i, j] = S[i, j] - a[i] - b[j]; a is constant along a row and
 * b along a column, so one adjusted matrix serves both directions and every consumer above works on it unchanged.  The vectors
 * are reductions over score matrices that may be query banks, scored in row blocks and never stored.  float64 throughout; S is
 * float32 (f64 = 0) or float64 (f64 = 1), leading dimension ldS >= Nc with any alignment.
 * itr_hub_lse_fold: one pass over the row block S [n_rows, Nc], every element read once and widened to double.
 *   row_lse [n_rows] (may be NULL): (1 / beta) log sum_j exp(beta S[r, j]); final, a block holds whole rows.
 *   col_state [Nc][2] (may be NULL), read AND written: per column (running sum of exp(beta x - beta m), running maximum m) over
 *     every block folded so far.  A sum of 0 means empty whatever the second slot holds: all-zero bytes are the starting state.
 *     A state whose maximum is NaN or +inf stands for that result and carries sum 1.
 *   -inf entries add nothing; only -inf gives -inf; a +inf gives +inf; a NaN gives NaN (np.logaddexp.reduce's results).
 *   Scores beyond any similarity's range, |beta S| >= 2^29 ln 2 = 3.7e8, count as +-inf.
 *   No floating-point atomics: partial sums go to the workspace and are combined in a fixed order, so the same call on the same
 *   inputs gives the same bits however the workgroups are scheduled.  Other row partitions may differ in the last bits.
 *   No host read-back and no allocation inside the call.  workspace: itr_hub_lse_workspace_bytes(n_rows, Nc) bytes, 8-byte aligned.
 * itr_hub_lse_finish: col_lse[j] = m_j + log(sum_j) / beta of a state (-inf for an empty column).
 * itr_hub_list_mean: out[r] = 0.5 * (float64 sum of the first k entries of list r, added best first one at a time) / k, for n
 *   best-first lists val [n, ld >= k] in the layout of row_val / col_val of itr_topk, itr_topk_merge and itr_topk_f64.
 * itr_hub_adjust: out[i, j] = dtype((double(S[i, j]) - a[i]) - b[j]): two float64 subtractions, each rounded on its own, nothing
 *   contracted or reassociated, then the cast to the dtype of S.  a [n_rows] or b [Nc] may be NULL (zeros).  out == S with
 *   ldo == ldS works in place; any other overlap of out with S, a or b is refused ("alias").
 * beta not finite and positive, k < 1, null pointers, ldS < Nc, negative sizes -> ITR_ERR_BADARG; k > ITR_TOPK_MAX ->
 * ITR_ERR_UNSUPPORTED; empty shapes -> ITR_OK, nothing written.  Every argument check comes before any device call.
 * Purely additive: no existing signature changes, ITR_ABI_VERSION stays 35. */
size_t itr_hub_lse_workspace_bytes(int64_t n_rows, int64_t Nc);
int itr_hub_lse_fold(const void *S, int f64, int64_t ldS, int64_t n_rows, int64_t Nc, double beta, double *row_lse,
                     double *col_state, void *workspace, size_t workspace_bytes, itr_stream_t stream);
int itr_hub_lse_finish(const double *col_state, int64_t Nc, double beta, double *col_lse, itr_stream_t stream);
int itr_hub_list_mean(const void *val, int f64, int64_t n, int64_t ld, int k, double *out, itr_stream_t stream);
int itr_hub_adjust(const void *S, int f64, int64_t ldS, int64_t n_rows, int64_t Nc, const double *a, const double *b, void *out,
                   int64_t ldo, itr_stream_t stream);

/* ---- a6 on candidate lists: xattn_score_t2i / xattn_score_i2t (Objectives.py:329-476) for LISTED (image, caption) pairs ----
 * The fine stage of coarse-to-fine retrieval: only the P listed pairs are scored (csrc/scan_pairs.hip), with the arithmetic of
 * itr_scan_xattn_scores (exact fp32 dot products, Gram-form cosine; same mode / norm / agg codes, lambda_softmax, lambda_lse).
 * The list is caption-major (CSR): the pairs of caption c are p in [cap_ptr[c], cap_ptr[c + 1]), pair p is
 * (image pair_img[p], caption c) and its score goes to out[pair_out[p]].  Duplicates are allowed.  A pair's score depends on
 * that pair alone: the same bits whatever else is listed, in whatever order.
 *   words [n_rows, D]; caption c = rows cap_off[c] .. cap_off[c] + cap_len[c] - 1, cap_len[c] in 1..64, or 0 for a caption
 *   that is not scored here (it must have no pairs).  R = 36 and D % 16 == 0, else ITR_ERR_UNSUPPORTED.
 *   An image index outside [0, Ni) is never dereferenced: that pair's score is NaN; an output slot outside [0, out_len) is skipped.
 * itr_scan_pairs_prepare fills the workspace (itr_scan_pairs_workspace_bytes) ONCE per image set and caption set: mode 0 the
 * regions' Gram matrices and the word norms, mode 1 the region norms and the captions' Gram matrices; itr_scan_pair_scores
 * may then be called for any number of lists with the same workspace, mode and operands. */
size_t itr_scan_pairs_workspace_bytes(int64_t Ni, int R, int64_t n_rows, int64_t Nc, int mode);
int itr_scan_pairs_prepare(const float *img, const float *words, const int64_t *cap_off, const int32_t *cap_len, int64_t Ni,
                           int64_t Nc, int64_t n_rows, int R, int D, int mode, void *workspace, size_t workspace_bytes,
                           itr_stream_t stream);
int itr_scan_pair_scores(const float *img, const float *words, const int64_t *cap_off, const int32_t *cap_len,
                         const int32_t *cap_ptr, const int32_t *pair_img, const int32_t *pair_out, int64_t P, int64_t Ni,
                         int64_t Nc, int64_t n_rows, int R, int D, int mode, int norm, int agg, float lambda_softmax,
                         float lambda_lse, float *out, int64_t out_len, void *workspace, size_t workspace_bytes,
                         itr_stream_t stream);
/* ---- a6, explained: the attention matrix func_attention returns next to the weighted context (Objectives.py:421-476, attnT at
 * :466 / :476; received by xattn_score_t2i :350 and xattn_score_i2t :398), the cosine similarities the score is aggregated from
 * (:354 / :400, cosine_similarity :10-15) and the score, for P LISTED (image, caption) pairs in any order (csrc/scan_attn.hip) ----
 * Pair p is (image pair_img[p], caption pair_cap[p]); operands, mode / norm / agg codes and lambdas as itr_scan_pair_scores, and
 * the workspace is the one itr_scan_pairs_prepare filled for the same mode, used unchanged (read only).
 *   attn:    the matrix after the first normalisation and Softmax(attn * lambda_softmax), always one [W_c, 36] row-major block
 *            per pair (word-major) at attn[attn_ptr[p]]; t2i: every word row sums to 1, i2t: every region column sums to 1.
 *   row_sim: t2i W_c floats at row_sim[row_ptr[p]] (one per word), i2t 36 floats at row_sim[p * 36] (one per region).
 *   score:   score[p], the aggregate of row_sim.
 *   attn_ptr / row_ptr: int64 [P + 1] device arrays supplied by the caller (prefix sums of W_c * 36 and of W_c over the list);
 *   attn_len / row_len: floats the two buffers hold.
 * cap_len[c] holds the TRUE length, 1..96 (unlike itr_scan_pair_scores).  In mode 1 the prepared workspace holds Gram matrices for
 * captions of up to 64 words only -- itr_scan_pairs_prepare must have been given length 0 for longer ones, as for the scores --
 * and this entry computes what it needs for 65..96 words itself.
 * R != 36, D % 16 != 0 or P * 96 * 36 >= 2^31: ITR_ERR_UNSUPPORTED.  A null pointer, a negative size, an unknown code or a short
 * workspace: ITR_ERR_BADARG.  What only the device can see is checked there before any dependent load or store: an image or
 * caption index out of range, a length outside 1..96, word rows outside [0, n_rows) or an output block outside its buffer give
 * score[p] = NaN and nothing else of that pair is read or written.  A pair's outputs depend on that pair alone: the same bits in
 * any list, order or blocking.  No atomics. */
int itr_scan_pair_attention(const float *img, const float *words, const int64_t *cap_off, const int32_t *cap_len,
                            const int32_t *pair_img, const int32_t *pair_cap, int64_t P, int64_t Ni, int64_t Nc, int64_t n_rows,
                            int R, int D, int mode, int norm, int agg, float lambda_softmax, float lambda_lse, float *attn,
                            const int64_t *attn_ptr, int64_t attn_len, float *row_sim, const int64_t *row_ptr, int64_t row_len,
                            float *score, void *workspace, size_t workspace_bytes, itr_stream_t stream);
/* ---- a7 on candidate lists: EncoderSimilarity.forward (Fusionmodule.py:406-451, with VisualSA :491-507, TextSA :543-559,
 * SCAN_attention :632-664, AttentionFiltration :615-619, GraphReasoning :581-587) for LISTED (image, caption) pairs ----
 * Only the listed pairs are scored (csrc/sgraf_pairs.hip); no (Ni, Nc) intermediate exists.  A pair's score depends on that pair
 * alone: the same bits in any list, order, chunk or direction.  Operands, weights, module and limits as itr_sgraf_scores
 * (R = 36, D % 32 == 0, S <= 1024, captions of 1..63 words; cap_len[c] == 0 marks a caption that is not scored here).
 *
 * itr_sgraf_pairs_prepare fills `state` (itr_sgraf_pairs_state_bytes) ONCE per image set, caption set, weights and module: the
 *   VisualSA / TextSA global vectors, the images' Gram matrices, SGR's folded and fragment-ordered weights.  `scratch`
 *   (itr_sgraf_pairs_prepare_scratch_bytes) holds its intermediates and is free again when the call has run.
 * itr_sgraf_pairs_plan turns an IMAGE-major list (CSR: the pairs of image i are p in [img_ptr[i], img_ptr[i + 1]), pair p is
 *   (image i, caption pair_cap[p])) into items of one image x whole captions (<= 16 captions, words + captions <= 64), on the
 *   device (P < 2^31 / 64 = 33 554 432 pairs per call, ITR_ERR_UNSUPPORTED above: a column index is 64 x the item index in int32):
 *   pair_len[P], pair_col[P] (first column of the pair's words, 64 columns per item), pair_capok[P] (the caption, or -1
 *   for a pair that cannot be scored: its score is NaN), item_begin[n_items + 1] (first pair; the buffer holds P + 1 entries),
 *   item_img[n_items] (buffer: P entries) and n_items_dev[0] = n_items.  workspace: itr_sgraf_pairs_plan_workspace_bytes(Ni).
 * itr_sgraf_pair_scores scores the chunk of pairs [p0, p0 + n_pairs) = items [it0, it0 + n_items) (whole items: p0 ==
 *   item_begin[it0], p0 + n_pairs == item_begin[it0 + n_items]) and writes out[pair_out[p]] (a slot outside [0, out_len) is
 *   skipped).  pair_img[P] is the image of every pair.  workspace: itr_sgraf_pair_scores_workspace_bytes(n_pairs, n_items, ...),
 *   monotone in both counts: the caller sizes chunks to the memory it has. */
size_t itr_sgraf_pairs_state_bytes(int64_t Ni, int64_t Nc, int64_t n_rows, int D, int S, int module, int sgr_step);
int itr_sgraf_pairs_prepare(const float *img, const float *words, const int64_t *cap_off, const int32_t *cap_len, int64_t Ni,
                            int64_t Nc, int64_t n_rows, int R, int D, int S, int module, int sgr_step,
                            const itr_sgraf_weights *w, void *state, size_t state_bytes, void *scratch, size_t scratch_bytes,
                            itr_stream_t stream);
size_t itr_sgraf_pairs_prepare_scratch_bytes(int64_t Ni, int64_t Nc, int64_t n_rows, int D, int S, int module);
size_t itr_sgraf_pairs_plan_workspace_bytes(int64_t Ni);
int itr_sgraf_pairs_plan(const int32_t *img_ptr, const int32_t *pair_cap, const int64_t *cap_off, const int32_t *cap_len, int64_t P,
                         int64_t Ni, int64_t Nc, int64_t n_rows, int32_t *pair_len, int32_t *pair_col, int32_t *pair_capok,
                         int32_t *item_begin, int32_t *item_img, int32_t *n_items_dev, void *workspace, size_t workspace_bytes,
                         itr_stream_t stream);
size_t itr_sgraf_pair_scores_workspace_bytes(int64_t n_pairs, int64_t n_items, int D, int S, int module, int sgr_step);
int itr_sgraf_pair_scores(const float *img, const float *words, const int64_t *cap_off, const int32_t *pair_img,
                          const int32_t *pair_capok, const int32_t *pair_len, const int32_t *pair_col, const int32_t *pair_out,
                          const int32_t *item_begin, const int32_t *item_img, int64_t p0, int64_t n_pairs, int64_t it0,
                          int64_t n_items, int64_t Ni, int64_t Nc, int64_t n_rows, int R, int D, int S, int module, int sgr_step,
                          const itr_sgraf_weights *w, const void *state, size_t state_bytes, float *out, int64_t out_len,
                          void *workspace, size_t workspace_bytes, itr_stream_t stream);
/* ---- a7 on candidate lists, explained: what the SGRAF score of a LISTED pair is made of (csrc/sgraf_attn.hip) ----
 * The word x region attention of SCAN_attention (Fusionmodule.py:632-664), AttentionFiltration's weights over the alignment nodes
 * (:615-619) or GraphReasoning's edges at every step (:581-587), and the score of EncoderSimilarity.forward (Fusionmodule.py:406-451).
 * Operands, state (itr_sgraf_pairs_prepare), plan arrays (itr_sgraf_pairs_plan) and the chunk range p0, n_pairs, it0, n_items exactly as
 * itr_sgraf_pair_scores; the attention, the local and the global node rows are computed by the same kernels on the same bits.
 * Narrower than the score entry: sim_dim % 16 == 0 and sim_dim <= 256 (ITR_ERR_UNSUPPORTED above: the item's node rows are held on chip).
 * Pair p of the chunk has W = pair_len[p] words, n = W + 1 nodes -- node 0 is the GLOBAL node, node 1 + w is word w -- and writes to
 * slot o = pair_out[p] of caller-owned buffers, laid out by caller-owned int64 prefix arrays of out_len + 1 entries:
 *   attn   [W, 36] row-major at attn[attn_ptr[o]]: the softmax weights of SCAN_attention, every word row sums to 1
 *   node_w n floats at node_w[node_ptr[o]] (module 0, SAF): l1norm(sigmoid(bn(attn_sim_w x_j))), sums to 1; unused for module 1
 *   edge   [sgr_step, n, n] at edge[edge_ptr[o]] (module 1, SGR): softmax(q k^T) of every step, every row sums to 1; unused for module 0
 *   score  score[o]
 * attn_len / node_len / edge_len: floats the buffers hold; out_len: slots.  Every block is checked against these on the device before the
 * first dependent access: a pair whose blocks do not fit, or which the plan marked as not scorable, gets score NaN and nothing else of it
 * is written; a slot outside [0, out_len) is skipped.  A pair's outputs depend on that pair alone (fixed K order, no atomics): the same
 * bits in any list, order, item or chunk.  workspace: itr_sgraf_pair_attention_workspace_bytes, monotone in both counts.
 * ITR_ABI_VERSION stays 35: these two entries are purely additive, no existing signature changed. */
size_t itr_sgraf_pair_attention_workspace_bytes(int64_t n_pairs, int64_t n_items, int D, int S, int module, int sgr_step);
int itr_sgraf_pair_attention(const float *img, const float *words, const int64_t *cap_off, const int32_t *pair_img,
                             const int32_t *pair_capok, const int32_t *pair_len, const int32_t *pair_col, const int32_t *pair_out,
                             const int32_t *item_begin, const int32_t *item_img, int64_t p0, int64_t n_pairs, int64_t it0,
                             int64_t n_items, int64_t Ni, int64_t Nc, int64_t n_rows, int R, int D, int S, int module, int sgr_step,
                             const itr_sgraf_weights *w, const void *state, size_t state_bytes, float *attn, const int64_t *attn_ptr,
                             int64_t attn_len, float *node_w, const int64_t *node_ptr, int64_t node_len, float *edge,
                             const int64_t *edge_ptr, int64_t edge_len, float *score, int64_t out_len, void *workspace,
                             size_t workspace_bytes, itr_stream_t stream);
/* Re-order n lists of K candidates by new scores (evaluation.py:169, :209: the order np.argsort(...)[::-1] gives these K
 * candidates): idx [n, K] candidates, val [n, K] their new scores -> idx_out / val_out in the ranker's order (larger score
 * first, the higher index on exact ties, -0.0 == +0.0, NaN as +inf; of two entries with the same candidate and score the one
 * that stood first stays first), scores with their original bits, perm_out [n, K] = old position of each entry.
 * 1 <= K <= ITR_TOPK_MAX; outputs must not alias inputs. */
int itr_rerank_lists(const int32_t *idx, const float *val, int64_t n, int K, int32_t *idx_out, float *val_out,
                     int32_t *perm_out, itr_stream_t stream);
/* Ensemble reranking: fuse the scores of M fine models on the same n lists of K candidates and re-order the lists by the fused
 * score.  idx [n, K] candidates in coarse order, val [M, n, K] the members' scores (member-major).  The fused score of an entry
 * is  ((double)val[0] + (double)val[1] + ... + (double)val[M-1]) / (double)M , added in member order -- the reference's ensemble
 * (sims + sims2) / 2 on float64 matrices (evaluation.py:377-381) restricted to the listed pairs -- and the order is the one
 * np.argsort(...)[::-1] (evaluation.py:169, :209) gives these K candidates under it, by the float64 rule: larger fused score
 * first, the higher index on exact ties, -0.0 == +0.0, NaN as +inf; of two entries with the same candidate and fused score the
 * one that stood first stays first.  idx_out [n, K], fused_out [n, K] (the computed doubles unchanged: a NaN stays NaN), val_out
 * [M, n, K] or NULL (member scores in the new order, original bits), perm_out [n, K] = old position of each entry.  With M = 1
 * idx_out and perm_out are itr_rerank_lists'; with M = 2 swapping the members changes no bit of idx_out, fused_out, perm_out.
 * 1 <= K <= ITR_TOPK_MAX, 1 <= M <= ITR_RERANK_MAX_MEMBERS (ITR_ERR_UNSUPPORTED above); outputs must not alias inputs.
 * Purely additive: no existing signature changes, ITR_ABI_VERSION stays 35. */
#define ITR_RERANK_MAX_MEMBERS 4
int itr_rerank_fuse_lists(const int32_t *idx, const float *val, int M, int64_t n, int K, int32_t *idx_out, double *fused_out,
                          float *val_out, int32_t *perm_out, itr_stream_t stream);

/* ---- a14: the training step  model.train_emb (itr/modalmodule/Models.py:198-225, :115-145): forward -> loss ->
 * backward -> clip_grad_norm_(2.0) -> Adam.  Backward contractions are itr_gemm_nt on transposed operands;
 * these are the pieces around them. ------------------------------------------------------------------------- */
/* z = x / (||x|| + eps) keeping the row norms (utils.py:10-15), and its backward
 *   dx = dz / (n + eps) - z (z . dz) / n. */
int itr_l2norm_fwd_save(const float *x, float *z, float *norms, int64_t rows, int dim, float eps, itr_stream_t stream);
int itr_l2norm_bwd(const float *dz, const float *z, const float *norms, float *dx, int64_t rows, int dim, float eps,
                   itr_stream_t stream);
/* out[c, r] = in[r, c] (row-major [rows, cols] -> [cols, rows]). */
int itr_transpose2d(const float *in, float *out, int64_t rows, int64_t cols, itr_stream_t stream);
/* out[c] (+)= sum_r x[r, c], fixed summation order (bias gradients). */
size_t itr_colsum_workspace_bytes(int64_t rows, int64_t cols);
int itr_colsum(const float *x, float *out, int64_t rows, int64_t cols, int accumulate, void *workspace,
               size_t workspace_bytes, itr_stream_t stream);
/* C = act(A B^T + bias) with the K range cut into slices when the output has too few 128 x 128 tiles to fill the chip (M N small, K long:
 * CAMERA's dilated convolutions as GEMMs); slices added in a fixed order.  TRAINING TAPE ONLY: a row's bits depend on the slice count,
 * hence on the shape of the call -- the evaluation keeps itr_gemm_nt.  Falls back to itr_gemm_nt when no split is chosen.  The slice
 * count aims at two resident workgroups per CU (512 / tiles, at most 8, slices of >= 128 k).  M <= 128 rows (ABI 30: a decoder step's
 * layers) take the 16-column-strip kernel over K slices and one pass that adds the slices, the bias and the activation; the workspace
 * for that is 16 M N floats. */
size_t itr_gemm_nt_splitk_workspace_bytes(int64_t M, int64_t N, int64_t K);
int itr_gemm_nt_splitk(const float *A, int64_t lda, const float *B, int64_t ldb, const float *bias, float *C, int64_t ldc, int64_t M,
                       int64_t N, int64_t K, int act, void *workspace, size_t workspace_bytes, itr_stream_t stream);
/* Weight gradient of a dense layer, dW = dY^T X:  C[P, Q] (+)= A[R, P]^T B[R, Q] (row-major, the REDUCED index is the row of
 * both operands: no transposed copies).  The rows are split into slices whose partial products (workspace) are added in slice
 * order: deterministic.  accumulate != 0 adds to C.  colsum_a (may be NULL) receives sum_r A[r, :] -- the bias gradient, from the
 * operand tiles the product loads anyway.  Exact fp32 MFMA (csrc/gemm_tn.hip). */
size_t itr_gemm_tn_workspace_bytes(int64_t R, int64_t P, int64_t Q);
int itr_gemm_tn(const float *A, int64_t lda, const float *B, int64_t ldb, float *C, int64_t ldc, int64_t R, int64_t P, int64_t Q,
                int accumulate, float *colsum_a, void *workspace, size_t workspace_bytes, itr_stream_t stream);
/* `batch` problems of one shape in one launch (operand z at A + z batch_a ...), each C_z = A_z^T B_z reduced in one pass. */
int itr_gemm_tn_batched(const float *A, int64_t lda, int64_t batch_a, const float *B, int64_t ldb, int64_t batch_b, float *C, int64_t ldc,
                        int64_t batch_c, int64_t R, int64_t P, int64_t Q, int64_t batch, itr_stream_t stream);

/* ---- a7 / a14: SGRAF.train_emb's similarity module on ALL pairs of the batch at once (EncoderSimilarity.forward in training mode and its
 * backward: itr/modalmodule/Fusionmodule.py:406-451, SCAN_attention :632-664, GraphReasoning :579-586, AttentionFiltration :613-618,
 * TextSA :549-564; caller Models.py:518-546).  Ragged IMAGE-MAJOR matrices over B images and C captions with T words in total
 * (cap_off[C + 1] = int32 word offsets, device):
 *   local rows b T + t;   node rows b (T + C) + cap_off[c] + c + j (j = 0 the global alignment, 1 .. W_c the words);   pair rows b C + c.
 * The dense layers between these stages are itr_gemm_nt / itr_gemm_tn; csrc/sgraf_train.hip holds the stages themselves:
 *   attn    P[(b,t), r] = softmax_r(smooth * l2norm_w(LeakyReLU_0.1(A[(b,r), t])))      A [B R, ldA] = regions . words^T
 *   ctx     X[(b,t), :] = (l2norm(sum_r P r img[b,r,:]) - words[t,:])^2,  cnorm = the context norms;  backward: d ctx [B T, D], d words
 *           (summed over the images; workspace = itr_sgt_ctx_bwd_workspace_bytes), then d P = itr_sgt_dp and d regions = itr_gemm_tn_batched
 *   pair_sqdiff  X[(b,c), :] = (img_glo[b] - cap_glo[c])^2
 *   nodes   scatter of the global / local alignment rows into the node matrix (backward != 0: the inverse copy)
 *   graph   E = softmax_r(q_v . k_r), Z_v = sum_r E[v,r] x_r per pair; E saved at b e_off[C] + e_off[c] (e_off = prefix sums of n_c^2)
 *   segbn   BatchNorm1d(1) with the batch statistics of ONE caption's B (W_c + 1) attention logits (the reference calls it per caption)
 *   saf_pool  sigmoid -> l1norm over the nodes of a pair -> weighted node sum
 *   seg_mean / seg_smry  caption mean; softmax(logit over the words of a caption) . words      (TextSA on packed captions)
 * Limits (ITR_ERR_UNSUPPORTED beyond; the caller then takes the grouped path): D % 4 == 0, D <= 2048, R <= 64, S % 4 == 0, LDS per pair. */
int itr_sgt_attn_fwd(const float *A, int64_t ldA, const int32_t *cap_off, int B, int C, int T, int R, int Wmax, float smooth, float eps,
                     float *P, itr_stream_t stream);
int itr_sgt_attn_bwd(const float *A, int64_t ldA, const float *P, const float *dP, const int32_t *cap_off, int B, int C, int T, int R,
                     int Wmax, float smooth, float eps, float *dA, itr_stream_t stream);
int itr_sgt_ctx_fwd(const float *P, const float *img, const float *words, int B, int T, int R, int D, float eps, float *X, float *cnorm,
                    itr_stream_t stream);
size_t itr_sgt_ctx_bwd_workspace_bytes(int B, int T, int D);
int itr_sgt_ctx_bwd(const float *P, const float *img, const float *words, const float *cnorm, const float *dX, int B, int T, int R, int D,
                    float eps, float *dctx, float *dwords, void *workspace, size_t workspace_bytes, itr_stream_t stream);
int itr_sgt_dp(const float *dctx, const float *img, int B, int T, int R, int D, float *dP, itr_stream_t stream);
int itr_sgt_pair_sqdiff_fwd(const float *img_glo, const float *cap_glo, int B, int C, int D, float *X, itr_stream_t stream);
int itr_sgt_pair_sqdiff_bwd(const float *img_glo, const float *cap_glo, const float *dX, int B, int C, int D, float *dimg_glo,
                            float *dcap_glo, itr_stream_t stream);
int itr_sgt_nodes(float *glo, float *loc, float *nodes, const int32_t *cap_off, const int32_t *node_cap, int B, int C, int T, int S,
                  int backward, itr_stream_t stream);
/* row0_only != 0: only node 0 of every pair is a query (the last reasoning step, whose output the reference reads at [:, 0, :]):
 * q / Z / dq are pair rows [B C, S], E one row of n weights per pair at its node offset [B (T + C)]. */
int itr_sgt_graph_fwd(const float *q, const float *k, const float *x, const int32_t *cap_off, const int32_t *e_off, int B, int C, int T, int S,
                      int nmax, int row0_only, float *E, float *Z, itr_stream_t stream);
int itr_sgt_graph_bwd(const float *q, const float *k, const float *x, const float *E, const float *dZ, const int32_t *cap_off,
                      const int32_t *e_off, int B, int C, int T, int S, int nmax, int row0_only, float *dq, float *dk, float *dx,
                      itr_stream_t stream);
int itr_sgt_segbn_fwd(const float *a, const int32_t *cap_off, int B, int C, int T, const float *gamma, const float *beta, float eps, float *y,
                      float *mean, float *var, float *invstd, itr_stream_t stream);
int itr_sgt_segbn_bwd(const float *dy, const float *a, const int32_t *cap_off, int B, int C, int T, const float *gamma, const float *mean,
                      const float *invstd, float *da, float *dgamma_c, float *dbeta_c, itr_stream_t stream);
int itr_sgt_saf_pool_fwd(const float *y, const float *nodes, const int32_t *cap_off, int B, int C, int T, int S, int nmax, float eps, float *out,
                         itr_stream_t stream);
int itr_sgt_saf_pool_bwd(const float *y, const float *nodes, const float *dout, const int32_t *cap_off, int B, int C, int T, int S, int nmax,
                         float eps, float *dy, float *dnodes, itr_stream_t stream);
/* spread == 0: out[c] = sum (mean != 0: mean) of the caption's rows of in [T, D]; spread != 0: out[t] = in[caption of t] (/ W_c if mean) */
int itr_sgt_seg_mean(const float *in, const int32_t *cap_off, int C, int D, float *out, int spread, int mean, itr_stream_t stream);
int itr_sgt_seg_smry_fwd(const float *logit, const float *words, const int32_t *cap_off, int C, int D, int Wmax, float *p, float *out,
                         itr_stream_t stream);
int itr_sgt_seg_smry_bwd(const float *p, const float *words, const float *dout, const int32_t *cap_off, int C, int D, int Wmax, float *dlogit,
                         float *dwords, itr_stream_t stream);
/* nn.Embedding backward: dE[tokens[r], :] += dx[r, :]; the rows of one token are added in row order (no atomics: the same bits every run). */
int itr_embed_scatter_add(const int64_t *tokens, const float *dx, int64_t n_tok, int64_t V, int E, float *dE,
                          itr_stream_t stream);
/* out[r, :] = table[idx[r], :]  (nn.Embedding forward; the last-valid-step gather of TextEncoder.py:57-60).  Indices
 * outside [0, V) read row 0 and set *bad_flag (device int) to 1. */
int itr_gather_rows(const int64_t *idx, int64_t n, const float *table, int64_t V, int E, float *out, int *bad_flag,
                    itr_stream_t stream);
/* One training batch assembled in ONE launch from tables that stay in device memory: the arithmetic of PrecompDataset.__getitem__
 * (itr/datamodule/data_loader.py:104-131) and collate_fn (itr/datamodule/data_loader.py:134-178) for B samples whose indices are
 * already in collate order (sorted by caption length, descending, stable).  A pure copy; nothing is allocated.
 *   images_out[b, :] = feat[img_idx[b], :]          row_elems = R * img_dim floats per row, feat [n_img, row_elems]
 *   boxes_out[b, :]  = boxes[img_idx[b], :]         box_elems = R * 4 floats    (boxes / boxes_out both NULL: skipped)
 *   wh_out[b, :]     = img_wh[img_idx[b], :]        2 floats                    (img_wh / wh_out both NULL: skipped)
 *   ragged ids (GRU families; packed / off / ids_out all NULL: skipped): caption c = cap_idx[b] owns the int64 ids
 *       packed[off[c] .. off[c + 1]) of packed[n_packed], off[n_cap + 1]; ids_out[b, :] (Lmax int64) = those ids, then zeros
 *       (the `targets` loop of collate_fn); ids beyond Lmax are dropped
 *   fixed-width ids (BERT families, VSRN): out_k[b, :] = tab_k[cap_idx[b], :] for up to three int64 tables [n_cap, W] (ids, mask,
 *       type ids) and fout[b, :] = ftab[cap_idx[b], :] for one float table [n_cap, W] (VSRN's mask); each pair may be NULL
 * A row is moved with 16-byte loads and stores when its byte length is a multiple of 16 and both bases are 16-byte aligned,
 * otherwise element by element (a slower path, not an error).  cap_idx may be NULL when no caption table is given.
 * An index outside [0, n_img) / [0, n_cap) reads row 0 and sets *bad_flag (device int) to 1, as itr_gather_rows does; so does a
 * ragged row whose offsets leave packed[] (it is written as zeros).
 * Checked on the host before any launch: null pointers (a table without its output or the reverse included) and negative sizes
 * -> ITR_ERR_BADARG; B, Lmax or a row width that needs more workgroups than one grid holds -> ITR_ERR_UNSUPPORTED; B == 0 ->
 * ITR_OK, nothing launched.
 * Purely additive: no existing signature changes, ITR_ABI_VERSION stays 35. */
int itr_collate_batch(const int64_t *img_idx, const int64_t *cap_idx, int64_t B, const float *feat, int64_t n_img, int64_t row_elems,
                      float *images_out, const float *boxes, int64_t box_elems, float *boxes_out, const float *img_wh, float *wh_out,
                      const int64_t *packed, int64_t n_packed, const int64_t *off, int64_t n_cap, int64_t Lmax, int64_t *ids_out,
                      const int64_t *tab0, const int64_t *tab1, const int64_t *tab2, const float *ftab, int64_t W, int64_t *out0,
                      int64_t *out1, int64_t *out2, float *fout, int *bad_flag, itr_stream_t stream);
/* clip_grad_norm_ (Models.py:223-224): itr_sq_sum writes itr_sq_sum_blocks(n) partial sums of squares of one gradient
 * tensor; itr_clip_coef turns all partials of all tensors into coef_and_norm[0] = min(1, max_norm / (||g|| + 1e-6)),
 * coef_and_norm[1] = ||g|| (device floats). */
int itr_sq_sum_blocks(int64_t n);
int itr_sq_sum(const float *g, int64_t n, float *partials, itr_stream_t stream);
int itr_clip_coef(const float *partials, int64_t nparts, float max_norm, float *coef_and_norm, itr_stream_t stream);
/* torch.optim.Adam step on one tensor (no weight decay / amsgrad); the gradient is multiplied by *grad_scale_dev
 * (device float, may be NULL) first; `step` is the 1-based update count.  A float beta stands for the decimal of at most six digits that
 * rounds to it (0.9f for 0.9, 0.999f for 0.999): 1 - beta and the bias corrections 1 - beta^step are formed in double from that decimal,
 * as torch forms them from the double it holds; a beta that six digits do not reproduce stands for itself.  (1.f - 0.999f is a relative
 * 1.3e-5 away from 1 - 0.999.)  The same holds for itr_adam_step_multi. */
int itr_adam_step(float *p, const float *g, float *m, float *v, int64_t n, float lr, float beta1, float beta2, float eps,
                  int64_t step, const float *grad_scale_dev, itr_stream_t stream);

/* The same two for ALL parameter tensors of a step in one launch each (a step has up to 67 tensors).  table_dev: one 48-byte record per
 * tensor {float *p; const float *g; float *m, *v; int64 n; int32 first_blk, nblk} (device copy of a host table; [first_blk, first_blk +
 * nblk) = the tensor's itr_sq_sum_blocks(n) workgroups of itr_sq_sum_multi, partials in the same layout as per-tensor itr_sq_sum calls:
 * the norm is bit-identical); blk_tensor[b] = tensor of workgroup b.  itr_adam_step_multi has its own maps: one workgroup per 256
 * elements, blk_first[t] = first workgroup of tensor t. */
int itr_sq_sum_multi(const void *table_dev, const int32_t *blk_tensor_dev, int64_t n_blocks, float *partials, itr_stream_t stream);
int itr_adam_step_multi(const void *table_dev, const int32_t *blk_tensor_dev, const int32_t *blk_first_dev, int64_t n_blocks, float lr,
                        float beta1, float beta2, float eps, int64_t step, const float *grad_scale_dev, itr_stream_t stream);

/* ---- transformer towers under autograd (SAEM: TransformerMapping / BertMapping, ImgEncoder.py:324-350, TextEncoder.py:75-152,
 * bert.py:113-300); the dense layers are itr_gemm_nt on transposed operands as for every other backward pass ----------------
 * nn.Dropout: y = x * keep / (1 - p), keep(i) from a counter-based hash of (seed, offset + i).  Stateless: the backward pass
 * is the same call on dy.  (The random stream is not torch's; only the distribution is the reference's.) */
int itr_dropout(const float *x, float *y, int64_t n, float p, uint64_t seed, uint64_t offset, itr_stream_t stream);
/* BERTLayerNorm(x + residual) (bert.py:113-126; residual may be NULL) keeping z = x + residual, the row means and
 * 1 / sqrt(var + eps); backward: dz (for x and for the residual) and t = dy * xhat (dgamma = column sums of t, dbeta of dy). */
int itr_add_ln_fwd(const float *x, const float *residual, const float *gamma, const float *beta, float *z, float *out,
                   float *mean, float *rstd, int64_t rows, int H, float eps, itr_stream_t stream);
int itr_ln_bwd(const float *dy, const float *z, const float *mean, const float *rstd, const float *gamma, float *dz, float *t,
               int64_t rows, int H, itr_stream_t stream);
/* gelu (bert.py:104-110): dy == NULL -> out = gelu(x);  else out = dy * gelu'(x). */
int itr_gelu(const float *x, const float *dy, float *out, int64_t n, itr_stream_t stream);
/* BERTSelfAttention (bert.py:175-215) for short sequences (L <= 64, head size <= 64): per (sequence, head)
 *   P = softmax(Q K^T * scale + (1 - mask01) * -10000);  ctx = dropout(P) V.
 * q / k / v: row b * L + i, column head * dk + d, row stride ld (the three thirds of one fused QKV GEMM output).
 * P [B, heads, L, L] keeps the probabilities for the backward pass, which returns dq / dk / dv with row stride ldg. */
int itr_mha_train_fwd(const float *q, const float *k, const float *v, int64_t ld, const float *mask01, int64_t B, int L,
                      int heads, int dk, float scale, float p_drop, uint64_t seed, float *P, float *ctx, int64_t ldc,
                      itr_stream_t stream);
int itr_mha_train_bwd(const float *q, const float *k, const float *v, int64_t ld, const float *mask01, int64_t B, int L,
                      int heads, int dk, float scale, float p_drop, uint64_t seed, const float *P, const float *dctx,
                      int64_t ldc, float *dq, float *dk_out, float *dv, int64_t ldg, itr_stream_t stream);
/* F.relu + F.max_pool1d over all positions (TextEncoder.py:122-124): x [B, npos, C] -> out [B, C], arg [B, C] (first position of
 * the maximum, -1 when it is 0); backward scatters dy to the arg-max position. */
int itr_relu_maxpool_arg(const float *x, int64_t B, int npos, int C, float *out, int32_t *arg, itr_stream_t stream);
int itr_relu_maxpool_bwd(const float *dy, const int32_t *arg, int64_t B, int npos, int C, float *dx, itr_stream_t stream);
/* backward of torch.mean(x, 1): dx[b, r, :] = scale * dy[b, :]. */
int itr_bcast_mid(const float *dy, float *dx, int64_t B, int R, int F, float scale, itr_stream_t stream);

/* ---- a18: training-only auxiliary losses (csrc/aux_loss.hip) ---------------------------------------------------------------
 * AngularLoss.angular_loss (Objectives.py:262-290) on its three n x n products M1 = anchors others^T, M2 = positives others^T,
 * Q = anchors positives^T (row-major, ld = n):  x[i][j] = 4 ab (M1 + M2)[i][j] - 2 (1 + ab) Q[i][i] over the j != i;
 *   max_violation:  loss = sum_i log(1 + exp(max_j x[i][j]))                 (stat = max, arg = its first column)
 *   otherwise:      loss = mean_i log(1 + sum_j exp(x[i][j])), evaluated as t + log(exp(-t) + sum exp(x - t))   (stat = t, den)
 * row / stat / den / arg are [n] scratch the backward reads; loss and grad_loss are device scalars.  The backward writes the
 * gradient of M1 (== that of M2) to dM and that of Q (its diagonal) to dQ, both dense [n, n]. */
int itr_angular_fwd(const float *M1, const float *M2, const float *Q, int n, float angle_bound, int max_violation, float *loss,
                    float *row, float *stat, float *den, int32_t *arg, itr_stream_t stream);
int itr_angular_bwd(const float *M1, const float *M2, const float *Q, int n, float angle_bound, int max_violation, const float *stat,
                    const float *den, const int32_t *arg, const float *grad_loss, float *dM, float *dQ, itr_stream_t stream);
/* DiversityRegularization (Objectives.py:521-542): smry [B, R, K] -> sum_b || Sn_b^T Sn_b - I ||_F^2 with Sn = F.normalize(S, dim=1)
 * (columns over the R regions, eps 1e-12).  part: [B] scratch; loss / grad_loss device scalars; R*K + K*K + K <= 15360. */
int itr_diversity_fwd(const float *smry, int64_t B, int R, int K, float *part, float *loss, itr_stream_t stream);
int itr_diversity_bwd(const float *smry, int64_t B, int R, int K, const float *grad_loss, float *d_smry, itr_stream_t stream);

/* ---- CAMERA towers under autograd (camera_.py:14-114, ImgEncoder.py:355-389, TextEncoder.py:162-192, Fusionmodule.py:674-692):
 * the pieces between the dense layers ---------------------------------------------------------------------------------------
 * out = a * b (backward: two more calls). */
int itr_ew_mul(const float *a, const float *b, float *out, int64_t n, itr_stream_t stream);
/* dx = dy * act'(.) from the OUTPUT y of the activation: act 1 relu, 2 tanh, 3 sigmoid, 4 LeakyReLU(0.1). */
int itr_act_bwd(const float *y, const float *dy, float *dx, int64_t n, int act, itr_stream_t stream);
/* GatedQueryAttLayer gate (camera_.py:41-44): q' = q * M[:, :dk], k' = k * M[:, dk:] on [rows, dk] operands, M [rows, 2 dk]. */
int itr_gate_apply(const float *q, const float *k, const float *M, float *qo, float *ko, int64_t rows, int dk, itr_stream_t stream);
int itr_gate_apply_bwd(const float *q, const float *k, const float *M, const float *dqo, const float *dko, float *dq, float *dk_out,
                       float *dM, int64_t rows, int dk, itr_stream_t stream);
/* nn.BatchNorm1d in training mode on x [N, C]: batch mean / biased variance per column; keeps mean and 1 / sqrt(var + eps).
 * scratch: itr_bn_train_scratch_bytes(N, C) bytes (partial sums of the row slices; fixed summation order). */
size_t itr_bn_train_scratch_bytes(int64_t N, int C);
int itr_bn_train_fwd(const float *x, const float *gamma, const float *beta, float *y, float *mean, float *invstd, int64_t N, int C,
                     float eps, void *scratch, itr_stream_t stream);
int itr_bn_train_bwd(const float *dy, const float *x, const float *mean, const float *invstd, const float *gamma, float *dx,
                     float *dgamma, float *dbeta, int64_t N, int C, void *scratch, itr_stream_t stream);
/* utils.l2norm with its default dim=1 on [B, R, D] (normalises ACROSS the R regions, ImgEncoder.py:378,384). */
int itr_l2norm_mid_fwd(const float *x, float *z, float *norms, int64_t B, int R, int D, float eps, itr_stream_t stream);
int itr_l2norm_mid_bwd(const float *dz, const float *z, const float *norms, float *dx, int64_t B, int R, int D, float eps,
                       itr_stream_t stream);
/* Multi-view summarisation (ImgEncoder.py:386-387): L = softmax(smry [B, R, K], dim=1); out [B, K, D] = L^T x.  scratch: B*R*K floats.
 * R, K <= 96.  The same contraction is SGRAF's SCAN_attention weighting (K = words, Fusionmodule.py:649-661) and the edge
 * aggregation of its graph reasoning (R = K = nodes, :581-584). */
int itr_smry_fwd(const float *smry, const float *x, float *L, float *out, int64_t B, int R, int K, int D, itr_stream_t stream);
int itr_smry_bwd(const float *x, const float *L, const float *dout, float *dx, float *dsmry, float *scratch, int64_t B, int R, int K,
                 int D, itr_stream_t stream);
/* C[b] (M x N) = op(A[b]) op(B[b]) for small dense row-major operands, op = identity / transpose (torch.bmm in GraphReasoning,
 * Fusionmodule.py:582-584, and its backward). */
int itr_bmm_small(const float *A, const float *B, float *C, int64_t batch, int M, int N, int K, int trans_a, int trans_b,
                  itr_stream_t stream);
/* MultiViewMatching (Fusionmodule.py:674-692) on top of the [Ni * k, Nc] view scores: S[i, c] = max_v T[i * k + v, c]. */
int itr_groupmax_fwd(const float *T, int64_t Ni, int k, int64_t Nc, float *S, int32_t *arg, itr_stream_t stream);
int itr_groupmax_bwd(const float *dS, const int32_t *arg, int64_t Ni, int k, int64_t Nc, float *dT, itr_stream_t stream);

/* ---- VSRN captioning branch under autograd (Fusionmodule.py:10-367, Objectives.py:138-158): single decoder steps ---------------
 * One nn.GRU step from gi = W_ih x + b_ih and gh = W_hh h + b_hh ([B, 3H], gate order r, z, n); gates [B, 3H] keeps r, z, n. */
int itr_gru_cell_fwd(const float *gi, const float *gh, const float *h, float *h_next, float *gates, int64_t B, int H,
                     itr_stream_t stream);
int itr_gru_cell_bwd(const float *dh_next, const float *gates, const float *gh, const float *h, float *dgi, float *dgh, float *dh,
                     int64_t B, int H, itr_stream_t stream);
/* y[b, n, :] = act(x[b, n, :] + v[b, :]) and its backward from the output (dx = dy act'(y), dv[b] = sum_n dx[b, n]); act 0 none, 1 relu,
 * 2 tanh, 3 sigmoid.  The decoder attention's linear1(cat(enc_out, h)) (Fusionmodule.py:136-140) = enc_out W_e^T + b (once per batch)
 * + h W_h^T (per step), added here. */
int itr_add_bcast_mid_act(const float *x, const float *v, float *y, int64_t B, int N, int H, int act, itr_stream_t stream);
int itr_add_bcast_mid_act_bwd(const float *y, const float *dy, float *dx, float *dv, int64_t B, int N, int H, int act, itr_stream_t stream);
/* The decoder attention's scores in one pass (ABI 30; Attention.forward, Fusionmodule.py:136-141: linear2(tanh(linear1(cat(enc, hidden))))):
 *   e[b, n] = sum_h w[h] tanh(x[b, n, h] + v[b, h])     x [B, N, H] = the encoder half of linear1 (+ bias), v [B, H] = the hidden half, w [H].
 * Backward from de [B, N], the tanh recomputed: dx[b, n, h] = de w[h] (1 - p^2), dv[b, h] = sum_n dx, dw_part[b, h] = sum_n de[b, n] p
 * (the caller sums dw_part [B, H] over b: itr_colsum).  B <= 65535 in the backward; rows of H % 4 == 0 floats must be 16-byte aligned. */
int itr_addattn_score(const float *x, const float *v, const float *w, float *e, int64_t B, int N, int H, itr_stream_t stream);
int itr_addattn_score_bwd(const float *x, const float *v, const float *w, const float *de, float *dx, float *dv, float *dw_part, int64_t B, int N,
                          int H, itr_stream_t stream);
/* loss[b] = -mask[b] * log_softmax(logits[b, :])[target[b]]  (F.log_softmax + NLLLoss(reduce=False) * mask); lse keeps the row
 * log-sum-exp for the backward pass dlogits = dloss[b] mask[b] (softmax - onehot). */
int itr_nll_logsoftmax_fwd(const float *logits, const int64_t *target, const float *mask, float *loss, float *lse, int64_t B, int V,
                           itr_stream_t stream);
int itr_nll_logsoftmax_bwd(const float *logits, const int64_t *target, const float *mask, const float *lse, const float *dloss,
                           float *dlogits, int64_t B, int V, itr_stream_t stream);

/* EncoderText (bi)GRU under autograd (TextEncoder.py:38-70): training forward that keeps the gate activations, and
 * backpropagation through time.  Same packed layout / sorting contract as itr_gru_fwd.  `out` [n_tok, D] is the RAW
 * sequence output ((fwd + bwd) / 2 for a bi-GRU); l2norm / last-step gather are separate differentiable steps.
 * Gradients: d_embed [V, E] is ACCUMULATED into (zero it first); d_w_* / d_b_* are overwritten.  Token ids: validated by the caller,
 * as for itr_gru_fwd.  The two directions of a bi-GRU run side by side (the reverse one on a per-device side stream, joined before
 * the call returns to the caller's stream order). */
size_t itr_gru_train_save_bytes(int64_t n_tok, int D, int bidirectional);
size_t itr_gru_train_workspace_bytes(int64_t n_tok, int64_t B, int E, int D);
int itr_gru_fwd_train(const int64_t *tokens, const int64_t *tok_off, const int32_t *len_dev, const int32_t *len_host,
                      int64_t B, int64_t n_tok, const float *embed, int64_t V, int E, int D, const float *w_ih,
                      const float *w_hh, const float *b_ih, const float *b_hh, const float *w_ih_rev,
                      const float *w_hh_rev, const float *b_ih_rev, const float *b_hh_rev, float *out, void *save,
                      size_t save_bytes, void *workspace, size_t workspace_bytes, itr_stream_t stream);
int itr_gru_bwd(const int64_t *tokens, const int64_t *tok_off, const int32_t *len_dev, const int32_t *len_host, int64_t B,
                int64_t n_tok, const float *embed, int64_t V, int E, int D, const float *w_ih, const float *w_hh,
                const float *w_ih_rev, const float *w_hh_rev, const void *save, const float *d_out, float *d_embed,
                float *d_w_ih, float *d_w_hh, float *d_b_ih, float *d_b_hh, float *d_w_ih_rev, float *d_w_hh_rev,
                float *d_b_ih_rev, float *d_b_hh_rev, void *workspace, size_t workspace_bytes, itr_stream_t stream);

/* SCAN t2i similarity of a TRAINING batch (xattn_score_t2i, Objectives.py:329-372, under autograd).
 *   A [Bi*R, ldA] = V E^T  raw dot products (itr_gemm_nt), G [Bi, R, R] = V_i V_i^T and enorm[n_tok] = ||e_w||
 *   (itr_scan_train_prepare);  captions packed: cap_off[Bc], cap_len[Bc] (any order), at most 96 words.
 *   R regions per image: 36 in every reference configuration (compile-time loop bounds); any other 1 <= R <= 100 runs the
 *   same kernels with run-time bounds (the evaluation entry point's path for images that are not 36 regions).  The backward
 *   holds one more R x W block in LDS: R > 36 together with max_len > 64 returns ITR_ERR_UNSUPPORTED.
 *   norm in {0 clipped_l2norm, 1 l2norm, 2 softmax, 3 no_norm, 4 clipped, 5 l1norm, 6 clipped_l1norm};
 *   agg in {0 LogSumExp, 1 Max, 2 Sum, 3 Mean}.
 * itr_scan_train_bwd (dS [Bi, Bc]) writes dA [Bi*R, ldA], per-pair Gram gradients dG_pairs [Bi, Bc, R, R] and
 * d_enorm_pairs [Bi, ldA]; the caller finishes with GEMMs  dV = dA E,  dE = dA^T V  and itr_scan_train_finish, which
 * ADDS (sum_c dG + its transpose) V_i to dV and  colsum_i(d_enorm_pairs) e / ||e||  (d_enorm [n_tok]) to dE; it sums the per-pair
 * Gram gradients IN PLACE (into the slot of caption 0 of every image: dG_pairs is scratch of the backward pass, not an output). */
int itr_scan_train_prepare(const float *V, const float *E, int64_t Bi, int64_t n_tok, int R, int D, float *G,
                           float *enorm, itr_stream_t stream);
int itr_scan_train_fwd(const float *A, int64_t ldA, const float *G, const float *enorm, const int64_t *cap_off,
                       const int32_t *cap_len, int64_t Bi, int64_t Bc, int64_t n_tok, int R, int D, int max_len, int norm,
                       int agg, float lambda_softmax, float lambda_lse, float *S, itr_stream_t stream);
int itr_scan_train_bwd(const float *A, int64_t ldA, const float *G, const float *enorm, const int64_t *cap_off,
                       const int32_t *cap_len, int64_t Bi, int64_t Bc, int64_t n_tok, int R, int D, int max_len, int norm,
                       int agg, float lambda_softmax, float lambda_lse, const float *dS, float *dA, float *dG_pairs,
                       float *d_enorm_pairs, itr_stream_t stream);
int itr_scan_train_finish(float *dG_pairs, int64_t Bi, int64_t Bc, const float *V, const float *E,
                          const float *enorm, const float *d_enorm, int64_t n_tok, int R, int D, float *dV, float *dE,
                          itr_stream_t stream);

/* SCAN i2t similarity of a TRAINING batch (xattn_score_i2t, Objectives.py:376-417, under autograd): regions attend over
 * the words of a caption.  A as above; H = packed caption Gram matrices (caption c: W_c x W_c floats at H + h_off[c],
 * h_total = sum W_c^2) and vnorm[Bi*R] = ||v_r|| (itr_scan_train_i2t_prepare; R as above, 1..100).  itr_scan_train_i2t_bwd writes dA,
 * per-pair dH partials dH_pairs [Bi, h_total] and d||v|| partials d_vnorm_pairs [Bc, Bi*R]; the caller sums them over
 * images / captions (itr_colsum), runs  dV = dA E,  dE = dA^T V  and itr_scan_train_i2t_finish, which ADDS
 * (dH_c + dH_c^T) E_c to dE and  d||v|| v / ||v||  to dV. */
int itr_scan_train_i2t_prepare(const float *V, const float *E, const int64_t *cap_off, const int32_t *cap_len,
                               const int64_t *h_off, int64_t Bi, int64_t Bc, int R, int D, float *H, float *vnorm,
                               itr_stream_t stream);
int itr_scan_train_i2t_fwd(const float *A, int64_t ldA, const float *H, const int64_t *h_off, const float *vnorm,
                           const int64_t *cap_off, const int32_t *cap_len, int64_t Bi, int64_t Bc, int64_t n_tok, int R,
                           int D, int max_len, int norm, int agg, float lambda_softmax, float lambda_lse, float *S,
                           itr_stream_t stream);
int itr_scan_train_i2t_bwd(const float *A, int64_t ldA, const float *H, const int64_t *h_off, int64_t h_total,
                           const float *vnorm, const int64_t *cap_off, const int32_t *cap_len, int64_t Bi, int64_t Bc,
                           int64_t n_tok, int R, int D, int max_len, int norm, int agg, float lambda_softmax,
                           float lambda_lse, const float *dS, float *dA, float *dH_pairs, float *d_vnorm_pairs,
                           itr_stream_t stream);
int itr_scan_train_i2t_finish(const float *dH, const int64_t *h_off, const int64_t *cap_off, const int32_t *cap_len,
                              int64_t Bc, const float *E, const float *V, const float *vnorm, const float *d_vnorm,
                              int64_t Bi, int R, int D, float *dV, float *dE, itr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ITR_HIP_H */
