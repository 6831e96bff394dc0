// Host functions that one translation unit of libitr_hip.so defines and another calls, grouped by the defining file.  The defining
// file includes this header too, so a definition that drifts from its declaration is a compile error.
#pragma once
#include "itr_common.h"

namespace itr {

// ---- caller-allocated workspaces: one function per workspace both sizes and carves it.  Given the caller's buffer the carver hands
// out the blocks, given a null base it only measures (the *_workspace_bytes entry points).  Every block starts on a 256-byte boundary.
static inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
struct WsCarver {
    char *base;
    size_t bytes = 0;      // taken so far
    explicit WsCarver(void *b) : base(static_cast<char *>(b)) {}
    template <typename T = char> T *take(size_t n) {
        T *q = base ? reinterpret_cast<T *>(base + bytes) : nullptr;
        bytes += align256(n);
        return q;
    }
};

// ---- gemm_f32.hip
int gemm_nt(const float *A, int64_t lda, const float *B, int64_t ldb, const float *bias, float *C, int64_t ldc, int64_t M, int64_t N, int64_t K,
            int act, hipStream_t st);
int gemm_nt_acc(const float *A, int64_t lda, const float *B, int64_t ldb, const float *bias, float *C, int64_t ldc, int64_t M, int64_t N,
                int64_t K, int act, hipStream_t st);
int gemm_nt_sqdiff(const float *A, int64_t lda, const float *B, int64_t ldb, const float *rowscale, const float *Z, int64_t ldz, float *C,
                   int64_t ldc, int64_t M, int64_t N, int64_t K, hipStream_t st);
// the two directions of a bi-GRU time step in one launch
bool gemm_pair_ok(int64_t lda, int64_t ldb, int64_t K);
int gemm_nt_pair(const float *A, const float *A2, int64_t lda, const float *B, const float *B2, int64_t ldb, const float *bias, const float *bias2,
                 float *C, float *C2, int64_t ldc, int64_t M, int64_t N, int64_t K, hipStream_t st);
// skinny GEMMs of the recurrence (M = batch): split-K with a deterministic reduction
int gemm_splitk_choice(int64_t M, int64_t N, int64_t K);
size_t gemm_splitk_scratch_bytes(int64_t M, int64_t N, int splits);
int gemm_nt_splitk(const float *A, int64_t lda, const float *B, int64_t ldb, const float *bias, float *C, int64_t ldc, int64_t M, int64_t N,
                   int64_t K, int act, int accumulate, int splits, float *scratch, hipStream_t st);
// the slices only, as many M x N slices as `scratch_bytes` holds at most
int gemm_nt_splitk_partials(const float *A, int64_t lda, const float *B, int64_t ldb, int64_t M, int64_t N, int64_t K, int splits, float *scratch,
                            size_t scratch_bytes, int *n_slices, hipStream_t st);
// ---- gemm_skinny.hip
bool gemm_skinny_ok(const float *A, int64_t lda, const float *B, int64_t ldb, int64_t M, int64_t N, int64_t K);
int gemm_skinny_partials(const float *A, int64_t lda, const float *B, int64_t ldb, int64_t M, int64_t N, int64_t K, int max_slices, float *part,
                         int *n_slices, hipStream_t st);
int gemm_skinny_direct(const float *A, int64_t lda, const float *B, int64_t ldb, const float *bias, float *C, int64_t ldc, int64_t M, int64_t N,
                       int64_t K, int act, hipStream_t st);
// ---- gemm_stream.hip
bool gemm_nt_stream(const float *A, int64_t lda, const float *B, int64_t ldb, const float *bias, float *C, int64_t ldc, int64_t M, int64_t N,
                    int64_t K, int act, hipStream_t st, int *rc, int algo);
// ---- gemm_tn.hip
size_t gemm_tn_workspace_bytes(int64_t R, int P, int Q);
int gemm_tn(const float *A, int64_t lda, const float *B, int64_t ldb, float *C, int64_t ldc, int64_t R, int P, int Q, int accumulate,
            float *colsum_a, void *workspace, size_t workspace_bytes, hipStream_t st);
// ---- norm.hip
int norm_rows(const float *x, float *y, int64_t rows, int dim, float eps, int kind, int take_abs, hipStream_t st);
// ---- scan_train.hip: once per (kernel, device), under a mutex
int allow_dynamic_lds(const void *kernel, size_t bytes);
// row L2 norms (no eps) and their backward dX[row] += dn[row] X[row] / ||X[row]||: the words in t2i, the regions in i2t (scan_train_i2t.hip)
__global__ void rownorm_train_kernel(const float *__restrict__ x, int64_t rows, int D, float *__restrict__ out);
__global__ void rownorm_bwd_kernel(const float *__restrict__ X, const float *__restrict__ xnorm, const float *__restrict__ dn, int64_t rows, int D,
                                   float *__restrict__ dX);
// ---- scan_xattn.hip
struct ScanTileMeta;
// the SCAN workspace: tile records and tile-packed words, then the t2i (mode 0) or the i2t (mode 1) buffers in the same space
struct ScanWs {
    float *gram, *wnorm, *vnorm, *cgram, *hblk, *wtiled;
    int64_t *coff;
    ScanTileMeta *meta;
    size_t bytes;
};
ScanWs scan_ws(void *base, int64_t Ni, int R, int64_t n_rows, int64_t Nc, int64_t n_tiles, int D, int mode);
int scan_prepare_impl(const float *img, const float *words, const int64_t *cap_off, const int32_t *cap_len, const int32_t *tile_begin_dev,
                      const int32_t *cap_order_dev, int64_t n_tiles, int64_t Ni, int64_t Nc, int64_t n_rows, int R, int D, int mode,
                      void *workspace, size_t workspace_bytes, int32_t *cap_col, itr_stream_t stream);
int scan_scores_impl(const float *img, int64_t n_tiles, int64_t Ni, int64_t Nc, int64_t n_rows, int R, int D, int mode, int norm, int agg,
                     float lambda_softmax, float lambda_lse, float *S, int64_t ldS, void *workspace, size_t workspace_bytes, float *emit_p,
                     float *emit_cn, int64_t img_index0, int64_t img_count, itr_stream_t stream);
// LDS-tiled Gram kernel of the evaluation path: G[n] = X_n X_n^T
__global__ void gram_kernel(const float *__restrict__ X, const int64_t *__restrict__ row_off, const int32_t *__restrict__ row_cnt, int fixed_rows,
                            int D, float *__restrict__ G, const int64_t *__restrict__ g_off, int upper2);
__global__ void gram_mfma_kernel(const float *__restrict__ X, int rows, int D, float *__restrict__ G, int upper2);
// row L2 norms (no eps) and the exclusive prefix sum of len^2 (caption Gram offsets): shared with scan_pairs.hip
__global__ void rownorm_kernel(const float *__restrict__ X, int64_t rows, int D, float *__restrict__ out);
__global__ void sq_prefix_kernel(const int32_t *__restrict__ len, int64_t n, int64_t *__restrict__ off);
// ---- sgr_fused.hip: all graph-reasoning steps of a group of captions in one workgroup
size_t sgr_fused_workspace_bytes(int64_t n_groups, int64_t n_caps, int sgr_step);
int sgr_fused_prepare(const int32_t *grp_begin, const int32_t *grp_order, int64_t n_groups, int64_t n_caps, const int32_t *cap_len,
                      const int32_t *cap_col, const float *const *wq, const float *const *wg, int sgr_step, void *ws, int *bad_flag, hipStream_t st);
int sgr_fused_plan_groups(const int32_t *grp_begin, const int32_t *grp_order, int64_t n_groups, int64_t n_caps, const int32_t *cap_len,
                          const int32_t *cap_col, int sgr_step, void *ws, int *bad_flag, hipStream_t st);
size_t sgr_fused_weights_bytes(int sgr_step);
int sgr_fused_pack_weights(const float *const *wq, const float *const *wg, int sgr_step, void *wbuf, hipStream_t st);
// packed_weights: null = the copy sgr_fused_prepare put into `ws`; else sgr_fused_pack_weights' buffer
int sgr_fused_scores(const float *xloc, const float *xglo, void *ws, int64_t n_groups, int64_t n_caps, int64_t nb, int64_t Nc, int64_t ncols,
                     const float *const *vq, const float *const *bg, int sgr_step, float *y0, bool persistent_walk, hipStream_t st,
                     const void *packed_weights = nullptr);
int sgr_fused_finish(void *ws, int64_t n_groups, int64_t n_caps, int sgr_step, int64_t Ni, float *S, int64_t ldS, hipStream_t st);
// ---- sgraf.hip: pieces of itr_sgraf_scores that the candidate-list entry (sgraf_pairs.hip) runs as well
int sgraf_global_nodes(const float *img, const float *words, const int64_t *cap_off, const int32_t *cap_len, int64_t Ni, int64_t Nc, int64_t n_rows,
                       int D, const itr_sgraf_weights *w, float *img_ave, float *g_emb_v, float *l_emb_v, float *img_glo, float *l_emb_t,
                       float *cap_ave, float *g_emb_t, float *cap_glo, const char *who, itr_stream_t stream);
int sgraf_fold_weights(const itr_sgraf_weights *w, int S, int sgr_step, float *WqT, float *WkT, float *const *Wfold, float *const *vfold, hipStream_t st);
struct SgrafStage {
    float *Xglo, *Xloc, *Qloc, *Qglo, *Yloc, *Yglo;     // node rows [nb * ldg, S] / [nb * ncols, S]; Q*, Yloc: step-by-step chain only
    const int32_t *cap_col, *cap_len;                   // per caption: first column of its words in a row of Xloc, word count
    int64_t Nc, ncols, ldg;
    int S, module, sgr_step, max_len;
    bool fused, persistent;
    const itr_sgraf_weights *w;
    float *const *Wfold, *const *vfold;
    void *fused_ws;
    int64_t n_node_groups;
    const void *packed_weights;                         // sgr_fused_scores' packed_weights
};
int sgraf_pair_stage(const SgrafStage &s, int64_t nb, float *Sout, int64_t ldS, int64_t i0, hipStream_t st);
// ---- sgraf_loc.hip
int sgraf_loc_fused(const float *P, const float *cn, const float *img, const float *wtiled, const float *W, const float *bias, float *X,
                    int64_t nb, int64_t n_tiles, int D, hipStream_t st);
int sgraf_loc_items(const float *P, const float *cn, const float *img, int64_t Ni, const int32_t *tile_img, const float *wtiled, const float *W,
                    const float *bias, float *X, int64_t n_tiles, int D, hipStream_t st);

}  // namespace itr
