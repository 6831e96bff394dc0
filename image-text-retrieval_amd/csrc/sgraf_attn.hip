// SGRAF similarity for a LIST of (image, caption) pairs WITH the weights the score is made of: the word x region attention of
// SCAN_attention (itr/modalmodule/Fusionmodule.py:632-664), AttentionFiltration's weights over the alignment nodes (:615-619) or
// GraphReasoning's edges at every step (:581-587), and the score of EncoderSimilarity.forward (:406-451).  sgraf_pairs.hip computes the same
// score and lets none of these weights leave the chip; this file is its explaining twin for the few best results of every query.
//
// Up to the node rows nothing is new: the item plan of itr_sgraf_pairs_plan and stages (a)-(c) of sgraf_pairs.hip (sgraf_pairs_nodes) run
// unchanged, so P[col, 36] of every item tile, the local node rows Xloc and the global node rows Xglo are the bits the score path sees.
//
// sgraf_reason_kernel<module>: ONE WORKGROUP PER ITEM (one image, <= 16 captions, <= 64 node rows; 256 threads), so that a weight element is
// streamed once per item, not once per pair.  The item's node rows are stacked caption by caption -- global node first, then the words -- into
//   X [64][S + 4]   node rows                            (LDS)
//   Q [64][S + 4]   Q' of the step, then Y               (LDS, SGR only)
//   E [64][68]      the edge weights of all the item's captions: row r holds the softmax over its own caption's columns (SGR only)
// SAF (one wave per caption, vector ALU): a_j = l1norm_j(sigmoid(bn_eval(w . x_j + b))) -> node_w, sim_vec = l2norm(sum_j a_j x_j),
//   score = sigmoid(sim_eval_w . sim_vec + b).
// SGR, per step k over ALL node rows of the item:
//   Q' = X Wfold_k^T + vfold_k      v_mfma_f32_16x16x4_f32; A from LDS, the weights from L2 as the B operand (folded query weights of the state:
//                                   q . k = x^T Wq^T Wk y + bq^T Wk y + terms constant along a softmax row)
//   E  = softmax_rows(Q'_c X_c^T)   the 64 x 64 product of the item on the matrix core, both operands from LDS; every row keeps the columns of
//                                   its own caption: softmax with four lanes per row, summed in an order relative to the caption's first
//                                   node -> `edge`, and E
//   Y  = E_c X_c                    per caption on the matrix core, A = its block of E, B = its rows of X, indexed from its first node
//   X' = relu(Y Wg_k^T + bg_k)      as Q'
// and after the last step score = sigmoid(sim_eval_w . x'_0 + b) per caption.  The wave that owns output-column tile nt (nt = wave, wave + 4,
// ...) accumulates all row tiles of it: every weight fragment is loaded once per workgroup.  Row tiles above the item's node count are skipped.
// K order is fixed and never depends on where a caption's rows sit in the item (projections: u = 0 .. S / 16 - 1, four MFMAs per u; softmax
// sums and Y: counted from the caption's first node), nothing is accumulated across captions and there are no atomics: an element of a pair's
// outputs is a function of that pair's node rows alone -- the same bits in any item, chunk, list or order.
//
// sgraf_attn_scatter_kernel copies a pair's W x 36 rows of P from the item tile to its block of `attn`.
//
// Index hygiene, on the device before the first dependent access: a pair whose output slot, attn, node_w or edge block does not lie inside its
// buffer, or which the plan marked as not scorable, gets score NaN (when the slot itself is valid) and nothing else of it is written; item
// records that do not describe <= 16 captions in <= 64 rows inside the chunk's columns are not followed.
//
// Budgets (gfx950 code object): SGR 108 VGPRs, dynamic LDS at S = 256 152,464 B of the 160 KB (one workgroup per CU); SAF 38
// VGPRs, 68,496 B (two per CU); no scratch, no spills.
#include "sgraf_pairs.h"

namespace itr {

constexpr int GR_THREADS = 256;
constexpr int GR_WAVES = GR_THREADS / 64;
constexpr int GR_LDE = GP_ITEM + 4;        // 68: pitch of the edge tile
constexpr int GR_MAXS = 256;               // sim_dim of the reference; two node-row buffers of 64 x (256 + 4) floats fit the LDS
constexpr float GR_BN_EPS = 1e-5f;

struct ReasonArgs {
    const float *Xloc, *Xglo;                                              // [ncols, S], [n_pairs, S] of the chunk
    const int32_t *grp_begin, *cap_col, *pair_len, *pair_cap, *pair_out;   // of the chunk (pair j = pair p0 + j of the list)
    const float *Wq[8], *vq[8], *Wg[8], *bg[8];
    const float *eval_w, *eval_b, *saf_w, *saf_b, *bn_w, *bn_b, *bn_mean, *bn_var;
    const int64_t *attn_ptr, *aux_ptr;                                     // [out_len + 1]; aux = node_ptr (SAF) / edge_ptr (SGR)
    float *aux, *score;                                                    // node_w / edge
    int64_t attn_len, aux_len, out_len, n_pairs, n_items, ncols;
    int S, steps, module;
};

// where pair j's outputs go, or false: refused (o = its slot, or -1 when even the slot is out of range)
__device__ __forceinline__ bool reason_out_ok(const ReasonArgs &g, int64_t j, int W, int64_t &o, int64_t &aux_base) {
    o = g.pair_out[j];
    aux_base = 0;
    if (o < 0 || o >= g.out_len) { o = -1; return false; }
    if (g.pair_cap[j] < 0 || W < 1 || W > GP_MAXW) return false;
    const int64_t n = W + 1;
    const int64_t ab = g.attn_ptr[o], xb = g.aux_ptr[o];
    const int64_t xn = g.module == 0 ? n : (int64_t)g.steps * n * n;
    aux_base = xb;
    return ab >= 0 && ab + (int64_t)W * SC_R <= g.attn_len && xb >= 0 && xb + xn <= g.aux_len;
}

struct ReasonMeta {
    int64_t aux_base[GP_MAXCAP];
    int64_t row_src[GP_ITEM];              // >= 0: float offset into Xloc; -(1 + j): global node of pair j; INT64_MIN: a row nobody owns
    int32_t slot[GP_MAXCAP], rbase[GP_MAXCAP], nn[GP_MAXCAP], emit[GP_MAXCAP];
    int32_t row_lo[GP_ITEM], row_hi[GP_ITEM], row_cap[GP_ITEM];
    float a[GP_ITEM];                      // SAF: the normalised weights of the item's node rows
    int32_t nrows, ncap;
    int32_t pad_[2];
};
static_assert(sizeof(ReasonMeta) % 16 == 0, "the node rows behind the records are read as float4");

static size_t reason_lds_bytes(int module, int S) {
    const size_t rows = (size_t)GP_ITEM * (S + 4) * 4;
    return sizeof(ReasonMeta) + (module == 1 ? 2 * rows + (size_t)GP_ITEM * GR_LDE * 4 : rows);
}

// Out[64][ld] = act(A[64][ld] W^T + bias) for the first `na` row tiles; A, Out in LDS (Out != A), W [S, S] row-major in global memory
template <bool RELU>
__device__ __forceinline__ void reason_project(const float *A, const float *__restrict__ W, const float *__restrict__ bias, float *Out, int S, int ld,
                                               int na, int wave, int fi, int fg) {
    for (int nt = wave; nt < S / 16; nt += GR_WAVES) {
        f32x4 acc[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) acc[a] = f32x4{0.f, 0.f, 0.f, 0.f};
        const float *wrow = W + (int64_t)(nt * 16 + fi) * S + 4 * fg;
        const float *arow = A + fi * ld + 4 * fg;
        for (int u = 0; u < S / 16; ++u) {
            const f32x4 b = *reinterpret_cast<const f32x4 *>(wrow + 16 * u);
#pragma unroll
            for (int a = 0; a < 4; ++a)
                if (a < na) {
                    const f32x4 x = *reinterpret_cast<const f32x4 *>(arow + a * 16 * ld + 16 * u);
                    acc[a] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[0], b[0], acc[a], 0, 0, 0);
                    acc[a] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[1], b[1], acc[a], 0, 0, 0);
                    acc[a] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[2], b[2], acc[a], 0, 0, 0);
                    acc[a] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[3], b[3], acc[a], 0, 0, 0);
                }
        }
        const float bv = bias[nt * 16 + fi];
#pragma unroll
        for (int a = 0; a < 4; ++a)
            if (a < na) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float v = acc[a][r] + bv;
                    Out[(a * 16 + 4 * fg + r) * ld + nt * 16 + fi] = RELU ? fmaxf(v, 0.f) : v;
                }
            }
    }
}

template <int MODULE>
__global__ __launch_bounds__(GR_THREADS) void sgraf_reason_kernel(ReasonArgs g) {
    extern __shared__ __attribute__((aligned(16))) char gr_smem[];
    ReasonMeta &m = *reinterpret_cast<ReasonMeta *>(gr_smem);
    const int S = g.S, ld = S + 4;
    float *X = reinterpret_cast<float *>(gr_smem + sizeof(ReasonMeta));
    float *Q = X + GP_ITEM * ld;
    float *E = Q + GP_ITEM * ld;
    const int tid = threadIdx.x, lane = tid & 63, fi = lane & 15, fg = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t t = blockIdx.x;
    // ---- the item's records: captions, node rows, where the outputs go
    if (tid == 0) {
        int64_t b = g.grp_begin[t], e = g.grp_begin[t + 1];
        b = b < 0 ? 0 : (b > g.n_pairs ? g.n_pairs : b);
        e = e < b ? b : (e > g.n_pairs ? g.n_pairs : e);
        if (e - b > GP_MAXCAP) e = b + GP_MAXCAP;
        const int ncap = (int)(e - b);
        int rows = 0;
        for (int j = 0; j < ncap; ++j) {
            const int64_t pj = b + j;
            const int W = g.pair_len[pj];
            const int64_t col = g.cap_col[pj];
            int64_t o, xb;
            const bool ok = reason_out_ok(g, pj, W, o, xb);
            const bool fits = W >= 1 && W <= GP_MAXW && rows + W + 1 <= GP_ITEM && col >= t * GP_ITEM && col + W <= (t + 1) * GP_ITEM && col + W <= g.ncols;
            m.slot[j] = (int32_t)o, m.aux_base[j] = xb, m.emit[j] = ok && fits;
            m.rbase[j] = rows, m.nn[j] = fits ? W + 1 : 0;
            if (!fits) continue;
            for (int r = 0; r <= W; ++r) {
                m.row_lo[rows + r] = rows, m.row_hi[rows + r] = rows + W + 1, m.row_cap[rows + r] = j;
                m.row_src[rows + r] = r == 0 ? -(1 + pj) : (col + r - 1) * (int64_t)S;
            }
            rows += W + 1;
        }
        m.nrows = rows, m.ncap = ncap;
        for (int r = rows; r < GP_ITEM; ++r) m.row_lo[r] = 0, m.row_hi[r] = 0, m.row_cap[r] = -1, m.row_src[r] = INT64_MIN;
    }
    __syncthreads();
    const int ncap = m.ncap;
    const int na = (m.nrows + 15) >> 4;                       // row tiles in use (workgroup-uniform)
    // ---- node rows -> LDS (rows nobody owns: zeros)
    for (int r = wave; r < GP_ITEM; r += GR_WAVES) {
        const int64_t src = m.row_src[r];
        const float *p = src >= 0 ? g.Xloc + src : (src != INT64_MIN ? g.Xglo + (-(src + 1)) * (int64_t)S : nullptr);
        for (int d = lane; d < S / 4; d += 64)
            *reinterpret_cast<f32x4 *>(X + r * ld + 4 * d) = p ? *reinterpret_cast<const f32x4 *>(p + 4 * d) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    __syncthreads();
    if (MODULE == 0) {
        // ---- AttentionFiltration, one wave per caption
        const float bscale = g.bn_w[0] / sqrtf(g.bn_var[0] + GR_BN_EPS);
        const float sb = g.saf_b[0], bm = g.bn_mean[0], bb = g.bn_b[0];
        for (int j = wave; j < ncap; j += GR_WAVES) {
            const int nn = m.nn[j], rb = m.rbase[j];
            const int64_t o = m.slot[j];
            if (nn == 0 || !m.emit[j]) {
                if (o >= 0 && lane == 0) g.score[o] = __builtin_nanf("");
                continue;
            }
            float mine = 0.f;
            for (int n = 0; n < nn; ++n) {
                const float *x = X + (rb + n) * ld;
                float s = 0.f;
                for (int d = lane; d < S; d += 64) s = fmaf(x[d], g.saf_w[d], s);
                s = wave_sum(s) + sb;
                const float a = 1.f / (1.f + expf(-((s - bm) * bscale + bb)));
                mine = lane == n ? a : mine;
            }
            const float asum = wave_sum(fabsf(mine));                       // lanes >= nn hold 0
            const float an = mine / (asum + 1e-8f);                         // l1norm
            if (lane < nn) {
                m.a[rb + lane] = an;
                g.aux[m.aux_base[j] + lane] = an;
            }
            __builtin_amdgcn_wave_barrier();
            float vec[GR_MAXS / 64];
#pragma unroll
            for (int u = 0; u < GR_MAXS / 64; ++u) vec[u] = 0.f;
            for (int n = 0; n < nn; ++n) {
                const float a = m.a[rb + n];
#pragma unroll
                for (int u = 0; u < GR_MAXS / 64; ++u) {
                    const int d = lane + 64 * u;
                    if (d < S) vec[u] = fmaf(a, X[(rb + n) * ld + d], vec[u]);
                }
            }
            float ss = 0.f, dot = 0.f;
#pragma unroll
            for (int u = 0; u < GR_MAXS / 64; ++u) {
                const int d = lane + 64 * u;
                if (d < S) { ss = fmaf(vec[u], vec[u], ss); dot = fmaf(vec[u], g.eval_w[d], dot); }
            }
            ss = wave_sum(ss);
            dot = wave_sum(dot);
            const float sc = dot / (sqrtf(ss) + 1e-8f) + g.eval_b[0];       // sim_eval_w . l2norm(vec) + b
            if (lane == 0) g.score[o] = 1.f / (1.f + expf(-sc));
        }
        return;
    }
    // ---- GraphReasoning x steps over all node rows of the item
    for (int k = 0; k < g.steps; ++k) {
        reason_project<false>(X, g.Wq[k], g.vq[k], Q, S, ld, na, wave, fi, fg);
        __syncthreads();
        // E = softmax_rows(Q' X^T) inside every caption's block: wave = row tile
        if (wave < na) {
            const int a = wave;
            f32x4 e[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) e[b] = f32x4{0.f, 0.f, 0.f, 0.f};
            const float *qrow = Q + (a * 16 + fi) * ld + 4 * fg;
            const float *krow = X + fi * ld + 4 * fg;
            for (int u = 0; u < S / 16; ++u) {
                const f32x4 q = *reinterpret_cast<const f32x4 *>(qrow + 16 * u);
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    if (b < na) {
                        const f32x4 x = *reinterpret_cast<const f32x4 *>(krow + b * 16 * ld + 16 * u);
                        e[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(q[0], x[0], e[b], 0, 0, 0);
                        e[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(q[1], x[1], e[b], 0, 0, 0);
                        e[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(q[2], x[2], e[b], 0, 0, 0);
                        e[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(q[3], x[3], e[b], 0, 0, 0);
                    }
            }
            // the raw tile -> E (this lane holds, per column tile b, column b * 16 + fi of rows a * 16 + 4 fg + r)
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (b < na) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) E[(a * 16 + 4 * fg + r) * GR_LDE + b * 16 + fi] = e[b][r];
                }
            __builtin_amdgcn_wave_barrier();                // (the row tile is this wave's own)
            // softmax over the row's own caption, four lanes per row.  Lane q takes columns lo + q, lo + q + 4, ...: the order of every
            // sum is relative to the caption's first node, never to where the caption sits in the item
            {
                const int row = a * 16 + (lane >> 2), q = lane & 3;
                const int lo = m.row_lo[row], hi = m.row_hi[row], n = hi - lo;
                const int cj = m.row_cap[row];
                float *er = E + row * GR_LDE;
                float mx = -INFINITY;
                for (int c = lo + q; c < hi; c += 4) mx = fmaxf(mx, er[c]);
                mx = fmaxf(mx, __shfl_xor(mx, 1, 64)); mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
                float den = 0.f;
                for (int c = lo + q; c < hi; c += 4) { const float v = expf(er[c] - mx); er[c] = v; den += v; }
                den += __shfl_xor(den, 1, 64); den += __shfl_xor(den, 2, 64);
                const float inv = 1.f / den;
                const bool emit = cj >= 0 && m.emit[cj];
                const int64_t off = emit ? m.aux_base[cj] + ((int64_t)k * n + (row - lo)) * n : 0;      // row (row - lo) of step k's [n, n] block
                for (int c = lo + q; c < hi; c += 4) {
                    const float pv = er[c] * inv;
                    er[c] = pv;
                    if (emit) g.aux[off + (c - lo)] = pv;
                }
            }
        }
        __syncthreads();
        // Y_c = E_c X_c -> Q, caption by caption with A and B indexed from the caption's first node (K order relative to the caption);
        // wave = output-column tiles
        for (int nt = wave; nt < S / 16; nt += GR_WAVES) {
            for (int j = 0; j < ncap; ++j) {
                const int n = m.nn[j], lo = m.rbase[j];
                const int T = (n + 15) >> 4;
                for (int a = 0; a < T; ++a) {
                    f32x4 y = f32x4{0.f, 0.f, 0.f, 0.f};
                    const bool ra_ok = 16 * a + fi < n;
                    const float *er = E + (lo + (ra_ok ? 16 * a + fi : 0)) * GR_LDE + lo;
                    for (int b = 0; b < T; ++b) {
#pragma unroll
                        for (int cc = 0; cc < 4; ++cc) {
                            const int kk = 16 * b + 4 * fg + cc;
                            const bool ok = kk < n;
                            const float av = (ok && ra_ok) ? er[kk] : 0.f;
                            const float bv = ok ? X[(lo + kk) * ld + nt * 16 + fi] : 0.f;
                            y = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, y, 0, 0, 0);
                        }
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int rr = 16 * a + 4 * fg + r;
                        if (rr < n) Q[(lo + rr) * ld + nt * 16 + fi] = y[r];
                    }
                }
            }
        }
        __syncthreads();
        reason_project<true>(Q, g.Wg[k], g.bg[k], X, S, ld, na, wave, fi, fg);
        __syncthreads();
    }
    // ---- score = sigmoid(sim_eval_w . x'_0 + b), one wave per caption
    for (int j = wave; j < ncap; j += GR_WAVES) {
        const int64_t o = m.slot[j];
        if (o < 0) continue;
        float sc = __builtin_nanf("");
        if (m.nn[j] != 0 && m.emit[j]) {
            const float *x = X + m.rbase[j] * ld;
            float s = 0.f;
            for (int d = lane; d < S; d += 64) s = fmaf(x[d], g.eval_w[d], s);
            s = wave_sum(s) + g.eval_b[0];
            sc = 1.f / (1.f + expf(-s));
        }
        if (lane == 0) g.score[o] = sc;
    }
}

// attn[attn_ptr[slot] ..] = the pair's W x 36 rows of P (contiguous in the item tile); one wave per pair
__global__ __launch_bounds__(256) void sgraf_attn_scatter_kernel(ReasonArgs g, const float *__restrict__ P, float *__restrict__ attn) {
    const int lane = threadIdx.x & 63;
    const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= g.n_pairs) return;
    const int W = g.pair_len[j];
    const int64_t col = g.cap_col[j];
    int64_t o, xb;
    if (!reason_out_ok(g, j, W, o, xb) || col < 0 || col + W > g.ncols) return;      // (the reasoning kernel writes the NaN score)
    const int64_t ab = g.attn_ptr[o];
    const float *src = P + col * SC_R;
    float *dst = attn + ab;
    if (((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 15) == 0) {
        for (int i = lane; i < W * (SC_R / 4); i += 64) reinterpret_cast<f32x4 *>(dst)[i] = reinterpret_cast<const f32x4 *>(src)[i];
    } else {
        for (int i = lane; i < W * SC_R; i += 64) dst[i] = src[i];
    }
}

static int ga_check_shape(const char *who, int64_t Ni, int64_t Nc, int64_t n_rows, int R, int D, int S, int module, int sgr_step) {
    const int rc = gp_check_shape(who, Ni, Nc, n_rows, R, D, S, module, sgr_step);
    if (rc != ITR_OK) return rc;
    ITR_UNSUPPORTED(S > GR_MAXS || S % 16 != 0, "%s: sim_dim must be a multiple of 16 and at most %d (two 64-row node buffers in LDS), got %d", who,
                    GR_MAXS, S);
    return ITR_OK;
}

}  // namespace itr

extern "C" size_t itr_sgraf_pair_attention_workspace_bytes(int64_t n_pairs, int64_t n_items, int D, int S, int module, int sgr_step) {
    if (n_pairs < 0 || n_items < 0 || D <= 0 || S <= 0) return 0;
    return itr::gp_chunk(nullptr, n_pairs, n_items, D, S, module, sgr_step, false).bytes;
}

extern "C" int itr_sgraf_pair_attention(const float *img, const float *words, const int64_t *cap_off, const int32_t *pair_img,
                                        const int32_t *pair_capok, const int32_t *pair_len, const int32_t *pair_col, const int32_t *pair_out,
                                        const int32_t *item_begin, const int32_t *item_img, int64_t p0, int64_t n_pairs, int64_t it0,
                                        int64_t n_items, int64_t Ni, int64_t Nc, int64_t n_rows, int R, int D, int S, int module, int sgr_step,
                                        const itr_sgraf_weights *w, const void *state, size_t state_bytes, float *attn, const int64_t *attn_ptr,
                                        int64_t attn_len, float *node_w, const int64_t *node_ptr, int64_t node_len, float *edge,
                                        const int64_t *edge_ptr, int64_t edge_len, float *score, int64_t out_len, void *workspace,
                                        size_t workspace_bytes, itr_stream_t stream) {
    using namespace itr;
    const char *who = "itr_sgraf_pair_attention";
    ITR_REQUIRE(img && words && cap_off && w && state && workspace, "%s: null pointer", who);
    int rc = ga_check_shape(who, Ni, Nc, n_rows, R, D, S, module, sgr_step);
    if (rc != ITR_OK) return rc;
    ITR_REQUIRE(p0 >= 0 && n_pairs >= 0 && it0 >= 0 && n_items >= 0 && out_len >= 0 && attn_len >= 0 && node_len >= 0 && edge_len >= 0,
                "%s: bad range", who);
    ITR_REQUIRE(n_pairs == 0 || (n_items >= 1 && n_items <= n_pairs), "%s: a chunk of %lld pairs cannot have %lld items", who, (long long)n_pairs,
                (long long)n_items);
    ITR_UNSUPPORTED(p0 + n_pairs >= 0x7fffffffLL / GP_ITEM, "%s: pair index overflow; split the lists", who);
    ITR_REQUIRE(n_pairs == 0 || (pair_img && pair_capok && pair_len && pair_col && pair_out && item_begin && item_img && attn && attn_ptr && score &&
                                 (module == 0 ? (node_w && node_ptr) : (edge && edge_ptr))),
                "%s: null pointer", who);
    ITR_REQUIRE((reinterpret_cast<uintptr_t>(img) & 15) == 0 && (reinterpret_cast<uintptr_t>(words) & 15) == 0, "%s: operands must be 16-byte aligned", who);
    const GpState s = gp_state(const_cast<void *>(state), Ni, Nc, n_rows, D, S, module, sgr_step);
    ITR_REQUIRE(state_bytes >= s.bytes, "%s: state buffer too small", who);
    const GpChunk k = gp_chunk(workspace, n_pairs, n_items, D, S, module, sgr_step, false);
    ITR_REQUIRE(workspace_bytes >= k.bytes, "%s: workspace too small", who);
    if (n_pairs == 0 || Ni == 0 || Nc == 0) return ITR_OK;
    hipStream_t st = as_stream(stream);
    rc = sgraf_pairs_nodes(img, words, cap_off, pair_img, pair_capok, pair_len, pair_col, item_begin, item_img, p0, n_pairs, it0, n_items, Ni, n_rows, D,
                           S, w, s, k, st);
    if (rc != ITR_OK) return rc;
    ReasonArgs a{};
    a.Xloc = k.Xloc, a.Xglo = k.Xglo, a.grp_begin = k.grp_begin, a.cap_col = k.cap_col;
    a.pair_len = pair_len + p0, a.pair_cap = pair_capok + p0, a.pair_out = pair_out + p0;
    for (int i = 0; i < 8; ++i) {
        const bool on = module == 1 && i < sgr_step;
        a.Wq[i] = on ? s.Wfold[i] : nullptr, a.vq[i] = on ? s.vfold[i] : nullptr;
        a.Wg[i] = on ? w->sgr_g_w[i] : nullptr, a.bg[i] = on ? w->sgr_g_b[i] : nullptr;
        ITR_REQUIRE(!on || (a.Wg[i] && a.bg[i]), "%s: null SGR weight", who);
    }
    a.eval_w = w->eval_w, a.eval_b = w->eval_b;
    a.saf_w = w->saf_w, a.saf_b = w->saf_b, a.bn_w = w->saf_bn_w, a.bn_b = w->saf_bn_b, a.bn_mean = w->saf_bn_mean, a.bn_var = w->saf_bn_var;
    ITR_REQUIRE(a.eval_w && a.eval_b && (module == 1 || (a.saf_w && a.saf_b && a.bn_w && a.bn_b && a.bn_mean && a.bn_var)), "%s: null weight", who);
    a.attn_ptr = attn_ptr, a.aux_ptr = module == 0 ? node_ptr : edge_ptr, a.aux = module == 0 ? node_w : edge, a.score = score;
    a.attn_len = attn_len, a.aux_len = module == 0 ? node_len : edge_len, a.out_len = out_len;
    a.n_pairs = n_pairs, a.n_items = n_items, a.ncols = n_items * GP_ITEM, a.S = S, a.steps = module == 1 ? sgr_step : 0, a.module = module;
    const size_t lds = reason_lds_bytes(module, S);
    if (module == 0) {
        rc = allow_dynamic_lds(reinterpret_cast<const void *>(sgraf_reason_kernel<0>), lds);
        if (rc != ITR_OK) return rc;
        hipLaunchKernelGGL(sgraf_reason_kernel<0>, dim3((unsigned)n_items), dim3(GR_THREADS), lds, st, a);
    } else {
        rc = allow_dynamic_lds(reinterpret_cast<const void *>(sgraf_reason_kernel<1>), lds);
        if (rc != ITR_OK) return rc;
        hipLaunchKernelGGL(sgraf_reason_kernel<1>, dim3((unsigned)n_items), dim3(GR_THREADS), lds, st, a);
    }
    ITR_CHECK_LAUNCH("sgraf reason");
    hipLaunchKernelGGL(sgraf_attn_scatter_kernel, dim3((unsigned)ceil_div(n_pairs, (int64_t)4)), dim3(256), 0, st, a, k.P, attn);
    ITR_CHECK_LAUNCH("sgraf attention scatter");
    return ITR_OK;
}
