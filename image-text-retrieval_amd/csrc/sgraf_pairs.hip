// SGRAF similarity (EncoderSimilarity.forward, itr/modalmodule/Fusionmodule.py:406-451, with SCAN_attention :632-664, AttentionFiltration
// :615-619 and GraphReasoning :581-587) for a LIST of (image, caption) pairs: the fine stage of coarse-to-fine retrieval.  Only the listed
// pairs are computed; nothing of size (Ni, Nc) exists, attention weights and node rows included.
//
// Unit of work.  The list arrives IMAGE-major (CSR img_ptr[Ni + 1] over pair_cap[P]).  itr_sgraf_pairs_plan packs each image's listed
// captions, in list order, into ITEMS: one image x whole captions with <= 16 captions and words + captions <= 64.  An item is at once
//   - a 64-column tile of the local-node kernel (sgraf_loc.hip, item form: the image comes from the item record), and
//   - a 64-node-row group of the fused graph steps (sgr_fused.hip: one global node per caption + its word nodes).
// itr_sgraf_pair_scores then scores a CHUNK = a range of items as ONE virtual image row whose "captions" are the chunk's pairs: the SAF
// pair kernel, the fused / step-by-step SGR kernels, the step GEMMs and the final kernel of the dense call (sgraf_pair_stage, sgraf.hip) run
// unchanged with nb = 1.  New here is what needs the image PER ITEM instead of per block:
//   (a) sgraf_pair_attn_kernel   SCAN_attention of one pair per wave: raw dot products (pair_mainloop.h), clipped l2norm over the words,
//                                softmax(9 x) over the regions, ||ctx|| in Gram form -> P[64 columns, 36] and 1 / (||ctx|| + eps) of the item tile
//   (b) sgraf_loc_items_kernel   the local-node kernel with the image pointer from the item record; the item's word rows are GATHERED into
//                                an item-tiled buffer per chunk (sgraf_pair_gather_kernel), because the generated D loop addresses 16
//                                consecutive rows per wave from one scalar base
//   (c) sgraf_pair_glo_kernel    (img_glo[i] - cap_glo[c])^2 per pair, then the GEMM with sim_tranglo_w and the row l2norm
//   (d) the plan / index kernels.
// sim_dim != 256: (b) is sgraf_pair_ctx_kernel (vector ALU) + GEMM + l2norm, the graph steps run step by step.  It works; it is not fast.
//
// A pair's score is its own: every kernel computes a node row or a pair from that pair's operands alone in a fixed order (no atomics on
// floats, no reduction across pairs), and the GEMMs' rows do not depend on the row count -- so the bits do not depend on the item, the
// chunk, the list, K or the list direction.
//
// Once per call (itr_sgraf_pairs_prepare): VisualSA / TextSA global vectors, the images' Gram matrices, the folded SGR query weights and
// their fragment-ordered copies.  Never per pair or per chunk.  Its intermediates live in a scratch buffer the caller frees after the call.
//
// Budgets.  sgraf_pair_attn_kernel: 512 threads (8 pairs), LDS 79,872 B, 126 VGPRs, no scratch: two workgroups per CU by
// registers and by LDS.  sgraf_loc_items_kernel: as sgraf_loc_kernel (250 VGPRs, 80 KB LDS, two workgroups per CU).  The other kernels
// are copies / elementwise: <= 26 VGPRs, at most 4 KB of LDS.
#include "sgraf_pairs.h"
#include "pair_mainloop.h"

namespace itr {

// ---------------------------------------------------------------------------------------------------------------- plan
// pass 0: items of image i (count); pass 1: the records.  One thread per image walks its pairs in list order (greedy: a caption opens a new
// item when the current one has 16 captions or would exceed 64 node rows).
template <int PASS>
__global__ __launch_bounds__(256) void sgraf_pairs_plan_kernel(const int32_t *__restrict__ img_ptr, const int32_t *__restrict__ pair_cap,
                                                               const int64_t *__restrict__ cap_off, const int32_t *__restrict__ cap_len,
                                                               int64_t P, int64_t Ni, int64_t Nc, int64_t n_rows, int32_t *__restrict__ img_items,
                                                               int32_t *__restrict__ pair_len, int32_t *__restrict__ pair_col,
                                                               int32_t *__restrict__ pair_capok, int32_t *__restrict__ item_begin,
                                                               int32_t *__restrict__ item_img) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= Ni) return;
    int64_t b = img_ptr[i], e = img_ptr[i + 1];
    b = b < 0 ? 0 : (b > P ? P : b);
    e = e < b ? b : (e > P ? P : e);
    int64_t item = PASS ? img_items[i] : 0;
    int ncap = 0, rows = 0, n = 0;
    for (int64_t p = b; p < e; ++p) {
        const int c = pair_cap[p];
        int len = (c >= 0 && c < Nc) ? cap_len[c] : 0;
        bool ok = len >= 1 && len <= GP_MAXW;
        if (ok) { const int64_t o = cap_off[c]; ok = o >= 0 && o + len <= n_rows; }
        if (!ok) len = 1;                                    // a defined one-word slot of zeros; the pair's score is NaN
        if (n == 0 || ncap == GP_MAXCAP || rows + len + 1 > GP_ITEM) {
            if (n) ++item;
            ++n;
            ncap = 0, rows = 0;
            if (PASS) { item_begin[item] = (int32_t)p; item_img[item] = (int32_t)i; }
        }
        if (PASS) {
            pair_len[p] = len;
            pair_col[p] = (int32_t)(item * GP_ITEM + (rows - ncap));      // words so far in this item
            pair_capok[p] = ok ? c : -1;
        }
        ++ncap;
        rows += len + 1;
    }
    if (!PASS) img_items[i] = n;
}

// exclusive prefix of the per-image item counts in place (img_items[Ni] = total); single workgroup
__global__ __launch_bounds__(1024) void sgraf_pairs_prefix_kernel(int32_t *__restrict__ img_items, int64_t n, int64_t P, int32_t *__restrict__ item_begin,
                                                                  int32_t *__restrict__ counts) {
    __shared__ int part[1024];
    const int t = threadIdx.x;
    const int64_t per = (n + 1023) / 1024;
    const int64_t b = t * per < n ? t * per : n, e = (b + per < n) ? b + per : n;
    int s = 0;
    for (int64_t i = b; i < e; ++i) s += img_items[i];
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        int run = 0;
        for (int i = 0; i < 1024; ++i) { const int v = part[i]; part[i] = run; run += v; }
        img_items[n] = run;
        item_begin[run] = (int32_t)P;
        counts[0] = run;
    }
    __syncthreads();
    int run = part[t];
    for (int64_t i = b; i < e; ++i) { const int v = img_items[i]; img_items[i] = run; run += v; }
}

// ---------------------------------------------------------------------------------------------------------------- chunk index
// cap_col[j] = column of pair p0 + j's first word inside the chunk; grp_order = identity; grp_begin[t] = first pair of item it0 + t
__global__ __launch_bounds__(256) void sgraf_pair_index_kernel(const int32_t *__restrict__ pair_col, const int32_t *__restrict__ item_begin, int64_t p0,
                                                               int64_t n_pairs, int64_t it0, int64_t n_items, int32_t *__restrict__ cap_col,
                                                               int32_t *__restrict__ grp_order, int32_t *__restrict__ grp_begin) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < n_pairs) {
        cap_col[j] = (int32_t)(pair_col[p0 + j] - it0 * GP_ITEM);
        grp_order[j] = (int32_t)j;
    }
    if (j <= n_items) grp_begin[j] = (int32_t)(item_begin[it0 + j] - p0);
}

// ---------------------------------------------------------------------------------------------------------------- (a) attention
struct AttnArgs {
    const float *img, *words, *gram;       // [Ni, 36, D], [n_rows, D], [Ni, 36, 36] (upper-triangular form)
    const int64_t *cap_off;
    const int32_t *pair_img, *pair_cap, *pair_len, *cap_col;      // the chunk's pairs (pair_cap < 0: not scored)
    float *P, *cn;                         // [ncols, 36], [ncols]
    int64_t n_pairs, Ni, ncols;
    int D;
};

struct AttnSmem {
    float park[GP_PAIRS][64 * SP_LDP];
    float st[GP_PAIRS][2][64];
};

__global__ __launch_bounds__(GP_THREADS) void sgraf_pair_attn_kernel(AttnArgs g) {
    extern __shared__ __attribute__((aligned(16))) char gp_smem[];
    AttnSmem &sm = *reinterpret_cast<AttnSmem *>(gp_smem);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t j = (int64_t)blockIdx.x * GP_PAIRS + wave;
    if (j >= g.n_pairs) return;                                   // (wave-uniform; no workgroup barrier below)
    const int c = __builtin_amdgcn_readfirstlane(g.pair_cap[j]);
    const int ii = __builtin_amdgcn_readfirstlane(g.pair_img[j]);
    const int W = __builtin_amdgcn_readfirstlane(g.pair_len[j]);
    const int64_t col0 = __builtin_amdgcn_readfirstlane(g.cap_col[j]);
    if (c < 0 || ii < 0 || ii >= g.Ni || W < 1 || W > GP_MAXW || col0 < 0 || col0 + W > g.ncols) return;   // P, cn stay zero
    float *pk = sm.park[wave];
    float *st0 = sm.st[wave][0];
    const float *vi = g.img + (int64_t)ii * SC_R * g.D;
    const float *ec = g.words + g.cap_off[c] * g.D;
    const int ncb = (W + 15) >> 4;
    if (ncb == 1) pair_mainloop<1>(vi, ec, W, g.D, lane, pk);
    else if (ncb == 2) pair_mainloop<2>(vi, ec, W, g.D, lane, pk);
    else if (ncb == 3) pair_mainloop<3>(vi, ec, W, g.D, lane, pk);
    else pair_mainloop<4>(vi, ec, W, g.D, lane, pk);
    __builtin_amdgcn_wave_barrier();
    // clipped_l2norm along the caption's words, per region (lane = region)
    if (lane < SC_R) {
        float s = 0.f;
        for (int w = 0; w < W; ++w) { const float b = leaky(pk[w * SP_LDP + lane]); s = fmaf(b, b, s); }
        st0[lane] = 1.f / (sqrtf(s) + 1e-8f);
    }
    __builtin_amdgcn_wave_barrier();
    // lane = word: softmax over the regions, ||ctx||^2 = e^T G e
    if (lane < W) {
        const float *G = g.gram + (int64_t)ii * (SC_R * SC_R);
        float e[SC_R];
        float mx = -INFINITY;
#pragma unroll
        for (int r = 0; r < SC_R; ++r) {
            e[r] = leaky(pk[lane * SP_LDP + r]) * st0[r] * 9.0f;
            mx = fmaxf(mx, e[r]);
        }
        float den = 0.f;
#pragma unroll
        for (int r = 0; r < SC_R; ++r) {
            e[r] = fast_exp(e[r] - mx);
            den += e[r];
        }
        float q = 0.f;
#pragma unroll
        for (int r = 0; r < SC_R; ++r) {
            float t = 0.f;
#pragma unroll
            for (int s = r; s < SC_R; ++s) t = fmaf(G[r * SC_R + s], e[s], t);
            q = fmaf(e[r], t, q);
        }
        const float rden = 1.f / den;
        q = q * rden * rden;
        const int64_t col = col0 + lane;
        f32x4 *pd = reinterpret_cast<f32x4 *>(g.P + col * SC_R);
#pragma unroll
        for (int r4 = 0; r4 < SC_R / 4; ++r4)
            pd[r4] = f32x4{e[4 * r4] * rden, e[4 * r4 + 1] * rden, e[4 * r4 + 2] * rden, e[4 * r4 + 3] * rden};
        g.cn[col] = 1.f / (sqrtf(fmaxf(q, 0.f)) + 1e-8f);
    }
}

// ---------------------------------------------------------------------------------------------------------------- (b) word rows, item-tiled
// col_src[col] = word row of column col, -1 for a column no caption owns (memset before)
__global__ __launch_bounds__(256) void sgraf_pair_colsrc_kernel(const int32_t *__restrict__ pair_cap, const int32_t *__restrict__ pair_len,
                                                                const int32_t *__restrict__ cap_col, const int64_t *__restrict__ cap_off,
                                                                int64_t n_pairs, int64_t ncols, int64_t *__restrict__ col_src) {
    const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= n_pairs) return;
    const int lane = threadIdx.x & 63;
    const int c = pair_cap[j], W = pair_len[j];
    const int64_t col = (int64_t)cap_col[j] + lane;
    if (c >= 0 && lane < W && col >= 0 && col < ncols) col_src[col] = cap_off[c] + lane;
}
// 4 columns per workgroup, one wave each
__global__ __launch_bounds__(256) void sgraf_pair_gather_kernel(const float *__restrict__ words, const int64_t *__restrict__ col_src, int64_t ncols,
                                                                int64_t n_rows, int D, float *__restrict__ wt) {
    const int64_t col = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (col >= ncols) return;
    const int lane = threadIdx.x & 63;
    const int64_t src = col_src[col];
    f32x4 *dst = reinterpret_cast<f32x4 *>(wt + col * D);
    if (src >= 0 && src < n_rows) {
        const f32x4 *s = reinterpret_cast<const f32x4 *>(words + src * D);
        for (int d = lane; d < D / 4; d += 64) dst[d] = s[d];
    } else {
        for (int d = lane; d < D / 4; d += 64) dst[d] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
}

// sim_dim != 256: A[col, d] = (cn[col] * sum_r P[col, r] V[item image][r, d] - E[col, d])^2 on the vector ALU; one workgroup per column
__global__ __launch_bounds__(256) void sgraf_pair_ctx_kernel(const float *__restrict__ P, const float *__restrict__ cn, const float *__restrict__ img,
                                                             int64_t Ni, const int32_t *__restrict__ item_img, const float *__restrict__ wt, int D,
                                                             float *__restrict__ A) {
    __shared__ float pw[SC_R];
    const int64_t col = blockIdx.x;
    int ii = item_img[col / GP_ITEM];
    ii = (ii >= 0 && ii < Ni) ? ii : 0;
    if (threadIdx.x < SC_R) pw[threadIdx.x] = P[col * SC_R + threadIdx.x] * cn[col];
    __syncthreads();
    const float *V = img + (int64_t)ii * SC_R * D;
    for (int d = threadIdx.x; d < D; d += 256) {
        float s = 0.f;
#pragma unroll 4
        for (int r = 0; r < SC_R; ++r) s = fmaf(pw[r], V[(int64_t)r * D + d], s);
        const float v = s - wt[col * D + d];
        A[col * D + d] = v * v;
    }
}

// ---------------------------------------------------------------------------------------------------------------- (c) global node
__global__ __launch_bounds__(256) void sgraf_pair_glo_kernel(const float *__restrict__ img_glo, const float *__restrict__ cap_glo,
                                                             const int32_t *__restrict__ pair_img, const int32_t *__restrict__ pair_cap, int64_t Ni,
                                                             int D, float *__restrict__ out) {
    const int64_t j = blockIdx.x;
    const int c = pair_cap[j];
    int ii = pair_img[j];
    ii = (ii >= 0 && ii < Ni) ? ii : 0;
    float *o = out + j * D;
    if (c < 0) { for (int d = threadIdx.x; d < D; d += 256) o[d] = 0.f; return; }
    const float *a = img_glo + (int64_t)ii * D, *b = cap_glo + (int64_t)c * D;
    for (int d = threadIdx.x; d < D; d += 256) { const float v = a[d] - b[d]; o[d] = v * v; }
}

// out[pair_out[p0 + j]] = the chunk's score j (NaN for a pair that was not scored)
__global__ __launch_bounds__(256) void sgraf_pair_scatter_kernel(const float *__restrict__ sc, const int32_t *__restrict__ pair_cap,
                                                                 const int32_t *__restrict__ pair_out, int64_t n_pairs, float *__restrict__ out,
                                                                 int64_t out_len) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n_pairs) return;
    const int64_t o = pair_out[j];
    if (o >= 0 && o < out_len) out[o] = pair_cap[j] >= 0 ? sc[j] : __builtin_nanf("");
}

// ---------------------------------------------------------------------------------------------------------------- workspaces
// (GpState, GpChunk and the shape check: sgraf_pairs.h)
// scratch of itr_sgraf_pairs_prepare (the global nodes' intermediates): a buffer of its own, free after the call
struct GpScratch {
    float *img_ave, *g_emb_v, *l_emb_v, *l_emb_t, *cap_ave, *g_emb_t, *WqT, *WkT;
    size_t bytes;
};
static GpScratch gp_scratch(void *base, int64_t Ni, int64_t Nc, int64_t n_rows, int D, int S, int module) {
    WsCarver c(base);
    GpScratch t{};
    t.img_ave = c.take<float>((size_t)Ni * D * 4), t.g_emb_v = c.take<float>((size_t)Ni * D * 4), t.l_emb_v = c.take<float>((size_t)Ni * SC_R * D * 4);
    t.l_emb_t = c.take<float>((size_t)n_rows * D * 4), t.cap_ave = c.take<float>((size_t)Nc * D * 4), t.g_emb_t = c.take<float>((size_t)Nc * D * 4);
    if (module == 1) t.WqT = c.take<float>((size_t)S * S * 4), t.WkT = c.take<float>((size_t)S * S * 4);
    t.bytes = c.bytes;
    return t;
}

// ---------------------------------------------------------------------------------------------------------------- stages (a)-(c) of a chunk
// shared with itr_sgraf_pair_attention (sgraf_attn.hip): both entries reach the node rows through these launches
int sgraf_pairs_nodes(const float *img, const float *words, const int64_t *cap_off, const int32_t *pair_img, const int32_t *pair_capok,
                      const int32_t *pair_len, const int32_t *pair_col, const int32_t *item_begin, const int32_t *item_img, int64_t p0,
                      int64_t n_pairs, int64_t it0, int64_t n_items, int64_t Ni, int64_t n_rows, int D, int S, const itr_sgraf_weights *w,
                      const GpState &s, const GpChunk &k, hipStream_t st) {
    int rc;
    const int64_t ncols = n_items * GP_ITEM;
    const int32_t *pimg = pair_img + p0, *pcap = pair_capok + p0, *plen = pair_len + p0;
#define GP_TRY(x) { rc = (x); if (rc != ITR_OK) return rc; }
    hipLaunchKernelGGL(sgraf_pair_index_kernel, dim3((unsigned)ceil_div(n_pairs + 1, (int64_t)256)), dim3(256), 0, st, pair_col, item_begin, p0, n_pairs,
                       it0, n_items, k.cap_col, k.grp_order, k.grp_begin);
    ITR_CHECK_LAUNCH("sgraf pairs index");
    // columns that no caption owns: zero weights, zero norm, zero word -> a defined node row nobody reads
    ITR_CHECK_HIP(hipMemsetAsync(k.P, 0, (size_t)ncols * SC_R * 4, st));
    ITR_CHECK_HIP(hipMemsetAsync(k.cn, 0, (size_t)ncols * 4, st));
    ITR_CHECK_HIP(hipMemsetAsync(k.col_src, 0xff, (size_t)ncols * 8, st));
    // (a) attention weights + context norms
    GP_TRY(allow_dynamic_lds(reinterpret_cast<const void *>(sgraf_pair_attn_kernel), sizeof(AttnSmem)));
    AttnArgs a{img, words, s.gram, cap_off, pimg, pcap, plen, k.cap_col, k.P, k.cn, n_pairs, Ni, ncols, D};
    hipLaunchKernelGGL(sgraf_pair_attn_kernel, dim3((unsigned)ceil_div(n_pairs, (int64_t)GP_PAIRS)), dim3(GP_THREADS), sizeof(AttnSmem), st, a);
    ITR_CHECK_LAUNCH("sgraf pairs attention");
    // (b) the item-tiled word rows, then the local nodes
    hipLaunchKernelGGL(sgraf_pair_colsrc_kernel, dim3((unsigned)ceil_div(n_pairs, (int64_t)4)), dim3(256), 0, st, pcap, plen, k.cap_col, cap_off, n_pairs,
                       ncols, k.col_src);
    hipLaunchKernelGGL(sgraf_pair_gather_kernel, dim3((unsigned)ceil_div(ncols, (int64_t)4)), dim3(256), 0, st, words, k.col_src, ncols, n_rows, D, k.wt);
    ITR_CHECK_LAUNCH("sgraf pairs gather");
    if (S == 256) {
        GP_TRY(sgraf_loc_items(k.P, k.cn, img, Ni, item_img + it0, k.wt, w->loc_w, w->loc_b, k.Xloc, n_items, D, st));
    } else {
        hipLaunchKernelGGL(sgraf_pair_ctx_kernel, dim3((unsigned)ncols), dim3(256), 0, st, k.P, k.cn, img, Ni, item_img + it0, k.wt, D, k.Aloc);
        ITR_CHECK_LAUNCH("sgraf pairs context");
        GP_TRY(gemm_nt(k.Aloc, D, w->loc_w, D, w->loc_b, k.Xloc, S, ncols, S, D, 0, st));
        GP_TRY(norm_rows(k.Xloc, k.Xloc, ncols, S, 1e-8f, 0, 0, st));
    }
    // (c) the global node of every pair
    hipLaunchKernelGGL(sgraf_pair_glo_kernel, dim3((unsigned)n_pairs), dim3(256), 0, st, s.img_glo, s.cap_glo, pimg, pcap, Ni, D, k.Aglo);
    ITR_CHECK_LAUNCH("sgraf pairs glo");
    GP_TRY(gemm_nt(k.Aglo, D, w->glo_w, D, w->glo_b, k.Xglo, S, n_pairs, S, D, 0, st));
    GP_TRY(norm_rows(k.Xglo, k.Xglo, n_pairs, S, 1e-8f, 0, 0, st));
#undef GP_TRY
    return ITR_OK;
}

}  // namespace itr

extern "C" size_t itr_sgraf_pairs_state_bytes(int64_t Ni, int64_t Nc, int64_t n_rows, int D, int S, int module, int sgr_step) {
    if (Ni < 0 || Nc < 0 || n_rows < 0 || D <= 0 || S <= 0) return 0;
    return itr::gp_state(nullptr, Ni, Nc, n_rows, D, S, module, sgr_step).bytes;
}

extern "C" int itr_sgraf_pairs_prepare(const float *img, const float *words, const int64_t *cap_off, const int32_t *cap_len, int64_t Ni,
                                       int64_t Nc, int64_t n_rows, int R, int D, int S, int module, int sgr_step,
                                       const itr_sgraf_weights *w, void *state, size_t state_bytes, void *scratch, size_t scratch_bytes,
                                       itr_stream_t stream) {
    using namespace itr;
    ITR_REQUIRE(img && words && cap_off && cap_len && w && state && scratch, "itr_sgraf_pairs_prepare: null pointer");
    int rc = gp_check_shape("itr_sgraf_pairs_prepare", Ni, Nc, n_rows, R, D, S, module, sgr_step);
    if (rc != ITR_OK) return rc;
    ITR_REQUIRE((reinterpret_cast<uintptr_t>(img) & 15) == 0 && (reinterpret_cast<uintptr_t>(words) & 15) == 0,
                "itr_sgraf_pairs_prepare: operands must be 16-byte aligned");
    const GpState s = gp_state(state, Ni, Nc, n_rows, D, S, module, sgr_step);
    ITR_REQUIRE(state_bytes >= s.bytes, "itr_sgraf_pairs_prepare: state buffer too small");
    const GpScratch x = gp_scratch(scratch, Ni, Nc, n_rows, D, S, module);
    ITR_REQUIRE(scratch_bytes >= x.bytes, "itr_sgraf_pairs_prepare: scratch buffer too small");
    if (Ni == 0 || Nc == 0) return ITR_OK;
    hipStream_t st = as_stream(stream);
    // cap_len 0 marks a caption that is not scored here (more than 63 words): its global vector is never read
    rc = sgraf_global_nodes(img, words, cap_off, cap_len, Ni, Nc, n_rows, D, w, x.img_ave, x.g_emb_v, x.l_emb_v, s.img_glo, x.l_emb_t, x.cap_ave,
                            x.g_emb_t, s.cap_glo, "itr_sgraf_pairs_prepare", stream);
    if (rc != ITR_OK) return rc;
    hipLaunchKernelGGL(gram_mfma_kernel, dim3((unsigned)Ni), dim3(256), 0, st, img, R, D, s.gram, 1);
    ITR_CHECK_LAUNCH("sgraf pairs gram");
    if (module == 1) {
        rc = sgraf_fold_weights(w, S, sgr_step, x.WqT, x.WkT, s.Wfold, s.vfold, st);
        if (rc != ITR_OK) return rc;
        if (gp_fused(module, S)) {
            rc = sgr_fused_pack_weights(s.Wfold, w->sgr_g_w, sgr_step, s.packed, st);
            if (rc != ITR_OK) return rc;
        }
    }
    return ITR_OK;
}

extern "C" size_t itr_sgraf_pairs_prepare_scratch_bytes(int64_t Ni, int64_t Nc, int64_t n_rows, int D, int S, int module) {
    if (Ni < 0 || Nc < 0 || n_rows < 0 || D <= 0 || S <= 0) return 0;
    return itr::gp_scratch(nullptr, Ni, Nc, n_rows, D, S, module).bytes;
}

extern "C" size_t itr_sgraf_pairs_plan_workspace_bytes(int64_t Ni) { return Ni < 0 ? 0 : itr::align256((size_t)(Ni + 1) * 4); }

extern "C" int itr_sgraf_pairs_plan(const int32_t *img_ptr, const int32_t *pair_cap, const int64_t *cap_off, const int32_t *cap_len, int64_t P,
                                    int64_t Ni, int64_t Nc, int64_t n_rows, int32_t *pair_len, int32_t *pair_col, int32_t *pair_capok,
                                    int32_t *item_begin, int32_t *item_img, int32_t *n_items_dev, void *workspace, size_t workspace_bytes,
                                    itr_stream_t stream) {
    using namespace itr;
    ITR_REQUIRE(P >= 0 && Ni >= 0 && Nc >= 0 && n_rows >= 0, "itr_sgraf_pairs_plan: bad shape");
    ITR_UNSUPPORTED(P >= 0x7fffffffLL / GP_ITEM, "itr_sgraf_pairs_plan: %lld pairs; split the lists", (long long)P);
    ITR_REQUIRE(img_ptr && cap_off && cap_len && item_begin && n_items_dev && workspace, "itr_sgraf_pairs_plan: null pointer");
    ITR_REQUIRE(P == 0 || (pair_cap && pair_len && pair_col && pair_capok && item_img), "itr_sgraf_pairs_plan: null pointer");
    ITR_REQUIRE(workspace_bytes >= itr_sgraf_pairs_plan_workspace_bytes(Ni), "itr_sgraf_pairs_plan: workspace too small");
    hipStream_t st = as_stream(stream);
    int32_t *img_items = static_cast<int32_t *>(workspace);
    const unsigned grid = (unsigned)ceil_div(Ni > 0 ? Ni : 1, (int64_t)256);
    hipLaunchKernelGGL(sgraf_pairs_plan_kernel<0>, dim3(grid), dim3(256), 0, st, img_ptr, pair_cap, cap_off, cap_len, P, Ni, Nc, n_rows, img_items,
                       pair_len, pair_col, pair_capok, item_begin, item_img);
    hipLaunchKernelGGL(sgraf_pairs_prefix_kernel, dim3(1), dim3(1024), 0, st, img_items, Ni, P, item_begin, n_items_dev);
    hipLaunchKernelGGL(sgraf_pairs_plan_kernel<1>, dim3(grid), dim3(256), 0, st, img_ptr, pair_cap, cap_off, cap_len, P, Ni, Nc, n_rows, img_items,
                       pair_len, pair_col, pair_capok, item_begin, item_img);
    ITR_CHECK_LAUNCH("sgraf pairs plan");
    return ITR_OK;
}

extern "C" size_t itr_sgraf_pair_scores_workspace_bytes(int64_t n_pairs, int64_t n_items, int D, int S, int module, int sgr_step) {
    if (n_pairs < 0 || n_items < 0 || D <= 0 || S <= 0) return 0;
    return itr::gp_chunk(nullptr, n_pairs, n_items, D, S, module, sgr_step).bytes;
}

extern "C" int itr_sgraf_pair_scores(const float *img, const float *words, const int64_t *cap_off, const int32_t *pair_img,
                                     const int32_t *pair_capok, const int32_t *pair_len, const int32_t *pair_col, const int32_t *pair_out,
                                     const int32_t *item_begin, const int32_t *item_img, int64_t p0, int64_t n_pairs, int64_t it0,
                                     int64_t n_items, int64_t Ni, int64_t Nc, int64_t n_rows, int R, int D, int S, int module, int sgr_step,
                                     const itr_sgraf_weights *w, const void *state, size_t state_bytes, float *out, int64_t out_len,
                                     void *workspace, size_t workspace_bytes, itr_stream_t stream) {
    using namespace itr;
    ITR_REQUIRE(img && words && cap_off && w && state && workspace, "itr_sgraf_pair_scores: null pointer");
    int rc = gp_check_shape("itr_sgraf_pair_scores", Ni, Nc, n_rows, R, D, S, module, sgr_step);
    if (rc != ITR_OK) return rc;
    ITR_REQUIRE(p0 >= 0 && n_pairs >= 0 && it0 >= 0 && n_items >= 0 && out_len >= 0, "itr_sgraf_pair_scores: bad range");
    ITR_REQUIRE(n_pairs == 0 || (n_items >= 1 && n_items <= n_pairs), "itr_sgraf_pair_scores: a chunk of %lld pairs cannot have %lld items",
                (long long)n_pairs, (long long)n_items);
    ITR_UNSUPPORTED(p0 + n_pairs >= 0x7fffffffLL / GP_ITEM, "itr_sgraf_pair_scores: pair index overflow; split the lists");
    ITR_REQUIRE(n_pairs == 0 || (pair_img && pair_capok && pair_len && pair_col && pair_out && item_begin && item_img && out),
                "itr_sgraf_pair_scores: null pointer");
    ITR_REQUIRE((reinterpret_cast<uintptr_t>(img) & 15) == 0 && (reinterpret_cast<uintptr_t>(words) & 15) == 0,
                "itr_sgraf_pair_scores: operands must be 16-byte aligned");
    const GpState s = gp_state(const_cast<void *>(state), Ni, Nc, n_rows, D, S, module, sgr_step);
    ITR_REQUIRE(state_bytes >= s.bytes, "itr_sgraf_pair_scores: state buffer too small");
    const GpChunk k = gp_chunk(workspace, n_pairs, n_items, D, S, module, sgr_step);
    ITR_REQUIRE(workspace_bytes >= k.bytes, "itr_sgraf_pair_scores: workspace too small");
    if (n_pairs == 0 || Ni == 0 || Nc == 0) return ITR_OK;
    hipStream_t st = as_stream(stream);
    const int64_t ncols = n_items * GP_ITEM;
    const int32_t *pcap = pair_capok + p0, *plen = pair_len + p0;
#define GP_TRY(x) { rc = (x); if (rc != ITR_OK) return rc; }
    GP_TRY(sgraf_pairs_nodes(img, words, cap_off, pair_img, pair_capok, pair_len, pair_col, item_begin, item_img, p0, n_pairs, it0, n_items, Ni, n_rows,
                             D, S, w, s, k, st));
    // SAF / SGR on the chunk as one virtual image row: caption j = pair p0 + j
    const bool fused = gp_fused(module, S);
    if (module == 1) ITR_CHECK_HIP(hipMemsetAsync(k.Yglo, 0, (size_t)n_pairs * S * 4, st));
    if (fused) {
        ITR_CHECK_HIP(hipMemsetAsync(k.fused_bad, 0, sizeof(int), st));
        GP_TRY(sgr_fused_plan_groups(k.grp_begin, k.grp_order, n_items, n_pairs, plen, k.cap_col, 0, k.fused_ws, k.fused_bad, st));
    }
    SgrafStage stg{};
    stg.Xglo = k.Xglo, stg.Xloc = k.Xloc, stg.Qloc = k.Qloc, stg.Qglo = k.Qglo, stg.Yloc = k.Yloc, stg.Yglo = k.Yglo;
    stg.cap_col = k.cap_col, stg.cap_len = plen, stg.Nc = n_pairs, stg.ncols = ncols, stg.ldg = n_pairs, stg.S = S, stg.module = module;
    stg.sgr_step = sgr_step, stg.max_len = GP_MAXW, stg.fused = fused, stg.persistent = true, stg.w = w;
    stg.Wfold = s.Wfold, stg.vfold = s.vfold, stg.fused_ws = k.fused_ws, stg.n_node_groups = n_items, stg.packed_weights = s.packed;
    GP_TRY(sgraf_pair_stage(stg, 1, k.sc, n_pairs, 0, st));
    if (fused) GP_TRY(sgr_fused_finish(k.fused_ws, n_items, n_pairs, 0, 1, k.sc, n_pairs, st));
    hipLaunchKernelGGL(sgraf_pair_scatter_kernel, dim3((unsigned)ceil_div(n_pairs, (int64_t)256)), dim3(256), 0, st, k.sc, pcap, pair_out + p0, n_pairs, out,
                       out_len);
    ITR_CHECK_LAUNCH("sgraf pairs scatter");
#undef GP_TRY
    return ITR_OK;
}
