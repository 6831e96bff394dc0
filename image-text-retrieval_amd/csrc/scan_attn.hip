// SCAN stacked cross attention for a LIST of (image, caption) pairs, WITH the intermediates the score is aggregated from: the
// attention matrix func_attention returns (Objectives.py:421-476, attnT at :466 / :476, received by xattn_score_t2i / _i2t at
// :350 / :398), the per-word (t2i) or per-region (i2t) cosine similarities (:354 / :400, cosine_similarity :10-15) and the
// aggregated score.  scan_pairs.hip computes the same numbers and keeps all but the score in registers and LDS; this file is its
// explaining twin for the few best results of every query.
//
// Unit of work: wave = pair, four pairs per 256-thread workgroup, pairs in list order (no caption-major plan: nothing is shared
// between the waves of a workgroup, and there is no barrier across waves).  Main loop: pair_mainloop.h, as in scan_pairs.hip --
// 36 gathered region rows as three 16-row MFMA tiles against ceil(W / 16) word-column tiles, both operands from global memory
// straight into v_mfma_f32_16x16x4_f32 fragments.  A caption of 65..96 words runs the main loop twice (columns 0..63 with four
// tiles, then the remaining one or two tiles): the image rows are streamed a second time, no wider instantiation is needed, and
// every column is accumulated in the same K order as in a short caption.
//
// Epilogue (wave-local): the raw 36 x W block is parked in LDS as [word][region] (pitch 37).  The arithmetic is that of
// scan_pairs.hip statement by statement (first normalisation, softmax, Gram-form cosine), so that scores agree; in place of the
// raw value the normalised attention weight is written back to the parked block, and the block then leaves through coalesced
// vector stores (lane l: elements l, l + 64, ... of the pair's [W, 36] row-major block).
//   t2i: lane = word (two rounds above 64 words); region Gram matrix and word norms from the prepared workspace.
//   i2t: lane = region; captions of up to 64 words read their W x W Gram matrix from the prepared workspace through wave-uniform
//        addresses.  The workspace holds no Gram matrix for 65..96 words (itr_scan_pairs_prepare is given length 0 for them), so
//        for these ||ctx||^2 is summed directly over D from the attention-weighted words: 96 x D multiply-adds per lane, correct,
//        not fast, and rare (Flickr30k has a handful of such captions).
// A pair's three outputs depend on that pair alone (fixed K order, wave-local epilogue, no atomics, nothing accumulated across
// waves): the same bits in any list, order or blocking.
//
// Budgets: 256 threads, static LDS 59,904 B (4 x (96 x 37 parked floats + 2 x 96 statistics)); registers: see DESIGN.md 4.3.2.
// Index hygiene, all on the device before the first dependent load: an image or caption index out of range, a caption length
// outside 1..96, word rows outside [0, n_rows) or an output block outside its buffer make the pair's score NaN and nothing else
// of that pair is read or written.
#include "pair_epilogue.h"

namespace itr {

constexpr int SA_WAVES = 4;                // pairs (= waves) per workgroup
constexpr int SA_THREADS = SA_WAVES * 64;
constexpr int SA_MAXW = 96;                // words per caption

struct AttnArgs {
    const float *img;            // [Ni, 36, D]
    const float *words;          // [n_rows, D]
    const int64_t *cap_off;      // [Nc]
    const int32_t *cap_len;      // [Nc] true lengths, 1..96
    const int32_t *pair_img;     // [P]
    const int32_t *pair_cap;     // [P]
    const float *gram;           // t2i [Ni, 36, 36] upper-triangular form
    const float *wnorm;          // t2i [n_rows]
    const float *vnorm;          // i2t [Ni * 36]
    const float *cgram;          // i2t [sum W^2] (captions of <= 64 words)
    const int64_t *cgram_off;    // i2t [Nc]
    const int64_t *attn_ptr;     // [P + 1]
    const int64_t *row_ptr;      // [P + 1] (t2i)
    float *attn, *row_sim, *score;
    int64_t attn_len, row_len, Ni, Nc, P, n_rows;
    int D, norm, agg;
    float ls, ll;
};

struct AttnSmem {
    float park[SA_WAVES][SA_MAXW * SP_LDP];
    float st[SA_WAVES][2][SA_MAXW];
};
static_assert(sizeof(AttnSmem) <= 64 * 1024, "static LDS");

// the aggregate of scan_pairs.hip's pair_aggregate, over one or two rounds of lanes
struct AttnAgg {
    float acc;
    __device__ __forceinline__ void add(float sim, bool on, bool first, int agg, float ll) {
        const float t = agg == 1 ? (on ? sim : -INFINITY) : (on ? (agg == 0 ? fast_exp(sim * ll) : sim) : 0.f);
        acc = first ? t : (agg == 1 ? fmaxf(acc, t) : acc + t);
    }
    __device__ __forceinline__ float finish(int n, int agg, float ll) const {
        if (agg == 1) return wave_max(acc);
        float r = wave_sum(acc);
        if (agg == 0) r = fast_log(r) / ll;
        else if (agg == 3) r /= (float)n;
        return r;
    }
};

// XA 0: t2i, 1: i2t
template <int XA>
__global__ __launch_bounds__(SA_THREADS) void scan_attn_kernel(AttnArgs g) {
    __shared__ __attribute__((aligned(16))) AttnSmem sm;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t p = (int64_t)blockIdx.x * SA_WAVES + wave;
    if (p >= g.P) return;                                      // wave-uniform; the kernel has no workgroup barrier
    const int ii = __builtin_amdgcn_readfirstlane(g.pair_img[p]);
    const int c = __builtin_amdgcn_readfirstlane(g.pair_cap[p]);
    bool ok = ii >= 0 && (int64_t)ii < g.Ni && c >= 0 && (int64_t)c < g.Nc;
    int W = 0;
    int64_t w0 = 0;
    if (ok) {
        W = __builtin_amdgcn_readfirstlane(g.cap_len[c]);
        w0 = g.cap_off[c];
        ok = W >= 1 && W <= SA_MAXW && w0 >= 0 && w0 + W <= g.n_rows;
    }
    const int64_t ab = g.attn_ptr[p];
    const int64_t rb = XA == 0 ? g.row_ptr[p] : p * SC_R;
    const int n_sim = XA == 0 ? W : SC_R;
    ok = ok && ab >= 0 && ab + (int64_t)W * SC_R <= g.attn_len && rb >= 0 && rb + n_sim <= g.row_len;
    if (!ok) {
        if (lane == 0) g.score[p] = __builtin_nanf("");
        return;
    }
    float *pk = sm.park[wave];
    float *st0 = sm.st[wave][0], *st1 = sm.st[wave][1];
    {
        const float *vi = g.img + (int64_t)ii * SC_R * g.D;
        const float *ec = g.words + w0 * g.D;
        const int ncb = (W + 15) >> 4;
        if (ncb == 1) pair_mainloop<1>(vi, ec, W, g.D, lane, pk);
        else if (ncb == 2) pair_mainloop<2>(vi, ec, W, g.D, lane, pk);
        else if (ncb == 3) pair_mainloop<3>(vi, ec, W, g.D, lane, pk);
        else pair_mainloop<4>(vi, ec, W, g.D, lane, pk);
        if (ncb == 5) pair_mainloop<1>(vi, ec + (int64_t)64 * g.D, W - 64, g.D, lane, pk + 64 * SP_LDP);
        else if (ncb == 6) pair_mainloop<2>(vi, ec + (int64_t)64 * g.D, W - 64, g.D, lane, pk + 64 * SP_LDP);
    }
    __builtin_amdgcn_wave_barrier();
    float score = 0.f;
    pair_dispatch_norm(g.norm, [&](auto NC) {
        constexpr int NORM = decltype(NC)::value;
        AttnAgg ag;
        ag.acc = 0.f;
        if (XA == 0) {
            // first normalisation: along the caption's words, per region (lane = region)
            if (NORM != 3 && NORM != 4) {
                if (lane < SC_R) {
                    PairNorm<NORM> na;
                    na.init();
                    for (int w = 0; w < W; ++w) na.pass1(pk[w * SP_LDP + lane]);
                    if (NORM == 2) for (int w = 0; w < W; ++w) na.pass2(pk[w * SP_LDP + lane]);
                    na.finish();
                    st0[lane] = na.s0;
                    st1[lane] = na.s1;
                }
                __builtin_amdgcn_wave_barrier();
            }
            // lane = word: softmax over the regions, then the cosine of the word and its context in Gram form
            const float *G = g.gram + (int64_t)ii * (SC_R * SC_R);
            for (int wb = 0; wb < W; wb += 64) {
                const int w = wb + lane;
                float sim = 0.f;
                if (w < W) {
                    float a[SC_R], e[SC_R];
                    float mx = -INFINITY;
#pragma unroll
                    for (int r = 0; r < SC_R; ++r) {
                        a[r] = pk[w * SP_LDP + r];
                        const float t0 = (NORM != 3 && NORM != 4) ? st0[r] : 1.f;
                        const float t1 = (NORM == 2) ? st1[r] : 1.f;
                        e[r] = PairNorm<NORM>::apply(a[r], t0, t1) * g.ls;
                        mx = fmaxf(mx, e[r]);
                    }
                    float den = 0.f, num = 0.f;
#pragma unroll
                    for (int r = 0; r < SC_R; ++r) {
                        e[r] = fast_exp(e[r] - mx);
                        den += e[r];
                        num = fmaf(e[r], a[r], num);
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
                    const float w1 = g.wnorm[w0 + w];
                    const float w2 = sqrtf(fmaxf(q, 0.f)) * rden;
                    sim = (num * rden) / fmaxf(w1 * w2, 1e-8f);          // cosine_similarity, Objectives.py:10-15
#pragma unroll
                    for (int r = 0; r < SC_R; ++r) pk[w * SP_LDP + r] = e[r] * rden;      // the word's attention over the regions
                    g.row_sim[rb + w] = sim;
                }
                ag.add(sim, w < W, wb == 0, g.agg, g.ll);
            }
            score = ag.finish(W, g.agg, g.ll);
        } else {
            // first normalisation: along the 36 regions, per word (lane = word)
            if (NORM != 3 && NORM != 4) {
                for (int wb = 0; wb < W; wb += 64) {
                    const int w = wb + lane;
                    if (w < W) {
                        PairNorm<NORM> na;
                        na.init();
#pragma unroll
                        for (int r = 0; r < SC_R; ++r) na.pass1(pk[w * SP_LDP + r]);
                        if (NORM == 2) {
#pragma unroll
                            for (int r = 0; r < SC_R; ++r) na.pass2(pk[w * SP_LDP + r]);
                        }
                        na.finish();
                        st0[w] = na.s0;
                        st1[w] = na.s1;
                    }
                }
                __builtin_amdgcn_wave_barrier();
            }
            // lane = region: softmax over the words; the weights replace the raw scores of the lane's own row
            float sim = 0.f;
            if (lane < SC_R) {
                float mx = -INFINITY;
                for (int w = 0; w < W; ++w) {
                    const float t0 = (NORM != 3 && NORM != 4) ? st0[w] : 1.f;
                    const float t1 = (NORM == 2) ? st1[w] : 1.f;
                    mx = fmaxf(mx, PairNorm<NORM>::apply(pk[w * SP_LDP + lane], t0, t1) * g.ls);
                }
                float den = 0.f, num = 0.f;
                for (int w = 0; w < W; ++w) {
                    const float t0 = (NORM != 3 && NORM != 4) ? st0[w] : 1.f;
                    const float t1 = (NORM == 2) ? st1[w] : 1.f;
                    const float av = pk[w * SP_LDP + lane];
                    const float ev = fast_exp(PairNorm<NORM>::apply(av, t0, t1) * g.ls - mx);
                    den += ev;
                    num = fmaf(ev, av, num);
                    pk[w * SP_LDP + lane] = ev;
                }
                float q = 0.f;
                if (W <= SP_MAXW) {
                    const float *H = g.cgram + g.cgram_off[c];
                    for (int u = 0; u < W; ++u) {
                        float t = 0.f;
                        for (int v = 0; v < W; ++v) t = fmaf(H[u * W + v], pk[v * SP_LDP + lane], t);
                        q = fmaf(pk[u * SP_LDP + lane], t, q);
                    }
                } else {
                    // no Gram matrix is prepared above 64 words: ||sum_w ev[w] e_w||^2 summed over D directly
                    const float *E = g.words + w0 * g.D;
                    for (int d = 0; d < g.D; d += 4) {
                        f32x4 cx = {0.f, 0.f, 0.f, 0.f};
                        for (int v = 0; v < W; ++v) {
                            const f32x4 ev4 = *reinterpret_cast<const f32x4 *>(E + (int64_t)v * g.D + d);
                            const float pv = pk[v * SP_LDP + lane];
#pragma unroll
                            for (int j = 0; j < 4; ++j) cx[j] = fmaf(ev4[j], pv, cx[j]);
                        }
#pragma unroll
                        for (int j = 0; j < 4; ++j) q = fmaf(cx[j], cx[j], q);
                    }
                }
                const float rden = 1.f / den;
                const float w1 = g.vnorm[(int64_t)ii * SC_R + lane];
                const float w2 = sqrtf(fmaxf(q, 0.f)) * rden;
                sim = (num * rden) / fmaxf(w1 * w2, 1e-8f);
                for (int w = 0; w < W; ++w) pk[w * SP_LDP + lane] *= rden;               // the region's attention over the words
                g.row_sim[rb + lane] = sim;
            }
            ag.add(sim, lane < SC_R, true, g.agg, g.ll);
            score = ag.finish(SC_R, g.agg, g.ll);
        }
    });
    __builtin_amdgcn_wave_barrier();
    // the pair's [W, 36] block, row-major, from the lanes that read it back from the parked block
    const int n = W * SC_R;
    float *dst = g.attn + ab;
    for (int i = lane; i < n; i += 64) {
        const int w = i / SC_R, r = i - w * SC_R;
        dst[i] = pk[w * SP_LDP + r];
    }
    if (lane == 0) g.score[p] = score;
}

}  // namespace itr

extern "C" int itr_scan_pair_attention(const float *img, const float *words, const int64_t *cap_off, const int32_t *cap_len,
                                       const int32_t *pair_img, const int32_t *pair_cap, int64_t P, int64_t Ni, int64_t Nc,
                                       int64_t n_rows, int R, int D, int mode, int norm, int agg, float lambda_softmax,
                                       float lambda_lse, float *attn, const int64_t *attn_ptr, int64_t attn_len, float *row_sim,
                                       const int64_t *row_ptr, int64_t row_len, float *score, void *workspace,
                                       size_t workspace_bytes, itr_stream_t stream) {
    using namespace itr;
    ITR_REQUIRE(img && words && cap_off && cap_len && workspace, "itr_scan_pair_attention: null pointer");
    ITR_REQUIRE(P >= 0 && attn_len >= 0 && row_len >= 0, "itr_scan_pair_attention: negative size");
    ITR_REQUIRE(P == 0 || (pair_img && pair_cap && attn && attn_ptr && row_sim && row_ptr && score), "itr_scan_pair_attention: null pointer");
    const int rc = pair_check_shape("itr_scan_pair_attention", Ni, Nc, n_rows, R, D, mode);
    if (rc != ITR_OK) return rc;
    if (norm < 0 || norm > 6) { set_error("unknown first norm type: %d", norm); return ITR_ERR_BADARG; }
    if (agg < 0 || agg > 3) { set_error("unknown aggfunc: %d", agg); return ITR_ERR_BADARG; }
    ITR_UNSUPPORTED(P * SA_MAXW * SC_R >= 0x80000000LL, "itr_scan_pair_attention: %lld pairs; split the list", (long long)P);
    ITR_REQUIRE((reinterpret_cast<uintptr_t>(img) & 15) == 0 && (reinterpret_cast<uintptr_t>(words) & 15) == 0,
                "itr_scan_pair_attention: operands must be 16-byte aligned");
    const PairWs w = pair_ws(workspace, Ni, R, n_rows, Nc, mode);
    ITR_REQUIRE(workspace_bytes >= w.bytes, "itr_scan_pair_attention: workspace too small");
    if (P == 0) return ITR_OK;
    AttnArgs a{};
    a.img = img; a.words = words; a.cap_off = cap_off; a.cap_len = cap_len; a.pair_img = pair_img; a.pair_cap = pair_cap;
    a.gram = w.gram; a.wnorm = w.wnorm; a.vnorm = w.vnorm; a.cgram = w.cgram; a.cgram_off = w.coff; a.attn_ptr = attn_ptr;
    a.row_ptr = row_ptr; a.attn = attn; a.row_sim = row_sim; a.score = score; a.attn_len = attn_len; a.row_len = row_len;
    a.Ni = Ni; a.Nc = Nc; a.P = P; a.n_rows = n_rows; a.D = D; a.norm = norm; a.agg = agg; a.ls = lambda_softmax; a.ll = lambda_lse;
    hipStream_t st = as_stream(stream);
    const unsigned grid = (unsigned)ceil_div(P, SA_WAVES);
    if (mode == 0) hipLaunchKernelGGL(scan_attn_kernel<0>, dim3(grid), dim3(SA_THREADS), 0, st, a);
    else hipLaunchKernelGGL(scan_attn_kernel<1>, dim3(grid), dim3(SA_THREADS), 0, st, a);
    ITR_CHECK_LAUNCH("scan_attn");
    return ITR_OK;
}
