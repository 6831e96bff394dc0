// The per-pair arithmetic of the SCAN training kernels, ONCE for both directions (scan_train.hip: t2i, scan_train_i2t.hip: i2t), and the
// host-side pieces the two files launch their pair kernels with.
//
// The two directions are one algorithm with the roles of regions and words exchanged.  The axis that is scored and aggregated is the
// QUERY axis (t2i: the caption's words, i2t: the image's regions), the axis attended over is the CONTEXT axis (t2i: regions, i2t: words):
//       b = f(a)                                     f: leaky(0.1) | id           (clipped_* | plain)
//       u[c, k] = first norm of b[c, :] along the query axis, per context item    (Objectives.py:436-457) | b
//       p[c, k] = softmax_c(lambda_s u[c, k])
//       num_k = sum_c p a      q_k = p_k^T Gram p_k      s_k = num_k / max(||query_k|| sqrt(q_k), 1e-8)
//       S = LSE_k(lambda_lse s_k) / lambda_lse | max | sum | mean
// Gram is the Gram matrix of the context rows (t2i: V_i V_i^T, i2t: E_c E_c^T).  Backward (dS given): ds_k -> dnum_k, dq_k, d||query_k||;
// dp = dnum a + 2 dq (Gram p);  softmax and first-norm backward to da, plus the direct path dnum p;  dGram partial = sum_k dq_k p_k p_k^T.
//
// The LDS blocks keep the [region][word] layout in BOTH directions (layout and bank behaviour are part of the speed); el<T2I>() does the
// exchange of roles.  A step takes the pair's LDS struct, which names its members alike in both files:
//       a, p, gp [R][W]   raw block, attention weights, Gram p          g [ctx][ctx]   the context Gram
//       cn, cs   [ctx]    first-norm statistics per context item       s, num, q, ds [qry]
// What differs between the directions -- where the Gram, the query norms and the partials live in memory, the backward's scratch block,
// the instantiation tables -- stays in the two .hip files.
#pragma once
#include "scan_common.h"
#include "itr_internal.h"

namespace itr {

constexpr int ST_RMAX = 100;  // regions per image the general instantiations hold (bottom-up features come as 36 fixed or 10..100 adaptive boxes)
constexpr int ST_MAXW = 96;   // words per caption: the longest Flickr30k caption has 82 tokens; 96 keeps the t2i pair in 64 KB of LDS.
                              // t2i kernels are instantiated for 32, 64 (3 workgroups per CU: every BASELINE batch) and 96.

// arr[region][word], addressed by (context item, query item)
template <bool T2I, typename Blk>
__device__ __forceinline__ auto &el(Blk &arr, int ctx, int qry) {
    if constexpr (T2I) return arr[ctx][qry];
    else return arr[qry][ctx];
}

// first norm: 0 clipped_l2norm, 1 l2norm, 2 softmax, 3 no_norm, 4 clipped, 5 l1norm, 6 clipped_l1norm
// (check_train_args admits 0..6).  Each test is a bit set over the code: written as `norm == 0 || norm == 4 || norm == 6` in a
// function of its own, the test came back as a chain of scalar branches inside the per-element loops, 2 % on both t2i pair kernels.
__device__ __forceinline__ bool norm_clips(int norm) { return (1u << 0 | 1u << 4 | 1u << 6) >> norm & 1u; }
__device__ __forceinline__ bool norm_is_l2(int norm) { return (1u << 0 | 1u << 1) >> norm & 1u; }
__device__ __forceinline__ bool norm_is_l1(int norm) { return (1u << 5 | 1u << 6) >> norm & 1u; }

// the pair's R x W block of A (or dA) <-> LDS; rows of image i, columns from `off`
template <typename Blk>
__device__ __forceinline__ void pair_load(Blk &a, const float *A, int64_t ldA, int64_t i, int64_t off, int R, int W) {
    for (int idx = threadIdx.x; idx < R * W; idx += 256) {
        const int r = idx / W, w = idx - r * W;
        a[r][w] = A[(i * R + r) * ldA + off + w];
    }
}
template <typename Blk>
__device__ __forceinline__ void pair_store(const Blk &da, float *dA, int64_t ldA, int64_t i, int64_t off, int R, int W) {
    for (int idx = threadIdx.x; idx < R * W; idx += 256) {
        const int r = idx / W, w = idx - r * W;
        dA[(i * R + r) * ldA + off + w] = da[r][w];
    }
}

// Everything up to s_k.  Called with sm.a and sm.g loaded and a barrier passed; returns with sm.{p,gp,cn,cs,s,num,q} valid.
// qnorm[k] = ||query_k||.
template <bool T2I, typename Smem>
__device__ __forceinline__ void pair_forward(Smem &sm, int n_ctx, int n_qry, const float *qnorm, int norm, float ls) {
    const int tid = threadIdx.x;
    const bool clip = norm_clips(norm), l2 = norm_is_l2(norm), l1 = norm_is_l1(norm);
    // first normalisation along the query axis, one lane per context item: u -> sm.p (Objectives.py:436-457)
    if (tid < n_ctx) {
        const int c = tid;
        float st = 0.f, mxa = -INFINITY;
        for (int k = 0; k < n_qry; ++k) {
            const float araw = el<T2I>(sm.a, c, k);
            const float b = clip ? leaky(araw) : araw;
            st += l2 ? b * b : (l1 ? fabsf(b) : 0.f);
            mxa = fmaxf(mxa, araw);
        }
        if (l2) st = sqrtf(st);
        if (norm == 2) {                            // softmax along the query axis
            st = 0.f;
            for (int k = 0; k < n_qry; ++k) st += expf(el<T2I>(sm.a, c, k) - mxa);
        }
        sm.cs[c] = norm == 2 ? mxa : st;            // l2: ||b||, l1: sum |b|, softmax: the maximum
        const float rn = (l2 || l1) ? 1.f / (st + 1e-8f) : (norm == 2 ? 1.f / st : 1.f);
        sm.cn[c] = rn;
        for (int k = 0; k < n_qry; ++k) {
            const float araw = el<T2I>(sm.a, c, k);
            el<T2I>(sm.p, c, k) = norm == 2 ? expf(araw - mxa) * rn : (clip ? leaky(araw) : araw) * rn;
        }
    }
    __syncthreads();
    if (tid < n_qry) {   // one lane per query item: softmax over the context
        const int k = tid;
        float mx = -INFINITY;
        for (int c = 0; c < n_ctx; ++c) {
            const float u = el<T2I>(sm.p, c, k) * ls;
            el<T2I>(sm.p, c, k) = u;
            mx = fmaxf(mx, u);
        }
        float den = 0.f;
        for (int c = 0; c < n_ctx; ++c) {
            const float e = expf(el<T2I>(sm.p, c, k) - mx);
            el<T2I>(sm.p, c, k) = e;
            den += e;
        }
        float num = 0.f;
        for (int c = 0; c < n_ctx; ++c) {
            const float pv = el<T2I>(sm.p, c, k) / den;
            el<T2I>(sm.p, c, k) = pv;
            num += pv * el<T2I>(sm.a, c, k);
        }
        sm.num[k] = num;
    }
    __syncthreads();
    // Gram p for every (region, word) -- one element per thread (before, the lane of a query item walked all ctx x ctx products itself:
    // a dozen active lanes of 256 for 1 296 dependent steps, most of the 0.55 + 0.97 ms the two t2i pair kernels took per step).
    // Consecutive threads take consecutive words in both directions, so the gp stores and the p (t2i) or g (i2t) loads spread over the banks.
    const int R = T2I ? n_ctx : n_qry, W = T2I ? n_qry : n_ctx;
    for (int idx = tid; idx < R * W; idx += 256) {
        const int r = idx / W, w = idx - r * W;
        const int c = T2I ? r : w, k = T2I ? w : r;
        float t = 0.f;
        for (int c2 = 0; c2 < n_ctx; ++c2) t += sm.g[c][c2] * el<T2I>(sm.p, c2, k);
        el<T2I>(sm.gp, c, k) = t;
    }
    __syncthreads();
    if (tid < n_qry) {
        const int k = tid;
        float q = 0.f;
        for (int c = 0; c < n_ctx; ++c) q += el<T2I>(sm.p, c, k) * el<T2I>(sm.gp, c, k);
        q = fmaxf(q, 0.f);
        sm.q[k] = q;
        sm.s[k] = sm.num[k] / fmaxf(qnorm[k] * sqrtf(q), 1e-8f);
    }
    __syncthreads();
}

// S of the pair from s_k (one thread)
__device__ __forceinline__ float pair_aggregate(const float *s, int n_qry, int agg, float ll) {
    float r;
    if (agg == 0) {
        float mx = -INFINITY;
        for (int k = 0; k < n_qry; ++k) mx = fmaxf(mx, s[k] * ll);
        float acc = 0.f;
        for (int k = 0; k < n_qry; ++k) acc += expf(s[k] * ll - mx);
        r = (logf(acc) + mx) / ll;
    } else if (agg == 1) {
        r = -INFINITY;
        for (int k = 0; k < n_qry; ++k) r = fmaxf(r, s[k]);
    } else {
        r = 0.f;
        for (int k = 0; k < n_qry; ++k) r += s[k];
        if (agg == 3) r /= (float)n_qry;
    }
    return r;
}
// ds_k from dS (one thread)
__device__ __forceinline__ void pair_aggregate_bwd(const float *s, float *ds, int n_qry, int agg, float ll, float dS) {
    if (agg == 0) {
        float mx = -INFINITY;
        for (int k = 0; k < n_qry; ++k) mx = fmaxf(mx, s[k] * ll);
        float acc = 0.f;
        for (int k = 0; k < n_qry; ++k) acc += expf(s[k] * ll - mx);
        for (int k = 0; k < n_qry; ++k) ds[k] = dS * expf(s[k] * ll - mx) / acc;
    } else if (agg == 1) {
        int best = 0;
        for (int k = 1; k < n_qry; ++k)
            if (s[k] > s[best]) best = k;      // torch.max: the first maximal index receives the gradient
        for (int k = 0; k < n_qry; ++k) ds[k] = (k == best) ? dS : 0.f;
    } else {
        const float kk = (agg == 3) ? dS / (float)n_qry : dS;
        for (int k = 0; k < n_qry; ++k) ds[k] = kk;
    }
}

// From sm.ds (and what pair_forward left) to the pair's dA block in `da` [R][W]; a barrier must separate it from the thread that wrote
// sm.ds.  dqs[k] receives dq_k, dnums[k] receives dnum_k, dqnorm[k] (global) receives d||query_k||.  `da` may BE sm.gp (i2t) and `dnums`
// may BE sm.num (t2i): each element is read before it is overwritten, by the same thread.
template <bool T2I, typename Smem, typename Blk>
__device__ __forceinline__ void pair_backward(Smem &sm, Blk &da, float *dqs, float *dnums, int n_ctx, int n_qry, const float *qnorm, float *dqnorm,
                                              int norm, float ls) {
    const int tid = threadIdx.x;
    const bool clip = norm_clips(norm), l2 = norm_is_l2(norm), l1 = norm_is_l1(norm);
    // ---- per query item: cosine backward, attention backward through the softmax -> du (kept in da)
    if (tid < n_qry) {
        const int k = tid;
        const float qn = qnorm[k];
        const float sq = sqrtf(sm.q[k]);
        const float den = qn * sq;
        float dnum = 0.f, dq = 0.f, dqn = 0.f;
        if (den > 1e-8f) {   // the clamp of cosine_similarity is inactive
            dnum = sm.ds[k] / den;
            const float dden = -sm.ds[k] * sm.num[k] / (den * den);
            dqn = dden * sq;
            dq = sq > 0.f ? dden * qn / (2.f * sq) : 0.f;
        } else {
            dnum = sm.ds[k] / 1e-8f;
        }
        dqs[k] = dq;
        dqnorm[k] = dqn;
        // dp = dnum a + 2 dq (Gram p);  du = ls * p (dp - sum_c p dp)
        float dot = 0.f;
        for (int c = 0; c < n_ctx; ++c) {
            const float dp = dnum * el<T2I>(sm.a, c, k) + 2.f * dq * el<T2I>(sm.gp, c, k);
            el<T2I>(da, c, k) = dp;
            dot += el<T2I>(sm.p, c, k) * dp;
        }
        for (int c = 0; c < n_ctx; ++c) el<T2I>(da, c, k) = ls * el<T2I>(sm.p, c, k) * (el<T2I>(da, c, k) - dot);   // = du
        dnums[k] = dnum;
    }
    __syncthreads();
    // ---- per context item: first-norm backward  u = b * cn,  cn = 1 / (sqrt(sum b^2) + eps)
    if (tid < n_ctx) {
        const int c = tid;
        const float rn = sm.cn[c], rt = sm.cs[c];
        // dot = sum_k du u-like term of the normalisation's Jacobian
        float dot = 0.f;
        for (int k = 0; k < n_qry; ++k) {
            const float araw = el<T2I>(sm.a, c, k);
            const float b = clip ? leaky(araw) : araw;
            if (l2 || l1) dot += el<T2I>(da, c, k) * b;
            else if (norm == 2) dot += el<T2I>(da, c, k) * expf(araw - rt) * rn;      // du . u
        }
        for (int k = 0; k < n_qry; ++k) {
            const float araw = el<T2I>(sm.a, c, k);
            const float b = clip ? leaky(araw) : araw;
            const float du = el<T2I>(da, c, k);
            float db;
            if (l2) db = du * rn - (rt > 0.f ? b * dot * rn * rn / rt : 0.f);                           // u = b / (||b|| + eps)
            else if (l1) db = du * rn - (b > 0.f ? 1.f : (b < 0.f ? -1.f : 0.f)) * dot * rn * rn;       // u = b / (sum |b| + eps)
            else if (norm == 2) { const float u = expf(araw - rt) * rn; db = u * (du - dot); }                // u = softmax(a)
            else db = du;
            if (clip) db *= (araw > 0.f) ? 1.f : 0.1f;    // LeakyReLU(0.1); slope at exactly 0 = 0.1 like torch
            el<T2I>(da, c, k) = db + dnums[k] * el<T2I>(sm.p, c, k);       // + the direct path of num = sum_c p a
        }
    }
    __syncthreads();
}

// dGram partial of this pair, [ctx x ctx] row-major at `out`:  sum_k dq_k p_k p_k^T
template <bool T2I, typename Blk>
__device__ __forceinline__ void pair_gram_partial(const Blk &p, const float *dqs, float *out, int n_ctx, int n_qry) {
    for (int idx = threadIdx.x; idx < n_ctx * n_ctx; idx += 256) {
        const int u = idx / n_ctx, v = idx - u * n_ctx;
        float acc = 0.f;
        for (int k = 0; k < n_qry; ++k) acc += dqs[k] * el<T2I>(p, u, k) * el<T2I>(p, v, k);
        out[idx] = acc;
    }
}

static int check_train_args(const char *who, int64_t Bi, int64_t Bc, int64_t n_tok, int R, int D, int norm, int agg, int max_len) {
    ITR_REQUIRE(Bi >= 1 && Bc >= 1 && n_tok >= 1 && D > 0, "%s: bad shape", who);
    ITR_UNSUPPORTED(R < 1 || R > ST_RMAX, "%s: 1..%d regions per image are supported, got %d", who, ST_RMAX, R);
    ITR_UNSUPPORTED(max_len > ST_MAXW, "%s: captions of at most %d words are supported, got %d", who, ST_MAXW, max_len);
    ITR_REQUIRE(norm >= 0 && norm <= 6, "%s: unknown first norm %d", who, norm);
    ITR_REQUIRE(agg >= 0 && agg <= 3, "%s: unknown aggregation %d", who, agg);
    ITR_UNSUPPORTED(Bi > 65535, "%s: at most 65535 images per training batch", who);
    return ITR_OK;
}

// One launch of a pair kernel instantiation, one workgroup per (caption, image), with its LDS block as dynamic shared memory (the
// general-R ones need up to 159 KB: more than the 64 KB a static declaration may have).
template <typename Smem, typename Args>
static int launch_pair(void (*kernel)(Args), const char *what, const Args &g, hipStream_t st) {
    static_assert(sizeof(Smem) <= 160 * 1024, "a pair's LDS block must fit one CU");
    const int rc = allow_dynamic_lds(reinterpret_cast<const void *>(kernel), sizeof(Smem));
    if (rc != ITR_OK) return rc;
    hipLaunchKernelGGL(kernel, dim3((unsigned)g.Bc, (unsigned)g.Bi), dim3(256), sizeof(Smem), st, g);
    ITR_CHECK_LAUNCH(what);
    return ITR_OK;
}

}  // namespace itr
