// SCAN stacked cross attention (xattn_score_t2i / xattn_score_i2t, itr/modalmodule/Objectives.py:329-476) for a LIST of
// (image, caption) pairs: the fine stage of coarse-to-fine retrieval, where a pooled model has shortlisted K candidates per
// query and only those pairs are scored.  Same arithmetic as scan_xattn.hip -- raw dot products A = V_i E_c^T with
// v_mfma_f32_16x16x4_f32 (exact fp32), the Gram-form epilogue (query . ctx = sum P A, ||ctx||^2 = P^T G P) -- but nothing
// here is dense: the work is proportional to the number of listed pairs.
//
// Unit of work: one caption x a block of SP_IMGS = 8 of the images listed for it.  The list arrives caption-major (CSR:
// cap_ptr[Nc + 1], pair_img[P], pair_out[P]); pairs_blkptr_kernel turns the per-caption counts into block offsets and every
// workgroup finds its caption by bisection (15 scalar loads at Nc = 25 000).
//
// Shape built (not the dense kernel's 4 x 36 rows x 64 zero-padded columns): a workgroup is 8 waves, WAVE ii OWNS PAIR ii of the
// block from its first load to its score.  Its A operand is the image's 36 gathered rows (img + img_idx * 36 * D) as three
// 16-row MFMA tiles (rows 36..47 repeat row 35, their results are dropped), its B operand the caption's words as NCB = ceil(W / 16)
// column tiles of 16 -- a run-time count 1..4, so a 13-word caption costs 16 columns of matrix-core work, not 64.  Both operands
// go from global memory straight into MFMA fragments (lane (fi, fg): 16 bytes at column k0 + 4 fg of row fi, the next 16-wide
// K chunk in flight while this one multiplies): no LDS and no barrier in the main loop.  The caption's rows are the same
// addresses in all 8 waves, so seven of eight reads of them are L1 / L2 hits -- that is the reuse of the caption operand; the
// gathered image rows (147 KB per pair at D = 1024) are what the kernel streams, and at NCB = 1 it waits for them, not for
// the matrix cores (12 MFMAs = 384 cycles per 3 KB per wave).
// A pair's score depends on that pair alone: the K order of its accumulation is fixed (k0 ascending, the MFMA's four k inside),
// the column tiles are independent accumulators, the epilogue is wave-local, nothing is accumulated across waves.  So a pair
// scores the same bits whatever else is listed, in whatever order, through either list direction.
//
// Epilogue (wave-local, VALU): the 36 x W raw block is parked in LDS as [word][region] (pitch 37: conflict-free for a lane per
// word and for a lane per region).  t2i: lane = word; the image's upper-triangular Gram matrix (gram_mfma_kernel, upper2) is read
// through wave-uniform addresses, 666 multiply-adds per word.  i2t: lane = region; the caption's W x W Gram
// matrix is staged once per workgroup in LDS (the only barrier of the kernel).
// Precomputed ONCE per image / caption by itr_scan_pairs_prepare, never per pair: t2i region Gram matrices and word norms,
// i2t region norms and caption Gram matrices.
//
// Budgets: 512 threads; LDS t2i 79,872 B (8 x 64 x 37 parked floats + 8 x 2 x 64 statistics), i2t 96,256 B (+ the 64 x 64 caption
// Gram).  VGPRs: t2i 152, i2t 100, no scratch -- set by the NCB = 4 body (48 accumulators + 2 x 28 operand registers, current +
// prefetched chunk) and, for t2i, the 72 registers a[36] / e[36] of the lane-per-word epilogue.  So one 8-wave workgroup per CU
// for t2i (registers) and for i2t (LDS): 2 waves per SIMD.  Bounding t2i to 128 registers for a second workgroup spills 115 of
// them; not taken.  Measured: about half of the gathered rows are L2 hits and the rest arrives at 1.6 TB/s, i.e.
// the kernel is bound by the loads it keeps in flight (occupancy, one chunk of prefetch), not by bandwidth or the matrix cores.
// Limits: R = 36, D % 16 == 0, captions of 1..64 words (cap_len 0 = "not scored here": ops routes 65..96 words elsewhere).
// Index hygiene: an image index outside [0, Ni), a caption length outside 1..64 or an output slot outside [0, out_len) is never
// dereferenced; the pair's score is NaN (bad image / length) or dropped (bad slot).
#include "pair_epilogue.h"

namespace itr {

constexpr int SP_IMGS = 8;                 // pairs (= waves) per workgroup
constexpr int SP_THREADS = SP_IMGS * 64;

struct PairArgs {
    const float *img;            // [Ni, 36, D]
    const float *words;          // [n_rows, D]
    const int64_t *cap_off;      // [Nc] first word row of caption c
    const int32_t *cap_len;      // [Nc] words of caption c (0: not scored)
    const int32_t *cap_ptr;      // [Nc + 1] CSR
    const int32_t *pair_img;     // [P]
    const int32_t *pair_out;     // [P]
    const int32_t *blk_ptr;      // [Nc + 1] first workgroup of caption c
    const float *gram;           // t2i [Ni, 36, 36] upper-triangular form
    const float *wnorm;          // t2i [n_rows]
    const float *vnorm;          // i2t [Ni * 36]
    const float *cgram;          // i2t [sum W^2]
    const int64_t *cgram_off;    // i2t [Nc]
    float *out;
    int64_t out_len, Ni, Nc, P;
    int D, norm, agg;
    float ls, ll;
};

struct PairSmem {
    float park[SP_IMGS][SP_MAXW * SP_LDP];
    float st[SP_IMGS][2][64];
};
constexpr size_t SP_LDS_T2I = sizeof(PairSmem);
constexpr size_t SP_LDS_I2T = sizeof(PairSmem) + SP_MAXW * SP_MAXW * 4;
static_assert(SP_LDS_I2T <= 160 * 1024, "a workgroup's LDS must fit one CU (one workgroup per CU in both modes: header)");

__device__ __forceinline__ float pair_aggregate(float sim, bool on, int n, int agg, float ll) {
    float r;
    if (agg == 1) {
        r = wave_max(on ? sim : -INFINITY);
    } else {
        r = wave_sum(on ? (agg == 0 ? fast_exp(sim * ll) : sim) : 0.f);
        if (agg == 0) r = fast_log(r) / ll;
        else if (agg == 3) r /= (float)n;
    }
    return r;
}

// XA 0: t2i, 1: i2t
template <int XA>
__global__ __launch_bounds__(SP_THREADS) void scan_pairs_kernel(PairArgs g) {
    extern __shared__ __attribute__((aligned(16))) char sp_smem[];
    PairSmem &sm = *reinterpret_cast<PairSmem *>(sp_smem);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = (int)blockIdx.x;
    const int Nc = (int)g.Nc;
    if (b >= g.blk_ptr[Nc]) return;                          // (workgroup-uniform: the grid is an upper bound)
    int lo = 0, hi = Nc;                                     // blk_ptr[lo] <= b < blk_ptr[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (g.blk_ptr[mid] <= b) lo = mid; else hi = mid;
    }
    const int c = lo;
    const int W = g.cap_len[c];
    const bool cap_ok = W >= 1 && W <= SP_MAXW;
    const int64_t p = (int64_t)g.cap_ptr[c] + (int64_t)(b - g.blk_ptr[c]) * SP_IMGS + wave;
    const bool have = p >= 0 && p < g.P && p < (int64_t)g.cap_ptr[c + 1];
    int ii = -1, oidx = -1;
    if (have) {
        ii = __builtin_amdgcn_readfirstlane(g.pair_img[p]);
        oidx = __builtin_amdgcn_readfirstlane(g.pair_out[p]);
    }
    const bool slot_ok = have && oidx >= 0 && (int64_t)oidx < g.out_len;
    const bool run = slot_ok && cap_ok && ii >= 0 && (int64_t)ii < g.Ni;      // wave-uniform
    float *pk = sm.park[wave];
    float *st0 = sm.st[wave][0], *st1 = sm.st[wave][1];
    const int64_t w0 = cap_ok ? g.cap_off[c] : 0;

    if (run) {
        const float *vi = g.img + (int64_t)ii * SC_R * g.D;
        const float *ec = g.words + w0 * g.D;
        const int ncb = (W + 15) >> 4;
        if (ncb == 1) pair_mainloop<1>(vi, ec, W, g.D, lane, pk);
        else if (ncb == 2) pair_mainloop<2>(vi, ec, W, g.D, lane, pk);
        else if (ncb == 3) pair_mainloop<3>(vi, ec, W, g.D, lane, pk);
        else pair_mainloop<4>(vi, ec, W, g.D, lane, pk);
    }
    float score = __builtin_nanf("");
    if (XA == 0) {
        if (run) {
            __builtin_amdgcn_wave_barrier();
            pair_dispatch_norm(g.norm, [&](auto NC) {
                constexpr int NORM = decltype(NC)::value;
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
                float sim = 0.f;
                if (lane < W) {
                    const float *G = g.gram + (int64_t)ii * (SC_R * SC_R);
                    float a[SC_R], e[SC_R];
                    float mx = -INFINITY;
#pragma unroll
                    for (int r = 0; r < SC_R; ++r) {
                        a[r] = pk[lane * SP_LDP + r];
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
                    const float w1 = g.wnorm[w0 + lane];
                    const float w2 = sqrtf(fmaxf(q, 0.f)) * rden;
                    sim = (num * rden) / fmaxf(w1 * w2, 1e-8f);          // cosine_similarity, Objectives.py:10-15
                }
                score = pair_aggregate(sim, lane < W, W, g.agg, g.ll);
            });
        }
    } else {
        float *hc = reinterpret_cast<float *>(sp_smem + sizeof(PairSmem));
        if (cap_ok) {
            const float *H = g.cgram + g.cgram_off[c];
            for (int idx = tid; idx < W * W; idx += SP_THREADS) hc[idx] = H[idx];
        }
        __syncthreads();
        if (run) {
            pair_dispatch_norm(g.norm, [&](auto NC) {
                constexpr int NORM = decltype(NC)::value;
                // first normalisation: along the 36 regions, per word (lane = word)
                if (NORM != 3 && NORM != 4) {
                    if (lane < W) {
                        PairNorm<NORM> na;
                        na.init();
#pragma unroll
                        for (int r = 0; r < SC_R; ++r) na.pass1(pk[lane * SP_LDP + r]);
                        if (NORM == 2) {
#pragma unroll
                            for (int r = 0; r < SC_R; ++r) na.pass2(pk[lane * SP_LDP + r]);
                        }
                        na.finish();
                        st0[lane] = na.s0;
                        st1[lane] = na.s1;
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
                    for (int u = 0; u < W; ++u) {
                        float t = 0.f;
                        for (int v = 0; v < W; ++v) t = fmaf(hc[u * W + v], pk[v * SP_LDP + lane], t);
                        q = fmaf(pk[u * SP_LDP + lane], t, q);
                    }
                    const float rden = 1.f / den;
                    const float w1 = g.vnorm[(int64_t)ii * SC_R + lane];
                    const float w2 = sqrtf(fmaxf(q, 0.f)) * rden;
                    sim = (num * rden) / fmaxf(w1 * w2, 1e-8f);
                }
                score = pair_aggregate(sim, lane < SC_R, SC_R, g.agg, g.ll);
            });
        }
    }
    if (slot_ok && lane == 0) g.out[oidx] = score;
}

// blk_ptr[c] = sum over c' < c of ceil(count(c') / SP_IMGS), blk_ptr[Nc] = total; single workgroup (Nc <= ~1e5).
__global__ __launch_bounds__(1024) void pairs_blkptr_kernel(const int32_t *__restrict__ cap_ptr, int64_t n, int32_t *__restrict__ blk_ptr) {
    __shared__ int part[1024];
    const int t = threadIdx.x;
    const int64_t per = (n + 1023) / 1024;
    const int64_t b = t * per < n ? t * per : n, e = (b + per < n) ? b + per : n;
    auto blocks = [&](int64_t i) {
        const int cnt = cap_ptr[i + 1] - cap_ptr[i];
        return cnt > 0 ? (cnt + SP_IMGS - 1) / SP_IMGS : 0;
    };
    int s = 0;
    for (int64_t i = b; i < e; ++i) s += blocks(i);
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        int run = 0;
        for (int i = 0; i < 1024; ++i) { const int v = part[i]; part[i] = run; run += v; }
        blk_ptr[n] = run;
    }
    __syncthreads();
    int run = part[t];
    for (int64_t i = b; i < e; ++i) { blk_ptr[i] = run; run += blocks(i); }
}

}  // namespace itr

extern "C" size_t itr_scan_pairs_workspace_bytes(int64_t Ni, int R, int64_t n_rows, int64_t Nc, int mode) {
    if (Ni < 0 || Nc < 0 || n_rows < 0 || R < 0) return 0;
    return itr::pair_ws(nullptr, Ni, R, n_rows, Nc, mode).bytes;
}

extern "C" int itr_scan_pairs_prepare(const float *img, const float *words, const int64_t *cap_off, const int32_t *cap_len, int64_t Ni,
                                      int64_t Nc, int64_t n_rows, int R, int D, int mode, void *workspace, size_t workspace_bytes,
                                      itr_stream_t stream) {
    using namespace itr;
    ITR_REQUIRE(img && words && cap_off && cap_len && workspace, "itr_scan_pairs_prepare: null pointer");
    const int rc = pair_check_shape("itr_scan_pairs_prepare", Ni, Nc, n_rows, R, D, mode);
    if (rc != ITR_OK) return rc;
    ITR_REQUIRE((reinterpret_cast<uintptr_t>(img) & 15) == 0 && (reinterpret_cast<uintptr_t>(words) & 15) == 0,
                "itr_scan_pairs_prepare: operands must be 16-byte aligned");
    const PairWs w = pair_ws(workspace, Ni, R, n_rows, Nc, mode);
    ITR_REQUIRE(workspace_bytes >= w.bytes, "itr_scan_pairs_prepare: workspace too small");
    if (Ni == 0 || Nc == 0) return ITR_OK;
    hipStream_t st = as_stream(stream);
    if (mode == 0) {
        hipLaunchKernelGGL(gram_mfma_kernel, dim3((unsigned)Ni), dim3(256), 0, st, img, R, D, w.gram, 1);
        ITR_CHECK_LAUNCH("scan pairs gram");
        if (n_rows > 0) {
            hipLaunchKernelGGL(rownorm_kernel, dim3((unsigned)ceil_div(n_rows, 4)), dim3(256), 0, st, words, n_rows, D, w.wnorm);
            ITR_CHECK_LAUNCH("scan pairs wnorm");
        }
    } else {
        hipLaunchKernelGGL(rownorm_kernel, dim3((unsigned)ceil_div(Ni * R, 4)), dim3(256), 0, st, img, Ni * R, D, w.vnorm);
        ITR_CHECK_LAUNCH("scan pairs vnorm");
        hipLaunchKernelGGL(sq_prefix_kernel, dim3(1), dim3(1024), 0, st, cap_len, Nc, w.coff);
        ITR_CHECK_LAUNCH("scan pairs cgram offsets");
        hipLaunchKernelGGL(gram_kernel, dim3((unsigned)Nc), dim3(256), 0, st, words, cap_off, cap_len, 0, D, w.cgram,
                           (const int64_t *)w.coff, 0);
        ITR_CHECK_LAUNCH("scan pairs caption gram");
    }
    return ITR_OK;
}

extern "C" int itr_scan_pair_scores(const float *img, const float *words, const int64_t *cap_off, const int32_t *cap_len,
                                    const int32_t *cap_ptr, const int32_t *pair_img, const int32_t *pair_out, int64_t P, int64_t Ni,
                                    int64_t Nc, int64_t n_rows, int R, int D, int mode, int norm, int agg, float lambda_softmax,
                                    float lambda_lse, float *out, int64_t out_len, void *workspace, size_t workspace_bytes,
                                    itr_stream_t stream) {
    using namespace itr;
    ITR_REQUIRE(img && words && cap_off && cap_len && cap_ptr && workspace, "itr_scan_pair_scores: null pointer");
    ITR_REQUIRE(P >= 0 && P < 0x7fffffffLL && out_len >= 0, "itr_scan_pair_scores: bad pair count");
    ITR_REQUIRE(P == 0 || (pair_img && pair_out && out), "itr_scan_pair_scores: null pointer");
    const int rc = pair_check_shape("itr_scan_pair_scores", Ni, Nc, n_rows, R, D, mode);
    if (rc != ITR_OK) return rc;
    if (norm < 0 || norm > 6) { set_error("unknown first norm type: %d", norm); return ITR_ERR_BADARG; }
    if (agg < 0 || agg > 3) { set_error("unknown aggfunc: %d", agg); return ITR_ERR_BADARG; }
    ITR_REQUIRE((reinterpret_cast<uintptr_t>(img) & 15) == 0 && (reinterpret_cast<uintptr_t>(words) & 15) == 0,
                "itr_scan_pair_scores: operands must be 16-byte aligned");
    const PairWs w = pair_ws(workspace, Ni, R, n_rows, Nc, mode);
    ITR_REQUIRE(workspace_bytes >= w.bytes, "itr_scan_pair_scores: workspace too small");
    if (P == 0 || Ni == 0 || Nc == 0) return ITR_OK;
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(pairs_blkptr_kernel, dim3(1), dim3(1024), 0, st, cap_ptr, Nc, w.blk_ptr);
    ITR_CHECK_LAUNCH("scan pairs block plan");
    // sum_c ceil(n_c / 8) <= P / 8 + Nc: the grid is this bound, surplus workgroups leave at once (no read-back of the total)
    const int64_t grid = P / SP_IMGS + (Nc < P ? Nc : P) + 1;
    ITR_UNSUPPORTED(grid > 0x7fffffffLL, "itr_scan_pair_scores: grid too large; split the list");
    PairArgs a{};
    a.img = img; a.words = words; a.cap_off = cap_off; a.cap_len = cap_len; a.cap_ptr = cap_ptr; a.pair_img = pair_img;
    a.pair_out = pair_out; a.blk_ptr = w.blk_ptr; a.gram = w.gram; a.wnorm = w.wnorm; a.vnorm = w.vnorm; a.cgram = w.cgram;
    a.cgram_off = w.coff; a.out = out; a.out_len = out_len; a.Ni = Ni; a.Nc = Nc; a.P = P; a.D = D; a.norm = norm; a.agg = agg;
    a.ls = lambda_softmax; a.ll = lambda_lse;
    if (mode == 0) {
        const int rc2 = allow_dynamic_lds(reinterpret_cast<const void *>(scan_pairs_kernel<0>), 160 * 1024);
        if (rc2 != ITR_OK) return rc2;
        hipLaunchKernelGGL(scan_pairs_kernel<0>, dim3((unsigned)grid), dim3(SP_THREADS), SP_LDS_T2I, st, a);
    } else {
        const int rc2 = allow_dynamic_lds(reinterpret_cast<const void *>(scan_pairs_kernel<1>), 160 * 1024);
        if (rc2 != ITR_OK) return rc2;
        hipLaunchKernelGGL(scan_pairs_kernel<1>, dim3((unsigned)grid), dim3(SP_THREADS), SP_LDS_I2T, st, a);
    }
    ITR_CHECK_LAUNCH("scan_pairs");
    return ITR_OK;
}
