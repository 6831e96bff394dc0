// SCAN i2t similarity for TRAINING batches (xattn_score_i2t + func_attention + cosine_similarity,
// Objectives.py:376-417, :420-476, :10-15, under autograd): the 36 regions of an image attend over the W words of a
// caption.  Same decomposition as scan_train.hip (t2i) with the roles of regions and words exchanged -- the per-pair
// arithmetic is the one copy in scan_train_pair.h, here with context = words, query = regions:
//       A[B_i * 36, n_tok] = V E^T  (one GEMM),  H_c = E_c E_c^T  (W x W per caption),  ||v_r||
//       b = f(a);  u[r, w] = first norm of b[:, w] over the 36 REGIONS, per word      (Objectives.py:436-457, dim 2 = queryL)
//       p[r, w] = softmax_w(lambda_s u[r, w])                                         (over the caption's words)
//       num_r = sum_w p a     q_r = p_r^T H_c p_r     s_r = num_r / max(||v_r|| sqrt(q_r), 1e-8)
//       S = LSE_r(lambda_lse s_r) / lambda_lse | max | sum | mean                      (over the 36 regions)
// Backward per (image, caption) pair: dA block (disjoint), dH partial [W x W] (summed over images by itr_colsum),
// d||v_r|| partial (summed over captions by itr_colsum).  Caller:  dV = dA E + d||v|| v / ||v||,
// dE = dA^T V + (dH + dH^T) E_c.
#include "scan_train_pair.h"

namespace itr {

struct ScanI2TArgs {
    const float *A;        // [Bi*36, ldA] raw dot products
    int64_t ldA;
    const float *H;        // packed caption Grams: caption c at H + h_off[c], W_c x W_c row-major
    const int64_t *h_off;  // [Bc]
    const float *vnorm;    // [Bi*36]
    const int64_t *cap_off;
    const int32_t *cap_len;
    int64_t Bi, Bc, h_total;
    int R;                 // regions per image: 36 in every reference configuration (FIXED instantiation), 1..ST_RMAX otherwise
    int norm, agg;
    float ls, ll;
    float *S;              // [Bi, Bc]
    const float *dS;
    float *dA;             // [Bi*36, ldA]
    float *dHp;            // [Bi, h_total]     per-pair partials of dH_c
    float *dvn;            // [Bc, Bi*36]       per-pair d||v_r||
};

// the W x W caption Gram makes the pair 80 KB -> dynamic LDS
template <int RMAX>
struct I2TSmem {
    float a[RMAX][ST_MAXW + 1];    // raw
    float p[RMAX][ST_MAXW + 1];    // u, then attention weights
    float gp[RMAX][ST_MAXW + 1];   // H p_r; the backward reuses it for dp / du / da
    float g[ST_MAXW][ST_MAXW + 1]; // caption Gram
    float cn[ST_MAXW];             // first-norm statistic per word: 1/(||b|| + eps) | 1/(sum|b| + eps) | 1/sum exp
    float cs[ST_MAXW];             // ||b||, sum |b|, or the column maximum (softmax)
    float s[RMAX], num[RMAX], q[RMAX], ds[RMAX];
    float dqs[RMAX], dnums[RMAX];  // backward
};
static_assert(sizeof(I2TSmem<SC_R>) == 80784 && sizeof(I2TSmem<ST_RMAX>) == 156816, "the LDS block decides how many pairs a CU holds");

// loads the pair's block of A and the caption's Gram, then everything up to s_r
template <int RMAX, bool FIXED>
__device__ __forceinline__ void i2t_pair_forward(const ScanI2TArgs &g, I2TSmem<RMAX> &sm, int64_t i, int64_t c, int W, int64_t off) {
    const int R = FIXED ? RMAX : g.R;
    pair_load(sm.a, g.A, g.ldA, i, off, R, W);
    const float *H = g.H + g.h_off[c];
    for (int idx = threadIdx.x; idx < W * W; idx += 256) sm.g[idx / W][idx % W] = H[idx];
    __syncthreads();
    pair_forward<false>(sm, W, R, g.vnorm + i * R, g.norm, g.ls);
}

template <int RMAX, bool FIXED>
__global__ __launch_bounds__(256) void scan_train_i2t_fwd_kernel(ScanI2TArgs g) {
    extern __shared__ __attribute__((aligned(16))) char i2t_smem[];
    I2TSmem<RMAX> &sm = *reinterpret_cast<I2TSmem<RMAX> *>(i2t_smem);
    const int R = FIXED ? RMAX : g.R;
    const int64_t c = blockIdx.x, i = blockIdx.y;
    const int W = g.cap_len[c];
    i2t_pair_forward<RMAX, FIXED>(g, sm, i, c, W, g.cap_off[c]);
    if (threadIdx.x == 0) g.S[i * g.Bc + c] = pair_aggregate(sm.s, R, g.agg, g.ll);
}

template <int RMAX, bool FIXED>
__global__ __launch_bounds__(256) void scan_train_i2t_bwd_kernel(ScanI2TArgs g) {
    extern __shared__ __attribute__((aligned(16))) char i2t_smem[];
    I2TSmem<RMAX> &sm = *reinterpret_cast<I2TSmem<RMAX> *>(i2t_smem);
    const int R = FIXED ? RMAX : g.R;
    const int64_t c = blockIdx.x, i = blockIdx.y;
    const int W = g.cap_len[c];
    const int64_t off = g.cap_off[c];
    i2t_pair_forward<RMAX, FIXED>(g, sm, i, c, W, off);
    const float dS = g.dS[i * g.Bc + c];
    if (threadIdx.x == 0) pair_aggregate_bwd(sm.s, sm.ds, R, g.agg, g.ll, dS);
    __syncthreads();
    // du, then da, in place over H p (sm.gp); dnum per region has an array of its own
    pair_backward<false>(sm, sm.gp, sm.dqs, sm.dnums, W, R, g.vnorm + i * R, g.dvn + c * (g.Bi * R) + i * R, g.norm, g.ls);
    pair_store(sm.gp, g.dA, g.ldA, i, off, R, W);
    pair_gram_partial<false>(sm.p, sm.dqs, g.dHp + i * g.h_total + g.h_off[c], W, R);   // dH partial of this pair
}

// dE_c += (dH_c + dH_c^T) E_c, one workgroup per caption;  dH_c = the colsum over images of the pair partials
__global__ __launch_bounds__(256) void i2t_gram_bwd_kernel(const float *__restrict__ dH, const int64_t *__restrict__ h_off,
                                                           const int64_t *__restrict__ cap_off, const int32_t *__restrict__ cap_len,
                                                           const float *__restrict__ E, int D, float *__restrict__ dE) {
    __shared__ float dh[ST_MAXW][ST_MAXW + 1];
    const int64_t c = blockIdx.x;
    const int W = cap_len[c];
    const float *src = dH + h_off[c];
    for (int idx = threadIdx.x; idx < W * W; idx += 256) dh[idx / W][idx % W] = src[idx];
    __syncthreads();
    const float *Ec = E + cap_off[c] * (int64_t)D;
    float *dEc = dE + cap_off[c] * (int64_t)D;
    for (int d = threadIdx.x; d < D; d += 256) {
        for (int u = 0; u < W; ++u) {
            float acc = 0.f;
            for (int v = 0; v < W; ++v) acc += (dh[u][v] + dh[v][u]) * Ec[(int64_t)v * D + d];
            dEc[(int64_t)u * D + d] += acc;
        }
    }
}

// H_c = E_c E_c^T for captions of up to ST_MAXW words (the evaluation path's gram_kernel stops at 64 rows):
// one workgroup per caption, 32-wide slices of D through LDS, up to 36 (row, row) pairs per thread.
__global__ __launch_bounds__(256) void caption_gram_kernel(const float *__restrict__ E, const int64_t *__restrict__ cap_off,
                                                           const int32_t *__restrict__ cap_len, int D, float *__restrict__ H,
                                                           const int64_t *__restrict__ h_off) {
    __shared__ float xs[ST_MAXW][33];
    const int64_t c = blockIdx.x;
    const int W = cap_len[c];
    const float *x = E + cap_off[c] * (int64_t)D;
    constexpr int NP = (ST_MAXW * ST_MAXW + 255) / 256;
    float acc[NP];
#pragma unroll
    for (int e = 0; e < NP; ++e) acc[e] = 0.f;
    for (int k0 = 0; k0 < D; k0 += 32) {
        for (int idx = threadIdx.x; idx < W * 32; idx += 256) {
            const int r = idx >> 5, k = idx & 31;
            xs[r][k] = (k0 + k < D) ? x[(int64_t)r * D + k0 + k] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < NP; ++e) {
            const int pidx = threadIdx.x + 256 * e;
            if (pidx < W * W) {
                const int r1 = pidx / W, r2 = pidx % W;
                float s_ = 0.f;
#pragma unroll
                for (int k = 0; k < 32; ++k) s_ += xs[r1][k] * xs[r2][k];
                acc[e] += s_;
            }
        }
        __syncthreads();
    }
    float *out = H + h_off[c];
#pragma unroll
    for (int e = 0; e < NP; ++e) {
        const int pidx = threadIdx.x + 256 * e;
        if (pidx < W * W) out[pidx] = acc[e];
    }
}

}  // namespace itr

using namespace itr;

extern "C" int itr_scan_train_i2t_prepare(const float *V, const float *E, const int64_t *cap_off, const int32_t *cap_len, const int64_t *h_off,
                                          int64_t Bi, int64_t Bc, int R, int D, float *H, float *vnorm, itr_stream_t stream) {
    ITR_REQUIRE(V && E && cap_off && cap_len && h_off && H && vnorm, "itr_scan_train_i2t_prepare: null pointer");
    ITR_REQUIRE(Bi >= 1 && Bc >= 1 && D > 0, "itr_scan_train_i2t_prepare: bad shape");
    ITR_UNSUPPORTED(R < 1 || R > ST_RMAX, "itr_scan_train_i2t_prepare: 1..%d regions per image are supported, got %d", ST_RMAX, R);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(caption_gram_kernel, dim3((unsigned)Bc), dim3(256), 0, st, E, cap_off, cap_len, D, H, h_off);
    ITR_CHECK_LAUNCH("scan_train_i2t gram");
    hipLaunchKernelGGL(rownorm_train_kernel, dim3((unsigned)ceil_div(Bi * R, 4)), dim3(256), 0, st, V, Bi * R, D, vnorm);
    ITR_CHECK_LAUNCH("scan_train_i2t rownorm");
    return ITR_OK;
}

extern "C" int itr_scan_train_i2t_fwd(const float *A, int64_t ldA, const float *H, const int64_t *h_off, const float *vnorm,
                                      const int64_t *cap_off, const int32_t *cap_len, int64_t Bi, int64_t Bc, int64_t n_tok, int R, int D,
                                      int max_len, int norm, int agg, float lambda_softmax, float lambda_lse, float *S, itr_stream_t stream) {
    ITR_REQUIRE(A && H && h_off && vnorm && cap_off && cap_len && S, "itr_scan_train_i2t_fwd: null pointer");
    ITR_REQUIRE(ldA >= n_tok, "itr_scan_train_i2t_fwd: ldA < n_tok");
    int rc = check_train_args("itr_scan_train_i2t_fwd", Bi, Bc, n_tok, R, D, norm, agg, max_len);
    if (rc != ITR_OK) return rc;
    ScanI2TArgs g{A, ldA, H, h_off, vnorm, cap_off, cap_len, Bi, Bc, 0, R, norm, agg, lambda_softmax, lambda_lse, S, nullptr, nullptr, nullptr, nullptr};
    hipStream_t st = as_stream(stream);
    if (R == SC_R) return launch_pair<I2TSmem<SC_R>>(scan_train_i2t_fwd_kernel<SC_R, true>, "scan_train_i2t_fwd", g, st);
    if (R < SC_R) return launch_pair<I2TSmem<SC_R>>(scan_train_i2t_fwd_kernel<SC_R, false>, "scan_train_i2t_fwd", g, st);
    return launch_pair<I2TSmem<ST_RMAX>>(scan_train_i2t_fwd_kernel<ST_RMAX, false>, "scan_train_i2t_fwd", g, st);
}

extern "C" int itr_scan_train_i2t_bwd(const float *A, int64_t ldA, const float *H, const int64_t *h_off, int64_t h_total, const float *vnorm,
                                      const int64_t *cap_off, const int32_t *cap_len, int64_t Bi, int64_t Bc, int64_t n_tok, int R, int D,
                                      int max_len, int norm, int agg, float lambda_softmax, float lambda_lse, const float *dS, float *dA,
                                      float *dH_pairs, float *d_vnorm_pairs, itr_stream_t stream) {
    ITR_REQUIRE(A && H && h_off && vnorm && cap_off && cap_len && dS && dA && dH_pairs && d_vnorm_pairs, "itr_scan_train_i2t_bwd: null pointer");
    ITR_REQUIRE(ldA >= n_tok && h_total >= 1, "itr_scan_train_i2t_bwd: bad leading dimension / Gram size");
    int rc = check_train_args("itr_scan_train_i2t_bwd", Bi, Bc, n_tok, R, D, norm, agg, max_len);
    if (rc != ITR_OK) return rc;
    ScanI2TArgs g{A, ldA, H, h_off, vnorm, cap_off, cap_len, Bi, Bc, h_total, R, norm, agg, lambda_softmax, lambda_lse, nullptr, dS, dA, dH_pairs,
                  d_vnorm_pairs};
    hipStream_t st = as_stream(stream);
    if (R == SC_R) return launch_pair<I2TSmem<SC_R>>(scan_train_i2t_bwd_kernel<SC_R, true>, "scan_train_i2t_bwd", g, st);
    if (R < SC_R) return launch_pair<I2TSmem<SC_R>>(scan_train_i2t_bwd_kernel<SC_R, false>, "scan_train_i2t_bwd", g, st);
    return launch_pair<I2TSmem<ST_RMAX>>(scan_train_i2t_bwd_kernel<ST_RMAX, false>, "scan_train_i2t_bwd", g, st);
}

extern "C" int itr_scan_train_i2t_finish(const float *dH, const int64_t *h_off, const int64_t *cap_off, const int32_t *cap_len, int64_t Bc,
                                         const float *E, const float *V, const float *vnorm, const float *d_vnorm, int64_t Bi, int R, int D,
                                         float *dV, float *dE, itr_stream_t stream) {
    ITR_REQUIRE(dH && h_off && cap_off && cap_len && E && V && vnorm && d_vnorm && dV && dE, "itr_scan_train_i2t_finish: null pointer");
    ITR_REQUIRE(Bi >= 1 && Bc >= 1 && D > 0, "itr_scan_train_i2t_finish: bad shape");
    ITR_UNSUPPORTED(R < 1 || R > ST_RMAX, "itr_scan_train_i2t_finish: 1..%d regions per image are supported, got %d", ST_RMAX, R);
    ITR_UNSUPPORTED(Bi * R > 65535, "itr_scan_train_i2t_finish: at most 65535 region rows per training batch");
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(i2t_gram_bwd_kernel, dim3((unsigned)Bc), dim3(256), 0, st, dH, h_off, cap_off, cap_len, E, D, dE);
    ITR_CHECK_LAUNCH("scan_train_i2t gram_bwd");
    hipLaunchKernelGGL(rownorm_bwd_kernel, dim3((unsigned)ceil_div(D, 256), (unsigned)(Bi * R)), dim3(256), 0, st, V, vnorm, d_vnorm,
                       Bi * R, D, dV);
    ITR_CHECK_LAUNCH("scan_train_i2t vnorm_bwd");
    return ITR_OK;
}
