// Ensemble reranking: fuse the scores M fine models gave the same top-K lists and re-order the lists by the fused score.  The
// fused score of an entry is the float64 mean of its member scores, accumulated in member order and divided by (double)M -- the
// reference's (sims + sims2) / 2 on float64 matrices (itr/metricmodule/evaluation.py:377-381), restricted to the listed pairs.
// The order is the one np.argsort(sims[index])[::-1] (evaluation.py:169 i2t, :209 t2i) gives those K candidates under the fused
// scores -- rank_key.h's float64 rule: larger score first, the higher index on exact ties, -0.0 == +0.0, NaN as +inf.  A candidate
// listed twice has two equal keys: the entry that stood earlier in the coarse list stays first (itr_rerank_lists' contract).
// fused_out carries the computed double unchanged (a NaN stays NaN), member scores move as bit patterns.  One workgroup of 64
// threads per list, one bitonic sort of <= 128 (key, index, position) entries in LDS; idx is a sort key only, never an address.
#include "itr_internal.h"
#include "select.h"

namespace itr {

constexpr int RF_THREADS = 64;

__global__ __launch_bounds__(RF_THREADS) void rerank_fuse_kernel(const int32_t *__restrict__ idx, const uint32_t *__restrict__ val, int M,
                                                                 int64_t n, int K, int32_t *__restrict__ idx_out,
                                                                 double *__restrict__ fused_out, uint32_t *__restrict__ val_out,
                                                                 int32_t *__restrict__ perm_out) {
    __shared__ unsigned long long key[ITR_TOPK_MAX];      // double_order_key(canon_f64(fused))
    __shared__ unsigned long long tie[ITR_TOPK_MAX];      // (index, ~position): the larger index first, then the lower position
    __shared__ double fused[ITR_TOPK_MAX];                // by OLD position
    const int64_t base = (int64_t)blockIdx.x * K;
    const int64_t plane = n * K;
    const int L = next_pow2(K);
    for (int i = threadIdx.x; i < L; i += RF_THREADS) {
        unsigned long long k = KEY_EMPTY, t = 0ull;            // the padding behind the list
        if (i < K) {
            double acc = (double)__uint_as_float(val[base + i]);
            for (int m = 1; m < M; ++m) acc += (double)__uint_as_float(val[(int64_t)m * plane + base + i]);
            const double f = acc / (double)M;
            fused[i] = f;
            k = double_order_key(canon_f64(f));
            t = key64((uint32_t)idx[base + i], ~(uint32_t)i);
        }
        key[i] = k;
        tie[i] = i < K ? t : (unsigned long long)(~(uint32_t)i);
    }
    __syncthreads();
    bitonic_desc<RF_THREADS>(L, 1, [&](int, int a, int b) {
        const unsigned long long x = key[a], y = key[b];
        const unsigned long long tx = tie[a], ty = tie[b];
        if (y > x || (y == x && ty > tx)) { key[a] = y; key[b] = x; tie[a] = ty; tie[b] = tx; }      // by key, then the larger tie word
    });
    for (int i = threadIdx.x; i < K; i += RF_THREADS) {
        const int o = (int)(~(uint32_t)tie[i]);             // old position, < K: the padding sorted behind every real entry
        idx_out[base + i] = (int32_t)(tie[i] >> 32);
        fused_out[base + i] = fused[o];
        perm_out[base + i] = o;
        if (val_out)
            for (int m = 0; m < M; ++m) val_out[(int64_t)m * plane + base + i] = val[(int64_t)m * plane + base + o];
    }
}

static bool overlaps(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    const char *pa = static_cast<const char *>(a), *pb = static_cast<const char *>(b);
    return pa < pb + b_bytes && pb < pa + a_bytes;
}

}  // namespace itr

extern "C" int itr_rerank_fuse_lists(const int32_t *idx, const float *val, int M, int64_t n, int K, int32_t *idx_out, double *fused_out,
                                     float *val_out, int32_t *perm_out, itr_stream_t stream) {
    ITR_REQUIRE(K >= 1, "itr_rerank_fuse_lists: K must be >= 1, got %d", K);
    ITR_UNSUPPORTED(K > ITR_TOPK_MAX, "itr_rerank_fuse_lists: K = %d > ITR_TOPK_MAX = %d", K, ITR_TOPK_MAX);
    ITR_REQUIRE(M >= 1, "itr_rerank_fuse_lists: M must be >= 1, got %d", M);
    ITR_UNSUPPORTED(M > ITR_RERANK_MAX_MEMBERS, "itr_rerank_fuse_lists: M = %d > ITR_RERANK_MAX_MEMBERS = %d", M, ITR_RERANK_MAX_MEMBERS);
    ITR_REQUIRE(n >= 0 && n < 0x7fffffffLL, "itr_rerank_fuse_lists: bad list count");
    if (n == 0) return ITR_OK;
    ITR_REQUIRE(idx && val && idx_out && fused_out && perm_out, "itr_rerank_fuse_lists: null pointer");
    const size_t e = (size_t)n * (size_t)K;
    const struct { const void *p; size_t bytes; } in[2] = {{idx, e * 4}, {val, e * 4 * (size_t)M}},
                                                  out[4] = {{idx_out, e * 4}, {fused_out, e * 8}, {perm_out, e * 4},
                                                            {val_out, val_out ? e * 4 * (size_t)M : 0}};
    for (const auto &o : out)
        for (const auto &i : in)
            ITR_REQUIRE(!itr::overlaps(o.p, o.bytes, i.p, i.bytes), "itr_rerank_fuse_lists: outputs must not alias the inputs");
    hipLaunchKernelGGL(itr::rerank_fuse_kernel, dim3((unsigned)n), dim3(itr::RF_THREADS), 0, itr::as_stream(stream), idx,
                       reinterpret_cast<const uint32_t *>(val), M, n, K, idx_out, fused_out, reinterpret_cast<uint32_t *>(val_out), perm_out);
    ITR_CHECK_LAUNCH("rerank_fuse_lists");
    return ITR_OK;
}
