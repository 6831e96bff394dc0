// Re-order top-K lists by new scores: the last step of coarse-to-fine retrieval.  A pooled model's K-list of a query (itr_topk)
// has been re-scored by the cross-attention model (itr_scan_pair_scores); the list is put into the order the reference's
// inds = np.argsort(sims[index])[::-1] (itr/metricmodule/evaluation.py:169 i2t, :209 t2i) would give those K candidates under
// the new scores -- rank_key.h: larger score first, the higher index on exact ties, -0.0 == +0.0, NaN as +inf.  A candidate listed
// twice has two equal keys: the entry that stood earlier in the coarse list stays first, so the result is one well-defined
// permutation.  Scores move as bit patterns.  One workgroup of 64 threads per list, one bitonic sort of <= 128 entries in LDS.
#include "itr_internal.h"
#include "rank_key.h"

namespace itr {

constexpr int RR_THREADS = 64;

__global__ __launch_bounds__(RR_THREADS) void rerank_lists_kernel(const int32_t *__restrict__ idx, const uint32_t *__restrict__ val, int K,
                                                                  int32_t *__restrict__ idx_out, uint32_t *__restrict__ val_out,
                                                                  int32_t *__restrict__ perm_out) {
    __shared__ unsigned long long key[ITR_TOPK_MAX];
    __shared__ int pos[ITR_TOPK_MAX];
    const int64_t base = (int64_t)blockIdx.x * K;
    int L = 1;
    while (L < K) L <<= 1;
    for (int i = threadIdx.x; i < L; i += RR_THREADS) {
        // every real key is > 0 (the smallest score key, that of -inf, is 0x007fffff): 0 marks the padding behind the list
        key[i] = i < K ? rank_key(__uint_as_float(val[base + i]), (uint32_t)idx[base + i]) : 0ull;
        pos[i] = i;
    }
    __syncthreads();
    for (int k = 2; k <= L; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < L; i += RR_THREADS) {
                const int p = i ^ j;
                if (p > i) {
                    const unsigned long long x = key[i], y = key[p];
                    const int px = pos[i], py = pos[p];
                    const bool y_first = y > x || (y == x && py < px);      // y sorts before x
                    if ((i & k) == 0 ? y_first : !y_first) { key[i] = y; key[p] = x; pos[i] = py; pos[p] = px; }
                }
            }
            __syncthreads();
        }
    for (int i = threadIdx.x; i < K; i += RR_THREADS) {
        const int o = pos[i];
        idx_out[base + i] = idx[base + o];
        val_out[base + i] = val[base + o];
        perm_out[base + i] = o;
    }
}

}  // namespace itr

extern "C" int itr_rerank_lists(const int32_t *idx, const float *val, int64_t n, int K, int32_t *idx_out, float *val_out, int32_t *perm_out,
                                itr_stream_t stream) {
    ITR_REQUIRE(K >= 1, "itr_rerank_lists: K must be >= 1, got %d", K);
    ITR_UNSUPPORTED(K > ITR_TOPK_MAX, "itr_rerank_lists: K = %d > ITR_TOPK_MAX = %d", K, ITR_TOPK_MAX);
    ITR_REQUIRE(n >= 0 && n < 0x7fffffffLL, "itr_rerank_lists: bad list count");
    if (n == 0) return ITR_OK;
    ITR_REQUIRE(idx && val && idx_out && val_out && perm_out, "itr_rerank_lists: null pointer");
    ITR_REQUIRE(idx != idx_out && val != val_out, "itr_rerank_lists: outputs must not alias the inputs");
    hipLaunchKernelGGL(itr::rerank_lists_kernel, dim3((unsigned)n), dim3(itr::RR_THREADS), 0, itr::as_stream(stream), idx,
                       reinterpret_cast<const uint32_t *>(val), K, idx_out, reinterpret_cast<uint32_t *>(val_out), perm_out);
    ITR_CHECK_LAUNCH("rerank_lists");
    return ITR_OK;
}
