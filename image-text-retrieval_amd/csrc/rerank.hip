// Re-order top-K lists by new scores: the last step of coarse-to-fine retrieval.  A pooled model's K-list of a query (itr_topk)
// has been re-scored by the cross-attention model (itr_scan_pair_scores); the list is put into the order the reference's
// inds = np.argsort(sims[index])[::-1] (itr/metricmodule/evaluation.py:169 i2t, :209 t2i) would give those K candidates under
// the new scores -- rank_key.h: larger score first, the higher index on exact ties, -0.0 == +0.0, NaN as +inf.  A candidate listed
// twice has two equal keys: the entry that stood earlier in the coarse list stays first, so the result is one well-defined
// permutation.  Scores move as bit patterns.  One workgroup of 64 threads per list, one bitonic sort of <= 128 entries in LDS.
#include "itr_internal.h"
#include "select.h"

namespace itr {

constexpr int RR_THREADS = 64;

__global__ __launch_bounds__(RR_THREADS) void rerank_lists_kernel(const int32_t *__restrict__ idx, const uint32_t *__restrict__ val, int K,
                                                                  int32_t *__restrict__ idx_out, uint32_t *__restrict__ val_out,
                                                                  int32_t *__restrict__ perm_out) {
    __shared__ unsigned long long key[ITR_TOPK_MAX];
    __shared__ int pos[ITR_TOPK_MAX];
    const int64_t base = (int64_t)blockIdx.x * K;
    const int L = next_pow2(K);
    for (int i = threadIdx.x; i < L; i += RR_THREADS) {
        key[i] = i < K ? rank_key(__uint_as_float(val[base + i]), (uint32_t)idx[base + i]) : KEY_EMPTY;      // the padding behind the list
        pos[i] = i;
    }
    __syncthreads();
    bitonic_desc<RR_THREADS>(L, 1, [&](int, int a, int b) {
        const unsigned long long x = key[a], y = key[b];
        const int px = pos[a], py = pos[b];
        if (y > x || (y == x && py < px)) { key[a] = y; key[b] = x; pos[a] = py; pos[b] = px; }      // by key, then the lower old position
    });
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
