// What the selection and re-ordering kernels share (topk.hip, topk_fold.hip, search.hip, rerank.hip, rerank_fuse.hip): the format of
// a list entry and the one sorting network.  All of them rest on rank_key.h: keys of distinct elements are distinct, so "the K largest
// keys" is one set in one order, whoever sorts it.
#pragma once
#include "rank_key.h"

namespace itr {

// A list entry is a 64-bit key (rank_key.h) with the bits of its score beside it.  Every real key is > 0 (the smallest score key, that
// of -inf, is 0x007fffff for fp32 and 0x000fffffffffffff for fp64), so key 0 is free to mark an EMPTY entry: a list shorter than K, the
// padding behind a sort.  An empty entry has index -1 and score bits 0; the index of a set one is its key's low 32 bits.
constexpr unsigned long long KEY_EMPTY = 0ull;
__device__ __forceinline__ bool key_set(unsigned long long k) { return k != KEY_EMPTY; }
__device__ __forceinline__ uint32_t key_idx(unsigned long long k) { return (uint32_t)k; }
__device__ __forceinline__ int32_t key_index(unsigned long long k) { return key_set(k) ? (int32_t)key_idx(k) : -1; }

__device__ __forceinline__ int next_pow2(int n) { int L = 1; while (L < n) L <<= 1; return L; }

// n_seg independent descending bitonic sorts of L (a power of two) entries each, thread-strided over a workgroup of THREADS.  The
// network does not know what an entry is or where it lies: order(seg, a, b) looks at the entries at a and b of segment seg and, when
// the one at b sorts before the one at a, exchanges them (with whatever moves along).  One functor, not a compare and a swap: the
// entries are then read once, ahead of the decision, in straight-line code.  Ends on a barrier; the caller provides the one between
// filling the entries and the first stage.
template <int THREADS, class Order>
__device__ __forceinline__ void bitonic_desc(int L, int n_seg, Order order) {
    const int total = L * n_seg, sh = __builtin_ctz(L);
    for (int k = 2; k <= L; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < total; i += THREADS) {
                const int li = i & (L - 1), p = li ^ j;
                if (p > li) {                              // the lower of a pair does the compare-exchange
                    const bool desc = (li & k) == 0;       // descending here, ascending elsewhere: the direction picks the operands
                    order(i >> sh, desc ? li : p, desc ? p : li);
                }
            }
            __syncthreads();                               // a stage reads what the previous one exchanged
        }
}

}  // namespace itr
