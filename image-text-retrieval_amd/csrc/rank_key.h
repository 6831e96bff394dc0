// The order of the ranker (rank.hip) and of the top-K lists (topk.hip): one definition, so that column 0 of a top-K list is the
// ranker's top-1 by construction.
#pragma once
#include "itr_internal.h"

namespace itr {

// (score, index) as ONE 64-bit key: larger score first, then the larger index -- exactly the tie rule of the counts
// (#{S_k > S_gt} + #{k > gt : S_k == S_gt} = #{key_k > key_gt}) and of the top-1 (np.argsort(...)[::-1]: the higher index wins).
// Keys of distinct elements are distinct, so the counts are those of a TOTAL order -- which is what makes i2t cheap: the best of an
// image's im_div ground-truth captions is the one with the LARGEST key, and  min_g #{key > gkey_g} = #{key > max_g gkey_g}:
// ONE compare per element instead of im_div.
// score_key canonicalises first: e + 0.0f folds -0.0 into +0.0 (equal as floats, different bit patterns) and fminf(., inf) maps NaN
// to +inf: a NaN score sorts as the LARGEST value, like np.argsort (NaN last ascending = first after [::-1]); the float64 kernels use
// the same rule.
__device__ __forceinline__ uint32_t score_key(float e) {
    const uint32_t u = __float_as_uint(fminf(e + 0.0f, INFINITY));
    return u ^ ((uint32_t)((int32_t)u >> 31) | 0x80000000u);      // = float_order_key, as three integer instructions
}
__device__ __forceinline__ unsigned long long key64(uint32_t hi, uint32_t lo) { return ((unsigned long long)hi << 32) | lo; }
__device__ __forceinline__ unsigned long long rank_key(float e, unsigned idx) { return key64(score_key(e), idx); }

// canon_f64: -0.0 -> +0.0 and NaN -> +inf (the fp32 kernels' rule, np.argsort's order); applied to every score the kernels load
__device__ __forceinline__ double canon_f64(double d) { return fmin(d + 0.0, (double)INFINITY); }
__device__ __forceinline__ unsigned long long double_order_key(double d) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(d);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

}  // namespace itr
