// Shared helpers for the gfx950 kernels of libitr_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>

#include "../../include/itr_hip.h"

// The library reads no environment variable: every variant the tests cross-check against is an argument of the ABI.

namespace itr {

void set_error(const char *fmt, ...);

#define ITR_REQUIRE(cond, ...)                 \
    do {                                       \
        if (!(cond)) {                         \
            itr::set_error(__VA_ARGS__);       \
            return ITR_ERR_BADARG;             \
        }                                      \
    } while (0)

#define ITR_UNSUPPORTED(cond, ...)             \
    do {                                       \
        if (cond) {                            \
            itr::set_error(__VA_ARGS__);       \
            return ITR_ERR_UNSUPPORTED;        \
        }                                      \
    } while (0)

// Launch-error check only (no sync): the ABI just enqueues work.
#define ITR_CHECK_LAUNCH(what)                                                         \
    do {                                                                               \
        hipError_t e__ = hipGetLastError();                                            \
        if (e__ != hipSuccess) {                                                       \
            itr::set_error("%s: HIP launch failed: %s", what, hipGetErrorString(e__)); \
            return ITR_ERR_HIP;                                                        \
        }                                                                              \
    } while (0)

#define ITR_CHECK_HIP(expr)                                                           \
    do {                                                                              \
        hipError_t e__ = (expr);                                                      \
        if (e__ != hipSuccess) {                                                      \
            itr::set_error("%s failed: %s", #expr, hipGetErrorString(e__));           \
            return ITR_ERR_HIP;                                                       \
        }                                                                             \
    } while (0)

static inline hipStream_t as_stream(itr_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

static inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- wave (64-lane) reductions --------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// gelu(x) = x/2 (1 + erf(x / sqrt 2)) (bert.py:29-34) with a branch-free erf: erf(t) = 1 - 2^(-log2(e) t Q(t)) for t = min(|x| / sqrt 2, 4),
// Q a degree-7 minimax fit of -ln(erfc t) / t (tools/fit_erf.py; max |erf error| 1.2e-7 in fp32 arithmetic, the size of libm's own;
// gelu max |error| 4.6e-7 against float64 over [-8, 8] -- torch's fp32 gelu: 1.2e-6).  17 vector instructions; libm's erff is two
// polynomial branches (~40 with the divergence handling), and in a GEMM epilogue every vector instruction is paid in fp32-MFMA
// time (they share the vector ALU): 64 activations per thread and 128 x 128 tile were 10-15 % of a K = 768 tile.
__device__ __forceinline__ float gelu_erf(float x) {
    const float t = fminf(fabsf(x) * 0.70710678118654752440f, 4.0f);
    float q = 3.144048969e-05f;
    q = fmaf(q, t, -3.088049125e-04f);
    q = fmaf(q, t, 1.032412169e-03f);
    q = fmaf(q, t, 5.369114806e-04f);
    q = fmaf(q, t, -1.958393678e-02f);
    q = fmaf(q, t, 1.029196009e-01f);
    q = fmaf(q, t, 6.365977526e-01f);
    q = fmaf(q, t, 1.128380299e+00f);
    const float r = 1.0f - __builtin_amdgcn_exp2f(q * t * -1.44269504088896341f);
    const float hx = 0.5f * x;
    return fmaf(hx, copysignf(r, x), hx);
}

__device__ __forceinline__ float apply_act(float v, int act) {
    switch (act) {
        case 1: return fmaxf(v, 0.f);
        case 2: return tanhf(v);
        case 3: return 1.f / (1.f + expf(-v));
        case 4: return gelu_erf(v);
        case 5: return v > 0.f ? v : 0.1f * v;
        case 6: return v != v ? 0.f : v;      // NaN -> 0 (pdist_cos: `res[res != res] = 0`, Objectives.py:321)
        default: return v;
    }
}

// One GRU cell update, gate order (r, z, n) of torch.nn.GRU (TextEncoder.py:38-70 runs nn.GRU):
//   r = s(gi_r + gh_r); z = s(gi_z + gh_z); n = tanh(gi_n + r * gh_n); h' = (1 - z) * n + z * h
// THE definition of the evaluation forward: every gate kernel (towers.hip: the per-step kernel and the persistent recurrence) calls
// it, with explicit fmaf -- hipcc is otherwise free to contract "a * b + c * d" either way, and all forms (and with them a sharded
// and a single-process evaluation) must agree bit for bit.
__device__ __forceinline__ float gru_cell(float ir, float iz, float in, float hr, float hz, float hn, float hp) {
    const float r = 1.f / (1.f + expf(-(ir + hr)));
    const float z = 1.f / (1.f + expf(-(iz + hz)));
    const float n = tanhf(fmaf(r, hn, in));
    return fmaf(z, hp, (1.f - z) * n);
}

// Order-preserving map float -> uint32 (larger float <=> larger key).
__device__ __forceinline__ uint32_t float_order_key(float f) {
    uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

}  // namespace itr
