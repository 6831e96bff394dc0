// What the pair kernels of the SCAN candidate-list path share beside their main loop (scan_pairs.hip: scores; scan_attn.hip:
// scores with the attention maps they are aggregated from): the first normalisation of the raw block, the workspace that
// itr_scan_pairs_prepare fills, and the shape checks of the entry points.
#pragma once
#include <type_traits>

#include "scan_common.h"
#include "itr_internal.h"
#include "pair_mainloop.h"

namespace itr {

constexpr int SP_MAXW = 64;                // words per caption whose Gram matrix the workspace holds

// statistics of the first normalisation (Objectives.py:436-457) along one group, NORM a compile-time constant
template <int NORM>
struct PairNorm {
    float s0, s1;
    __device__ __forceinline__ void init() { s0 = (NORM == 2) ? -INFINITY : 0.f; s1 = 0.f; }
    __device__ __forceinline__ void pass1(float a) {
        if (NORM == 0) { const float b = leaky(a); s0 = fmaf(b, b, s0); }
        else if (NORM == 1) s0 = fmaf(a, a, s0);
        else if (NORM == 2) s0 = fmaxf(s0, a);
        else if (NORM == 5) s0 += fabsf(a);
        else if (NORM == 6) s0 += fabsf(leaky(a));
    }
    __device__ __forceinline__ void pass2(float a) { if (NORM == 2) s1 += fast_exp(a - s0); }
    __device__ __forceinline__ void finish() {
        if (NORM == 0 || NORM == 1) s0 = 1.f / (sqrtf(s0) + 1e-8f);
        else if (NORM == 5 || NORM == 6) s0 = 1.f / (s0 + 1e-8f);
        else if (NORM == 2) s1 = 1.f / s1;
    }
    static __device__ __forceinline__ float apply(float a, float t0, float t1) {
        if (NORM == 0 || NORM == 6) return leaky(a) * t0;
        if (NORM == 1 || NORM == 5) return a * t0;
        if (NORM == 2) return fast_exp(a - t0) * t1;
        if (NORM == 4) return leaky(a);
        return a;
    }
};

template <typename F>
__device__ __forceinline__ void pair_dispatch_norm(int norm, F &&f) {
    switch (norm) {
        case 0: f(std::integral_constant<int, 0>{}); break;
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 3: f(std::integral_constant<int, 3>{}); break;
        case 4: f(std::integral_constant<int, 4>{}); break;
        case 5: f(std::integral_constant<int, 5>{}); break;
        default: f(std::integral_constant<int, 6>{}); break;
    }
}

struct PairWs {
    int32_t *blk_ptr;
    float *gram, *wnorm, *vnorm, *cgram;
    int64_t *coff;
    size_t bytes;
};
static inline PairWs pair_ws(void *base, int64_t Ni, int R, int64_t n_rows, int64_t Nc, int mode) {
    WsCarver c(base);
    PairWs w{};
    w.blk_ptr = c.take<int32_t>((size_t)(Nc + 1) * 4);
    if (mode == 0) {
        w.gram = c.take<float>((size_t)Ni * R * R * 4);
        w.wnorm = c.take<float>((size_t)n_rows * 4);
    } else {
        w.vnorm = c.take<float>((size_t)Ni * R * 4);
        w.coff = c.take<int64_t>((size_t)Nc * 8);
        w.cgram = c.take<float>((size_t)n_rows * SP_MAXW * 4);
    }
    w.bytes = c.bytes;
    return w;
}

static inline int pair_check_shape(const char *who, int64_t Ni, int64_t Nc, int64_t n_rows, int R, int D, int mode) {
    ITR_REQUIRE(Ni >= 0 && Nc >= 0 && n_rows >= 0, "%s: bad shape", who);
    ITR_REQUIRE(Nc < 0x7fffffffLL && Ni < 0x7fffffffLL, "%s: index overflow", who);
    if (mode != 0 && mode != 1) { set_error("unknown cross_attn mode %d", mode); return ITR_ERR_BADARG; }
    ITR_UNSUPPORTED(R != SC_R, "%s: this build handles %d regions per image, got %d", who, SC_R, R);
    ITR_UNSUPPORTED(D <= 0 || D % SP_BK != 0, "%s: embed dim must be a multiple of %d, got %d", who, SP_BK, D);
    return ITR_OK;
}

}  // namespace itr
