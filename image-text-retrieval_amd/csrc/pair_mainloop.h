// The main loop of the pair kernels (scan_pairs.hip, sgraf_pairs.hip): raw dot products of ONE (image, caption) pair by one wave, both
// operands from global memory straight into MFMA fragments.
#pragma once
#include "scan_common.h"

namespace itr {

constexpr int SP_LDP = SC_R + 1;           // 37: pitch of a parked word column
constexpr int SP_BK = 16;                  // K chunk: one float4 per operand row per lane

// Raw dot products of one pair: 36 (48) region rows x NCB * 16 word columns over K = D, parked as pk[word * 37 + region].
template <int NCB>
__device__ __forceinline__ void pair_mainloop(const float *__restrict__ vi, const float *__restrict__ ec, int W, int D, int lane,
                                              float *__restrict__ pk) {
    const int fi = lane & 15, fg = lane >> 4;
    const float *ap[3], *bp[NCB];
#pragma unroll
    for (int mt = 0; mt < 3; ++mt) {
        int row = mt * 16 + fi;
        row = row < SC_R ? row : SC_R - 1;
        ap[mt] = vi + (int64_t)row * D + 4 * fg;
    }
#pragma unroll
    for (int nt = 0; nt < NCB; ++nt) {
        int w = nt * 16 + fi;
        w = w < W ? w : W - 1;                 // columns past the caption repeat its last word; the epilogue never reads them
        bp[nt] = ec + (int64_t)w * D + 4 * fg;
    }
    f32x4 acc[3][NCB];
#pragma unroll
    for (int mt = 0; mt < 3; ++mt)
#pragma unroll
        for (int nt = 0; nt < NCB; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 ac[3], bc[NCB], an[3], bn[NCB];
#pragma unroll
    for (int mt = 0; mt < 3; ++mt) ac[mt] = *reinterpret_cast<const f32x4 *>(ap[mt]);
#pragma unroll
    for (int nt = 0; nt < NCB; ++nt) bc[nt] = *reinterpret_cast<const f32x4 *>(bp[nt]);
    for (int k0 = 0; k0 < D; k0 += SP_BK) {
        const int kn = (k0 + SP_BK < D) ? k0 + SP_BK : k0;     // last chunk: a harmless re-read instead of a branch
#pragma unroll
        for (int mt = 0; mt < 3; ++mt) an[mt] = *reinterpret_cast<const f32x4 *>(ap[mt] + kn);
#pragma unroll
        for (int nt = 0; nt < NCB; ++nt) bn[nt] = *reinterpret_cast<const f32x4 *>(bp[nt] + kn);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int mt = 0; mt < 3; ++mt)
#pragma unroll
                for (int nt = 0; nt < NCB; ++nt)
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(ac[mt][j], bc[nt][j], acc[mt][nt], 0, 0, 0);
#pragma unroll
        for (int mt = 0; mt < 3; ++mt) ac[mt] = an[mt];
#pragma unroll
        for (int nt = 0; nt < NCB; ++nt) bc[nt] = bn[nt];
    }
    // accumulator q of tile (mt, nt): region mt*16 + 4 fg + q, word nt*16 + fi
#pragma unroll
    for (int mt = 0; mt < 3; ++mt)
#pragma unroll
        for (int nt = 0; nt < NCB; ++nt)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = mt * 16 + 4 * fg + q;
                if (r < SC_R) pk[(nt * 16 + fi) * SP_LDP + r] = acc[mt][nt][q];
            }
}

}  // namespace itr
