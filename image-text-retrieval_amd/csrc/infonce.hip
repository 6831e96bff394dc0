// InfoNCE (softmax contrastive) loss on the B x B score matrix the hinge of hinge.hip takes: row i is image i, column j caption j,
// the positive is the diagonal.  It stands next to ContrastiveLoss.forward (itr/modalmodule/Objectives.py:93-115) and replaces no
// line of the reference.
//     z = scale * S (one fp32 product, scale = 1 / temperature);   A(i) = {i} u {j : group[j] != group[i]}
//     row_lse[i] = log sum_{j in A(i)} exp z[i,j]      col_lse[j] = log sum_{i in A(j)} exp z[i,j]
//     loss = ( sum_i (row_lse[i] - z[i,i]) + sum_j (col_lse[j] - z[j,j]) ) / (2 B)
//     dS[i,j] = g scale / (2 B) (exp(z[i,j] - row_lse[i]) + exp(z[i,j] - col_lse[j]) - 2 [i == j]),  0 at masked entries
// An off-diagonal entry (i, j) with group[i] == group[j] is masked (the rule of itr_hinge_groups_*): it is skipped, never fed
// into the arithmetic.  Every log-sum-exp is a running (max, sum) pair, the sum relative to the maximum; a pair with sum 0 is the
// empty set (a non-empty one has sum >= 1: its maximum adds exp(0)), so no infinity appears anywhere.
//
// Forward, one launch + a finishing workgroup.  S is read twice, both times in whole 256-byte row segments:
//   row pass     one wave per row (four rows per workgroup), lanes stride the columns, pairs merged by wave shuffles;
//   column pass  a workgroup owns 64 adjacent columns and one slice of the rows: lane l keeps the pair of column c0 + l over the
//                rows of its wave, the four waves' pairs are merged in LDS, and the slice's pairs go to the workspace;
//   finish       one workgroup of 1024 threads merges the slices of every column in slice order (col_lse) and sums the 2B terms in a
//                fixed order in float64 (thread-strided partials, wave tree, waves in order).  No float atomics: two runs give the
//                same bits.
// group == NULL and an all-distinct group vector take the same instructions in the same order, so their outputs agree bit for bit.
// Backward: one pass, one wave per row, every entry of dS written once.
#include <cmath>

#include "itr_common.h"

// No contraction in this file: z = scale * S is ONE rounded product wherever it appears.  Fused into the subtraction that follows it
// (z - max, lse - z[i,i]) it would be a different number at each site, and exp(z - max) of the maximum itself would not be exactly 1:
// B = 1 and a one-group batch would not give exactly 0, and merging two pairs would depend on their order.
#pragma clang fp contract(off)

namespace itr {

constexpr int NCE_THREADS = 256;
constexpr int NCE_WAVES = NCE_THREADS / 64;
constexpr int NCE_COLS = 64;            // columns of a column-pass workgroup: one 256-byte row segment per wave load
constexpr int NCE_MAX_SLICES = 16;
constexpr int NCE_FINISH_THREADS = 1024;

static inline int nce_slices(int B) { return (int)(ceil_div(B, NCE_COLS) < NCE_MAX_SLICES ? ceil_div(B, NCE_COLS) : NCE_MAX_SLICES); }

struct Lse {
    float m, s;          // s == 0: empty
};

// z joins the set
__device__ __forceinline__ void lse_add(Lse &a, float z) {
    const float M = a.s == 0.f ? z : fmaxf(a.m, z);
    const float old = a.s == 0.f ? 0.f : a.s * expf(a.m - M);
    a.s = old + expf(z - M);
    a.m = M;
}

// union of two sets; symmetric in its arguments, bit for bit
__device__ __forceinline__ Lse lse_merge(Lse a, Lse b) {
    if (b.s == 0.f) return a;
    if (a.s == 0.f) return b;
    const float M = fmaxf(a.m, b.m);
    return Lse{M, a.s * expf(a.m - M) + b.s * expf(b.m - M)};
}

// blockIdx.x < row_blocks: rows 4 * blockIdx.x + wave.  Else column block cb and row slice sl of the column pass.
__global__ __launch_bounds__(NCE_THREADS) void infonce_fwd_kernel(const float *__restrict__ S, const int32_t *__restrict__ group,
                                                                  int B, int64_t ldS, float scale, int row_blocks, int slices,
                                                                  int slice_rows, float *__restrict__ row_lse,
                                                                  float *__restrict__ part_m,      // [slices, B]
                                                                  float *__restrict__ part_s) {
    __shared__ float s_m[NCE_WAVES][NCE_COLS];
    __shared__ float s_s[NCE_WAVES][NCE_COLS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (blockIdx.x < (unsigned)row_blocks) {
        const int i = blockIdx.x * NCE_WAVES + wave;
        if (i >= B) return;
        const int32_t gi = group ? group[i] : 0;
        const float *row = S + (int64_t)i * ldS;
        Lse a{0.f, 0.f};
        for (int j = lane; j < B; j += 4 * 64) {
            // four row segments in flight per wave
            float v[4];
            int32_t gv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int ju = j + u * 64;
                v[u] = ju < B ? row[ju] : 0.f;
                gv[u] = (group && ju < B) ? group[ju] : 0;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int ju = j + u * 64;
                if (ju >= B) continue;
                if (group && ju != i && gv[u] == gi) continue;
                lse_add(a, scale * v[u]);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a = lse_merge(a, Lse{__shfl_xor(a.m, o, 64), __shfl_xor(a.s, o, 64)});
        if (lane == 0) row_lse[i] = a.m + logf(a.s);          // the diagonal is in every row: s >= 1
        return;
    }
    const int cblk = (blockIdx.x - row_blocks) / slices, sl = (blockIdx.x - row_blocks) % slices;
    const int c = cblk * NCE_COLS + lane;
    const int r0 = sl * slice_rows, r1 = min(B, r0 + slice_rows);
    const bool live = c < B;
    const int32_t gc = (group && live) ? group[c] : 0;
    Lse a{0.f, 0.f};
    for (int r = r0 + wave; r < r1; r += 4 * NCE_WAVES) {
        // four row segments in flight per wave
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int ru = r + u * NCE_WAVES;
            v[u] = (live && ru < r1) ? S[(int64_t)ru * ldS + c] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int ru = r + u * NCE_WAVES;
            if (!live || ru >= r1) continue;
            if (group && ru != c && group[ru] == gc) continue;
            lse_add(a, scale * v[u]);
        }
    }
    s_m[wave][lane] = a.m;
    s_s[wave][lane] = a.s;
    __syncthreads();
    if (wave == 0 && live) {
        Lse t{s_m[0][lane], s_s[0][lane]};
#pragma unroll
        for (int w = 1; w < NCE_WAVES; ++w) t = lse_merge(t, Lse{s_m[w][lane], s_s[w][lane]});
        part_m[(int64_t)sl * B + c] = t.m;
        part_s[(int64_t)sl * B + c] = t.s;
    }
}

// one workgroup: col_lse from the slices' pairs, then loss = sum of the 2B terms / (2B)
__global__ __launch_bounds__(NCE_FINISH_THREADS) void infonce_finish_kernel(const float *__restrict__ S, int B, int64_t ldS, float scale,
                                                                     int slices, const float *__restrict__ row_lse,
                                                                     const float *__restrict__ part_m,
                                                                     const float *__restrict__ part_s,
                                                                     float *__restrict__ col_lse, float *__restrict__ loss) {
    __shared__ double s_acc[NCE_FINISH_THREADS / 64];
    double acc = 0.0;
    for (int c = threadIdx.x; c < B; c += NCE_FINISH_THREADS) {
        // all slices' pairs of the column in flight at once, merged in slice order
        Lse q[NCE_MAX_SLICES];
#pragma unroll
        for (int sl = 0; sl < NCE_MAX_SLICES; ++sl)
            q[sl] = sl < slices ? Lse{part_m[(int64_t)sl * B + c], part_s[(int64_t)sl * B + c]} : Lse{0.f, 0.f};
        Lse t = q[0];
#pragma unroll
        for (int sl = 1; sl < NCE_MAX_SLICES; ++sl) t = lse_merge(t, q[sl]);
        const float cl = t.m + logf(t.s);
        col_lse[c] = cl;
        const float d = scale * S[(int64_t)c * ldS + c];
        acc += (double)(row_lse[c] - d) + (double)(cl - d);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) s_acc[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < NCE_FINISH_THREADS / 64; ++w) t += s_acc[w];
        loss[0] = (float)(t / (2.0 * (double)B));
    }
}

// one wave per row i of dS, four rows per workgroup
__global__ __launch_bounds__(NCE_THREADS) void infonce_bwd_kernel(const float *__restrict__ S, const int32_t *__restrict__ group,
                                                                  int B, int64_t ldS, float scale,
                                                                  const float *__restrict__ row_lse,
                                                                  const float *__restrict__ col_lse,
                                                                  const float *__restrict__ grad_loss, float *__restrict__ dS,
                                                                  int64_t lddS) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * NCE_WAVES + (threadIdx.x >> 6);
    if (i >= B) return;
    const float coef = grad_loss[0] * (scale / (2.f * (float)B));
    const float rl = row_lse[i];
    const int32_t gi = group ? group[i] : 0;
    const float *row = S + (int64_t)i * ldS;
    float *out = dS + (int64_t)i * lddS;
    for (int j = lane; j < B; j += 64) {
        if (group && j != i && group[j] == gi) {
            out[j] = 0.f;
            continue;
        }
        const float z = scale * row[j];
        const float p = expf(z - rl) + expf(z - col_lse[j]);
        out[j] = coef * (j == i ? p - 2.f : p);
    }
}

}  // namespace itr

extern "C" size_t itr_infonce_workspace_bytes(int B) {
    if (B < 1) return 0;
    return (size_t)2 * itr::nce_slices(B) * (size_t)B * sizeof(float);
}

extern "C" int itr_infonce_fwd(const float *S, const int32_t *group, int B, int64_t ldS, float scale, float *loss,
                               float *row_lse, float *col_lse, void *workspace, itr_stream_t stream) {
    ITR_REQUIRE(S && loss && row_lse && col_lse && workspace, "itr_infonce_fwd: null pointer");
    ITR_REQUIRE(B >= 1 && ldS >= B, "itr_infonce_fwd: bad shape B=%d ldS=%lld", B, (long long)ldS);
    ITR_REQUIRE(std::isfinite(scale) && scale > 0.f, "itr_infonce_fwd: scale (1 / temperature) must be finite and positive, got %g",
                (double)scale);
    hipStream_t st = itr::as_stream(stream);
    const int slices = itr::nce_slices(B);
    const int slice_rows = (int)itr::ceil_div(B, slices);
    const int row_blocks = (int)itr::ceil_div(B, itr::NCE_WAVES);
    const int64_t col_blocks = itr::ceil_div(B, itr::NCE_COLS) * slices;
    float *part_m = static_cast<float *>(workspace);
    float *part_s = part_m + (int64_t)slices * B;
    hipLaunchKernelGGL(itr::infonce_fwd_kernel, dim3((unsigned)(row_blocks + col_blocks)), dim3(itr::NCE_THREADS), 0, st, S, group,
                       B, ldS, scale, row_blocks, slices, slice_rows, row_lse, part_m, part_s);
    ITR_CHECK_LAUNCH("infonce_fwd");
    hipLaunchKernelGGL(itr::infonce_finish_kernel, dim3(1), dim3(itr::NCE_FINISH_THREADS), 0, st, S, B, ldS, scale, slices, row_lse,
                       part_m, part_s, col_lse, loss);
    ITR_CHECK_LAUNCH("infonce_finish");
    return ITR_OK;
}

extern "C" int itr_infonce_bwd(const float *S, const int32_t *group, int B, int64_t ldS, float scale, const float *row_lse,
                               const float *col_lse, const float *grad_loss, float *dS, int64_t lddS, itr_stream_t stream) {
    ITR_REQUIRE(S && row_lse && col_lse && grad_loss && dS, "itr_infonce_bwd: null pointer");
    ITR_REQUIRE(B >= 1 && ldS >= B && lddS >= B, "itr_infonce_bwd: bad shape B=%d ldS=%lld lddS=%lld", B, (long long)ldS,
                (long long)lddS);
    ITR_REQUIRE(std::isfinite(scale) && scale > 0.f, "itr_infonce_bwd: scale (1 / temperature) must be finite and positive, got %g",
                (double)scale);
    hipLaunchKernelGGL(itr::infonce_bwd_kernel, dim3((unsigned)itr::ceil_div(B, itr::NCE_WAVES)), dim3(itr::NCE_THREADS), 0,
                       itr::as_stream(stream), S, group, B, ldS, scale, row_lse, col_lse, grad_loss, dS, lddS);
    ITR_CHECK_LAUNCH("infonce_bwd");
    return ITR_OK;
}
