// Score distillation: the B x B score matrix S of a pooled student (the matrix hinge.hip and infonce.hip take: row i is image i, column j
// caption j) is pulled towards the ranking distribution of a fine teacher's matrix T over the same batch, row-wise and column-wise.
// It stands next to ContrastiveLoss.forward (itr/modalmodule/Objectives.py:93-115) and replaces no line of the reference.
//     z_s = scale_s * S,  z_t = scale_t * T (one fp32 product each; scale = 1 / temperature);  T carries no gradient
//     p_row[i,:] = softmax_j z_t[i,:]     q_row[i,:] = softmax_j z_s[i,:]     p_col[:,j] = softmax_i z_t[:,j]     q_col[:,j] = softmax_i z_s[:,j]
//     KL_row[i] = sum_j p_row[i,j] (z_t[i,j] - z_s[i,j]) - (lse_t_row[i] - lse_s_row[i])          (KL_col[j] alike, over i)
//     loss = ( sum_i KL_row[i] + sum_j KL_col[j] ) / (2 B)
//     dS[i,j] = g scale_s / (2 B) ( (q_row - p_row)[i,j] + (q_col - p_col)[i,j] )
// There is NO group mask: every row and every column runs over the whole batch.  The mask of the hinge and of InfoNCE keeps the other
// captions of an image from being mined as negatives of a hard one-hot target; here the target is the teacher's distribution, and the
// teacher scores those captions highly by itself -- they become soft positives, which is what "several positives per query" asks for.
//
// The running partial of a row or column is five floats: a (max, sum) pair for z_s and a (max, sum, weighted sum) triple for z_t, the
// weighted sum accumulating exp(z_t - max_t) (z_t - z_s) and rescaled together with the sum whenever the maximum moves.  From them
//     KL = w_t / s_t - ((m_t + log s_t) - (m_s + log s_s)).
// The two log-sum-exps are the same instructions on their operands, so with T bit-equal to S at equal scales z_t - z_s is exactly 0, the
// weighted sum stays 0, the two log-sum-exps have the same bits, and loss and dS are bit-zero.  At B = 1 the cross term and the difference
// of the log-sum-exps are both the rounded z_t - z_s: loss 0, dS 0.  A partial with sum 0 is the empty set (a non-empty one has sum >= 1).
//
// Forward, one launch + a finishing workgroup, the geometry of infonce.hip.  S and T are read twice, in whole 256-byte row segments:
//   row pass     one wave per row (four rows per workgroup), lanes stride the columns, partials merged by wave shuffles;
//   column pass  a workgroup owns 64 adjacent columns and one slice of the rows: lane l keeps the partial of column c0 + l over the
//                rows of its wave, the four waves' partials are merged in LDS in wave order, the slice's partial goes to the workspace;
//   finish       one workgroup merges the slices of every column in slice order and sums the 2B terms in a fixed order in float64
//                (thread-strided partials, wave tree, waves in order).  No float atomics: two runs give the same bits.
// Backward: one launch, one wave per row, every entry of dS written once from the four saved log-sum-exp vectors, four exp per entry.
#include <cmath>

#include "itr_common.h"

// No contraction in this file: z = scale * X is ONE rounded product wherever it appears (forward and backward see the same z), and the
// student's and the teacher's log-sum-exp stay the same instruction sequence -- the bit-zero property above rests on both.
#pragma clang fp contract(off)

namespace itr {

constexpr int DST_THREADS = 256;
constexpr int DST_WAVES = DST_THREADS / 64;
constexpr int DST_COLS = 64;            // columns of a column-pass workgroup: one 256-byte row segment per wave load
constexpr int DST_MAX_SLICES = 16;
constexpr int DST_FINISH_THREADS = 1024;
constexpr int DST_FIELDS = 5;           // floats of a partial

static inline int dst_slices(int B) { return (int)(ceil_div(B, DST_COLS) < DST_MAX_SLICES ? ceil_div(B, DST_COLS) : DST_MAX_SLICES); }

struct Kl {
    float ms, ss;        // student: maximum, sum relative to it.  ss == 0: empty (then st == 0 too: both sets hold the same entries)
    float mt, st, wt;    // teacher: maximum, sum, sum weighted with z_t - z_s
};

__device__ __forceinline__ Kl kl_empty() { return Kl{0.f, 0.f, 0.f, 0.f, 0.f}; }

// the entry (z_s, z_t) joins
__device__ __forceinline__ void kl_add(Kl &a, float zs, float zt) {
    const bool empty = a.ss == 0.f;
    const float Ms = empty ? zs : fmaxf(a.ms, zs);
    const float Mt = empty ? zt : fmaxf(a.mt, zt);
    const float fs = empty ? 0.f : expf(a.ms - Ms);
    const float ft = empty ? 0.f : expf(a.mt - Mt);
    const float et = expf(zt - Mt);
    a.ss = a.ss * fs + expf(zs - Ms);
    a.st = a.st * ft + et;
    a.wt = a.wt * ft + et * (zt - zs);
    a.ms = Ms;
    a.mt = Mt;
}

// union of two partials
__device__ __forceinline__ Kl kl_merge(Kl a, Kl b) {
    if (b.ss == 0.f) return a;
    if (a.ss == 0.f) return b;
    const float Ms = fmaxf(a.ms, b.ms), Mt = fmaxf(a.mt, b.mt);
    const float fas = expf(a.ms - Ms), fbs = expf(b.ms - Ms);
    const float fat = expf(a.mt - Mt), fbt = expf(b.mt - Mt);
    return Kl{Ms, a.ss * fas + b.ss * fbs, Mt, a.st * fat + b.st * fbt, a.wt * fat + b.wt * fbt};
}

__device__ __forceinline__ Kl kl_shfl_xor(const Kl &a, int o) {
    return Kl{__shfl_xor(a.ms, o, 64), __shfl_xor(a.ss, o, 64), __shfl_xor(a.mt, o, 64), __shfl_xor(a.st, o, 64), __shfl_xor(a.wt, o, 64)};
}

// a non-empty partial -> its two log-sum-exps and its KL term
__device__ __forceinline__ float kl_term(const Kl &a, float &lse_s, float &lse_t) {
    lse_s = a.ms + logf(a.ss);
    lse_t = a.mt + logf(a.st);
    return a.wt / a.st - (lse_t - lse_s);
}

// blockIdx.x < row_blocks: rows 4 * blockIdx.x + wave.  Else column block cb and row slice sl of the column pass.
__global__ __launch_bounds__(DST_THREADS) void distill_fwd_kernel(const float *__restrict__ S, const float *__restrict__ T, int B,
                                                                  int64_t ldS, int64_t ldT, float scale_s, float scale_t,
                                                                  int row_blocks, int slices, int slice_rows,
                                                                  float *__restrict__ row_lse_s, float *__restrict__ row_lse_t,
                                                                  float *__restrict__ row_kl,       // [B]
                                                                  float *__restrict__ part) {       // [DST_FIELDS, slices, B]
    __shared__ float s_part[DST_FIELDS][DST_WAVES][DST_COLS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (blockIdx.x < (unsigned)row_blocks) {
        const int i = blockIdx.x * DST_WAVES + wave;
        if (i >= B) return;
        const float *srow = S + (int64_t)i * ldS;
        const float *trow = T + (int64_t)i * ldT;
        Kl a = kl_empty();
        for (int j = lane; j < B; j += 4 * 64) {
            // four row segments of each matrix in flight per wave
            float vs[4], vt[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int ju = j + u * 64;
                vs[u] = ju < B ? srow[ju] : 0.f;
                vt[u] = ju < B ? trow[ju] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (j + u * 64 < B) kl_add(a, scale_s * vs[u], scale_t * vt[u]);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a = kl_merge(a, kl_shfl_xor(a, o));
        if (lane == 0) {
            float ls, lt;
            row_kl[i] = kl_term(a, ls, lt);          // B >= 1 entries in every row: the sums are >= 1
            row_lse_s[i] = ls;
            row_lse_t[i] = lt;
        }
        return;
    }
    const int cblk = (blockIdx.x - row_blocks) / slices, sl = (blockIdx.x - row_blocks) % slices;
    const int c = cblk * DST_COLS + lane;
    const int r0 = sl * slice_rows, r1 = min(B, r0 + slice_rows);
    const bool live = c < B;
    Kl a = kl_empty();
    for (int r = r0 + wave; r < r1; r += 4 * DST_WAVES) {
        // four row segments of each matrix in flight per wave
        float vs[4], vt[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int ru = r + u * DST_WAVES;
            vs[u] = (live && ru < r1) ? S[(int64_t)ru * ldS + c] : 0.f;
            vt[u] = (live && ru < r1) ? T[(int64_t)ru * ldT + c] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (live && r + u * DST_WAVES < r1) kl_add(a, scale_s * vs[u], scale_t * vt[u]);
    }
    s_part[0][wave][lane] = a.ms;
    s_part[1][wave][lane] = a.ss;
    s_part[2][wave][lane] = a.mt;
    s_part[3][wave][lane] = a.st;
    s_part[4][wave][lane] = a.wt;
    __syncthreads();
    if (wave == 0 && live) {
        Kl t{s_part[0][0][lane], s_part[1][0][lane], s_part[2][0][lane], s_part[3][0][lane], s_part[4][0][lane]};
#pragma unroll
        for (int w = 1; w < DST_WAVES; ++w)
            t = kl_merge(t, Kl{s_part[0][w][lane], s_part[1][w][lane], s_part[2][w][lane], s_part[3][w][lane], s_part[4][w][lane]});
        const int64_t plane = (int64_t)slices * B, at = (int64_t)sl * B + c;
        part[0 * plane + at] = t.ms;
        part[1 * plane + at] = t.ss;
        part[2 * plane + at] = t.mt;
        part[3 * plane + at] = t.st;
        part[4 * plane + at] = t.wt;
    }
}

// one workgroup: the columns' log-sum-exps and KL terms from the slices' partials, then loss = sum of the 2B terms / (2B)
__global__ __launch_bounds__(DST_FINISH_THREADS) void distill_finish_kernel(int B, int slices, const float *__restrict__ row_kl,
                                                                            const float *__restrict__ part,
                                                                            float *__restrict__ col_lse_s, float *__restrict__ col_lse_t,
                                                                            float *__restrict__ loss) {
    __shared__ double s_acc[DST_FINISH_THREADS / 64];
    const int64_t plane = (int64_t)slices * B;
    double acc = 0.0;
    for (int c = threadIdx.x; c < B; c += DST_FINISH_THREADS) {
        // four slices' partials of the column in flight at once, merged in slice order
        Kl t = kl_empty();
        for (int s0 = 0; s0 < slices; s0 += 4) {
            Kl q[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t at = (int64_t)(s0 + u) * B + c;
                q[u] = s0 + u < slices ? Kl{part[at], part[plane + at], part[2 * plane + at], part[3 * plane + at], part[4 * plane + at]}
                                       : kl_empty();
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) t = kl_merge(t, q[u]);
        }
        float ls, lt;
        const float kl = kl_term(t, ls, lt);
        col_lse_s[c] = ls;
        col_lse_t[c] = lt;
        acc += (double)row_kl[c] + (double)kl;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) s_acc[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < DST_FINISH_THREADS / 64; ++w) t += s_acc[w];
        loss[0] = (float)(t / (2.0 * (double)B));
    }
}

// one wave per row i of dS, four rows per workgroup
__global__ __launch_bounds__(DST_THREADS) void distill_bwd_kernel(const float *__restrict__ S, const float *__restrict__ T, int B,
                                                                  int64_t ldS, int64_t ldT, float scale_s, float scale_t,
                                                                  const float *__restrict__ row_lse_s, const float *__restrict__ col_lse_s,
                                                                  const float *__restrict__ row_lse_t, const float *__restrict__ col_lse_t,
                                                                  const float *__restrict__ grad_loss, float *__restrict__ dS,
                                                                  int64_t lddS) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * DST_WAVES + (threadIdx.x >> 6);
    if (i >= B) return;
    const float coef = grad_loss[0] * (scale_s / (2.f * (float)B));
    const float rls = row_lse_s[i], rlt = row_lse_t[i];
    const float *srow = S + (int64_t)i * ldS;
    const float *trow = T + (int64_t)i * ldT;
    float *out = dS + (int64_t)i * lddS;
    for (int j = lane; j < B; j += 64) {
        const float zs = scale_s * srow[j], zt = scale_t * trow[j];
        const float row = expf(zs - rls) - expf(zt - rlt);
        const float col = expf(zs - col_lse_s[j]) - expf(zt - col_lse_t[j]);
        out[j] = coef * (row + col);
    }
}

static inline size_t dst_workspace_floats(int B) { return (size_t)DST_FIELDS * dst_slices(B) * (size_t)B + (size_t)B; }

}  // namespace itr

extern "C" size_t itr_distill_workspace_bytes(int B) {
    if (B < 1) return 0;
    return itr::dst_workspace_floats(B) * sizeof(float);
}

extern "C" int itr_distill_fwd(const float *S, const float *T, int B, int64_t ldS, int64_t ldT, float scale_s, float scale_t, float *loss,
                               float *row_lse_s, float *col_lse_s, float *row_lse_t, float *col_lse_t, void *workspace,
                               itr_stream_t stream) {
    ITR_REQUIRE(S && T && loss && row_lse_s && col_lse_s && row_lse_t && col_lse_t && workspace, "itr_distill_fwd: null pointer");
    ITR_REQUIRE(B >= 1 && ldS >= B && ldT >= B, "itr_distill_fwd: bad shape B=%d ldS=%lld ldT=%lld", B, (long long)ldS, (long long)ldT);
    ITR_REQUIRE(std::isfinite(scale_s) && scale_s > 0.f && std::isfinite(scale_t) && scale_t > 0.f,
                "itr_distill_fwd: scale (1 / temperature) must be finite and positive, got scale_s=%g scale_t=%g", (double)scale_s,
                (double)scale_t);
    hipStream_t st = itr::as_stream(stream);
    const int slices = itr::dst_slices(B);
    const int slice_rows = (int)itr::ceil_div(B, slices);
    const int row_blocks = (int)itr::ceil_div(B, itr::DST_WAVES);
    const int64_t col_blocks = itr::ceil_div(B, itr::DST_COLS) * slices;
    float *part = static_cast<float *>(workspace);
    float *row_kl = part + (int64_t)itr::DST_FIELDS * slices * B;
    hipLaunchKernelGGL(itr::distill_fwd_kernel, dim3((unsigned)(row_blocks + col_blocks)), dim3(itr::DST_THREADS), 0, st, S, T, B, ldS,
                       ldT, scale_s, scale_t, row_blocks, slices, slice_rows, row_lse_s, row_lse_t, row_kl, part);
    ITR_CHECK_LAUNCH("distill_fwd");
    hipLaunchKernelGGL(itr::distill_finish_kernel, dim3(1), dim3(itr::DST_FINISH_THREADS), 0, st, B, slices, row_kl, part, col_lse_s,
                       col_lse_t, loss);
    ITR_CHECK_LAUNCH("distill_finish");
    return ITR_OK;
}

extern "C" int itr_distill_bwd(const float *S, const float *T, int B, int64_t ldS, int64_t ldT, float scale_s, float scale_t,
                               const float *row_lse_s, const float *col_lse_s, const float *row_lse_t, const float *col_lse_t,
                               const float *grad_loss, float *dS, int64_t lddS, itr_stream_t stream) {
    ITR_REQUIRE(S && T && row_lse_s && col_lse_s && row_lse_t && col_lse_t && grad_loss && dS, "itr_distill_bwd: null pointer");
    ITR_REQUIRE(B >= 1 && ldS >= B && ldT >= B && lddS >= B, "itr_distill_bwd: bad shape B=%d ldS=%lld ldT=%lld lddS=%lld", B,
                (long long)ldS, (long long)ldT, (long long)lddS);
    ITR_REQUIRE(std::isfinite(scale_s) && scale_s > 0.f && std::isfinite(scale_t) && scale_t > 0.f,
                "itr_distill_bwd: scale (1 / temperature) must be finite and positive, got scale_s=%g scale_t=%g", (double)scale_s,
                (double)scale_t);
    hipLaunchKernelGGL(itr::distill_bwd_kernel, dim3((unsigned)itr::ceil_div(B, itr::DST_WAVES)), dim3(itr::DST_THREADS), 0,
                       itr::as_stream(stream), S, T, B, ldS, ldT, scale_s, scale_t, row_lse_s, col_lse_s, row_lse_t, col_lse_t,
                       grad_loss, dS, lddS);
    ITR_CHECK_LAUNCH("distill_bwd");
    return ITR_OK;
}
