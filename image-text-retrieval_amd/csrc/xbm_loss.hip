// Cross-batch memory (XBM): the hinge of hinge.hip and the InfoNCE loss of infonce.hip on batch u memory.  The step's B x B matrix
// S (image i vs caption j) is joined by R [B, n] (image i vs memory caption k) and C [n, B] (memory image k vs caption j); the
// memory holds detached embeddings of earlier steps, so it only adds negatives.  Replaces no line of the reference.
//     row i's candidates: S[i, :] then R[i, :]  (index t in [0, B + n): t < B in-batch, else memory slot t - B)
//     col j's candidates: S[:, j] then C[:, j]
//     dropped (no negative, never fed into the arithmetic, gradient bit-zero):
//         S (i, j), i != j:  mask_batch && group[i] == group[j]          (the rule of itr_hinge_groups_*)
//         R (i, k):          group[i] == bank_group[k]                    (always: a stored caption of the query's own image)
//         C (k, j):          bank_group[k] == group[j]
//     hinge     cost = max(0, (margin + s) - d), d = S[q, q]; sum form: all costs; max form: largest cost per row and per column
//     InfoNCE   z = scale * s (one rounded product: no contraction in this file), log-sum-exp over the kept candidates as a running
//               (max, sum) pair, loss = (sum_i (row_lse[i] - z[i,i]) + sum_j (col_lse[j] - z[j,j])) / (2 B)
//
// Forward, one launch + a finishing workgroup (the layout of infonce.hip; n is 10-100 x B, so the column side has B + n rows):
//   row pass     one wave per row i (four rows per workgroup): lanes stride the B + n contiguous candidates, eight row segments in
//                flight, partials merged by wave shuffles;
//   column pass  a workgroup owns 64 adjacent columns and one slice of the B + n candidate rows: every wave reads whole 256-byte row
//                segments, lane l keeps the partial of column c0 + l, the four waves' partials are merged in LDS in wave order and go
//                to the workspace.  xbm_geom() picks the slice count so that the column pass alone fills the chip at B = 128;
//   finish       one workgroup of 1024 threads merges every column's slices in slice order and sums the 2B terms in float64 in a
//                fixed order.  No float atomics: two runs give the same bits.
// A partial is (cost sum, violator count), (largest cost, its index) or (max, sum of exp).  In the SUM form of the hinge row_arg /
// col_arg carry the violator counts: the diagonal's gradient is -g (row_arg[i] + col_arg[i]), and the backward needs no second walk
// over R and C.
// Backward: one launch, one thread per entry of dS | dR (flat over B x (B + n)) and of dC (flat over n x B), every entry written
// once, zeros included; the mask is checked again, so arg vectors that name a dropped entry still give it no gradient.
#include <climits>
#include <cmath>

#include "itr_common.h"

#pragma clang fp contract(off)

namespace itr {

constexpr int XBM_THREADS = 256;
constexpr int XBM_WAVES = XBM_THREADS / 64;
constexpr int XBM_COLS = 64;              // columns of a column-pass workgroup: one 256-byte row segment per wave load
constexpr int XBM_MAX_SLICES = 128;
constexpr int XBM_TARGET_WGS = 512;       // two column-pass workgroups for each of the 256 CUs
constexpr int XBM_MIN_SLICE_ROWS = 16;    // one round of four loads in flight for each of the four waves
constexpr int XBM_ROW_UNROLL = 8;
constexpr int XBM_FINISH_THREADS = 1024;
constexpr int XBM_BWD_UNROLL = 4;
constexpr int XBM_BWD_PER_BLOCK = XBM_THREADS * XBM_BWD_UNROLL;

enum { XBM_SUM = 0, XBM_MAX = 1, XBM_NCE = 2 };

struct XbmGeom {
    int slices, slice_rows;
};

// slices = min(128, ceil(512 / column groups), ceil((B + n) / 16)), then rounded so that no slice is empty
static inline XbmGeom xbm_geom(int B, int n) {
    const int64_t T = (int64_t)B + n;
    int64_t s = ceil_div(XBM_TARGET_WGS, ceil_div(B, XBM_COLS));
    if (s > XBM_MAX_SLICES) s = XBM_MAX_SLICES;
    if (s > ceil_div(T, XBM_MIN_SLICE_ROWS)) s = ceil_div(T, XBM_MIN_SLICE_ROWS);
    if (s < 1) s = 1;
    const int64_t rows = ceil_div(T, s);
    return XbmGeom{(int)ceil_div(T, rows), (int)rows};
}

// SUM: x cost sum, k violators.  MAX: x largest cost, k its index.  NCE: x running maximum, y sum of exp relative to it (0: empty).
struct XbmAcc {
    float x, y;
    int k;
};

template <int MODE>
__device__ __forceinline__ XbmAcc xbm_init() {
    return XbmAcc{0.f, 0.f, MODE == XBM_MAX ? INT_MAX : 0};
}

// candidate t with score v joins.  p: margin (hinge) or scale (InfoNCE); d: the positive's score (hinge)
template <int MODE>
__device__ __forceinline__ void xbm_add(XbmAcc &a, float v, int t, bool diag, float p, float d) {
    if (MODE == XBM_NCE) {
        const float z = p * v;
        const float M = a.y == 0.f ? z : fmaxf(a.x, z);
        const float old = a.y == 0.f ? 0.f : a.y * expf(a.x - M);
        a.y = old + expf(z - M);
        a.x = M;
        return;
    }
    const float c = diag ? 0.f : fmaxf((p + v) - d, 0.f);
    if (MODE == XBM_SUM) {
        a.x += c;
        a.k += c > 0.f ? 1 : 0;
    } else if (c > a.x || (c == a.x && t < a.k)) {      // larger cost wins; on equal costs the earlier candidate
        a.x = c;
        a.k = t;
    }
}

template <int MODE>
__device__ __forceinline__ XbmAcc xbm_merge(XbmAcc a, XbmAcc b) {
    if (MODE == XBM_SUM) return XbmAcc{a.x + b.x, 0.f, a.k + b.k};
    if (MODE == XBM_MAX) return (b.x > a.x || (b.x == a.x && b.k < a.k)) ? b : a;
    if (b.y == 0.f) return a;
    if (a.y == 0.f) return b;
    const float M = fmaxf(a.x, b.x);
    return XbmAcc{M, a.y * expf(a.x - M) + b.y * expf(b.x - M), 0};
}

// blockIdx.x < row_blocks: rows 4 * blockIdx.x + wave.  Else column group cblk and slice sl of the column pass.
template <int MODE>
__global__ __launch_bounds__(XBM_THREADS) void xbm_fwd_kernel(const float *__restrict__ S, int64_t ldS, const float *__restrict__ R,
                                                              int64_t ldR, const float *__restrict__ C, int64_t ldC,
                                                              const int32_t *__restrict__ group,
                                                              const int32_t *__restrict__ bank_group, int B, int n, int mask_batch,
                                                              float p, int row_blocks, int slices, int slice_rows,
                                                              float *__restrict__ row_val,        // [B] row cost | row_lse
                                                              int32_t *__restrict__ row_arg,      // [B] (hinge)
                                                              float *__restrict__ part_x,         // [slices, B]
                                                              int32_t *__restrict__ part_w) {     // [slices, B]: k, or the bits of y
    __shared__ float s_x[XBM_WAVES][XBM_COLS];
    __shared__ float s_y[XBM_WAVES][XBM_COLS];
    __shared__ int s_k[XBM_WAVES][XBM_COLS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int T = B + n;
    if (blockIdx.x < (unsigned)row_blocks) {
        const int i = blockIdx.x * XBM_WAVES + wave;
        if (i >= B) return;
        const int32_t gi = group[i];
        const float *srow = S + (int64_t)i * ldS;
        const float d = srow[i];
        XbmAcc a = xbm_init<MODE>();
        for (int t0 = lane; t0 < T; t0 += XBM_ROW_UNROLL * 64) {
            float v[XBM_ROW_UNROLL];
            int32_t gv[XBM_ROW_UNROLL];
#pragma unroll
            for (int u = 0; u < XBM_ROW_UNROLL; ++u) {
                const int t = t0 + u * 64;
                v[u] = 0.f;
                gv[u] = 0;
                if (t < B) {
                    v[u] = srow[t];
                    gv[u] = group[t];
                } else if (t < T) {
                    v[u] = R[(int64_t)i * ldR + (t - B)];
                    gv[u] = bank_group[t - B];
                }
            }
#pragma unroll
            for (int u = 0; u < XBM_ROW_UNROLL; ++u) {
                const int t = t0 + u * 64;
                if (t >= T) continue;
                const bool diag = t == i;
                const bool dropped = t < B ? (!diag && mask_batch && gv[u] == gi) : gv[u] == gi;
                if (dropped) continue;
                xbm_add<MODE>(a, v[u], t, diag, p, d);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
            a = xbm_merge<MODE>(a, XbmAcc{__shfl_xor(a.x, o, 64), __shfl_xor(a.y, o, 64), __shfl_xor(a.k, o, 64)});
        if (lane == 0) {
            if (MODE == XBM_NCE) {
                row_val[i] = a.x + logf(a.y);          // the diagonal is in every row: y >= 1
            } else {
                row_val[i] = a.x;
                row_arg[i] = a.k;
            }
        }
        return;
    }
    const int cblk = (blockIdx.x - row_blocks) / slices, sl = (blockIdx.x - row_blocks) % slices;
    const int c = cblk * XBM_COLS + lane;
    const int r0 = sl * slice_rows, r1 = min(T, r0 + slice_rows);
    const bool live = c < B;
    const int32_t gc = live ? group[c] : 0;
    const float d = (live && MODE != XBM_NCE) ? S[(int64_t)c * ldS + c] : 0.f;
    XbmAcc a = xbm_init<MODE>();
    for (int r = r0 + wave; r < r1; r += 4 * XBM_WAVES) {
        // four row segments in flight per wave
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int ru = r + u * XBM_WAVES;
            v[u] = 0.f;
            if (live && ru < r1) v[u] = ru < B ? S[(int64_t)ru * ldS + c] : C[(int64_t)(ru - B) * ldC + c];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int ru = r + u * XBM_WAVES;
            if (!live || ru >= r1) continue;
            const int32_t gr = ru < B ? group[ru] : bank_group[ru - B];
            const bool diag = ru == c;
            const bool dropped = ru < B ? (!diag && mask_batch && gr == gc) : gr == gc;
            if (dropped) continue;
            xbm_add<MODE>(a, v[u], ru, diag, p, d);
        }
    }
    s_x[wave][lane] = a.x;
    s_y[wave][lane] = a.y;
    s_k[wave][lane] = a.k;
    __syncthreads();
    if (wave == 0 && live) {
        XbmAcc t{s_x[0][lane], s_y[0][lane], s_k[0][lane]};
#pragma unroll
        for (int w = 1; w < XBM_WAVES; ++w) t = xbm_merge<MODE>(t, XbmAcc{s_x[w][lane], s_y[w][lane], s_k[w][lane]});
        part_x[(int64_t)sl * B + c] = t.x;
        part_w[(int64_t)sl * B + c] = MODE == XBM_NCE ? __float_as_int(t.y) : t.k;
    }
}

// one workgroup: every column's slices merged in slice order, then the 2B terms summed in float64
template <int MODE>
__global__ __launch_bounds__(XBM_FINISH_THREADS) void xbm_finish_kernel(const float *__restrict__ S, int64_t ldS, int B, float p,
                                                                        int slices, const float *__restrict__ row_val,
                                                                        const float *__restrict__ part_x,
                                                                        const int32_t *__restrict__ part_w,
                                                                        float *__restrict__ col_lse, int32_t *__restrict__ col_arg,
                                                                        float *__restrict__ loss) {
    __shared__ double s_acc[XBM_FINISH_THREADS / 64];
    double acc = 0.0;
    for (int c = threadIdx.x; c < B; c += XBM_FINISH_THREADS) {
        XbmAcc t = xbm_init<MODE>();
        for (int sl = 0; sl < slices; ++sl) {
            const float x = part_x[(int64_t)sl * B + c];
            const int32_t w = part_w[(int64_t)sl * B + c];
            t = xbm_merge<MODE>(t, XbmAcc{x, MODE == XBM_NCE ? __int_as_float(w) : 0.f, MODE == XBM_NCE ? 0 : w});
        }
        if (MODE == XBM_NCE) {
            const float cl = t.x + logf(t.y);
            col_lse[c] = cl;
            const float d = p * S[(int64_t)c * ldS + c];
            acc += (double)(row_val[c] - d) + (double)(cl - d);
        } else {
            col_arg[c] = t.k;
            acc += (double)row_val[c] + (double)t.x;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) s_acc[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < XBM_FINISH_THREADS / 64; ++w) t += s_acc[w];
        loss[0] = (float)(MODE == XBM_NCE ? t / (2.0 * (double)B) : t);
    }
}

struct XbmBwdArgs {
    const float *S, *R, *C;
    int64_t ldS, ldR, ldC;
    const int32_t *group, *bank_group;
    int B, n, mask_batch;
    float p;
    const float *row_lse, *col_lse;          // InfoNCE
    const int32_t *row_arg, *col_arg;        // hinge
    const float *grad_loss;
    float *dS, *dR, *dC;
    int64_t lddS, lddR, lddC;
};

// max form: is the hinge of row q (rows = true) or of column q active?  The saved arg is range- and mask-checked again.
__device__ __forceinline__ bool xbm_arg_active(const XbmBwdArgs &a, int q, bool rows, float dqq) {
    const int t = rows ? a.row_arg[q] : a.col_arg[q];
    if (t == q || t < 0 || t >= a.B + a.n) return false;
    const int32_t gq = a.group[q];
    float v;
    if (t < a.B) {
        if (a.mask_batch && a.group[t] == gq) return false;
        v = rows ? a.S[(int64_t)q * a.ldS + t] : a.S[(int64_t)t * a.ldS + q];
    } else {
        if (a.bank_group[t - a.B] == gq) return false;
        v = rows ? a.R[(int64_t)q * a.ldR + (t - a.B)] : a.C[(int64_t)(t - a.B) * a.ldC + q];
    }
    return (a.p + v) - dqq > 0.f;
}

// blockIdx.x < rs_blocks: entries of dS | dR, flat over B x (B + n).  Else entries of dC, flat over n x B.
template <int MODE>
__global__ __launch_bounds__(XBM_THREADS) void xbm_bwd_kernel(const XbmBwdArgs a, int64_t rs_blocks) {
    const int B = a.B, n = a.n, T = B + n;
    const float g = a.grad_loss[0];
    const float coef = MODE == XBM_NCE ? g * (a.p / (2.f * (float)B)) : g;
    if ((int64_t)blockIdx.x < rs_blocks) {
        const int64_t total = (int64_t)B * T;
#pragma unroll
        for (int u = 0; u < XBM_BWD_UNROLL; ++u) {
            const int64_t e = (int64_t)blockIdx.x * XBM_BWD_PER_BLOCK + u * XBM_THREADS + threadIdx.x;
            if (e >= total) return;
            const int i = (int)(e / T), t = (int)(e % T);
            const int32_t gi = a.group[i];
            if (t < B) {
                const int j = t;
                float *out = a.dS + (int64_t)i * a.lddS + j;
                if (j != i && a.mask_batch && a.group[j] == gi) {
                    *out = 0.f;
                    continue;
                }
                const float sij = a.S[(int64_t)i * a.ldS + j];
                if (MODE == XBM_NCE) {
                    const float z = a.p * sij;
                    const float pr = expf(z - a.row_lse[i]) + expf(z - a.col_lse[j]);
                    *out = coef * (j == i ? pr - 2.f : pr);
                    continue;
                }
                if (j == i) {
                    const int cnt = MODE == XBM_SUM ? a.row_arg[i] + a.col_arg[i]
                                                    : (int)xbm_arg_active(a, i, true, sij) + (int)xbm_arg_active(a, i, false, sij);
                    *out = -g * (float)cnt;
                    continue;
                }
                const bool row_on = (a.p + sij) - a.S[(int64_t)i * a.ldS + i] > 0.f;
                const bool col_on = (a.p + sij) - a.S[(int64_t)j * a.ldS + j] > 0.f;
                if (MODE == XBM_SUM) {
                    *out = g * (float)((int)row_on + (int)col_on);
                } else {
                    float v = 0.f;
                    if (row_on && a.row_arg[i] == j) v += g;
                    if (col_on && a.col_arg[j] == i) v += g;
                    *out = v;
                }
            } else {
                const int k = t - B;
                float *out = a.dR + (int64_t)i * a.lddR + k;
                if (a.bank_group[k] == gi) {
                    *out = 0.f;
                    continue;
                }
                const float r = a.R[(int64_t)i * a.ldR + k];
                if (MODE == XBM_NCE) {
                    *out = coef * expf(a.p * r - a.row_lse[i]);
                    continue;
                }
                const bool on = (a.p + r) - a.S[(int64_t)i * a.ldS + i] > 0.f && (MODE == XBM_SUM || a.row_arg[i] == t);
                *out = on ? g : 0.f;
            }
        }
        return;
    }
    const int64_t total = (int64_t)n * B;
#pragma unroll
    for (int u = 0; u < XBM_BWD_UNROLL; ++u) {
        const int64_t e = ((int64_t)blockIdx.x - rs_blocks) * XBM_BWD_PER_BLOCK + u * XBM_THREADS + threadIdx.x;
        if (e >= total) return;
        const int k = (int)(e / B), j = (int)(e % B);
        float *out = a.dC + (int64_t)k * a.lddC + j;
        if (a.bank_group[k] == a.group[j]) {
            *out = 0.f;
            continue;
        }
        const float c = a.C[(int64_t)k * a.ldC + j];
        if (MODE == XBM_NCE) {
            *out = coef * expf(a.p * c - a.col_lse[j]);
            continue;
        }
        const bool on = (a.p + c) - a.S[(int64_t)j * a.ldS + j] > 0.f && (MODE == XBM_SUM || a.col_arg[j] == B + k);
        *out = on ? g : 0.f;
    }
}

// table[(head + r) % M, :] = src[r, :] for r < count, in 32-bit words: one launch writes a push across the wrap
__global__ __launch_bounds__(XBM_THREADS) void xbm_ring_write_kernel(const uint32_t *__restrict__ src, uint32_t *__restrict__ table,
                                                                     int64_t M, int64_t width, int64_t head, int64_t total) {
    const int64_t e = (int64_t)blockIdx.x * XBM_THREADS + threadIdx.x;
    if (e >= total) return;
    const int64_t r = e / width, w = e % width;
    table[((head + r) % M) * width + w] = src[e];
}

struct XbmShape {
    const float *S, *R, *C;
    int64_t ldS, ldR, ldC;
    const int32_t *group, *bank_group;
    int B, n;
};

static int xbm_check(const char *who, const XbmShape &s) {
    ITR_REQUIRE(s.B >= 1 && s.n >= 0, "%s: bad shape B=%d n=%d", who, s.B, s.n);
    ITR_REQUIRE(s.S && s.group && (s.n == 0 || (s.R && s.C && s.bank_group)), "%s: null pointer", who);
    ITR_REQUIRE(s.ldS >= s.B && s.ldR >= s.n && s.ldC >= s.B, "%s: bad shape B=%d n=%d ldS=%lld ldR=%lld ldC=%lld", who, s.B, s.n,
                (long long)s.ldS, (long long)s.ldR, (long long)s.ldC);
    ITR_REQUIRE((int64_t)s.B * ((int64_t)s.B + 2 * (int64_t)s.n) < ((int64_t)1 << 31),
                "%s: too large: B (B + 2 n) must stay below 2^31, got B=%d n=%d", who, s.B, s.n);
    return ITR_OK;
}

template <int MODE>
static int xbm_fwd(const char *who, const XbmShape &s, int mask_batch, float p, float *loss, float *row_lse, float *col_lse,
                   int32_t *row_arg, int32_t *col_arg, void *workspace, itr_stream_t stream) {
    hipStream_t st = as_stream(stream);
    const XbmGeom geo = xbm_geom(s.B, s.n);
    const int row_blocks = (int)ceil_div(s.B, XBM_WAVES);
    const int64_t col_blocks = ceil_div(s.B, XBM_COLS) * geo.slices;
    float *part_x = static_cast<float *>(workspace);
    int32_t *part_w = reinterpret_cast<int32_t *>(part_x + (int64_t)geo.slices * s.B);
    float *row_cost = reinterpret_cast<float *>(part_w + (int64_t)geo.slices * s.B);
    float *row_val = MODE == XBM_NCE ? row_lse : row_cost;
    hipLaunchKernelGGL(xbm_fwd_kernel<MODE>, dim3((unsigned)(row_blocks + col_blocks)), dim3(XBM_THREADS), 0, st, s.S, s.ldS, s.R,
                       s.ldR, s.C, s.ldC, s.group, s.bank_group, s.B, s.n, mask_batch, p, row_blocks, geo.slices, geo.slice_rows,
                       row_val, row_arg, part_x, part_w);
    ITR_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(xbm_finish_kernel<MODE>, dim3(1), dim3(XBM_FINISH_THREADS), 0, st, s.S, s.ldS, s.B, p, geo.slices, row_val,
                       part_x, part_w, col_lse, col_arg, loss);
    ITR_CHECK_LAUNCH(who);
    return ITR_OK;
}

template <int MODE>
static int xbm_bwd(const char *who, const XbmBwdArgs &a, itr_stream_t stream) {
    const int64_t rs_blocks = ceil_div((int64_t)a.B * ((int64_t)a.B + a.n), XBM_BWD_PER_BLOCK);
    const int64_t c_blocks = ceil_div((int64_t)a.n * a.B, XBM_BWD_PER_BLOCK);
    hipLaunchKernelGGL(xbm_bwd_kernel<MODE>, dim3((unsigned)(rs_blocks + c_blocks)), dim3(XBM_THREADS), 0, as_stream(stream), a,
                       rs_blocks);
    ITR_CHECK_LAUNCH(who);
    return ITR_OK;
}

}  // namespace itr

extern "C" size_t itr_xbm_workspace_bytes(int B, int n) {
    if (B < 1 || n < 0) return 0;
    return ((size_t)2 * itr::xbm_geom(B, n).slices + 1) * (size_t)B * sizeof(float);
}

extern "C" int itr_xbm_hinge_fwd(const float *S, int64_t ldS, const float *R, int64_t ldR, const float *C, int64_t ldC,
                                 const int32_t *group, const int32_t *bank_group, int B, int n, int mask_batch, float margin,
                                 int max_violation, float *loss, int32_t *row_arg, int32_t *col_arg, void *workspace,
                                 itr_stream_t stream) {
    const itr::XbmShape s{S, R, C, ldS, ldR, ldC, group, bank_group, B, n};
    if (int rc = itr::xbm_check("itr_xbm_hinge_fwd", s)) return rc;
    ITR_REQUIRE(loss && row_arg && col_arg && workspace, "itr_xbm_hinge_fwd: null pointer");
    return max_violation ? itr::xbm_fwd<itr::XBM_MAX>("itr_xbm_hinge_fwd", s, mask_batch, margin, loss, nullptr, nullptr, row_arg, col_arg,
                                                      workspace, stream)
                         : itr::xbm_fwd<itr::XBM_SUM>("itr_xbm_hinge_fwd", s, mask_batch, margin, loss, nullptr, nullptr, row_arg, col_arg,
                                                      workspace, stream);
}

extern "C" int itr_xbm_hinge_bwd(const float *S, int64_t ldS, const float *R, int64_t ldR, const float *C, int64_t ldC,
                                 const int32_t *group, const int32_t *bank_group, int B, int n, int mask_batch, float margin,
                                 int max_violation, const int32_t *row_arg, const int32_t *col_arg, const float *grad_loss, float *dS,
                                 int64_t lddS, float *dR, int64_t lddR, float *dC, int64_t lddC, itr_stream_t stream) {
    const itr::XbmShape s{S, R, C, ldS, ldR, ldC, group, bank_group, B, n};
    if (int rc = itr::xbm_check("itr_xbm_hinge_bwd", s)) return rc;
    ITR_REQUIRE(row_arg && col_arg && grad_loss && dS && (n == 0 || (dR && dC)), "itr_xbm_hinge_bwd: null pointer");
    ITR_REQUIRE(lddS >= B && lddR >= n && lddC >= B, "itr_xbm_hinge_bwd: bad shape B=%d n=%d lddS=%lld lddR=%lld lddC=%lld", B, n,
                (long long)lddS, (long long)lddR, (long long)lddC);
    const itr::XbmBwdArgs a{S, R, C, ldS, ldR, ldC, group, bank_group, B, n, mask_batch, margin, nullptr, nullptr, row_arg, col_arg,
                            grad_loss, dS, dR, dC, lddS, lddR, lddC};
    return max_violation ? itr::xbm_bwd<itr::XBM_MAX>("itr_xbm_hinge_bwd", a, stream)
                         : itr::xbm_bwd<itr::XBM_SUM>("itr_xbm_hinge_bwd", a, stream);
}

extern "C" int itr_xbm_infonce_fwd(const float *S, int64_t ldS, const float *R, int64_t ldR, const float *C, int64_t ldC,
                                   const int32_t *group, const int32_t *bank_group, int B, int n, int mask_batch, float scale,
                                   float *loss, float *row_lse, float *col_lse, void *workspace, itr_stream_t stream) {
    const itr::XbmShape s{S, R, C, ldS, ldR, ldC, group, bank_group, B, n};
    if (int rc = itr::xbm_check("itr_xbm_infonce_fwd", s)) return rc;
    ITR_REQUIRE(loss && row_lse && col_lse && workspace, "itr_xbm_infonce_fwd: null pointer");
    ITR_REQUIRE(std::isfinite(scale) && scale > 0.f, "itr_xbm_infonce_fwd: scale (1 / temperature) must be finite and positive, got %g",
                (double)scale);
    return itr::xbm_fwd<itr::XBM_NCE>("itr_xbm_infonce_fwd", s, mask_batch, scale, loss, row_lse, col_lse, nullptr, nullptr, workspace,
                                      stream);
}

extern "C" int itr_xbm_infonce_bwd(const float *S, int64_t ldS, const float *R, int64_t ldR, const float *C, int64_t ldC,
                                   const int32_t *group, const int32_t *bank_group, int B, int n, int mask_batch, float scale,
                                   const float *row_lse, const float *col_lse, const float *grad_loss, float *dS, int64_t lddS,
                                   float *dR, int64_t lddR, float *dC, int64_t lddC, itr_stream_t stream) {
    const itr::XbmShape s{S, R, C, ldS, ldR, ldC, group, bank_group, B, n};
    if (int rc = itr::xbm_check("itr_xbm_infonce_bwd", s)) return rc;
    ITR_REQUIRE(row_lse && col_lse && grad_loss && dS && (n == 0 || (dR && dC)), "itr_xbm_infonce_bwd: null pointer");
    ITR_REQUIRE(lddS >= B && lddR >= n && lddC >= B, "itr_xbm_infonce_bwd: bad shape B=%d n=%d lddS=%lld lddR=%lld lddC=%lld", B, n,
                (long long)lddS, (long long)lddR, (long long)lddC);
    ITR_REQUIRE(std::isfinite(scale) && scale > 0.f, "itr_xbm_infonce_bwd: scale (1 / temperature) must be finite and positive, got %g",
                (double)scale);
    const itr::XbmBwdArgs a{S, R, C, ldS, ldR, ldC, group, bank_group, B, n, mask_batch, scale, row_lse, col_lse, nullptr, nullptr,
                            grad_loss, dS, dR, dC, lddS, lddR, lddC};
    return itr::xbm_bwd<itr::XBM_NCE>("itr_xbm_infonce_bwd", a, stream);
}

extern "C" int itr_xbm_ring_write(const void *src, void *table, int64_t capacity, int64_t width, int64_t head, int64_t count,
                                  itr_stream_t stream) {
    ITR_REQUIRE(capacity >= 1 && width >= 1 && head >= 0 && head < capacity && count >= 0 && count <= capacity,
                "itr_xbm_ring_write: bad shape capacity=%lld width=%lld head=%lld count=%lld", (long long)capacity, (long long)width,
                (long long)head, (long long)count);
    ITR_REQUIRE(capacity * width < ((int64_t)1 << 40), "itr_xbm_ring_write: table too large");
    if (count == 0) return ITR_OK;
    ITR_REQUIRE(src && table, "itr_xbm_ring_write: null pointer");
    const int64_t total = count * width;
    ITR_REQUIRE(itr::ceil_div(total, itr::XBM_THREADS) < ((int64_t)1 << 31), "itr_xbm_ring_write: push too large");
    hipLaunchKernelGGL(itr::xbm_ring_write_kernel, dim3((unsigned)itr::ceil_div(total, itr::XBM_THREADS)), dim3(itr::XBM_THREADS), 0,
                       itr::as_stream(stream), static_cast<const uint32_t *>(src), static_cast<uint32_t *>(table), capacity, width,
                       head, total);
    ITR_CHECK_LAUNCH("itr_xbm_ring_write");
    return ITR_OK;
}
