// Hubness correction of a similarity matrix before ranking (CSLS, inverted softmax): S'[i, j] = S[i, j] - a[i] - b[j].  The vectors
// are row and column statistics of score matrices that may be query banks several times the gallery, scored in row blocks and never
// stored; this file holds the reductions (float64 throughout) and the adjustment.  DESIGN.md 4.4.4.
//
// itr_hub_lse_fold: ONE pass over a row block, every element read once and widened to double, for both directions:
//   row_lse[r]  = (1 / beta) log sum_j exp(beta S[r, j])                     (final: a block holds whole rows)
//   col_state[j] = (sum_r exp(beta (S[r, j] - m_j)), m_j = max_r S[r, j])     (running, over all blocks folded so far)
// A sum of 0 means "empty" whatever the second slot holds, so all-zero bytes are the starting state.  A maximum that is not finite
// decides the result on its own (NaN: NaN; +inf: +inf; such a state carries sum 1), and a column of only -inf stays empty (-inf).
//
// One WAVE owns a tile of `rpw` rows x HF_COLS = 256 columns (a lane: 4 columns), read HF_G = 4 rows at a time with the next group's
// loads in flight.  No atomics, and one barrier, at the end:
// The two directions need different shifts (beta S reaches 1e4: one shift per tile would flush whole rows to zero), but not two
// exps: exp(beta x) = p * 2^n is taken apart ONCE per element (hub_split: the reduction and polynomial of a double exp), and a shift
// by a power of two is an integer subtracted from n before p is scaled (ldexp):
//   columns: the lane alone sees its columns' rows.  Per group: the largest n, the running sum rescaled to it (ldexp, exact), then
//            one ldexp and one add per element; the maximum of x rides along for the state;
//   rows:    the largest n of the row over the strip (4 local + an integer wave reduction), one ldexp and add per element, a wave sum.
// A wave stores its rows' (sum, n) to the workspace, [strip][n_rows][2]; its columns go back to the state's form, (sum of
// exp(beta x - beta m), m), with one exp per column, and the 4 waves of a workgroup, stacked in rows, combine them in LDS, top to
// bottom, into one slab entry per column, [workgroup row][Nc][2].  The finishing kernel combines old state and slabs in index order, one thread per column / row.  Nothing
// depends on how workgroups are scheduled: the same call gives the same bits.  Another partition of the rows sums in another order.
#include <math.h>

#include "itr_internal.h"

namespace itr {

constexpr int HF_THREADS = 256;
constexpr int HF_WAVES = HF_THREADS / 64;
constexpr int HF_E = 4;                                   // columns of a lane
constexpr int HF_COLS = 64 * HF_E;                        // columns of a strip
constexpr int HF_G = 4;                                   // rows of a group
constexpr int64_t HF_WANT_WAVES = 4096;                   // tiles the plan aims at (256 CUs x 4 SIMDs x 4)
constexpr int HF_MAX_RPW = 256;                           // rows of a tile at most (bounds the column slabs: Nc * 16 B per tile)

struct HubPlan {
    int64_t strips, tiles, slabs;                         // column strips, row tiles (one per wave), column slabs (one per workgroup)
    int rpw;                                              // rows per tile (a multiple of HF_G)
    double *col_part, *row_part;
    size_t bytes;
};

// The one place that sizes and carves the workspace (itr_hub_lse_workspace_bytes measures with a null base).
static HubPlan hub_plan(void *base, int64_t n_rows, int64_t Nc) {
    HubPlan p;
    p.strips = ceil_div(Nc, (int64_t)HF_COLS);
    // as few rows per tile as still gives every SIMD several waves, never fewer than two groups; more rows per tile = smaller slabs
    int64_t rpw = ceil_div(n_rows * (p.strips > 0 ? p.strips : 1), HF_WANT_WAVES);
    rpw = ceil_div(rpw, (int64_t)HF_G) * HF_G;
    if (rpw < 2 * HF_G) rpw = 2 * HF_G;
    if (rpw > HF_MAX_RPW) rpw = HF_MAX_RPW;
    p.rpw = (int)rpw;
    p.tiles = ceil_div(n_rows, rpw);
    WsCarver ws(base);
    p.slabs = ceil_div(p.tiles, (int64_t)HF_WAVES);
    p.col_part = ws.take<double>((size_t)p.slabs * (size_t)Nc * 2 * sizeof(double));
    p.row_part = ws.take<double>((size_t)p.strips * (size_t)n_rows * 2 * sizeof(double));
    p.bytes = ws.bytes;
    return p;
}

// max that keeps a NaN once it has seen one (fmax drops it)
__device__ __forceinline__ double hub_nanmax(double a, double b) { return (a != a) ? a : ((b != b || b > a) ? b : a); }

__device__ __forceinline__ double hub_wave_nanmax(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = hub_nanmax(v, __shfl_xor(v, o, 64));
    return v;
}
// every lane gets the same bits: lane i adds lane i ^ o, the tree is symmetric
__device__ __forceinline__ double hub_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// exp(d) = p * 2^n with p = exp(d - n ln 2) in [0.70, 1.42]: the argument reduction and the polynomial of a double exp, WITHOUT the
// final scaling -- that is an integer added to the exponent, so a row and a column that need different shifts share p.  n ln 2 is
// taken off in two pieces (fdlibm's split: n * HN_LN2_HI is exact for |n| < 2^20 and within an ulp of the difference up to 2^29);
// the Taylor series to degree 13 is below 5e-18 on |r| <= 0.347.  What has no finite exp gets p = 0 and a sentinel n that wins or
// loses every integer maximum as the value would: NaN > +inf > every finite n > -inf.  |d| >= 2^29 ln 2 = 3.7e8 counts as +-inf.
constexpr int HN_NAN = 1 << 30, HN_INF = (1 << 30) - 1, HN_NINF = -(1 << 30);
constexpr double HN_LOG2E = 1.4426950408889634074, HN_LN2_HI = 6.93147180369123816490e-01, HN_LN2_LO = 1.90821492927058770002e-10;
__device__ __forceinline__ void hub_split(double d, double &p, int &n) {
    const double t = d * HN_LOG2E;
    const bool nan = d != d, hi = t >= 536870912.0, lo = t <= -536870912.0, special = nan || hi || lo;
    const double nf = rint(special ? 0.0 : t);
    double r = fma(-nf, HN_LN2_HI, special ? 0.0 : d);
    r = fma(-nf, HN_LN2_LO, r);
    double q = 1.0 / 6227020800.0;
    q = fma(q, r, 1.0 / 479001600.0);
    q = fma(q, r, 1.0 / 39916800.0);
    q = fma(q, r, 1.0 / 3628800.0);
    q = fma(q, r, 1.0 / 362880.0);
    q = fma(q, r, 1.0 / 40320.0);
    q = fma(q, r, 1.0 / 5040.0);
    q = fma(q, r, 1.0 / 720.0);
    q = fma(q, r, 1.0 / 120.0);
    q = fma(q, r, 1.0 / 24.0);
    q = fma(q, r, 1.0 / 6.0);
    q = fma(q, r, 0.5);
    q = fma(q, r, 1.0);
    q = fma(q, r, 1.0);
    p = special ? 0.0 : q;
    n = nan ? HN_NAN : hi ? HN_INF : lo ? HN_NINF : (int)nf;
}
// the maximum a sentinel stands for (a finite n: the maximum of x itself)
__device__ __forceinline__ double hub_class_max(int n, double m) {
    return n == HN_NAN ? NAN : n == HN_INF ? INFINITY : n == HN_NINF ? -INFINITY : m;
}
__device__ __forceinline__ int hub_wave_max_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int w = __shfl_xor(v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}

// (sum, max) as it is stored: empty = sum 0; a maximum that is not finite stands for the result, with sum 1
__device__ __forceinline__ void hub_store(double *dst, double s, double m) {
    const bool fin = m - m == 0.0;                        // finite
    dst[0] = fin ? s : (m == -INFINITY ? 0.0 : 1.0);
    dst[1] = m == -INFINITY ? 0.0 : m;
}

// Combine `n` stored (sum, max) items, `stride` doubles apart, after an optional leading item `first`, in index order.
__device__ __forceinline__ void hub_combine(const double *first, const double *part, int64_t n, int64_t stride, double beta, double &s_out,
                                            double &m_out) {
    double m = -INFINITY;
    if (first && first[0] != 0.0) m = hub_nanmax(m, first[1]);
    for (int64_t p = 0; p < n; ++p)
        if (part[p * stride] != 0.0) m = hub_nanmax(m, part[p * stride + 1]);
    double s = 0.0;
    if (m - m == 0.0) {                                   // finite: every item that is not empty has a finite maximum
        if (first && first[0] != 0.0) s += first[0] * exp(beta * (first[1] - m));
        for (int64_t p = 0; p < n; ++p)
            if (part[p * stride] != 0.0) s += part[p * stride] * exp(beta * (part[p * stride + 1] - m));
    }
    s_out = s;
    m_out = m;
}

// T: float / double.  VEC: S and its rows are 16-byte aligned and every strip of the launch lies inside the matrix (the host launches
// the right-edge strip on its own, VEC = false): a lane owns 4 ADJACENT columns and takes them with 16-byte loads; otherwise a lane
// owns columns lane, lane + 64, .. of the strip (scalar loads, coalesced across the wave) and columns past Nc read as -inf, which
// adds nothing.  Rows past the block read as -inf too.
template <typename T, bool VEC, bool ROWS, bool COLS>
__global__ __launch_bounds__(HF_THREADS) void hub_fold_kernel(const T *__restrict__ S, int64_t ldS, int64_t n_rows, int64_t Nc, double beta,
                                                              int rpw, int64_t strip0, double *__restrict__ col_part,
                                                              double *__restrict__ row_part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t strip = strip0 + blockIdx.x, tile = (int64_t)blockIdx.y * HF_WAVES + wave;
    const int64_t r0 = tile * rpw;                        // (a wave past the block has r1 <= r0: it folds nothing and hands over an empty state)
    const int64_t r1 = r0 + rpw < n_rows ? r0 + rpw : n_rows;
    const int64_t c0 = strip * HF_COLS;
    int64_t col[HF_E];
#pragma unroll
    for (int e = 0; e < HF_E; ++e) col[e] = c0 + (VEC ? lane * HF_E + e : lane + 64 * e);

    auto load = [&](int64_t r, double (*v)[HF_E]) {
#pragma unroll
        for (int g = 0; g < HF_G; ++g) {
            const bool rin = r + g < r1;
            const T *row = S + (rin ? r + g : r1 - 1) * ldS;
            if constexpr (VEC) {
                if constexpr (sizeof(T) == 4) {
                    const float4 q = *reinterpret_cast<const float4 *>(row + col[0]);
                    v[g][0] = q.x; v[g][1] = q.y; v[g][2] = q.z; v[g][3] = q.w;
                } else {
                    const double2 q0 = *reinterpret_cast<const double2 *>(row + col[0]);
                    const double2 q1 = *reinterpret_cast<const double2 *>(row + col[2]);
                    v[g][0] = q0.x; v[g][1] = q0.y; v[g][2] = q1.x; v[g][3] = q1.y;
                }
#pragma unroll
                for (int e = 0; e < HF_E; ++e) v[g][e] = rin ? v[g][e] : -INFINITY;
            } else {
#pragma unroll
                for (int e = 0; e < HF_E; ++e) {
                    const bool in = rin && col[e] < Nc;
                    const double x = (double)row[col[e] < Nc ? col[e] : Nc - 1];
                    v[g][e] = in ? x : -INFINITY;
                }
            }
        }
    };

    double cs[HF_E], cm[HF_E];                            // the lane's columns over the tile's rows: sum of 2^(n - cn) p, maximum of x,
    int cn[HF_E];                                         // and the power of two the sum is scaled by
#pragma unroll
    for (int e = 0; e < HF_E; ++e) { cs[e] = 0.0; cm[e] = -INFINITY; cn[e] = HN_NINF; }

    double cur[HF_G][HF_E], nxt[HF_G][HF_E];
    load(r0, cur);
    for (int64_t r = r0; r < r1; r += HF_G) {
        if (r + HF_G < r1) load(r + HF_G, nxt);           // (uniform) the next group is in flight while this one is folded
        double p[HF_G][HF_E];                             // exp(beta x) = p * 2^n, ONCE per element for both directions
        int n[HF_G][HF_E];
#pragma unroll
        for (int g = 0; g < HF_G; ++g)
#pragma unroll
            for (int e = 0; e < HF_E; ++e) hub_split(beta * cur[g][e], p[g][e], n[g][e]);
        if constexpr (COLS) {
#pragma unroll
            for (int e = 0; e < HF_E; ++e) {
                int gn = n[0][e];
                double gm = cur[0][e];
#pragma unroll
                for (int g = 1; g < HF_G; ++g) {
                    gn = n[g][e] > gn ? n[g][e] : gn;
                    gm = hub_nanmax(gm, cur[g][e]);
                }
                const int nn = gn > cn[e] ? gn : cn[e];
                double s = ldexp(cs[e], cn[e] - nn);      // (exact; an empty sum is 0 and stays 0)
#pragma unroll
                for (int g = 0; g < HF_G; ++g) s += ldexp(p[g][e], n[g][e] - nn);
                cs[e] = s;
                cn[e] = nn;
                cm[e] = hub_nanmax(cm[e], gm);
            }
        }
        if constexpr (ROWS) {
            int rn[HF_G];
            double rs[HF_G];
#pragma unroll
            for (int g = 0; g < HF_G; ++g) {
                int m = n[g][0];
#pragma unroll
                for (int e = 1; e < HF_E; ++e) m = n[g][e] > m ? n[g][e] : m;
                rn[g] = m;
            }
#pragma unroll
            for (int g = 0; g < HF_G; ++g) rn[g] = hub_wave_max_i(rn[g]);
#pragma unroll
            for (int g = 0; g < HF_G; ++g) {
                double s = 0.0;
#pragma unroll
                for (int e = 0; e < HF_E; ++e) s += ldexp(p[g][e], n[g][e] - rn[g]);
                rs[g] = s;
            }
#pragma unroll
            for (int g = 0; g < HF_G; ++g) rs[g] = hub_wave_sum(rs[g]);
            if (lane < HF_G && r + lane < r1) {
                double s = rs[0];
                int m = rn[0];
#pragma unroll
                for (int g = 1; g < HF_G; ++g)
                    if (lane == g) { s = rs[g]; m = rn[g]; }
                double *dst = row_part + (strip * n_rows + r + lane) * 2;      // rows keep the power-of-two form: (sum, n)
                dst[0] = s;
                dst[1] = (double)m;
            }
        }
#pragma unroll
        for (int g = 0; g < HF_G; ++g)
#pragma unroll
            for (int e = 0; e < HF_E; ++e) cur[g][e] = nxt[g][e];
    }
    if constexpr (COLS) {                                 // the workgroup's tiles, top to bottom, make one slab entry per column
        __shared__ double sh[HF_WAVES][HF_COLS][2];
#pragma unroll
        for (int e = 0; e < HF_E; ++e) {                  // -> the state's form: sum of exp(beta x - beta m), m the maximum of x
            const bool fin = cn[e] > HN_NINF && cn[e] < HN_INF;
            const double sc = exp(fma((double)cn[e], HN_LN2_LO, fma((double)cn[e], HN_LN2_HI, -(beta * cm[e]))));
            hub_store(sh[wave][col[e] - c0], fin ? cs[e] * sc : 0.0, hub_class_max(cn[e], cm[e]));
        }
        __syncthreads();
        const int64_t c = c0 + threadIdx.x;
        if (c < Nc) {
            double s, m;
            hub_combine(nullptr, &sh[0][threadIdx.x][0], HF_WAVES, HF_COLS * 2, beta, s, m);
            hub_store(col_part + ((int64_t)blockIdx.y * Nc + c) * 2, s, m);
        }
    }
}

__device__ __forceinline__ double hub_lse_of(double s, double m, double beta) {
    if (s == 0.0) return -INFINITY;
    return m - m == 0.0 ? m + log(s) / beta : m;
}

// thread t < Nc: column t (old state + row-tile slabs -> new state); thread Nc + r: row r (strip slabs -> row_lse)
__global__ __launch_bounds__(256) void hub_fold_finish_kernel(const double *__restrict__ col_part, const double *__restrict__ row_part,
                                                              int64_t n_rows, int64_t Nc, int64_t slabs, int64_t strips, double beta,
                                                              double *col_state, double *__restrict__ row_lse, int64_t n_col_items) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    double s, m;
    if (t < n_col_items) {
        hub_combine(col_state + t * 2, col_part + t * 2, slabs, Nc * 2, beta, s, m);
        hub_store(col_state + t * 2, s, m);
    } else if (t - n_col_items < (row_lse ? n_rows : 0)) {
        const int64_t r = t - n_col_items;
        // the strips' (sum, n) in strip order: log(sum_i s_i 2^(n_i - N)) + N ln 2, N ln 2 in its two pieces
        const double *part = row_part + r * 2;
        int N = HN_NINF;
        for (int64_t q = 0; q < strips; ++q) N = (int)part[q * n_rows * 2 + 1] > N ? (int)part[q * n_rows * 2 + 1] : N;
        s = 0.0;
        for (int64_t q = 0; q < strips; ++q) s += ldexp(part[q * n_rows * 2], (int)part[q * n_rows * 2 + 1] - N);
        m = (double)N;
        row_lse[r] = (N == HN_NAN || N == HN_INF || N == HN_NINF) ? hub_class_max(N, 0.0)
                                                                  : (m * HN_LN2_HI + (m * HN_LN2_LO + log(s))) / beta;
    }
}

__global__ __launch_bounds__(256) void hub_lse_finish_kernel(const double *__restrict__ col_state, int64_t Nc, double beta,
                                                             double *__restrict__ col_lse) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < Nc) col_lse[j] = hub_lse_of(col_state[j * 2], col_state[j * 2 + 1], beta);
}

// out[r] = 0.5 * ((((v0 + v1) + v2) + ..) / k): the float64 sum of the list's first k entries, best first, one at a time
template <typename T>
__global__ __launch_bounds__(256) void hub_list_mean_kernel(const T *__restrict__ val, int64_t n, int64_t ld, int k, double *__restrict__ out) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const T *v = val + r * ld;
    double s = (double)v[0];
    for (int i = 1; i < k; ++i) s += (double)v[i];
    out[r] = 0.5 * (s / (double)k);
}

// Two float64 subtractions, each rounded on its own, then the cast.  A thread reads its element before it writes it: in place is safe.
template <typename T>
__global__ __launch_bounds__(256) void hub_adjust_kernel(const T *S, int64_t ldS, int64_t n_rows, int64_t Nc, const double *__restrict__ a,
                                                         const double *__restrict__ b, T *out, int64_t ldo) {
#pragma clang fp contract(off) reassociate(off)
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= Nc) return;
    const double bj = b ? b[j] : 0.0;
    for (int64_t i = blockIdx.y; i < n_rows; i += gridDim.y) {
        const double ai = a ? a[i] : 0.0;
        const double x = (double)S[i * ldS + j];
        const double y = x - ai;
        out[i * ldo + j] = (T)(y - bj);
    }
}

template <typename T, bool VEC>
static void hub_fold_launch(const T *S, int64_t ldS, int64_t n_rows, int64_t Nc, double beta, const HubPlan &p, int64_t strip0, int64_t n_strips,
                            bool rows, bool cols, hipStream_t st) {
    const dim3 grid((unsigned)n_strips, (unsigned)ceil_div(p.tiles, (int64_t)HF_WAVES)), block(HF_THREADS);
    if (rows && cols)
        hipLaunchKernelGGL((hub_fold_kernel<T, VEC, true, true>), grid, block, 0, st, S, ldS, n_rows, Nc, beta, p.rpw, strip0, p.col_part, p.row_part);
    else if (rows)
        hipLaunchKernelGGL((hub_fold_kernel<T, VEC, true, false>), grid, block, 0, st, S, ldS, n_rows, Nc, beta, p.rpw, strip0, p.col_part, p.row_part);
    else
        hipLaunchKernelGGL((hub_fold_kernel<T, VEC, false, true>), grid, block, 0, st, S, ldS, n_rows, Nc, beta, p.rpw, strip0, p.col_part, p.row_part);
}

template <typename T>
static int hub_fold_impl(const T *S, int64_t ldS, int64_t n_rows, int64_t Nc, double beta, double *row_lse, double *col_state, const HubPlan &p,
                         hipStream_t st) {
    const bool rows = row_lse != nullptr, cols = col_state != nullptr;
    const bool vec = ((reinterpret_cast<uintptr_t>(S) & 15) == 0) && ((ldS * (int64_t)sizeof(T)) % 16 == 0);
    const int64_t n_vec = vec ? Nc / HF_COLS : 0;          // full strips read with 16-byte loads; the rest (all, or the right edge) scalar
    if (n_vec > 0) {
        hub_fold_launch<T, true>(S, ldS, n_rows, Nc, beta, p, 0, n_vec, rows, cols, st);
        ITR_CHECK_LAUNCH("hub_lse_fold");
    }
    if (p.strips > n_vec) {
        hub_fold_launch<T, false>(S, ldS, n_rows, Nc, beta, p, n_vec, p.strips - n_vec, rows, cols, st);
        ITR_CHECK_LAUNCH("hub_lse_fold_scalar");
    }
    const int64_t n_col_items = cols ? Nc : 0, items = n_col_items + (rows ? n_rows : 0);
    hipLaunchKernelGGL(hub_fold_finish_kernel, dim3((unsigned)ceil_div(items, (int64_t)256)), dim3(256), 0, st, p.col_part, p.row_part, n_rows, Nc,
                       p.slabs, p.strips, beta, col_state, row_lse, n_col_items);
    ITR_CHECK_LAUNCH("hub_lse_fold_finish");
    return ITR_OK;
}

// byte ranges [p, p + n) and [q, q + m) share a byte
static bool hub_overlap(const void *p, size_t n, const void *q, size_t m) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return n > 0 && m > 0 && a < b + m && b < a + n;
}

}  // namespace itr

extern "C" size_t itr_hub_lse_workspace_bytes(int64_t n_rows, int64_t Nc) {
    if (n_rows <= 0 || Nc <= 0 || n_rows >= 0x7fffffffLL || Nc >= 0x7fffffffLL) return 0;
    return itr::hub_plan(nullptr, n_rows, Nc).bytes;
}

extern "C" int itr_hub_lse_fold(const void *S, int f64, int64_t ldS, int64_t n_rows, int64_t Nc, double beta, double *row_lse, double *col_state,
                                void *workspace, size_t workspace_bytes, itr_stream_t stream) {
    ITR_REQUIRE(beta > 0.0 && beta - beta == 0.0, "itr_hub_lse_fold: beta = %g is not finite and positive", beta);
    ITR_REQUIRE(n_rows >= 0 && Nc >= 0 && ldS >= Nc, "itr_hub_lse_fold: bad shape (n_rows %lld, Nc %lld, ldS %lld)", (long long)n_rows,
                (long long)Nc, (long long)ldS);
    ITR_REQUIRE(n_rows < 0x7fffffffLL && Nc < 0x7fffffffLL, "itr_hub_lse_fold: index overflow");
    if (n_rows == 0 || Nc == 0) return ITR_OK;
    ITR_REQUIRE(S, "itr_hub_lse_fold: null pointer S");
    if (!row_lse && !col_state) return ITR_OK;             // neither direction asked for
    const itr::HubPlan p = itr::hub_plan(workspace, n_rows, Nc);
    ITR_REQUIRE(workspace && workspace_bytes >= p.bytes, "itr_hub_lse_fold: workspace of %zu bytes, itr_hub_lse_workspace_bytes asks for %zu",
                workspace ? workspace_bytes : (size_t)0, p.bytes);
    ITR_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "itr_hub_lse_fold: workspace is not 8-byte aligned");
    hipStream_t st = itr::as_stream(stream);
    return f64 ? itr::hub_fold_impl(static_cast<const double *>(S), ldS, n_rows, Nc, beta, row_lse, col_state, p, st)
               : itr::hub_fold_impl(static_cast<const float *>(S), ldS, n_rows, Nc, beta, row_lse, col_state, p, st);
}

extern "C" int itr_hub_lse_finish(const double *col_state, int64_t Nc, double beta, double *col_lse, itr_stream_t stream) {
    ITR_REQUIRE(beta > 0.0 && beta - beta == 0.0, "itr_hub_lse_finish: beta = %g is not finite and positive", beta);
    ITR_REQUIRE(Nc >= 0 && Nc < 0x7fffffffLL, "itr_hub_lse_finish: bad Nc %lld", (long long)Nc);
    if (Nc == 0) return ITR_OK;
    ITR_REQUIRE(col_state && col_lse, "itr_hub_lse_finish: null pointer col_state / col_lse");
    hipLaunchKernelGGL(itr::hub_lse_finish_kernel, dim3((unsigned)itr::ceil_div(Nc, (int64_t)256)), dim3(256), 0, itr::as_stream(stream), col_state,
                       Nc, beta, col_lse);
    ITR_CHECK_LAUNCH("hub_lse_finish");
    return ITR_OK;
}

extern "C" int itr_hub_list_mean(const void *val, int f64, int64_t n, int64_t ld, int k, double *out, itr_stream_t stream) {
    ITR_REQUIRE(k >= 1, "itr_hub_list_mean: k = %d < 1", k);
    ITR_UNSUPPORTED(k > ITR_TOPK_MAX, "itr_hub_list_mean: k = %d above ITR_TOPK_MAX = %d", k, ITR_TOPK_MAX);
    ITR_REQUIRE(n >= 0 && n < 0x7fffffffLL && ld >= k, "itr_hub_list_mean: bad shape (n %lld, ld %lld, k %d)", (long long)n, (long long)ld, k);
    if (n == 0) return ITR_OK;
    ITR_REQUIRE(val && out, "itr_hub_list_mean: null pointer val / out");
    const dim3 grid((unsigned)itr::ceil_div(n, (int64_t)256)), block(256);
    hipStream_t st = itr::as_stream(stream);
    if (f64)
        hipLaunchKernelGGL(itr::hub_list_mean_kernel<double>, grid, block, 0, st, static_cast<const double *>(val), n, ld, k, out);
    else
        hipLaunchKernelGGL(itr::hub_list_mean_kernel<float>, grid, block, 0, st, static_cast<const float *>(val), n, ld, k, out);
    ITR_CHECK_LAUNCH("hub_list_mean");
    return ITR_OK;
}

extern "C" int itr_hub_adjust(const void *S, int f64, int64_t ldS, int64_t n_rows, int64_t Nc, const double *a, const double *b, void *out,
                              int64_t ldo, itr_stream_t stream) {
    ITR_REQUIRE(n_rows >= 0 && Nc >= 0 && ldS >= Nc && ldo >= Nc, "itr_hub_adjust: bad shape (n_rows %lld, Nc %lld, ldS %lld, ldo %lld)",
                (long long)n_rows, (long long)Nc, (long long)ldS, (long long)ldo);
    ITR_REQUIRE(n_rows < 0x7fffffffLL && Nc < 0x7fffffffLL, "itr_hub_adjust: index overflow");
    if (n_rows == 0 || Nc == 0) return ITR_OK;
    ITR_REQUIRE(S && out, "itr_hub_adjust: null pointer S / out");
    const size_t el = f64 ? 8 : 4;
    const size_t s_bytes = ((size_t)(n_rows - 1) * (size_t)ldS + (size_t)Nc) * el, o_bytes = ((size_t)(n_rows - 1) * (size_t)ldo + (size_t)Nc) * el;
    // in place (the same matrix, element for element) is the one overlap a thread's read-then-write makes safe
    ITR_REQUIRE((out == S && ldo == ldS) || !itr::hub_overlap(S, s_bytes, out, o_bytes),
                "itr_hub_adjust: out and S alias partially (in place needs out == S and ldo == ldS)");
    ITR_REQUIRE(!(a && itr::hub_overlap(a, (size_t)n_rows * 8, out, o_bytes)) && !(b && itr::hub_overlap(b, (size_t)Nc * 8, out, o_bytes)),
                "itr_hub_adjust: out and a / b alias");
    const int64_t gy = n_rows < 1024 ? n_rows : 1024;
    const dim3 grid((unsigned)itr::ceil_div(Nc, (int64_t)256), (unsigned)gy), block(256);
    hipStream_t st = itr::as_stream(stream);
    if (f64)
        hipLaunchKernelGGL(itr::hub_adjust_kernel<double>, grid, block, 0, st, static_cast<const double *>(S), ldS, n_rows, Nc, a, b,
                           static_cast<double *>(out), ldo);
    else
        hipLaunchKernelGGL(itr::hub_adjust_kernel<float>, grid, block, 0, st, static_cast<const float *>(S), ldS, n_rows, Nc, a, b,
                           static_cast<float *>(out), ldo);
    ITR_CHECK_LAUNCH("hub_adjust");
    return ITR_OK;
}
