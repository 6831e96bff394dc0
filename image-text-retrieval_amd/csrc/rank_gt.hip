// Positions under ANY ground-truth relation (R-Precision, mAP@R, Recall@K with several positives per query) without sorting.
//
// rank.hip counts every row / column against ONE threshold, the ground truth of the layout caption j <-> image j / im_div.  Here the
// ground truth is a sparse relation given in both CSR forms, and a query has a SET of thresholds: the keys of its positives.  The
// position of a positive in its query's ranked list is still a count,
//     pos = #{k : key_k > key_positive}      (rank_key.h: (score, index) is one key of a total order),
// so one streaming pass over the line serves all of its positives at once: with the line's thresholds sorted ascending, an element
// falls into the bucket b = #{thr < key} (a binary search, after ONE compare against the smallest threshold -- in a trained model
// almost nothing passes it), buckets are counted in an LDS histogram, and pos of the s-th smallest threshold is the sum of the
// buckets above s.
//
//   gather : key of every positive whose row lies in the block -> i2t_key / t2i_key [nnz]             (one thread per entry)
//   sort   : per query, its keys ascending + the entry each came from (rank sort, one thread per entry) -> workspace
//   rows   : a workgroup owns a row; GT_ROW_CAP thresholds per pass over the row; positions are final (plain stores)
//   columns: a workgroup owns a strip of GT_STRIP columns x a chunk of rows; a lane owns 4 adjacent columns and the four waves walk
//            down interleaved rows; GT_COL_CAP thresholds of the strip per pass; one global atomic per (positive, workgroup), so row
//            blocks and other workgroups just add.
// A query with more positives than a pass holds takes more passes over its line; every count is exact for any number of them.
// float64 matrices take the same kernels with scalar loads and a two-word key (ordered double, then the index).
// No index of the relation becomes an address unchecked: segment bounds are clamped to [0, nnz], gallery indices are compared
// against the matrix, entries of the workspace's permutations against nnz.
#include "itr_internal.h"
#include "rank_key.h"
#include <type_traits>

namespace itr {

constexpr int GT_THREADS = 256;
constexpr int GT_WAVES = GT_THREADS / 64;
constexpr int GT_ROW_CAP = 256;       // thresholds of a row in LDS per pass (one per thread)
constexpr int GT_ROW_HIST = 8192;     // counters of the row histogram: as many copies of the n buckets as fit (256 copies up to n = 32)
constexpr int GT_STRIP = 256;         // columns of a strip: 64 lanes x 4
constexpr int GT_COL_CAP = 2048;      // thresholds of a strip in LDS per pass
constexpr int GT_COL_U = 4;           // rows a wave requests before it consumes the first
constexpr int GT_COL_WGS = 1024;      // workgroups the column pass aims at (256 CUs x 4)
static_assert(GT_ROW_CAP == GT_THREADS && GT_STRIP == GT_THREADS, "one thread per row threshold / per strip column");

template <bool F64> using gt_elem = typename std::conditional<F64, double, float>::type;

// fp32: hi = rank_key (the index is inside), lo unused.  float64: hi = ordered canonical double, lo = index.
struct GtKey { unsigned long long hi; uint32_t lo; };
template <bool F64> __device__ __forceinline__ GtKey gt_key(gt_elem<F64> e, uint32_t idx) {
    if constexpr (F64) return GtKey{double_order_key(canon_f64(e)), idx};
    else return GtKey{rank_key(e, idx), 0u};
}
template <bool F64> __device__ __forceinline__ bool gt_less(const GtKey &a, const GtKey &b) {
    if constexpr (F64) return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo);
    else return a.hi < b.hi;
}

__device__ __forceinline__ int gt_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the segment of entry e: the first i in [0, n_seg) with ptr[i + 1] > e (n_seg - 1 when a malformed ptr has none)
__device__ __forceinline__ int gt_segment(const int32_t *__restrict__ ptr, int n_seg, int e) {
    int lo = 0, hi = n_seg;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ptr[mid + 1] > e) hi = mid; else lo = mid + 1;
    }
    return lo < n_seg ? lo : n_seg - 1;
}

template <bool F64>
__global__ void gt_gather_kernel(const gt_elem<F64> *__restrict__ S, int64_t ldS, int64_t row0, int64_t nrows, int Ni, int Nc, int nnz,
                                 const int32_t *__restrict__ img_ptr, const int32_t *__restrict__ img_cap,
                                 const int32_t *__restrict__ cap_ptr, const int32_t *__restrict__ cap_img,
                                 unsigned long long *__restrict__ i2t_key, unsigned long long *__restrict__ t2i_key) {
    const int64_t e64 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e64 >= nnz) return;
    const int e = (int)e64;
    {
        const int64_t li = (int64_t)gt_segment(img_ptr, Ni, e) - row0;
        const int c = img_cap[e];
        if (li >= 0 && li < nrows && c >= 0 && c < Nc) i2t_key[e] = gt_key<F64>(S[li * ldS + c], (uint32_t)c).hi;
    }
    {
        const int j = gt_segment(cap_ptr, Nc, e);
        const int i = cap_img[e];
        const int64_t li = (int64_t)i - row0;
        if (li >= 0 && li < nrows && i < Ni) t2i_key[e] = gt_key<F64>(S[li * ldS + j], (uint32_t)i).hi;
    }
}

// Rank sort inside every query's segment: entry e goes to slot #{u in its segment : key_u < key_e} (keys of a segment are
// distinct).  Quadratic in the positives of a query, which is nothing for tens of them; the row part only for the block's rows.
template <bool F64>
__global__ void gt_sort_kernel(int64_t row0, int64_t nrows, int Ni, int Nc, int nnz, const int32_t *__restrict__ img_ptr,
                               const int32_t *__restrict__ img_cap, const int32_t *__restrict__ cap_ptr, const int32_t *__restrict__ cap_img,
                               const unsigned long long *__restrict__ i2t_key, const unsigned long long *__restrict__ t2i_key,
                               unsigned long long *__restrict__ row_sorted, int32_t *__restrict__ row_perm,
                               unsigned long long *__restrict__ col_sorted, int32_t *__restrict__ col_perm, int32_t *__restrict__ t2i_pos,
                               int init) {
    const int64_t e64 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e64 >= nnz) return;
    const int e = (int)e64;
    if (init) t2i_pos[e] = 0;
    const int i = gt_segment(img_ptr, Ni, e);
    if (i >= row0 && i < row0 + nrows) {
        const int lo = gt_clamp(img_ptr[i], 0, nnz), hi = gt_clamp(img_ptr[i + 1], lo, nnz);
        const GtKey me{i2t_key[e], F64 ? (uint32_t)img_cap[e] : 0u};
        int rank = 0;
        for (int u = lo; u < hi; ++u) rank += gt_less<F64>(GtKey{i2t_key[u], F64 ? (uint32_t)img_cap[u] : 0u}, me);
        if (lo + rank < nnz) { row_sorted[lo + rank] = me.hi; row_perm[lo + rank] = e; }
    }
    const int j = gt_segment(cap_ptr, Nc, e);
    {
        const int lo = gt_clamp(cap_ptr[j], 0, nnz), hi = gt_clamp(cap_ptr[j + 1], lo, nnz);
        const GtKey me{t2i_key[e], F64 ? (uint32_t)cap_img[e] : 0u};
        int rank = 0;
        for (int u = lo; u < hi; ++u) rank += gt_less<F64>(GtKey{t2i_key[u], F64 ? (uint32_t)cap_img[u] : 0u}, me);
        if (lo + rank < nnz) { col_sorted[lo + rank] = me.hi; col_perm[lo + rank] = e; }
    }
}

// bucket of a key that is above thr[0]: #{s < n : thr[s] < key}, in [1, n]
template <bool F64>
__device__ __forceinline__ int gt_bucket(const unsigned long long *s_hi, const uint32_t *s_lo, int n, const GtKey &k) {
    int a = 1, z = n;
    while (a < z) {
        const int m = (a + z) >> 1;
        if (gt_less<F64>(GtKey{s_hi[m], F64 ? s_lo[m] : 0u}, k)) a = m + 1; else z = m;
    }
    return a;
}

// ---- i2t: one workgroup per row of the block ----------------------------------------------------------------------------------
template <bool F64>
__global__ __launch_bounds__(GT_THREADS) void gt_rows_kernel(const gt_elem<F64> *__restrict__ S, int64_t ldS, int64_t row0, int Nc, int nnz,
                                                             const int32_t *__restrict__ img_ptr, const int32_t *__restrict__ img_cap,
                                                             const unsigned long long *__restrict__ row_sorted,
                                                             const int32_t *__restrict__ row_perm, int32_t *__restrict__ i2t_pos) {
    __shared__ unsigned long long s_hi[GT_ROW_CAP];
    __shared__ uint32_t s_lo[F64 ? GT_ROW_CAP : 1];
    // Untrained scores pass the smallest threshold almost everywhere, and a wave's 64 adds then fall on a handful of buckets: the
    // histogram is kept in 2^lc copies, bucket-major, a thread adding to copy (tid mod 2^lc) -- adjacent lanes on adjacent banks, and
    // up to 32 thresholds every thread has a copy of its own.
    __shared__ int s_hist[GT_ROW_HIST];
    __shared__ int s_tot[GT_ROW_CAP];
    const int tid = threadIdx.x;
    const int64_t gi = row0 + blockIdx.x;
    const int lo = gt_clamp(img_ptr[gi], 0, nnz), hi = gt_clamp(img_ptr[gi + 1], lo, nnz);
    if (hi == lo) return;                                                  // an image without positives contributes no entries
    const gt_elem<F64> *row = S + (int64_t)blockIdx.x * ldS;
    // fp32: scalar elements up to the first 16-byte boundary, float4 from there, scalar remainder.  float64: scalar throughout.
    int head = Nc, nvec = 0;
    if constexpr (!F64) {
        head = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(row) & 15u)) & 15u) >> 2);
        head = head < Nc ? head : Nc;
        nvec = (Nc - head) >> 2;
    }
    for (int p0 = lo; p0 < hi; p0 += GT_ROW_CAP) {
        const int n = hi - p0 < GT_ROW_CAP ? hi - p0 : GT_ROW_CAP;
        int my_entry = -1;
        if (tid < n) {
            s_hi[tid] = row_sorted[p0 + tid];
            my_entry = row_perm[p0 + tid];
            if constexpr (F64) s_lo[tid] = (unsigned)my_entry < (unsigned)nnz ? (uint32_t)img_cap[my_entry] : 0u;
        }
        int lc = 8;
        while ((n << lc) > GT_ROW_HIST) --lc;                              // (n <= 256: lc >= 5)
        const int copies = 1 << lc, mine = tid & (copies - 1);
        for (int k = tid; k < (n << lc); k += GT_THREADS) s_hist[k] = 0;
        __syncthreads();
        const GtKey tmin{s_hi[0], F64 ? s_lo[0] : 0u};
        auto visit = [&](gt_elem<F64> e, int col) {
            const GtKey k = gt_key<F64>(e, (uint32_t)col);
            if (gt_less<F64>(tmin, k)) atomicAdd(&s_hist[((gt_bucket<F64>(s_hi, s_lo, n, k) - 1) << lc) + mine], 1);
        };
        for (int c = tid; c < head; c += GT_THREADS) visit(row[c], c);
        if constexpr (!F64) {
            const float4 *rv = reinterpret_cast<const float4 *>(row + head);
            for (int v0 = tid; v0 < nvec; v0 += GT_THREADS * 4) {
                float4 x[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int v = v0 + q * GT_THREADS;
                    x[q] = rv[v < nvec ? v : nvec - 1];
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int v = v0 + q * GT_THREADS;
                    if (v < nvec) {
                        const int c = head + 4 * v;
                        visit(x[q].x, c); visit(x[q].y, c + 1); visit(x[q].z, c + 2); visit(x[q].w, c + 3);
                    }
                }
            }
            for (int c = head + 4 * nvec + tid; c < Nc; c += GT_THREADS) visit(row[c], c);
        }
        __syncthreads();
        if (tid < n) {                                                     // bucket tid over its copies (rotated: no two threads on a bank)
            int tot = 0;
            for (int c = 0; c < copies; ++c) tot += s_hist[(tid << lc) + ((c + tid) & (copies - 1))];
            s_tot[tid] = tot;
        }
        __syncthreads();
        if (tid < n && (unsigned)my_entry < (unsigned)nnz) {
            int acc = 0;
            for (int s = tid; s < n; ++s) acc += s_tot[s];
            i2t_pos[my_entry] = acc;
        }
        __syncthreads();
    }
}

// ---- t2i: a strip of GT_STRIP columns x rows_per_wg rows per workgroup -----------------------------------------------------------
// Every pass takes as many of the strip's still uncounted thresholds as LDS holds, column after column (a column's slice of its
// sorted list is sorted), walks the rows once against them and adds the buckets' suffix sums to the positives' global counters.
template <bool F64>
__global__ __launch_bounds__(GT_THREADS) void gt_cols_kernel(const gt_elem<F64> *__restrict__ S, int64_t ldS, int64_t row0, int64_t nrows, int Nc,
                                                             int nnz, const int32_t *__restrict__ cap_ptr, const int32_t *__restrict__ cap_img,
                                                             const unsigned long long *__restrict__ col_sorted,
                                                             const int32_t *__restrict__ col_perm, int32_t *__restrict__ t2i_pos,
                                                             int rows_per_wg) {
    __shared__ unsigned long long s_hi[GT_COL_CAP];
    __shared__ uint32_t s_lo[F64 ? GT_COL_CAP : 1];
    __shared__ int s_hist[GT_COL_CAP];
    __shared__ int s_off[GT_STRIP + 1];
    __shared__ int s_scan[GT_THREADS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t cb = (int64_t)blockIdx.x * GT_STRIP;
    const int64_t r_begin = (int64_t)blockIdx.y * rows_per_wg;
    const int64_t r_end = r_begin + rows_per_wg < nrows ? r_begin + rows_per_wg : nrows;
    // this thread's column of the strip: its segment of the sorted keys
    int lo = 0, hi = 0;
    if (cb + tid < Nc) {
        lo = gt_clamp(cap_ptr[cb + tid], 0, nnz);
        hi = gt_clamp(cap_ptr[cb + tid + 1], lo, nnz);
    }
    int done = 0;
    // this lane's four columns of the matrix
    const int64_t c0 = cb + lane * 4;
    const int ncol = c0 >= Nc ? 0 : (Nc - c0 >= 4 ? 4 : (int)(Nc - c0));
    bool vec = false;
    if constexpr (!F64) vec = cb + GT_STRIP <= Nc && (ldS & 3) == 0 && (reinterpret_cast<uintptr_t>(S) & 15) == 0;
    for (;;) {
        // sequential allocation of the pass's GT_COL_CAP slots: column t takes min(what it has left, what is left of the budget)
        int rem = hi - lo - done;
        rem = rem < GT_COL_CAP ? rem : GT_COL_CAP;                         // (saturated: the sums below stay small)
        s_scan[tid] = rem;
        __syncthreads();
        for (int d = 1; d < GT_THREADS; d <<= 1) {
            const int t = tid >= d ? s_scan[tid - d] : 0;
            __syncthreads();
            s_scan[tid] += t;
            __syncthreads();
        }
        const int total = s_scan[GT_THREADS - 1];
        if (total == 0) break;                                             // (uniform)
        int off = s_scan[tid] - rem;
        off = off < GT_COL_CAP ? off : GT_COL_CAP;
        const int take = rem < GT_COL_CAP - off ? rem : GT_COL_CAP - off;
        s_off[tid] = off;
        if (tid == 0) s_off[GT_STRIP] = total < GT_COL_CAP ? total : GT_COL_CAP;
        for (int k = 0; k < take; ++k) {
            s_hi[off + k] = col_sorted[lo + done + k];
            if constexpr (F64) {
                const int pe = col_perm[lo + done + k];
                s_lo[off + k] = (unsigned)pe < (unsigned)nnz ? (uint32_t)cap_img[pe] : 0u;
            }
            s_hist[off + k] = 0;
        }
        __syncthreads();
        int o[4], n[4];
        GtKey cmin[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            o[u] = s_off[lane * 4 + u];
            n[u] = s_off[lane * 4 + u + 1] - o[u];
            cmin[u] = n[u] > 0 ? GtKey{s_hi[o[u]], F64 ? s_lo[o[u]] : 0u} : GtKey{~0ull, 0xffffffffu};      // (no key is above all ones)
        }
        auto load_row = [&](int64_t r, gt_elem<F64> (&v)[4]) {
            const gt_elem<F64> *p = S + r * ldS + c0;
            if constexpr (!F64) {
                if (vec) {
                    const float4 x = *reinterpret_cast<const float4 *>(p);
                    v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
                    return;
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = u < ncol ? p[u] : (gt_elem<F64>)0;
        };
        for (int64_t rr = r_begin + wave; rr < r_end; rr += GT_WAVES * GT_COL_U) {
            gt_elem<F64> v[GT_COL_U][4];
#pragma unroll
            for (int q = 0; q < GT_COL_U; ++q) {
                const int64_t r = rr + q * GT_WAVES;
                load_row(r < r_end ? r : r_end - 1, v[q]);
            }
#pragma unroll
            for (int q = 0; q < GT_COL_U; ++q) {
                const int64_t r = rr + q * GT_WAVES;
                if (r < r_end) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const GtKey k = gt_key<F64>(v[q][u], (uint32_t)(row0 + r));
                        if (gt_less<F64>(cmin[u], k))
                            atomicAdd(&s_hist[o[u] + gt_bucket<F64>(s_hi + o[u], s_lo + (F64 ? o[u] : 0), n[u], k) - 1], 1);
                    }
                }
            }
        }
        __syncthreads();
        int acc = 0;
        for (int s = take - 1; s >= 0; --s) {
            acc += s_hist[off + s];
            const int pe = col_perm[lo + done + s];
            if (acc && (unsigned)pe < (unsigned)nnz) atomicAdd(&t2i_pos[pe], acc);
        }
        done += take;
        __syncthreads();
    }
}

struct GtWs { unsigned long long *row_sorted, *col_sorted, *key_i, *key_t; int32_t *row_perm, *col_perm; size_t bytes; };
static GtWs gt_ws(void *base, int64_t nnz, int f64) {
    WsCarver c(base);
    const size_t n = (size_t)(nnz > 0 ? nnz : 0);
    GtWs w;
    w.row_sorted = c.take<unsigned long long>(n * 8);
    w.col_sorted = c.take<unsigned long long>(n * 8);
    w.row_perm = c.take<int32_t>(n * 4);
    w.col_perm = c.take<int32_t>(n * 4);
    w.key_i = c.take<unsigned long long>(f64 ? n * 8 : 0);
    w.key_t = c.take<unsigned long long>(f64 ? n * 8 : 0);
    w.bytes = c.bytes;
    return w;
}

static unsigned gt_entry_blocks(int64_t nnz) { return (unsigned)ceil_div(nnz, (int64_t)256); }

template <bool F64>
static int gt_count(const gt_elem<F64> *S, int64_t ldS, int64_t row0, int64_t n_rows_local, int64_t Nc, int64_t Ni, int64_t nnz,
                    const int32_t *img_ptr, const int32_t *img_cap, const int32_t *cap_ptr, const int32_t *cap_img,
                    const unsigned long long *i2t_key, const unsigned long long *t2i_key, int32_t *i2t_pos, int32_t *t2i_pos, int init,
                    const GtWs &ws, hipStream_t st) {
    hipLaunchKernelGGL(gt_sort_kernel<F64>, dim3(gt_entry_blocks(nnz)), dim3(256), 0, st, row0, n_rows_local, (int)Ni, (int)Nc, (int)nnz, img_ptr,
                       img_cap, cap_ptr, cap_img, i2t_key, t2i_key, ws.row_sorted, ws.row_perm, ws.col_sorted, ws.col_perm, t2i_pos, init);
    ITR_CHECK_LAUNCH("rank_gt_sort");
    hipLaunchKernelGGL(gt_rows_kernel<F64>, dim3((unsigned)n_rows_local), dim3(GT_THREADS), 0, st, S, ldS, row0, (int)Nc, (int)nnz, img_ptr, img_cap,
                       ws.row_sorted, ws.row_perm, i2t_pos);
    ITR_CHECK_LAUNCH("rank_gt_rows");
    const int64_t ns = ceil_div(Nc, (int64_t)GT_STRIP);
    int64_t gy = ceil_div((int64_t)GT_COL_WGS, ns);
    const int64_t gy_max = ceil_div(n_rows_local, (int64_t)(GT_WAVES * GT_COL_U));
    gy = gy < gy_max ? gy : gy_max;
    int64_t rpw = ceil_div(ceil_div(n_rows_local, gy), (int64_t)(GT_WAVES * GT_COL_U)) * (GT_WAVES * GT_COL_U);
    gy = ceil_div(n_rows_local, rpw);
    ITR_REQUIRE(gy <= 65535 && rpw < 0x7fffffffLL, "itr_rank_gt: too many local rows per call");
    hipLaunchKernelGGL(gt_cols_kernel<F64>, dim3((unsigned)ns, (unsigned)gy), dim3(GT_THREADS), 0, st, S, ldS, row0, n_rows_local, (int)Nc, (int)nnz,
                       cap_ptr, cap_img, ws.col_sorted, ws.col_perm, t2i_pos, (int)rpw);
    ITR_CHECK_LAUNCH("rank_gt_cols");
    return ITR_OK;
}

}  // namespace itr

#define ITR_GT_SHAPE(who)                                                                                                                  \
    ITR_REQUIRE(Nc >= 0 && Ni >= 0 && nnz >= 0 && ldS >= Nc && row0 >= 0 && n_rows_local >= 0 && row0 + n_rows_local <= Ni, who ": bad shape"); \
    ITR_UNSUPPORTED(nnz >= 0x7fffffffLL || Nc >= 0x7fffffffLL || Ni >= 0x7fffffffLL, who ": nnz, Ni and Nc must be below 2^31")

extern "C" size_t itr_rank_gt_workspace_bytes(int64_t nnz, int f64) { return itr::gt_ws(nullptr, nnz, f64).bytes; }

extern "C" int itr_rank_gt_gather(const float *S, int64_t ldS, int64_t row0, int64_t n_rows_local, int64_t Nc, int64_t Ni, int64_t nnz,
                                  const int32_t *img_ptr, const int32_t *img_cap, const int32_t *cap_ptr, const int32_t *cap_img,
                                  uint64_t *i2t_key, uint64_t *t2i_key, itr_stream_t stream) {
    ITR_GT_SHAPE("itr_rank_gt_gather");
    if (nnz == 0 || n_rows_local == 0 || Nc == 0) return ITR_OK;
    ITR_REQUIRE(S && img_ptr && img_cap && cap_ptr && cap_img && i2t_key && t2i_key, "itr_rank_gt_gather: null pointer");
    hipLaunchKernelGGL(itr::gt_gather_kernel<false>, dim3(itr::gt_entry_blocks(nnz)), dim3(256), 0, itr::as_stream(stream), S, ldS, row0,
                       n_rows_local, (int)Ni, (int)Nc, (int)nnz, img_ptr, img_cap, cap_ptr, cap_img,
                       reinterpret_cast<unsigned long long *>(i2t_key), reinterpret_cast<unsigned long long *>(t2i_key));
    ITR_CHECK_LAUNCH("rank_gt_gather");
    return ITR_OK;
}

extern "C" int itr_rank_gt_count(const float *S, int64_t ldS, int64_t row0, int64_t n_rows_local, int64_t Nc, int64_t Ni, int64_t nnz,
                                 const int32_t *img_ptr, const int32_t *cap_ptr, const uint64_t *i2t_key, const uint64_t *t2i_key,
                                 int32_t *i2t_pos, int32_t *t2i_pos, int flags, void *workspace, size_t workspace_bytes, itr_stream_t stream) {
    ITR_GT_SHAPE("itr_rank_gt_count");
    ITR_REQUIRE((flags & ~ITR_RANK_GT_INIT) == 0, "itr_rank_gt_count: unknown flag bits %d", flags);
    if (nnz == 0 || n_rows_local == 0 || Nc == 0) return ITR_OK;
    ITR_REQUIRE(S && img_ptr && cap_ptr && i2t_key && t2i_key && i2t_pos && t2i_pos, "itr_rank_gt_count: null pointer");
    ITR_REQUIRE(workspace && workspace_bytes >= itr_rank_gt_workspace_bytes(nnz, 0) && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0,
                "itr_rank_gt_count: workspace missing, misaligned or smaller than itr_rank_gt_workspace_bytes");
    const itr::GtWs ws = itr::gt_ws(workspace, nnz, 0);
    return itr::gt_count<false>(S, ldS, row0, n_rows_local, Nc, Ni, nnz, img_ptr, nullptr, cap_ptr, nullptr,
                                reinterpret_cast<const unsigned long long *>(i2t_key), reinterpret_cast<const unsigned long long *>(t2i_key),
                                i2t_pos, t2i_pos, (flags & ITR_RANK_GT_INIT) ? 1 : 0, ws, itr::as_stream(stream));
}

extern "C" int itr_rank_gt_positions_f64(const double *S, int64_t ldS, int64_t Ni, int64_t Nc, int64_t nnz, const int32_t *img_ptr,
                                         const int32_t *img_cap, const int32_t *cap_ptr, const int32_t *cap_img, int32_t *i2t_pos,
                                         int32_t *t2i_pos, void *workspace, size_t workspace_bytes, itr_stream_t stream) {
    const int64_t row0 = 0, n_rows_local = Ni;
    ITR_GT_SHAPE("itr_rank_gt_positions_f64");
    if (nnz == 0 || Ni == 0 || Nc == 0) return ITR_OK;
    ITR_REQUIRE(S && img_ptr && img_cap && cap_ptr && cap_img && i2t_pos && t2i_pos, "itr_rank_gt_positions_f64: null pointer");
    ITR_REQUIRE(workspace && workspace_bytes >= itr_rank_gt_workspace_bytes(nnz, 1) && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0,
                "itr_rank_gt_positions_f64: workspace missing, misaligned or smaller than itr_rank_gt_workspace_bytes");
    const itr::GtWs ws = itr::gt_ws(workspace, nnz, 1);
    hipStream_t st = itr::as_stream(stream);
    hipLaunchKernelGGL(itr::gt_gather_kernel<true>, dim3(itr::gt_entry_blocks(nnz)), dim3(256), 0, st, S, ldS, row0, Ni, (int)Ni, (int)Nc, (int)nnz,
                       img_ptr, img_cap, cap_ptr, cap_img, ws.key_i, ws.key_t);
    ITR_CHECK_LAUNCH("rank_gt_gather_f64");
    return itr::gt_count<true>(S, ldS, 0, Ni, Nc, Ni, nnz, img_ptr, img_cap, cap_ptr, cap_img, ws.key_i, ws.key_t, i2t_pos, t2i_pos, 1, ws, st);
}
