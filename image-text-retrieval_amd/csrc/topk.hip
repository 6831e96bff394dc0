// Top-K retrieval lists (itr/metricmodule/evaluation.py:156-222): the reference argsorts every row (i2t) and every column (t2i) of
// the similarity matrix, `inds = np.argsort(sims[index])[::-1]`, and keeps only inds[0] and the position of the ground truth.  Here
// the K best entries of every line are SELECTED on the GPU, in the ranker's order (rank_key.h): larger score first, the higher index
// on exact ties, -0.0 == +0.0, NaN as +inf.  Keys of distinct elements are distinct, so "the K largest keys" is one well-defined set
// in one well-defined order: column 0 is the ranker's top-1, and lists merged over row blocks (or ranks) equal the whole-matrix list
// for every partition.  Returned scores are the ORIGINAL bits of S at the returned index (read back, never rebuilt from a key).
//
// Both directions use the same filter: a line keeps its current K best keys sorted in LDS; an element is a candidate only when its key
// exceeds the K-th of them (the running threshold), candidates are appended behind the list, and when the candidate space could
// overflow, list + candidates are sorted (bitonic, in LDS) and cut back to K -- which raises the threshold.  On random scores almost
// nothing passes once the first merge has set the threshold; ascending lines (every element passes) only merge more often.
//   i2t (rows):    one workgroup per row walks it in chunks of 1 024 scores (float4 where S is 16-byte aligned and ldS % 4 == 0).
//   t2i (columns): one workgroup per strip of 32 columns and chunk of rows; a lane owns one column (a wave reads 2 rows x 128 bytes),
//                  the 32 lists sit side by side in LDS.  Partial lists of several row chunks are merged by topk_merge_kernel -- the
//                  same kernel that merges the partial lists of several row blocks or ranks (itr_topk_merge).
// Two passes over S (one per direction), not one: a fused pass would have to keep K-lists for every column of a tile next to the
// rows' state (K up to 128: 1 KB per column), which does not fit LDS at a useful tile width.  DESIGN.md 4.5.
#include "itr_internal.h"
#include "select.h"

namespace itr {

constexpr int TK_THREADS = 256;
constexpr int TK_ROW_CAP = 2048;      // LDS entries of a row: its K-list + candidates
constexpr int TK_COL_CAP = 256;       // LDS entries of a column of a strip
constexpr int TK_COL_ROWS = 64;       // rows a strip consumes between two overflow checks (<= TK_COL_CAP - ITR_TOPK_MAX)
constexpr int TK_MERGE_THREADS = 64;
static_assert(TK_COL_CAP - ITR_TOPK_MAX >= TK_COL_ROWS, "a strip's candidate space must hold one step of rows");
static_assert(TK_ROW_CAP - ITR_TOPK_MAX >= TK_THREADS * 4, "a row's candidate space must hold one chunk");

// float64 key: the ordered canonical double, then the index (the fp32 key's rule in 96 bits)
struct Key96 { unsigned long long s; uint32_t i; uint32_t pad; };
__device__ __forceinline__ bool key_gt(unsigned long long a, unsigned long long b) { return a > b; }
__device__ __forceinline__ bool key_gt(const Key96 &a, const Key96 &b) { return a.s > b.s || (a.s == b.s && a.i > b.i); }
// select.h's entry convention for the 96-bit key: empty when its score key is 0
__device__ __forceinline__ uint32_t key_idx(const Key96 &k) { return k.i; }
__device__ __forceinline__ bool key_set(const Key96 &k) { return k.s != 0; }

template <typename T> struct TopkTraits;
template <> struct TopkTraits<float> {
    typedef unsigned long long Key;
    static __device__ __forceinline__ Key key(float v, uint32_t i) { return rank_key(v, i); }
    static __device__ __forceinline__ Key zero() { return 0ull; }
};
template <> struct TopkTraits<double> {
    typedef Key96 Key;
    static __device__ __forceinline__ Key key(double v, uint32_t i) { Key96 k; k.s = double_order_key(canon_f64(v)); k.i = i; k.pad = 0; return k; }
    static __device__ __forceinline__ Key zero() { Key96 k; k.s = 0; k.i = 0; k.pad = 0; return k; }
};

// n_seg independent descending sorts (select.h's network, ordered by key_gt) of L keys each, segment q at buf + q * stride
template <typename Key>
__device__ __forceinline__ void sort_desc(Key *buf, int L, int stride, int n_seg) {
    bitonic_desc<TK_THREADS>(L, n_seg, [=](int q, int a, int b) {
        Key *s = buf + q * stride;
        const Key x = s[a], y = s[b];
        if (key_gt(y, x)) { s[a] = y; s[b] = x; }
    });
}

// ---- i2t: one workgroup per row -------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(TK_THREADS) void topk_rows_kernel(const T *__restrict__ S, int64_t ldS, int64_t Nc, int K,
                                                               int32_t *__restrict__ idx_out, T *__restrict__ val_out) {
    typedef TopkTraits<T> Tr;
    typedef typename Tr::Key Key;
    constexpr int E = 16 / sizeof(T);                 // scores per lane per chunk: one 16-byte load
    constexpr int CHUNK = TK_THREADS * E;
    __shared__ Key buf[TK_ROW_CAP];                    // [0, K): the sorted list; [K, K + s_cnt): candidates
    __shared__ int s_cnt;
    const int tid = threadIdx.x, lane = tid & 63;
    const T *row = S + (int64_t)blockIdx.x * ldS;
    const bool vec = ((reinterpret_cast<uintptr_t>(S) & 15) == 0) && (ldS % E == 0);
    for (int i = tid; i < K; i += TK_THREADS) buf[i] = Tr::zero();
    if (tid == 0) s_cnt = 0;
    Key thr = Tr::zero();
    __syncthreads();
    // list + cnt candidates -> sorted, the first K kept; every thread calls it with the same cnt, no append in flight
    auto merge = [&](int cnt) {
        const int n = K + cnt, L = next_pow2(n);
        for (int i = n + tid; i < L; i += TK_THREADS) buf[i] = Tr::zero();
        __syncthreads();
        sort_desc(buf, L, L, 1);
        thr = buf[K - 1];                              // zero while fewer than K scores have been seen: everything passes
        if (tid == 0) s_cnt = 0;
        __syncthreads();
    };
    auto load = [&](int64_t c0, T *v) {
        const int64_t c = c0 + (int64_t)tid * E;
        if (vec && c0 + CHUNK <= Nc) {
            if constexpr (sizeof(T) == 4) {
                const float4 q = *reinterpret_cast<const float4 *>(row + c);
                v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
            } else {
                const double2 q = *reinterpret_cast<const double2 *>(row + c);
                v[0] = q.x; v[1] = q.y;
            }
        } else {
#pragma unroll
            for (int u = 0; u < E; ++u) v[u] = c + u < Nc ? row[c + u] : T(0);
        }
    };
    T cur[E], nxt[E];
    load(0, cur);
    for (int64_t c0 = 0; c0 < Nc; c0 += CHUNK) {
        if (c0 + CHUNK < Nc) load(c0 + CHUNK, nxt);   // the next chunk is in flight while this one is filtered
        const int cnt = s_cnt;
        __syncthreads();                               // (every wave has read the count before any appends again)
        if (cnt + CHUNK > TK_ROW_CAP - K) merge(cnt);
#pragma unroll
        for (int u = 0; u < E; ++u) {
            const int64_t c = c0 + (int64_t)tid * E + u;
            const Key k = Tr::key(cur[u], (uint32_t)c);
            const bool pass = c < Nc && key_gt(k, thr);
            const unsigned long long m = __builtin_amdgcn_ballot_w64(pass);
            if (m) {                                   // one LDS atomic per wave, slots by lane prefix
                int base = 0;
                if (lane == 0) base = atomicAdd(&s_cnt, (int)__builtin_popcountll(m));
                base = __shfl(base, 0, 64);
                const int off = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                if (pass) buf[K + base + off] = k;
            }
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < E; ++u) cur[u] = nxt[u];
    }
    merge(s_cnt);
    const int64_t o = (int64_t)blockIdx.x * K;
    for (int i = tid; i < K; i += TK_THREADS) {        // K <= Nc: every entry is set
        const uint32_t c = key_idx(buf[i]);
        idx_out[o + i] = (int32_t)c;
        val_out[o + i] = row[c];
    }
}

// ---- t2i: one workgroup per strip of COLS columns x one chunk of rows ----------------------------------------------------------------
// FINAL = false: partial lists (key, score) at [blockIdx.y][Nc][K], empty entries key 0 / score 0 (fp32 only);
// FINAL = true: (global row, score), empty entries -1 / 0.
template <typename T, int COLS, bool FINAL>
__global__ __launch_bounds__(TK_THREADS) void topk_cols_kernel(const T *__restrict__ S, int64_t ldS, int64_t row0, int64_t nrows, int64_t Nc,
                                                               int K, int64_t rows_per_chunk, unsigned long long *__restrict__ key_out,
                                                               int32_t *__restrict__ idx_out, T *__restrict__ val_out) {
    typedef TopkTraits<T> Tr;
    typedef typename Tr::Key Key;
    constexpr int RSTEP = TK_THREADS / COLS;           // rows per load of the workgroup
    constexpr int U = TK_COL_ROWS / RSTEP;             // loads per lane per step
    __shared__ Key buf[COLS][TK_COL_CAP];
    __shared__ int s_cnt[COLS];
    const int tid = threadIdx.x, c = tid % COLS, sub = tid / COLS;
    const int64_t gcol = (int64_t)blockIdx.x * COLS + c;
    const bool colok = gcol < Nc;
    const int64_t r_begin = (int64_t)blockIdx.y * rows_per_chunk;
    const int64_t r_end = r_begin + rows_per_chunk < nrows ? r_begin + rows_per_chunk : nrows;
    for (int i = tid; i < COLS * K; i += TK_THREADS) buf[i / K][i % K] = Tr::zero();
    if (tid < COLS) s_cnt[tid] = 0;
    Key thr = Tr::zero();
    __syncthreads();
    auto merge = [&]() {                               // no append in flight
        int mx = 0;
        for (int q = 0; q < COLS; ++q) mx = s_cnt[q] > mx ? s_cnt[q] : mx;
        const int L = next_pow2(K + mx);
        for (int i = tid; i < COLS * L; i += TK_THREADS) {
            const int q = i / L, li = i % L;
            if (li >= K + s_cnt[q]) buf[q][li] = Tr::zero();
        }
        __syncthreads();
        sort_desc(&buf[0][0], L, TK_COL_CAP, COLS);
        thr = buf[c][K - 1];
        if (tid < COLS) s_cnt[tid] = 0;
        __syncthreads();
    };
    auto load = [&](int64_t r, T *v) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t rr = r + u * RSTEP + sub;
            v[u] = (colok && rr < r_end) ? S[rr * ldS + gcol] : T(0);
        }
    };
    T cur[U], nxt[U];
    load(r_begin, cur);
    for (int64_t r = r_begin; r < r_end; r += TK_COL_ROWS) {
        if (r + TK_COL_ROWS < r_end) load(r + TK_COL_ROWS, nxt);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t rr = r + u * RSTEP + sub;
            const Key k = Tr::key(cur[u], (uint32_t)(row0 + rr));
            if (colok && rr < r_end && key_gt(k, thr)) buf[c][K + atomicAdd(&s_cnt[c], 1)] = k;
        }
        __syncthreads();
        // one more step of rows could overflow a column's candidate space: merge now (the decision is uniform by construction)
        if (__syncthreads_or(sub == 0 && s_cnt[c] + TK_COL_ROWS > TK_COL_CAP - K)) merge();
#pragma unroll
        for (int u = 0; u < U; ++u) cur[u] = nxt[u];
    }
    merge();
    const int64_t base = (int64_t)blockIdx.y * Nc * K;
    for (int i = tid; i < COLS * K; i += TK_THREADS) {
        const int q = i / K, j = i % K;
        const int64_t gc = (int64_t)blockIdx.x * COLS + q;
        if (gc >= Nc) continue;
        const Key k = buf[q][j];
        const bool set = key_set(k);
        const int64_t o = base + gc * K + j;
        if constexpr (FINAL) idx_out[o] = set ? (int32_t)key_idx(k) : -1;
        else key_out[o] = k;
        val_out[o] = set ? S[((int64_t)key_idx(k) - row0) * ldS + gc] : T(0);
    }
}

// ---- merge of sorted partial column lists [P][Nc][K_in] (row chunks of one call, row blocks, ranks) --------------------------------
// One thread per column, a P-way merge of the lists' heads (held in LDS).  Scores move as bit patterns.
__global__ __launch_bounds__(TK_MERGE_THREADS) void topk_merge_kernel(const unsigned long long *__restrict__ pk, const uint32_t *__restrict__ pv,
                                                                     int P, int64_t Nc, int K_in, int K, unsigned long long *__restrict__ key_out,
                                                                     int32_t *__restrict__ idx_out, uint32_t *__restrict__ val_out) {
    __shared__ unsigned long long head[ITR_TOPK_MAX_PARTS][TK_MERGE_THREADS];
    __shared__ uint8_t pos[ITR_TOPK_MAX_PARTS][TK_MERGE_THREADS];
    const int t = threadIdx.x;
    const int64_t j = (int64_t)blockIdx.x * TK_MERGE_THREADS + t;
    if (j >= Nc) return;                               // (no barrier below: every thread touches only its own LDS column)
    for (int p = 0; p < P; ++p) {
        pos[p][t] = 0;
        head[p][t] = pk[((int64_t)p * Nc + j) * K_in];
    }
    for (int o = 0; o < K; ++o) {
        unsigned long long best = 0;
        int bp = -1;
        for (int p = 0; p < P; ++p) {
            const unsigned long long h = head[p][t];
            if (h > best) { best = h; bp = p; }
        }
        uint32_t v = 0;
        if (bp >= 0) {
            const int h = pos[bp][t];
            const int64_t at = ((int64_t)bp * Nc + j) * K_in + h;
            v = pv[at];
            pos[bp][t] = (uint8_t)(h + 1);
            head[bp][t] = h + 1 < K_in ? pk[at + 1] : 0ull;
        }
        const int64_t w = j * K + o;
        if (key_out) key_out[w] = best;
        if (idx_out) idx_out[w] = key_index(best);
        val_out[w] = v;
    }
}

// Row chunks of the fp32 column pass: chunks of >= 2 048 rows (a partial list is then short next to the rows it summarises), at most 4
// (enough workgroups to fill the chip at Nc = 25 000: 782 strips x 3).  A single chunk writes the caller's lists directly.
struct TopkPlan { int64_t chunks, rows_per_chunk; };
static TopkPlan topk_plan(int64_t n_rows, int K) {
    TopkPlan p;
    int64_t rpc = 16 * (int64_t)K > 2048 ? 16 * (int64_t)K : 2048;
    p.chunks = n_rows > 0 ? ceil_div(n_rows, rpc) : 1;
    if (p.chunks > 4) p.chunks = 4;
    p.rows_per_chunk = ceil_div(ceil_div(n_rows > 0 ? n_rows : 1, p.chunks), (int64_t)TK_COL_ROWS) * TK_COL_ROWS;
    p.chunks = ceil_div(n_rows > 0 ? n_rows : 1, p.rows_per_chunk);
    return p;
}

struct TopkWs { unsigned long long *keys; float *vals; size_t bytes; };
static TopkWs topk_ws(void *base, int64_t n_rows, int64_t Nc, int K) {
    WsCarver c(base);
    TopkWs w{nullptr, nullptr, 0};
    const TopkPlan p = topk_plan(n_rows, K);
    if (p.chunks > 1 && Nc > 0) {
        w.keys = c.take<unsigned long long>((size_t)(p.chunks * Nc * K) * 8);
        w.vals = c.take<float>((size_t)(p.chunks * Nc * K) * 4);
    }
    w.bytes = c.bytes;
    return w;
}

static int merge_launch(const unsigned long long *pk, const float *pv, int P, int64_t Nc, int K_in, int K, unsigned long long *key_out,
                        int32_t *idx_out, float *val_out, hipStream_t st) {
    hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)ceil_div(Nc, (int64_t)TK_MERGE_THREADS)), dim3(TK_MERGE_THREADS), 0, st, pk,
                       reinterpret_cast<const uint32_t *>(pv), P, Nc, K_in, K, key_out, idx_out, reinterpret_cast<uint32_t *>(val_out));
    ITR_CHECK_LAUNCH("topk_merge");
    return ITR_OK;
}

}  // namespace itr

extern "C" size_t itr_topk_workspace_bytes(int64_t n_rows_local, int64_t Nc, int K) {
    if (K < 1 || K > ITR_TOPK_MAX || n_rows_local < 0 || Nc < 0) return 0;
    return itr::topk_ws(nullptr, n_rows_local, Nc, K).bytes;
}

extern "C" int itr_topk(const float *S, int64_t ldS, int64_t row0, int64_t n_rows_local, int64_t Nc, int K, int32_t *row_idx,
                        float *row_val, uint64_t *col_key, float *col_val, void *workspace, size_t workspace_bytes, itr_stream_t stream) {
    ITR_REQUIRE(S, "itr_topk: null pointer S");
    ITR_REQUIRE(!row_idx == !row_val && !col_key == !col_val, "itr_topk: pass both outputs of a direction, or neither");
    ITR_REQUIRE(row_idx || col_key, "itr_topk: no direction requested (all outputs NULL)");
    ITR_REQUIRE(K >= 1, "itr_topk: K must be >= 1, got %d", K);
    ITR_UNSUPPORTED(K > ITR_TOPK_MAX, "itr_topk: K = %d > ITR_TOPK_MAX = %d", K, ITR_TOPK_MAX);
    ITR_REQUIRE(Nc >= 0 && ldS >= Nc && row0 >= 0 && n_rows_local >= 0, "itr_topk: bad shape");
    ITR_REQUIRE(Nc < 0x7fffffffLL && row0 + n_rows_local < 0x7fffffffLL, "itr_topk: index overflow");
    ITR_REQUIRE(!row_idx || Nc == 0 || K <= Nc, "itr_topk: K = %d is longer than a row (%lld columns)", K, (long long)Nc);
    if (n_rows_local == 0 || Nc == 0) return ITR_OK;
    ITR_REQUIRE(n_rows_local <= 0x7fffffffLL, "itr_topk: too many rows per call");
    hipStream_t st = itr::as_stream(stream);
    if (row_idx) {
        hipLaunchKernelGGL(itr::topk_rows_kernel<float>, dim3((unsigned)n_rows_local), dim3(itr::TK_THREADS), 0, st, S, ldS, Nc, K,
                           row_idx, row_val);
        ITR_CHECK_LAUNCH("topk_rows");
    }
    if (col_key) {
        const itr::TopkPlan p = itr::topk_plan(n_rows_local, K);
        const size_t need = itr_topk_workspace_bytes(n_rows_local, Nc, K);
        ITR_REQUIRE(need == 0 || (workspace && workspace_bytes >= need && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0),
                    "itr_topk: workspace missing, misaligned or smaller than itr_topk_workspace_bytes");
        const itr::TopkWs ws = itr::topk_ws(need ? workspace : nullptr, n_rows_local, Nc, K);
        unsigned long long *kdst = p.chunks > 1 ? ws.keys : reinterpret_cast<unsigned long long *>(col_key);
        float *vdst = p.chunks > 1 ? ws.vals : col_val;
        dim3 grid((unsigned)itr::ceil_div(Nc, (int64_t)32), (unsigned)p.chunks);
        hipLaunchKernelGGL((itr::topk_cols_kernel<float, 32, false>), grid, dim3(itr::TK_THREADS), 0, st, S, ldS, row0, n_rows_local, Nc, K,
                           p.rows_per_chunk, kdst, (int32_t *)nullptr, vdst);
        ITR_CHECK_LAUNCH("topk_cols");
        if (p.chunks > 1) {
            const int rc = itr::merge_launch(ws.keys, ws.vals, (int)p.chunks, Nc, K, K, reinterpret_cast<unsigned long long *>(col_key),
                                             nullptr, col_val, st);
            if (rc != ITR_OK) return rc;
        }
    }
    return ITR_OK;
}

extern "C" int itr_topk_merge(const uint64_t *part_key, const float *part_val, int n_parts, int64_t Nc, int K_in, int K, int32_t *col_idx,
                              float *col_val, itr_stream_t stream) {
    ITR_REQUIRE(part_key && part_val && col_idx && col_val, "itr_topk_merge: null pointer");
    ITR_REQUIRE(K >= 1 && K_in >= 1 && n_parts >= 1, "itr_topk_merge: K, K_in and n_parts must be >= 1");
    ITR_UNSUPPORTED(K > ITR_TOPK_MAX || K_in > ITR_TOPK_MAX, "itr_topk_merge: K = %d / K_in = %d > ITR_TOPK_MAX = %d", K, K_in, ITR_TOPK_MAX);
    ITR_UNSUPPORTED(n_parts > ITR_TOPK_MAX_PARTS, "itr_topk_merge: %d parts > ITR_TOPK_MAX_PARTS = %d", n_parts, ITR_TOPK_MAX_PARTS);
    ITR_REQUIRE((int64_t)K <= (int64_t)n_parts * K_in, "itr_topk_merge: K = %d is longer than the merged lists (%d x %d)", K, n_parts, K_in);
    ITR_REQUIRE(Nc >= 0, "itr_topk_merge: bad shape");
    if (Nc == 0) return ITR_OK;
    return itr::merge_launch(reinterpret_cast<const unsigned long long *>(part_key), part_val, n_parts, Nc, K_in, K, nullptr, col_idx,
                             col_val, itr::as_stream(stream));
}

extern "C" int itr_topk_f64(const double *S, int64_t ldS, int64_t n_rows, int64_t Nc, int K, int32_t *row_idx, double *row_val,
                            int32_t *col_idx, double *col_val, itr_stream_t stream) {
    ITR_REQUIRE(S, "itr_topk_f64: null pointer S");
    ITR_REQUIRE(!row_idx == !row_val && !col_idx == !col_val, "itr_topk_f64: pass both outputs of a direction, or neither");
    ITR_REQUIRE(row_idx || col_idx, "itr_topk_f64: no direction requested (all outputs NULL)");
    ITR_REQUIRE(K >= 1, "itr_topk_f64: K must be >= 1, got %d", K);
    ITR_UNSUPPORTED(K > ITR_TOPK_MAX, "itr_topk_f64: K = %d > ITR_TOPK_MAX = %d", K, ITR_TOPK_MAX);
    ITR_REQUIRE(Nc >= 0 && ldS >= Nc && n_rows >= 0, "itr_topk_f64: bad shape");
    ITR_REQUIRE(Nc < 0x7fffffffLL && n_rows < 0x7fffffffLL, "itr_topk_f64: index overflow");
    if (n_rows == 0 || Nc == 0) return ITR_OK;
    ITR_REQUIRE(!row_idx || K <= Nc, "itr_topk_f64: K = %d is longer than a row (%lld columns)", K, (long long)Nc);
    ITR_REQUIRE(!col_idx || K <= n_rows, "itr_topk_f64: K = %d is longer than a column (%lld rows)", K, (long long)n_rows);
    hipStream_t st = itr::as_stream(stream);
    if (row_idx) {
        hipLaunchKernelGGL(itr::topk_rows_kernel<double>, dim3((unsigned)n_rows), dim3(itr::TK_THREADS), 0, st, S, ldS, Nc, K, row_idx, row_val);
        ITR_CHECK_LAUNCH("topk_rows_f64");
    }
    if (col_idx) {
        hipLaunchKernelGGL((itr::topk_cols_kernel<double, 16, true>), dim3((unsigned)itr::ceil_div(Nc, (int64_t)16), 1), dim3(itr::TK_THREADS), 0,
                           st, S, ldS, (int64_t)0, n_rows, Nc, K, n_rows, (unsigned long long *)nullptr, col_idx, col_val);
        ITR_CHECK_LAUNCH("topk_cols_f64");
    }
    return ITR_OK;
}
