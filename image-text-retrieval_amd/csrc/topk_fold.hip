// Running top-K column lists (t2i), folded one row block at a time: the sibling of topk.hip's column pass for a similarity matrix that
// is never stored.  The state is topk.hip's column part itself -- col_key [Nc, K] (rank_key(score, GLOBAL row), best first, 0 = empty)
// and col_val [Nc, K] (the score's original bits) -- and a call leaves in it the K largest keys of (the lists before) U (this block's
// entries).  Keys of distinct elements are distinct, so that set and its order are one well-defined thing: the result does not depend
// on how the rows were cut into blocks, on the order of the blocks, or on how the workgroups of a call are scheduled.
//
// One workgroup owns a strip of TF_COLS = 32 columns for the whole call (nobody else reads or writes their lists: the merge needs no
// inter-workgroup order).  A lane owns 4 ADJACENT columns and one row in TF_RL = 32: a 16-byte load per row (global_load_dwordx4; four scalar loads
// when S is not 16-byte aligned or ldS % 4 != 0, and for the strip on the matrix's right edge when Nc % 32 != 0: a launch of its own), TF_U = 4 rows in flight per lane, the next step's loads
// issued before this step is filtered.  The K-th key of each of the lane's columns is its threshold, in registers for a step (reloaded from LDS, where a merge leaves it): ONE 64-bit
// compare per element.  What passes goes to the column's TF_CAND candidate slots in LDS (slot = integer LDS atomic; the order of the
// slots never reaches the output, the candidates are sorted before use).  A lane whose candidate finds its column full keeps the
// element (a bit per element in a register) and asks for a merge; after the merge -- which empties the slots and reloads the
// thresholds -- it offers the element again.  So no candidate is ever dropped and the candidate space is a constant, whatever passes:
// ascending columns or empty lists (everything passes) only merge more often.
//
// The merge works on the lists where they are, in global memory (a strip's lists are ONE contiguous range of TF_COLS * K entries):
//   1. the candidates of every column are sorted (bitonic, in LDS, scores carried with their keys);
//   2. every entry of the union learns its final position: a candidate at j lands on j + #{old entries above it} (binary search in
//      the old list, the whole strip at once: one chain of log2 K dependent loads per merge), an old entry at i on
//      i + #{candidates above it} (binary search in LDS; TF_OLD * 256 entries at a time, those that move wait in registers);
//      entries of columns without candidates are not even read;
//   3. after a barrier (every read of those columns' old lists is done) the entries that moved and land inside the first K are
//      written; the one that lands on K - 1 is the column's new threshold.
// No serial chain over K, no workspace, nothing order-dependent.  DESIGN.md 4.4.2.
#include "itr_internal.h"
#include "select.h"

namespace itr {

constexpr int TF_THREADS = 256;
constexpr int TF_COLS = 32;                               // columns of a strip
constexpr int TF_CL = TF_COLS / 4;                        // lanes across a strip (4 adjacent columns each)
constexpr int TF_RL = TF_THREADS / TF_CL;                 // rows of one load of the workgroup
constexpr int TF_U = 4;                                   // loads in flight per lane
constexpr int TF_STEP = TF_RL * TF_U;                     // rows between two barriers
constexpr int TF_CAND = 64;                               // candidate slots per column (a power of two)
constexpr int TF_OLD = 2;                                 // old entries a thread holds in registers between the two halves of a merge
static_assert((TF_CAND & (TF_CAND - 1)) == 0, "the candidate sort pads to a power of two inside the slots");
static_assert(TF_OLD * TF_THREADS >= ITR_TOPK_MAX && 4 * TF_U <= 32, "a merge group holds at least one column / the todo mask");

__device__ __forceinline__ int tf_min(int a, int b) { return a < b ? a : b; }

// VEC: S is 16-byte aligned, ldS % 4 == 0 and every strip of the launch lies inside the matrix (the host launches the right-edge
// strip of such a matrix on its own, with VEC = false).  A template parameter, so that the 16-byte load and the four guarded scalar
// loads are two kernels: in one kernel hipcc folds the two forms into a dwordx3 + dword pair behind exec-mask branches.
template <bool VEC>
__global__ __launch_bounds__(TF_THREADS, 4) void topk_fold_kernel(const float *__restrict__ S, int64_t ldS, int64_t row0, int64_t nrows, int64_t Nc,
                                                                  int K, int64_t strip0, unsigned long long *col_key, uint32_t *col_val) {
    __shared__ unsigned long long ck[TF_COLS][TF_CAND];   // candidates of a column: keys ...
    __shared__ uint32_t cv[TF_COLS][TF_CAND];             // ... and the bits of their scores
    __shared__ int16_t cpos[TF_COLS][TF_CAND];            // where a candidate lands (-1: below the K-th)
    __shared__ int s_cnt[TF_COLS];                        // candidates offered since the last merge (may exceed TF_CAND)
    __shared__ unsigned long long s_thr[TF_COLS];
    const int tid = threadIdx.x, lc = (tid % TF_CL) * 4, rl = tid / TF_CL;
    const int64_t c0 = (strip0 + blockIdx.x) * TF_COLS;     // first column of the strip
    const int64_t gcol = c0 + lc;
    const int ncols = (int)(Nc - c0 < TF_COLS ? Nc - c0 : TF_COLS);
    unsigned long long *lk = col_key + c0 * K;            // the strip's lists: ncols * K contiguous entries
    uint32_t *lv = col_val + c0 * K;

    const int n = (int)nrows;                             // (row0 + nrows < 2^31: checked by the caller)
    const uint32_t grow = (uint32_t)row0 + (uint32_t)rl;  // global row of this lane's row in the first load
    // Loads are unconditional (straight-line code, nothing waits on a branch): a row past the block reads the block's last row and a
    // column past the matrix its last column; neither is ever offered (the to-do mask, a threshold of ~0).
    auto load = [&](int r, float (*v)[4]) {
#pragma unroll
        for (int u = 0; u < TF_U; ++u) {
            const int rr = tf_min(r + u * TF_RL + rl, n - 1);
            const float *row = S + (int64_t)rr * ldS;
            if constexpr (VEC) {
                const float4 q = *reinterpret_cast<const float4 *>(row + gcol);
                v[u][0] = q.x; v[u][1] = q.y; v[u][2] = q.z; v[u][3] = q.w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[u][e] = row[gcol + e < Nc ? gcol + e : Nc - 1];
            }
        }
    };

    float cur[TF_U][4], nxt[TF_U][4];
    load(0, cur);
    if (tid < TF_COLS) {                                  // (the first rows are on their way while the thresholds are fetched)
        s_cnt[tid] = 0;
        s_thr[tid] = tid < ncols ? lk[(int64_t)tid * K + K - 1] : ~0ull;     // a column past the edge: nothing passes
    }
    __syncthreads();

    // candidates -> lists.  Every thread calls it, behind a barrier that follows the last append.
    auto merge = [&]() {
        int mx = 0;
        for (int q = 0; q < TF_COLS; ++q) mx = s_cnt[q] > mx ? s_cnt[q] : mx;
        if (mx == 0) return;                               // (uniform)
        const int L = next_pow2(tf_min(mx, TF_CAND)), total_c = TF_COLS * L;
        for (int i = tid; i < total_c; i += TF_THREADS) {
            const int q = i / L, li = i % L;
            if (li >= tf_min(s_cnt[q], TF_CAND)) { ck[q][li] = 0ull; cv[q][li] = 0u; }
        }
        __syncthreads();
        bitonic_desc<TF_THREADS>(L, TF_COLS, [&](int q, int a, int b) {      // TF_COLS descending sorts of L entries, scores carried
            const unsigned long long x = ck[q][a], y = ck[q][b];
            if (y > x) {
                const uint32_t vx = cv[q][a], vy = cv[q][b];
                ck[q][a] = y; ck[q][b] = x;
                cv[q][a] = vy; cv[q][b] = vx;
            }
        });
        // where every candidate lands: its index among its column's candidates + #{old entries above it} (binary search in the old
        // list, where it lies; empty entries, key 0, are below every key).  The whole strip at once: ONE chain of dependent loads.
        for (int i = tid; i < total_c; i += TF_THREADS) {
            const int col = i / L, j = i % L;
            int at = -1;
            if (j < tf_min(s_cnt[col], TF_CAND)) {
                const unsigned long long key = ck[col][j];
                const unsigned long long *old = lk + (int64_t)col * K;
                int lo = 0, hi = K;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (old[mid] > key) lo = mid + 1; else hi = mid;
                }
                at = j + lo < K ? j + lo : -1;
            }
            cpos[col][j] = (int16_t)at;
        }
        // old entries, as many columns at a time as TF_OLD entries per thread hold (their lists are one contiguous range; the entries
        // wait in registers until every read of these columns' lists is done); a group without candidates is left alone
        const int mg = tf_min(TF_COLS, TF_OLD * TF_THREADS / K);       // K <= 16: the whole strip in one group; K = 128: 4 columns
        for (int g0 = 0; g0 < ncols; g0 += mg) {
            const int g1 = tf_min(g0 + mg, ncols), total_o = (g1 - g0) * K;
            int any = 0;
            for (int q = g0; q < g1; ++q) any |= s_cnt[q];
            if (any == 0) continue;                        // (uniform)
            unsigned long long ok[TF_OLD];
            uint32_t ov[TF_OLD];
            int op[TF_OLD];
#pragma unroll
            for (int q = 0; q < TF_OLD; ++q) {
                const int e = tid + q * TF_THREADS;
                op[q] = -1;
                ok[q] = 0ull;
                ov[q] = 0u;
                if (e < total_o) {
                    const int col = g0 + e / K, i = e % K, m = tf_min(s_cnt[col], TF_CAND);
                    if (m > 0) {                           // (a column without candidates is not even read)
                        const unsigned long long key = lk[(int64_t)g0 * K + e];
                        int lo = 0, hi = m;                // #{candidates above key}: the candidates are sorted, best first
                        while (lo < hi) {
                            const int mid = (lo + hi) >> 1;
                            if (ck[col][mid] > key) lo = mid + 1; else hi = mid;
                        }
                        const int at = i + lo;
                        if (at == K - 1) s_thr[col] = key;
                        if (lo > 0 && at < K) { op[q] = col * K + at; ok[q] = key; ov[q] = lv[(int64_t)g0 * K + e]; }
                    }
                }
            }
            __syncthreads();                               // every read of these columns' old lists is done (the candidates' too)
#pragma unroll
            for (int q = 0; q < TF_OLD; ++q)
                if (op[q] >= 0) {
                    lk[op[q]] = ok[q];
                    lv[op[q]] = ov[q];
                }
            const int lo_c = g0 * L, hi_c = g1 * L;
            for (int i = lo_c + tid; i < hi_c; i += TF_THREADS) {
                const int col = i / L, j = i % L, at = cpos[col][j];
                if (at >= 0) {
                    const int64_t w = (int64_t)col * K + at;
                    lk[w] = ck[col][j];
                    lv[w] = cv[col][j];
                    if (at == K - 1) s_thr[col] = ck[col][j];
                }
            }
        }
        __syncthreads();                                   // (the counts are read until here)
        if (tid < TF_COLS) s_cnt[tid] = 0;
        __syncthreads();
    };

    for (int r = 0; r < n; r += TF_STEP) {
        load(r + TF_STEP, nxt);                            // the next step is in flight while this one is filtered
        const bool last = r + TF_STEP >= n;
        unsigned todo = 0;                                 // elements of this step not yet compared or placed
#pragma unroll
        for (int u = 0; u < TF_U; ++u)
            if (r + u * TF_RL + rl < n) todo |= 0xfu << (4 * u);
        // offer what is left of the step; true when a column's slots were full
        auto offer = [&]() {
            bool over = false;
            unsigned long long thr[4];                     // the K-th keys of the lane's columns: registers for the step, LDS across merges
#pragma unroll
            for (int e = 0; e < 4; ++e) thr[e] = s_thr[lc + e];
#pragma unroll
            for (int u = 0; u < TF_U; ++u)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const unsigned bit = 1u << (4 * u + e);
                    if (todo & bit) {
                        const unsigned long long k = rank_key(cur[u][e], grow + (uint32_t)(r + u * TF_RL));
                        bool placed = true;
                        if (k > thr[e]) {
                            const int slot = atomicAdd(&s_cnt[lc + e], 1);
                            if (slot < TF_CAND) {
                                ck[lc + e][slot] = k;
                                cv[lc + e][slot] = __float_as_uint(cur[u][e]);
                            } else {
                                placed = false;            // the column's slots are full: merge, then offer it again
                            }
                        }
                        if (placed) todo &= ~bit; else over = true;
                    }
                }
            return over;
        };
        // The first offer is straight-line code behind the loads (no join with the merge's edges: the next step's loads stay in
        // flight); the rare path below has the one call site of the merge, which also serves the end of the block.
        bool again = __syncthreads_or(offer());
        if (again || last)
            for (;;) {
                merge();
                if (!again) break;                         // that was the block's last merge
                again = __syncthreads_or(offer());
                if (!again && !last) break;
            }
#pragma unroll
        for (int u = 0; u < TF_U; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e) cur[u][e] = nxt[u][e];
    }
}

}  // namespace itr

extern "C" size_t itr_topk_fold_workspace_bytes(int64_t n_rows_local, int64_t Nc, int K) {
    (void)n_rows_local; (void)Nc; (void)K;
    return 0;                                              // a strip is merged where it lies: no partial lists
}

extern "C" int itr_topk_fold_cols(const float *S, int64_t ldS, int64_t row0, int64_t n_rows_local, int64_t Nc, int K, uint64_t *col_key,
                                  float *col_val, void *workspace, size_t workspace_bytes, itr_stream_t stream) {
    (void)workspace; (void)workspace_bytes;
    ITR_REQUIRE(S, "itr_topk_fold_cols: null pointer S");
    ITR_REQUIRE(col_key && col_val, "itr_topk_fold_cols: null pointer col_key / col_val");
    ITR_UNSUPPORTED(K < 1 || K > ITR_TOPK_MAX, "itr_topk_fold_cols: K = %d outside 1 .. ITR_TOPK_MAX = %d", K, ITR_TOPK_MAX);
    ITR_REQUIRE(Nc >= 0 && ldS >= Nc && row0 >= 0 && n_rows_local >= 0, "itr_topk_fold_cols: bad shape");
    ITR_REQUIRE(Nc < 0x7fffffffLL && row0 + n_rows_local < 0x7fffffffLL, "itr_topk_fold_cols: index overflow");
    ITR_REQUIRE(n_rows_local < 0x7fff0000LL, "itr_topk_fold_cols: too many rows per call");       // (the kernel counts rows in 32 bits)
    if (n_rows_local == 0 || Nc == 0) return ITR_OK;
    hipStream_t st = itr::as_stream(stream);
    unsigned long long *ck = reinterpret_cast<unsigned long long *>(col_key);
    uint32_t *cv = reinterpret_cast<uint32_t *>(col_val);
    const int64_t strips = itr::ceil_div(Nc, (int64_t)itr::TF_COLS), full = Nc / itr::TF_COLS;
    const bool vec = ((reinterpret_cast<uintptr_t>(S) & 15) == 0) && (ldS % 4 == 0);
    const int64_t n_vec = vec ? full : 0;                  // strips read with 16-byte loads; the rest (all, or the right edge) scalar
    if (n_vec > 0) {
        hipLaunchKernelGGL(itr::topk_fold_kernel<true>, dim3((unsigned)n_vec), dim3(itr::TF_THREADS), 0, st, S, ldS, row0, n_rows_local, Nc, K,
                           (int64_t)0, ck, cv);
        ITR_CHECK_LAUNCH("topk_fold");
    }
    if (strips > n_vec) {
        hipLaunchKernelGGL(itr::topk_fold_kernel<false>, dim3((unsigned)(strips - n_vec)), dim3(itr::TF_THREADS), 0, st, S, ldS, row0,
                           n_rows_local, Nc, K, n_vec, ck, cv);
        ITR_CHECK_LAUNCH("topk_fold_scalar");
    }
    return ITR_OK;
}
