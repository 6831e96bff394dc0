// Query-time search: the K best gallery rows of a few queries, scored and selected in ONE pass over the gallery.  The questions the
// reference answers with a split-sized matrix (Objectives.py:18-21 cosine_sim, then inds = np.argsort(sims[index])[::-1],
// evaluation.py:169, :209) are asked here for 1 .. ITR_SEARCH_MAX_QUERIES queries against a gallery that is read once; the score
// matrix is never written.
//
// Score: the bits of itr_cosine_scores(queries, gallery).  Every kernel behind that entry keeps ONE fp32 accumulator per element and
// never splits K, but its chain is not k-ascending: the 128 x 128 x 32 tile kernels (gemm_f32.hip) feed v_mfma_f32_32x32x2_f32 -- bit
// for bit D = fma(a_k1, b_k1, fma(a_k0, b_k0, C)) -- with k0 = 8 b + j from lane group 0 and k1 = 8 b + 4 + j from lane group 1, j = 0 .. 3,
// so inside every block of 8 the order is k = 0, 4, 1, 5, 2, 6, 3, 7, blocks ascending, and D is padded with zeros to a multiple of 32
// (fmaf(0, 0, acc) steps: they only turn an underflowed -0.0 into +0.0).  s(q, g) here is exactly that chain from +0.0, on the vector
// ALU with explicit fmaf; nothing else about the order is free.
// Order: rank_key(score, row0 + local row) of rank_key.h.  Keys of distinct rows are distinct, so "the K largest keys of a query" is
// one set in one order, whatever the slabs, the scheduling or the grouping of the queries.
//
// Shape.  The gallery is cut into n_slabs slabs of ceil(N / n_slabs) rows; ONE workgroup of 256 threads owns a slab and walks it in
// tiles of SR_TR rows, a tile in chunks of SR_KC = 32 floats of D.  A chunk goes global -> registers (16-byte loads where base and
// leading dimension allow it, guarded scalar loads otherwise; the next chunk's loads are issued before this chunk is multiplied) ->
// LDS (rows padded to 36 floats: conflict-free 16-byte reads), next to the same chunk of the (zero-padded) queries.  A thread owns
// RT rows x 4 queries: per block of 8 k it reads 2 (RT + 4) 16-byte LDS words and issues 32 RT fmaf.  Three instances by the number of queries:
//     n_queries <=  4:   1 query group  x 256 row threads, RT = 1, tile 256 rows
//     n_queries <= 16:   4 query groups x  64 row threads, RT = 4, tile 256 rows
//     n_queries <= 64:  16 query groups x  16 row threads, RT = 8, tile 128 rows
// Selection follows topk.hip / topk_fold.hip: the K-th key of every query is its threshold (0 while the list is short: every key is
// > 0), a score whose key beats it goes to one of the query's candidate slots in LDS (integer LDS atomic; the slot order never
// reaches the output), and before a step of rows is offered every query whose slots could overflow in that step is merged: list
// (in the slab's part, global memory) + candidates are sorted (bitonic, in LDS, score bits carried with their keys) and cut back to
// K, which raises the threshold.  A step offers at most one row per row thread and the slots hold two steps, so nothing is ever
// dropped: ascending galleries only merge more often.  The slab's part is [n_queries][K] in the layout of itr_topk's column part.
// search_merge_kernel then merges the slabs' parts, up to 32 at a time (one workgroup per query and group: one bitonic sort of all
// their entries), in as many levels as it takes; the last level writes key / val / idx.  DESIGN.md 4.4.5.
#include "itr_internal.h"
#include "select.h"

namespace itr {

constexpr int SR_THREADS = 256;
constexpr int SR_KC = 32;                                 // floats of D per chunk
constexpr int SR_LD = SR_KC + 4;                          // LDS row stride (floats): 16 lanes x 16 bytes hit 64 distinct banks
constexpr int SR_SLOTS = 2048;                            // candidate slots of a workgroup, all queries together
constexpr int SR_SORT = 1024;                             // entries of the merge's sort buffer
constexpr int SR_MERGE_PARTS = 32;                        // parts one merge workgroup takes
constexpr int SR_MERGE_CAP = SR_MERGE_PARTS * ITR_TOPK_MAX;
static_assert(ITR_SEARCH_MAX_QUERIES == 64, "the widest instance holds 16 query groups of 4");

__device__ __forceinline__ int sr_min(int a, int b) { return a < b ? a : b; }

// n_seg independent descending sorts (select.h's network) of L entries, segment s at [s * L, (s + 1) * L); the scores' bits move
// with their keys
__device__ __forceinline__ void sr_sort_desc(unsigned long long *k, uint32_t *v, int L, int n_seg) {
    bitonic_desc<SR_THREADS>(L, n_seg, [=](int s, int a, int b) {
        a += s * L; b += s * L;
        const unsigned long long x = k[a], y = k[b];
        if (y > x) {
            const uint32_t vx = v[a], vy = v[b];
            k[a] = y; k[b] = x;
            v[a] = vy; v[b] = vx;
        }
    });
}

// NQG query groups of 4.  VEC: both operands are 16-byte aligned with leading dimensions that are multiples of 4.
template <int NQG, bool VEC>
__global__ __launch_bounds__(SR_THREADS, 2) void search_slab_kernel(const float *__restrict__ Qm, int64_t ldq, int n_queries,
                                                                 const float *__restrict__ Gm, int64_t ldg, int64_t row0, int64_t n_gallery,
                                                                 int D, int K, int64_t rows_per_slab, unsigned long long *part_key,
                                                                 uint32_t *part_val) {
    constexpr int NRT = SR_THREADS / NQG;                 // row threads
    constexpr int RT = NQG == 1 ? 1 : NQG == 4 ? 4 : 8;   // rows per thread
    constexpr int TR = NRT * RT;                          // rows per tile
    constexpr int NQ = 4 * NQG;                           // queries, padded
    constexpr int CAND = SR_SLOTS / NQ;                   // candidate slots per query: two steps of NRT rows
    constexpr int GU = TR * (SR_KC / 4) / SR_THREADS;     // 16-byte gallery loads per thread and chunk
    constexpr int QU = (NQ * (SR_KC / 4) + SR_THREADS - 1) / SR_THREADS;
    static_assert(CAND == 2 * NRT && ITR_TOPK_MAX + CAND <= SR_SORT, "slots hold two steps / the sort buffer holds a list and its slots");
    static_assert((TR + NQ) * SR_LD * 4 >= SR_SORT * 12, "the sort buffer lies in the staging space");

    // the chunk of the tile's rows, then of the queries; between two tiles the same space is the merge's sort buffer (keys, then scores)
    __shared__ __attribute__((aligned(16))) float stage_buf[(TR + NQ) * SR_LD];
    float *gl = stage_buf, *ql = stage_buf + TR * SR_LD;
    unsigned long long *sk = reinterpret_cast<unsigned long long *>(stage_buf);
    uint32_t *sv = reinterpret_cast<uint32_t *>(stage_buf) + 2 * SR_SORT;
    __shared__ unsigned long long ck[NQ][CAND];           // candidates: keys ...
    __shared__ uint32_t cv[NQ][CAND];                     // ... and the bits of their scores
    __shared__ unsigned long long s_thr[NQ];
    __shared__ int s_cnt[NQ];
    __shared__ int s_mq[NQ];
    __shared__ int s_nm;

    const int tid = threadIdx.x, rt = tid % NRT, qg = tid / NRT;
    const int64_t r_begin = (int64_t)blockIdx.x * rows_per_slab;
    const int64_t r_end = r_begin + rows_per_slab < n_gallery ? r_begin + rows_per_slab : n_gallery;
    unsigned long long *lk = part_key + (int64_t)blockIdx.x * n_queries * K;     // this slab's part: [n_queries][K]
    uint32_t *lv = part_val + (int64_t)blockIdx.x * n_queries * K;

    for (int i = tid; i < n_queries * K; i += SR_THREADS) { lk[i] = 0ull; lv[i] = 0u; }
    if (tid < NQ) {
        s_cnt[tid] = 0;
        s_thr[tid] = tid < n_queries ? 0ull : ~0ull;      // a padded query: nothing passes
    }
    __syncthreads();
    if (r_begin >= r_end) return;                         // an empty slab: an empty part (uniform)

    const int n_rows = (int)(r_end - r_begin);            // (< 2^31: checked by the caller)
    const int n_tiles = (n_rows + TR - 1) / TR, n_ch = (D + SR_KC - 1) / SR_KC;
    const int L = next_pow2(K + CAND), G = SR_SORT / L;

    // chunk `c` of tile `t` -> registers.  A row past the slab reads the slab's last row (never offered); k past D reads 0 (the GEMM's padding).
    float4 gr[GU], qr[QU];
    auto load = [&](int t, int c) {
        const int k0 = c * SR_KC;
#pragma unroll
        for (int u = 0; u < GU; ++u) {
            const int e = tid + u * SR_THREADS, r = sr_min(t * TR + e / (SR_KC / 4), n_rows - 1), k = k0 + (e % (SR_KC / 4)) * 4;
            const float *p = Gm + (r_begin + r) * ldg + k;
            if (VEC && k + 4 <= D) {
                gr[u] = *reinterpret_cast<const float4 *>(p);
            } else {
                gr[u].x = k + 0 < D ? p[0] : 0.f;
                gr[u].y = k + 1 < D ? p[1] : 0.f;
                gr[u].z = k + 2 < D ? p[2] : 0.f;
                gr[u].w = k + 3 < D ? p[3] : 0.f;
            }
        }
#pragma unroll
        for (int u = 0; u < QU; ++u) {
            const int e = tid + u * SR_THREADS, q = e / (SR_KC / 4), k = k0 + (e % (SR_KC / 4)) * 4;
            qr[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (q < n_queries) {
                const float *p = Qm + (int64_t)q * ldq + k;
                if (VEC && k + 4 <= D) {
                    qr[u] = *reinterpret_cast<const float4 *>(p);
                } else {
                    qr[u].x = k + 0 < D ? p[0] : 0.f;
                    qr[u].y = k + 1 < D ? p[1] : 0.f;
                    qr[u].z = k + 2 < D ? p[2] : 0.f;
                    qr[u].w = k + 3 < D ? p[3] : 0.f;
                }
            }
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int u = 0; u < GU; ++u) {
            const int e = tid + u * SR_THREADS;
            *reinterpret_cast<float4 *>(&gl[(e / (SR_KC / 4)) * SR_LD + (e % (SR_KC / 4)) * 4]) = gr[u];
        }
#pragma unroll
        for (int u = 0; u < QU; ++u) {
            const int e = tid + u * SR_THREADS;
            if (e < NQ * (SR_KC / 4)) *reinterpret_cast<float4 *>(&ql[(e / (SR_KC / 4)) * SR_LD + (e % (SR_KC / 4)) * 4]) = qr[u];
        }
    };

    // list + candidates -> list, for every query holding more than `limit` candidates.  Every thread calls it, behind a barrier that
    // follows the last append.
    auto merge = [&](int limit) {
        if (tid == 0) {
            int n = 0;
            for (int q = 0; q < n_queries; ++q)
                if (s_cnt[q] > limit) s_mq[n++] = q;
            s_nm = n;
        }
        __syncthreads();
        const int nm = s_nm;
        for (int m0 = 0; m0 < nm; m0 += G) {
            const int ns = sr_min(G, nm - m0);
            for (int e = tid; e < ns * L; e += SR_THREADS) {
                const int q = s_mq[m0 + e / L], li = e % L, cnt = s_cnt[q];
                unsigned long long key = 0ull;
                uint32_t val = 0u;
                if (li < K) { key = lk[q * K + li]; val = lv[q * K + li]; }
                else if (li < K + cnt) { key = ck[q][li - K]; val = cv[q][li - K]; }
                sk[e] = key; sv[e] = val;
            }
            __syncthreads();
            sr_sort_desc(sk, sv, L, ns);
            for (int e = tid; e < ns * K; e += SR_THREADS) {
                const int s = e / K, i = e % K, q = s_mq[m0 + s];
                const unsigned long long key = sk[s * L + i];
                lk[q * K + i] = key; lv[q * K + i] = sv[s * L + i];
                if (i == K - 1) s_thr[q] = key;
                if (i == 0) s_cnt[q] = 0;
            }
            __syncthreads();
        }
    };

    float acc[RT][4];
    load(0, 0);
    for (int t = 0; t < n_tiles; ++t) {
#pragma unroll
        for (int i = 0; i < RT; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
        for (int c = 0; c < n_ch; ++c) {
            __syncthreads();                              // the previous chunk has been read by everyone
            stage();
            __syncthreads();
            if (c + 1 < n_ch) load(t, c + 1);             // in flight while this chunk is multiplied
            else if (t + 1 < n_tiles) load(t + 1, 0);
            const float *qp = &ql[(4 * qg) * SR_LD];
#pragma unroll 1
            for (int kk = 0; kk < SR_KC; kk += 8) {       // one 8-block of the GEMM's chain: k = 0, 4, 1, 5, 2, 6, 3, 7
                float4 qlo[4], qhi[4], glo[RT], ghi[RT];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    qlo[j] = *reinterpret_cast<const float4 *>(qp + j * SR_LD + kk);
                    qhi[j] = *reinterpret_cast<const float4 *>(qp + j * SR_LD + kk + 4);
                }
#pragma unroll
                for (int i = 0; i < RT; ++i) {
                    glo[i] = *reinterpret_cast<const float4 *>(&gl[(rt + i * NRT) * SR_LD + kk]);
                    ghi[i] = *reinterpret_cast<const float4 *>(&gl[(rt + i * NRT) * SR_LD + kk + 4]);
                }
#pragma unroll
                for (int i = 0; i < RT; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        float a = acc[i][j];
                        a = fmaf(qlo[j].x, glo[i].x, a);
                        a = fmaf(qhi[j].x, ghi[i].x, a);
                        a = fmaf(qlo[j].y, glo[i].y, a);
                        a = fmaf(qhi[j].y, ghi[i].y, a);
                        a = fmaf(qlo[j].z, glo[i].z, a);
                        a = fmaf(qhi[j].z, ghi[i].z, a);
                        a = fmaf(qlo[j].w, glo[i].w, a);
                        a = fmaf(qhi[j].w, ghi[i].w, a);
                        acc[i][j] = a;
                    }
            }
        }
        // the tile's scores -> candidates, one step of NRT rows at a time
#pragma unroll
        for (int i = 0; i < RT; ++i) {
            __syncthreads();                              // the appends of the previous step are counted
            if (__syncthreads_or(tid < NQ && s_cnt[tid] > CAND - NRT)) merge(CAND - NRT);
            const int r = t * TR + rt + i * NRT;
            if (r < n_rows) {
                const uint32_t grow = (uint32_t)(row0 + r_begin + r);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int q = 4 * qg + j;
                    const unsigned long long key = rank_key(acc[i][j], grow);
                    if (key > s_thr[q]) {
                        const int slot = atomicAdd(&s_cnt[q], 1);
                        ck[q][slot] = key;
                        cv[q][slot] = __float_as_uint(acc[i][j]);
                    }
                }
            }
        }
    }
    __syncthreads();
    merge(0);
}

// Parts [P][n_queries][K] -> [gridDim.x][n_queries][K]: workgroup (g, q) sorts the entries of parts g * 32 .. of query q and keeps
// the first K.  FINAL (one group): key / val / idx of the call, idx may be null.
template <bool FINAL>
__global__ __launch_bounds__(SR_THREADS) void search_merge_kernel(const unsigned long long *__restrict__ pk, const uint32_t *__restrict__ pv, int P,
                                                                  int n_queries, int K, unsigned long long *key_out, uint32_t *val_out,
                                                                  int32_t *idx_out) {
    __shared__ unsigned long long sk[SR_MERGE_CAP];
    __shared__ uint32_t sv[SR_MERGE_CAP];
    const int tid = threadIdx.x, q = blockIdx.y, p0 = blockIdx.x * SR_MERGE_PARTS, np = sr_min(SR_MERGE_PARTS, P - p0);
    const int n = np > 0 ? np * K : 0, L = next_pow2(n > K ? n : K);
    for (int e = tid; e < L; e += SR_THREADS) {
        unsigned long long key = 0ull;
        uint32_t val = 0u;
        if (e < n) {
            const int64_t at = ((int64_t)(p0 + e / K) * n_queries + q) * K + e % K;
            key = pk[at]; val = pv[at];
        }
        sk[e] = key; sv[e] = val;
    }
    __syncthreads();
    sr_sort_desc(sk, sv, L, 1);
    const int64_t o = ((int64_t)blockIdx.x * n_queries + q) * K;
    for (int i = tid; i < K; i += SR_THREADS) {
        const unsigned long long key = sk[i];
        key_out[o + i] = key;
        val_out[o + i] = sv[i];                           // (an empty entry carries score bits 0)
        if (FINAL && idx_out) idx_out[o + i] = key_index(key);
    }
}

struct SearchPlan { int nqg; int64_t slabs, rows_per_slab; };
// n_slabs = 0: slabs of at least one tile and 8 K rows (a short slab lists most of its rows), at most as many as the chip holds at once
static SearchPlan search_plan(int64_t n_queries, int64_t n_gallery, int K, int n_slabs) {
    SearchPlan p;
    p.nqg = n_queries <= 4 ? 1 : n_queries <= 16 ? 4 : 16;
    const int64_t tr = p.nqg == 16 ? 128 : 256, cap = 512;      // two workgroups per CU: LDS, and 2 waves per SIMD
    int64_t s = n_slabs;
    if (s <= 0) {
        const int64_t rmin = tr > 8 * (int64_t)K ? tr : 8 * (int64_t)K;
        s = n_gallery / rmin;
        s = s < 1 ? 1 : s > cap ? cap : s;
    }
    p.slabs = s;
    p.rows_per_slab = n_gallery > 0 ? ceil_div(n_gallery, s) : 1;
    return p;
}

// The merge levels: parts[0] parts of the slabs, then what every merge level but the last leaves.  The walk that sizes the workspace
// is the one itr_search_topk's launches follow; all zero (no parts, null pointers) is an empty gallery.
struct SearchWs { int64_t parts[3]; unsigned long long *key[3]; uint32_t *val[3]; size_t bytes; };
static SearchWs search_ws(void *base, int64_t n_queries, int64_t n_gallery, int K, int n_slabs) {
    WsCarver c(base);
    SearchWs w{};
    int64_t parts = search_plan(n_queries, n_gallery, K, n_slabs).slabs;
    for (int lvl = 0; lvl < 3; ++lvl) {
        w.parts[lvl] = parts;
        w.key[lvl] = c.take<unsigned long long>((size_t)(parts * n_queries * K) * 8);
        w.val[lvl] = c.take<uint32_t>((size_t)(parts * n_queries * K) * 4);
        if (parts <= SR_MERGE_PARTS) break;
        parts = ceil_div(parts, (int64_t)SR_MERGE_PARTS);
    }
    w.bytes = c.bytes;
    return w;
}
static_assert(ITR_SEARCH_MAX_SLABS <= SR_MERGE_PARTS * SR_MERGE_PARTS * SR_MERGE_PARTS, "three levels bring every slab count down to one group");

template <int NQG>
static void slab_launch(bool vec, unsigned slabs, hipStream_t st, const float *Q, int64_t ldq, int nq, const float *G, int64_t ldg, int64_t row0,
                        int64_t n, int D, int K, int64_t rps, unsigned long long *pk, uint32_t *pv) {
    if (vec) hipLaunchKernelGGL((search_slab_kernel<NQG, true>), dim3(slabs), dim3(SR_THREADS), 0, st, Q, ldq, nq, G, ldg, row0, n, D, K, rps, pk, pv);
    else hipLaunchKernelGGL((search_slab_kernel<NQG, false>), dim3(slabs), dim3(SR_THREADS), 0, st, Q, ldq, nq, G, ldg, row0, n, D, K, rps, pk, pv);
}

}  // namespace itr

extern "C" size_t itr_search_topk_workspace_bytes(int64_t n_queries, int64_t n_gallery, int K, int n_slabs) {
    if (K < 1 || K > ITR_TOPK_MAX || n_queries < 1 || n_queries > ITR_SEARCH_MAX_QUERIES || n_gallery < 0 || n_slabs < 0 ||
        n_slabs > ITR_SEARCH_MAX_SLABS)
        return 0;
    return itr::search_ws(nullptr, n_queries, n_gallery, K, n_slabs).bytes;
}

extern "C" int itr_search_topk(const float *queries, int64_t ldq, int64_t n_queries, const float *gallery, int64_t ldg, int64_t row0,
                               int64_t n_gallery, int64_t D, int K, int n_slabs, uint64_t *key, float *val, int32_t *idx, void *workspace,
                               size_t workspace_bytes, itr_stream_t stream) {
    ITR_REQUIRE(n_queries >= 0 && n_gallery >= 0 && row0 >= 0, "itr_search_topk: negative size");
    ITR_REQUIRE(D >= 1 && D < 0x7fffffffLL, "itr_search_topk: D = %lld must be >= 1", (long long)D);
    ITR_REQUIRE(ldq >= D && ldg >= D, "itr_search_topk: leading dimension below D");
    ITR_REQUIRE(row0 + n_gallery < 0x7fffffffLL, "itr_search_topk: index overflow (rows beyond the key's 32-bit index)");
    ITR_REQUIRE(n_slabs >= 0 && n_slabs <= ITR_SEARCH_MAX_SLABS, "itr_search_topk: n_slabs = %d outside 0 .. %d", n_slabs, ITR_SEARCH_MAX_SLABS);
    ITR_UNSUPPORTED(K < 1 || K > ITR_TOPK_MAX, "itr_search_topk: K = %d outside 1 .. ITR_TOPK_MAX = %d", K, ITR_TOPK_MAX);
    ITR_UNSUPPORTED(n_queries > ITR_SEARCH_MAX_QUERIES, "itr_search_topk: %lld queries > ITR_SEARCH_MAX_QUERIES = %d", (long long)n_queries,
                    ITR_SEARCH_MAX_QUERIES);
    if (n_queries == 0) return ITR_OK;
    ITR_REQUIRE(queries && key && val && (gallery || n_gallery == 0), "itr_search_topk: null pointer");
    hipStream_t st = itr::as_stream(stream);
    const int nq = (int)n_queries;
    unsigned long long *kout = reinterpret_cast<unsigned long long *>(key);
    uint32_t *vout = reinterpret_cast<uint32_t *>(val);
    itr::SearchWs ws{};                                    // an empty gallery: no parts, the last merge level writes empty lists
    if (n_gallery > 0) {
        const size_t need = itr_search_topk_workspace_bytes(n_queries, n_gallery, K, n_slabs);
        ITR_REQUIRE(workspace && workspace_bytes >= need && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0,
                    "itr_search_topk: workspace missing, misaligned or smaller than itr_search_topk_workspace_bytes");
        const itr::SearchPlan p = itr::search_plan(n_queries, n_gallery, K, n_slabs);
        ws = itr::search_ws(workspace, n_queries, n_gallery, K, n_slabs);
        const bool vec = ((reinterpret_cast<uintptr_t>(queries) | reinterpret_cast<uintptr_t>(gallery)) & 15) == 0 && ldq % 4 == 0 && ldg % 4 == 0;
        if (p.nqg == 1) itr::slab_launch<1>(vec, (unsigned)p.slabs, st, queries, ldq, nq, gallery, ldg, row0, n_gallery, (int)D, K, p.rows_per_slab, ws.key[0], ws.val[0]);
        else if (p.nqg == 4) itr::slab_launch<4>(vec, (unsigned)p.slabs, st, queries, ldq, nq, gallery, ldg, row0, n_gallery, (int)D, K, p.rows_per_slab, ws.key[0], ws.val[0]);
        else itr::slab_launch<16>(vec, (unsigned)p.slabs, st, queries, ldq, nq, gallery, ldg, row0, n_gallery, (int)D, K, p.rows_per_slab, ws.key[0], ws.val[0]);
        ITR_CHECK_LAUNCH("search_slab");
    }
    int lvl = 0;
    for (; ws.parts[lvl] > itr::SR_MERGE_PARTS; ++lvl) {
        hipLaunchKernelGGL(itr::search_merge_kernel<false>, dim3((unsigned)ws.parts[lvl + 1], nq), dim3(itr::SR_THREADS), 0, st, ws.key[lvl],
                           ws.val[lvl], (int)ws.parts[lvl], nq, K, ws.key[lvl + 1], ws.val[lvl + 1], (int32_t *)nullptr);
        ITR_CHECK_LAUNCH("search_merge");
    }
    hipLaunchKernelGGL(itr::search_merge_kernel<true>, dim3(1, nq), dim3(itr::SR_THREADS), 0, st, ws.key[lvl], ws.val[lvl], (int)ws.parts[lvl], nq,
                       K, kout, vout, idx);
    ITR_CHECK_LAUNCH("search_merge");
    return ITR_OK;
}
