// One training batch assembled on the device from tables that stay in HBM (itr_collate_batch, include/itr_hip.h): the work of
// PrecompDataset.__getitem__ + collate_fn (itr/datamodule/data_loader.py:104-131, :134-178) as ONE launch of a pure copy.
//
// The launch is a flat list of at most 8 jobs over one 1-D grid.  A job copies B rows; a workgroup owns one (row, chunk) of
// one job, a chunk being 256 threads x 4 units, a unit 16 / 8 / 4 bytes:
//     row job     dst[b, :] = src[idx[b], :]                                   features, boxes, image sizes, fixed-width id tables
//     ragged job  dst[b, j] = j < len(c) ? packed[off[c] + j] : 0,  c = idx[b]   GRU caption ids, zero padded to Lmax
// A row moves in 16-byte units when its byte length is a multiple of 16 and both bases are 16-byte aligned (then every row is),
// otherwise element by element.  Each thread issues its 4 loads before its 4 stores, so a wave keeps 4 KB in flight; lanes of a
// wave touch consecutive units (1 KB per instruction with 16-byte units).
//
// An index outside its table reads row 0 and raises *bad_flag (the contract of itr_gather_rows); a ragged row whose offsets
// leave the packed array is written as zeros and raises it too.  Nothing is allocated, nothing is read from the environment.
#include "itr_internal.h"

namespace itr {

constexpr int CL_THREADS = 256, CL_UNROLL = 4, CL_CHUNK = CL_THREADS * CL_UNROLL, CL_MAX_JOBS = 8;
// gridDim.x * blockDim.x has to stay below 2^32
constexpr int64_t CL_MAX_BLOCKS = ((int64_t)1 << 24) - 1;

struct CollateJob {
    const void *src;
    void *dst;
    const int64_t *idx;        // [B] row of the table per output row
    const int64_t *off;        // ragged: [n_rows + 1] offsets into src (int64 ids); row jobs: null
    int64_t n_rows;            // rows of the table (bound of idx)
    int64_t row_units;         // units per OUTPUT row
    int64_t n_packed;          // ragged: elements of src
    uint32_t first_block, chunks_per_row;
    int unit_log2;             // 4, 3, 2: bytes per unit
};
struct CollateArgs {
    CollateJob job[CL_MAX_JOBS];
    int n_jobs;
};

template <typename T>
__device__ __forceinline__ void copy_chunk(const T *__restrict__ src, T *__restrict__ dst, int64_t u0, int64_t n) {
    T v[CL_UNROLL];
#pragma unroll
    for (int k = 0; k < CL_UNROLL; ++k) {
        const int64_t u = u0 + k * CL_THREADS;
        if (u < n) v[k] = src[u];
    }
#pragma unroll
    for (int k = 0; k < CL_UNROLL; ++k) {
        const int64_t u = u0 + k * CL_THREADS;
        if (u < n) dst[u] = v[k];
    }
}

__global__ __launch_bounds__(CL_THREADS) void collate_batch_kernel(CollateArgs a, int *__restrict__ bad) {
    int j = a.n_jobs - 1;
    while (j > 0 && blockIdx.x < a.job[j].first_block) --j;
    const CollateJob &jb = a.job[j];
    const uint32_t local = blockIdx.x - jb.first_block;
    const int64_t b = local / jb.chunks_per_row;
    const int64_t u0 = (int64_t)(local % jb.chunks_per_row) * CL_CHUNK + threadIdx.x;
    const int64_t n = jb.row_units;
    int64_t r = jb.idx[b];
    bool is_bad = r < 0 || r >= jb.n_rows;
    if (is_bad) r = 0;
    if (jb.off) {
        int64_t o0 = jb.off[r], len = jb.off[r + 1] - o0;
        if (o0 < 0 || len < 0 || o0 + len > jb.n_packed) {
            is_bad = true;
            len = 0;
        }
        const int64_t *__restrict__ src = static_cast<const int64_t *>(jb.src) + o0;
        int64_t *__restrict__ dst = static_cast<int64_t *>(jb.dst) + b * n;
        int64_t v[CL_UNROLL];
#pragma unroll
        for (int k = 0; k < CL_UNROLL; ++k) {
            const int64_t u = u0 + k * CL_THREADS;
            v[k] = u < len ? src[u] : 0;
        }
#pragma unroll
        for (int k = 0; k < CL_UNROLL; ++k) {
            const int64_t u = u0 + k * CL_THREADS;
            if (u < n) dst[u] = v[k];
        }
    } else if (jb.unit_log2 == 4) {
        copy_chunk(static_cast<const f32x4 *>(jb.src) + r * n, static_cast<f32x4 *>(jb.dst) + b * n, u0, n);
    } else if (jb.unit_log2 == 3) {
        copy_chunk(static_cast<const int64_t *>(jb.src) + r * n, static_cast<int64_t *>(jb.dst) + b * n, u0, n);
    } else {
        copy_chunk(static_cast<const float *>(jb.src) + r * n, static_cast<float *>(jb.dst) + b * n, u0, n);
    }
    if (is_bad && threadIdx.x == 0) atomicExch(bad, 1);
}

static bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Appends a job; returns false when its workgroups no longer fit the grid.
static bool add_job(CollateArgs &a, int64_t &blocks, int64_t B, const void *src, void *dst, const int64_t *idx, const int64_t *off,
                    int64_t n_rows, int64_t row_elems, int elem_log2, int64_t n_packed) {
    if (row_elems == 0) return true;
    CollateJob &jb = a.job[a.n_jobs];
    const int64_t row_bytes = row_elems << elem_log2;
    const bool wide = !off && (row_bytes & 15) == 0 && aligned16(src) && aligned16(dst);
    jb.unit_log2 = wide ? 4 : elem_log2;
    jb.row_units = row_bytes >> jb.unit_log2;
    const int64_t cpr = ceil_div(jb.row_units, CL_CHUNK);
    if (cpr > CL_MAX_BLOCKS || B > (CL_MAX_BLOCKS - blocks) / cpr) return false;
    jb.src = src; jb.dst = dst; jb.idx = idx; jb.off = off;
    jb.n_rows = n_rows; jb.n_packed = n_packed;
    jb.first_block = (uint32_t)blocks;
    jb.chunks_per_row = (uint32_t)cpr;
    blocks += B * cpr;
    ++a.n_jobs;
    return true;
}

}  // namespace itr

using namespace itr;

extern "C" int itr_collate_batch(const int64_t *img_idx, const int64_t *cap_idx, int64_t B, const float *feat, int64_t n_img, int64_t row_elems,
                                 float *images_out, const float *boxes, int64_t box_elems, float *boxes_out, const float *img_wh, float *wh_out,
                                 const int64_t *packed, int64_t n_packed, const int64_t *off, int64_t n_cap, int64_t Lmax, int64_t *ids_out,
                                 const int64_t *tab0, const int64_t *tab1, const int64_t *tab2, const float *ftab, int64_t W, int64_t *out0,
                                 int64_t *out1, int64_t *out2, float *fout, int *bad_flag, itr_stream_t stream) {
    const bool ragged = packed || off || ids_out;
    const bool fixed = tab0 || tab1 || tab2 || ftab || out0 || out1 || out2 || fout;
    ITR_REQUIRE(img_idx && feat && images_out && bad_flag, "itr_collate_batch: null pointer (img_idx, feat, images_out, bad_flag)");
    ITR_REQUIRE(!!boxes == !!boxes_out && !!img_wh == !!wh_out, "itr_collate_batch: null pointer (boxes / img_wh table without its output, or the reverse)");
    ITR_REQUIRE(!ragged || (packed && off && ids_out), "itr_collate_batch: null pointer (ragged ids need packed, off and ids_out)");
    ITR_REQUIRE(!!tab0 == !!out0 && !!tab1 == !!out1 && !!tab2 == !!out2 && !!ftab == !!fout,
                "itr_collate_batch: null pointer (fixed-width table without its output, or the reverse)");
    ITR_REQUIRE(!(ragged || fixed) || cap_idx, "itr_collate_batch: null pointer (cap_idx)");
    ITR_REQUIRE(B >= 0 && n_img > 0 && row_elems >= 0, "itr_collate_batch: bad shape (B %lld, n_img %lld, row_elems %lld)", (long long)B,
                (long long)n_img, (long long)row_elems);
    ITR_REQUIRE(!boxes || box_elems >= 0, "itr_collate_batch: bad shape (box_elems %lld)", (long long)box_elems);
    ITR_REQUIRE(!(ragged || fixed) || n_cap > 0, "itr_collate_batch: bad shape (n_cap %lld)", (long long)n_cap);
    ITR_REQUIRE(!ragged || (Lmax >= 0 && n_packed >= 0), "itr_collate_batch: bad shape (Lmax %lld, n_packed %lld)", (long long)Lmax,
                (long long)n_packed);
    ITR_REQUIRE(!fixed || W >= 0, "itr_collate_batch: bad shape (W %lld)", (long long)W);
    ITR_UNSUPPORTED(row_elems > ((int64_t)1 << 40) || box_elems > ((int64_t)1 << 40) || (ragged && Lmax > ((int64_t)1 << 40)) ||
                        (fixed && W > ((int64_t)1 << 40)),
                    "itr_collate_batch: a row of more than 2^40 elements does not fit the grid (row_elems %lld, Lmax %lld, W %lld)",
                    (long long)row_elems, (long long)Lmax, (long long)W);
    if (B == 0) return ITR_OK;

    CollateArgs a;
    a.n_jobs = 0;
    int64_t blocks = 0;
    bool ok = add_job(a, blocks, B, feat, images_out, img_idx, nullptr, n_img, row_elems, 2, 0);
    if (boxes) ok = ok && add_job(a, blocks, B, boxes, boxes_out, img_idx, nullptr, n_img, box_elems, 2, 0);
    if (img_wh) ok = ok && add_job(a, blocks, B, img_wh, wh_out, img_idx, nullptr, n_img, 2, 2, 0);
    if (ragged) ok = ok && add_job(a, blocks, B, packed, ids_out, cap_idx, off, n_cap, Lmax, 3, n_packed);
    if (tab0) ok = ok && add_job(a, blocks, B, tab0, out0, cap_idx, nullptr, n_cap, W, 3, 0);
    if (tab1) ok = ok && add_job(a, blocks, B, tab1, out1, cap_idx, nullptr, n_cap, W, 3, 0);
    if (tab2) ok = ok && add_job(a, blocks, B, tab2, out2, cap_idx, nullptr, n_cap, W, 3, 0);
    if (ftab) ok = ok && add_job(a, blocks, B, ftab, fout, cap_idx, nullptr, n_cap, W, 2, 0);
    ITR_UNSUPPORTED(!ok, "itr_collate_batch: B = %lld rows of this width need more than %lld workgroups: split the batch", (long long)B,
                    (long long)CL_MAX_BLOCKS);
    if (blocks == 0) return ITR_OK;
    hipLaunchKernelGGL(collate_batch_kernel, dim3((unsigned)blocks), dim3(CL_THREADS), 0, as_stream(stream), a, bad_flag);
    ITR_CHECK_LAUNCH("collate_batch");
    return ITR_OK;
}
