// What the two entry points over SGRAF candidate lists share (sgraf_pairs.hip: the scores; sgraf_attn.hip: the scores with the attention,
// filtration and graph-edge weights they are made of): the item geometry, the prepared state, the per-chunk workspace and stages (a)-(c)
// of sgraf_pairs.hip -- attention, gathered word rows + local nodes, global node -- as ONE host function, so that both entries run the same
// kernels on the same bits up to the node rows.
#pragma once
#include "scan_common.h"
#include "itr_internal.h"

namespace itr {

constexpr int GP_PAIRS = 8;                // pairs (= waves) per workgroup of the attention kernel
constexpr int GP_THREADS = GP_PAIRS * 64;
constexpr int GP_MAXW = 63;                // words per caption: 63 + the global node = 64 graph nodes
constexpr int GP_ITEM = SC_NT;             // 64 columns / node rows per item
constexpr int GP_MAXCAP = 16;              // captions per item

struct GpState {
    float *img_glo, *cap_glo, *gram, *Wfold[8], *vfold[8];
    void *packed;
    size_t bytes;
};
static inline bool gp_fused(int module, int S) { return module == 1 && S == 256; }
static inline GpState gp_state(void *base, int64_t Ni, int64_t Nc, int64_t n_rows, int D, int S, int module, int sgr_step) {
    WsCarver c(base);
    GpState t{};
    t.img_glo = c.take<float>((size_t)Ni * D * 4), t.cap_glo = c.take<float>((size_t)Nc * D * 4);
    t.gram = c.take<float>((size_t)Ni * SC_R * SC_R * 4);
    if (module == 1) {
        for (int k = 0; k < 8; ++k) t.Wfold[k] = c.take<float>((size_t)S * S * 4), t.vfold[k] = c.take<float>((size_t)S * 4);
        if (gp_fused(module, S)) t.packed = c.take(sgr_fused_weights_bytes(sgr_step > 0 ? sgr_step : 1));
    }
    t.bytes = c.bytes;
    return t;
}

struct GpChunk {
    float *wt, *P, *cn, *Xloc, *Aloc, *Aglo, *Xglo, *Yglo, *Qloc, *Yloc, *Qglo, *sc;
    int64_t *col_src;
    int32_t *cap_col, *grp_begin, *grp_order;
    void *fused_ws;
    int *fused_bad;
    size_t bytes;
};
// with_steps: the buffers of the SAF / SGR stage of itr_sgraf_pair_scores (the explaining entry keeps its node rows on chip instead)
static inline GpChunk gp_chunk(void *base, int64_t n_pairs, int64_t n_items, int D, int S, int module, int sgr_step, bool with_steps = true) {
    const int64_t ncols = n_items * GP_ITEM;
    WsCarver c(base);
    GpChunk t{};
    t.wt = c.take<float>((size_t)ncols * D * 4);
    t.P = c.take<float>((size_t)ncols * SC_R * 4), t.cn = c.take<float>((size_t)ncols * 4);
    t.Xloc = c.take<float>((size_t)ncols * S * 4);
    if (S != 256) t.Aloc = c.take<float>((size_t)ncols * D * 4);
    t.Aglo = c.take<float>((size_t)n_pairs * D * 4);
    t.Xglo = c.take<float>((size_t)n_pairs * S * 4);
    if (module == 1 && with_steps) {
        t.Yglo = c.take<float>((size_t)n_pairs * S * 4);
        if (!gp_fused(module, S)) {
            t.Qloc = c.take<float>((size_t)ncols * S * 4), t.Yloc = c.take<float>((size_t)ncols * S * 4), t.Qglo = c.take<float>((size_t)n_pairs * S * 4);
        } else {
            t.fused_ws = c.take(sgr_fused_workspace_bytes(n_items, n_pairs, 0));      // (0: group records only, the packed weights live in the state)
            t.fused_bad = c.take<int>(256);
        }
    }
    t.sc = c.take<float>((size_t)n_pairs * 4);
    t.col_src = c.take<int64_t>((size_t)ncols * 8);
    t.cap_col = c.take<int32_t>((size_t)n_pairs * 4), t.grp_order = c.take<int32_t>((size_t)n_pairs * 4);
    t.grp_begin = c.take<int32_t>((size_t)(n_items + 1) * 4);
    t.bytes = c.bytes;
    return t;
}

static inline int gp_check_shape(const char *who, int64_t Ni, int64_t Nc, int64_t n_rows, int R, int D, int S, int module, int sgr_step) {
    if (module != 0 && module != 1) { set_error("Invalid input of config.module_name in configs.py"); return ITR_ERR_BADARG; }
    ITR_REQUIRE(Ni >= 0 && Nc >= 0 && n_rows >= 0 && D > 0 && S > 0, "%s: bad shape", who);
    ITR_REQUIRE(Nc < 0x7fffffffLL && Ni <= 65535, "%s: at most 65535 images and 2^31 - 1 captions per call", who);
    ITR_UNSUPPORTED(R != SC_R, "%s: VisualSA is built for %d regions (BatchNorm1d(36)), got %d", who, SC_R, R);
    ITR_UNSUPPORTED(S > 1024 || (D % SC_BK) != 0, "%s: need sim_dim <= 1024 and embed dim %% 32 == 0", who);
    ITR_UNSUPPORTED(module == 1 && (sgr_step < 1 || sgr_step > 8), "%s: sgr_step must be in [1, 8]", who);
    ITR_UNSUPPORTED(module == 1 && S % 16 != 0, "%s: SGR needs sim_dim %% 16 == 0", who);
    return ITR_OK;
}

// The chunk index (cap_col, grp_order, grp_begin) and stages (a)-(c) for the chunk of pairs [p0, p0 + n_pairs) = items [it0, it0 + n_items):
// on return (in stream order) k.P / k.cn hold the attention weights and context norms of the item tiles, k.Xloc the local node rows and
// k.Xglo the global node row of every pair.  Arguments as itr_sgraf_pair_scores, already checked.
int sgraf_pairs_nodes(const float *img, const float *words, const int64_t *cap_off, const int32_t *pair_img, const int32_t *pair_capok,
                      const int32_t *pair_len, const int32_t *pair_col, const int32_t *item_begin, const int32_t *item_img, int64_t p0,
                      int64_t n_pairs, int64_t it0, int64_t n_items, int64_t Ni, int64_t n_rows, int D, int S, const itr_sgraf_weights *w,
                      const GpState &s, const GpChunk &k, hipStream_t st);

}  // namespace itr
