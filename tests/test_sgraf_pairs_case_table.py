"""No GPU: the case table of the SGRAF candidate-list sweep (tests/helpers/sgraf_pairs_cases.py) is fit for its purpose.

References: the float64 mirror (sgraf_eval_cases.mirror up to the node rows, then its own SAF / SGR stage or the mirror of
sgraf_reason_kernel) is the oracle's function (1e-11) on every compared tensor, so its float32 run measures that algebra's own rounding.
Per case: sharpness >= 2, scores spanning >= 0.05 (cases of at least four scores: fewer cannot be asked to span), and
16 * max(e32_oracle, e32_mirror) never looser than what the older tests hold the kernels to (scores 5e-6; attn, node_w, edge 2e-5).
Planning mirrors: the item planner, the prefix ranges, the chunk bytes and the chunk cuts on hand-checked input, and per case the facts
its name claims.  Coverage: every seam value keeps a case (stated here a second time), and taking the sole carrier of a value out of
the table is noticed.  Sensitivity: each of the 14 named defects moves some compared tensor of every case that claims it by at least
10 x the bound the GPU sweep applies.  Pins: the constants the mirrors copy are checked against the source text of csrc/ and ops.py.
The float32 references are matrix products, so e32_oracle and e32_mirror depend on the BLAS that runs them: the assertion
16 * max(e32) <= older bound is a statement about the table on the BLAS in use (the seeds leave a quarter of the cap as margin) and may fail
under another one; every other assertion here is float64 or integer arithmetic.  The GPU test never relies on it: it applies
min(tol, older bound).  Wall time on the CPU: profiles/sgraf_pairs_seams/README.md."""
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import sgraf_pairs_cases as C       # noqa: E402
import sgraf_eval_cases as E        # noqa: E402
import train_prim_cases as P        # noqa: E402

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "image-text-retrieval_amd")
ALL_W = (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49, 62, 63)

# what the table must hold, stated here a second time: an edit that shrinks SEAMS in the helper does not shrink the requirement
BOTH = {
    'W': ALL_W, 'ncb': (1, 2, 3, 4), 'T': (1, 2, 3, 4), 'sgr_step': (1, 2, 3, 8), 'by': ('caption', 'image'),
    'item_shape': ('closed_by_16_captions', '16x1word', 'exact_fill', 'one_over', '63_alone_then_another', 'straddles_row_tile', 'one_pair',
                   'unlisted_image_between', 'pair_twice_in_a_list'),
    'rows': (16, 17, 32, 33, 48, 49, 64), 'na': (1, 2, 3, 4), 'caps_per_item': (1, 4, 5, 16), 'class': ('s', 'l'),
    'pairs_per_chunk': (1, 3, 4, 5, 7, 8, 9, 16, 17, 255, 256, 257),
    'cut': ('after_first_item', 'inside_an_image', 'last_chunk_one_item'), 'chunks': ('one', 'several'),
    'Ni': (1, 255, 256, 257, 1024, 1025, 2049), 'per': (1, 2, 3), 'image': (0, 255, 256, 1023, 1024, 2048),
    'long': (64, 82, 191), 'long_at': ('first', 'middle', 'last'),
}
REQUIRED = {
    'scores': dict(BOTH, route=('saf256', 'saf_generic', 'sgr_fused', 'sgr_chain'), S_saf=(16, 64, 256, 512, 1024), S_sgr=(16, 64, 256, 512, 1024),
                   K=(1, 10, 37), items_per_chunk=(1, 2, 256, 257, 1024, 1025), walk32=('below', 'above', 'twice'), walk64=('below',), D=(32, 64, 96, 256, 288, 1024)),
    'attention': dict(BOTH, route=('reason_saf', 'reason_sgr'), S_saf=(16, 48, 64, 80, 128, 192, 256), S_sgr=(16, 48, 64, 80, 128, 192, 256),
                      out_tiles=(1, 3, 4, 5, 8, 12, 16), vec_trips=(1, 2, 3, 4), D=(32, 64, 96, 256, 288, 1024)),
}


def missing(cs, required):
    seen = {}
    for c in cs:
        for k, vs in c.seams().items():
            seen.setdefault(k, set()).update(str(v) for v in vs)
    return [(k, v) for k, vs in required.items() for v in vs if str(v) not in seen.get(k, ())]


@pytest.mark.parametrize("kernel", C.KERNELS)
def test_every_seam_value_has_a_case(kernel):
    assert C.cases(kernel)
    assert not missing(C.cases(kernel), REQUIRED[kernel])
    assert not missing(C.cases(kernel), C.SEAMS[kernel])
    for k, vs in REQUIRED[kernel].items():          # the helper's own list asks for no less
        assert set(str(v) for v in vs) <= set(str(v) for v in C.SEAMS[kernel][k]), k


@pytest.mark.parametrize("kernel", C.KERNELS)
def test_taking_out_a_sole_carrier_is_noticed(kernel):
    """The mutation check: for every required value carried by exactly one case, the table without that case fails the coverage."""
    sole, req = {}, REQUIRED[kernel]
    for k, vs in req.items():
        for v in vs:
            carriers = [c for c in C.cases(kernel) if str(v) in set(str(s) for s in c.seams().get(k, ()))]
            if len(carriers) == 1:
                sole.setdefault(carriers[0].name, []).append((k, v))
    assert len(sole) >= 6, sole         # (Ni = 255 .. 2049, 255 | 256 | 257 pairs, the item shapes, ...)
    for name, what in sole.items():
        rest = [c for c in C.cases(kernel) if c.name != name]
        assert set(what) <= set(missing(rest, req)), (name, what)


def test_planning_mirrors():
    # the greedy planner: 31 + 31 words fill an item, a third caption opens the next; an image with no pairs; item numbers run on
    lens, off = (31, 31, 5), [0, 31, 62]
    plan = C.item_plan([0, 3, 3, 5], [0, 1, 2, 1, 0], off, lens, 3, 67)
    assert plan == ([31, 31, 5, 31, 31], [0, 31, 64, 128, 159], [0, 1, 2, 1, 0], [0, 2, 3, 5], [0, 0, 2], 3)
    # refused captions: index -1, index >= Nc, rows behind n_rows -> a one-word slot, pair_capok -1
    plan = C.item_plan([0, 4], [-1, 2, 1, 0], off, lens, 2, 61)
    assert plan == ([1, 1, 1, 31], [0, 1, 2, 3], [-1, -1, -1, 0], [0, 4], [0], 1)
    # 16 one-word captions close an item at 32 rows; the 17th opens the next
    plan = C.item_plan([0, 17], [0] * 17, [0], (1,), 1, 1)
    assert plan[1][15:] == [15, 64] and plan[3] == [0, 16, 17] and plan[5] == 2
    # img_ptr outside [0, P] is clamped
    assert C.item_plan([-3, 9], [0, 0], [0], (1,), 1, 1)[3] == [0, 2]
    assert [C.prefix_ranges(n)[0] for n in (1, 1023, 1024, 1025, 2048, 2049)] == [1, 1, 1, 2, 2, 3]
    assert C.prefix_ranges(1025)[1][511:514] == [(1022, 1024), (1024, 1025), (1025, 1025)]
    for n in (5, 1024, 1025, 2049):                  # the thread-by-thread scan is the plain prefix sum
        counts = [(7 * k) % 3 for k in range(n)]
        want, run = [], 0
        for v in counts:
            want.append(run)
            run += v
        assert C.prefix_items(counts) == (want, run)
    assert C.align256(0) == 0 and C.align256(1) == 256 and C.align256(256) == 256
    assert C.chunk_bytes(1, 1, 32, 256, False) == 8192 + 9216 + 256 + 65536 + 256 + 1024 + 256 + 512 + 3 * 256
    assert C.chunk_bytes(1, 1, 32, 256, True, with_steps=False) == C.chunk_bytes(1, 1, 32, 256, False)
    assert C.chunk_bytes(1, 1, 32, 64, False) - (8192 + 9216 + 256 + 16384 + 256 + 256 + 256 + 512 + 3 * 256) == 8192          # Aloc
    assert C.chunk_bytes(3, 2, 32, 256, True) - C.chunk_bytes(3, 2, 32, 256, False) == 3072 + C.fused_ws_bytes(2, 3) + 256
    assert C.fused_ws_bytes(2, 3) == 1024 + 256 + 256 + 256 + 256 + 0 + 256
    assert C.chunks_within(lambda a, b: 10 * (b - a), 5, 25) == [(0, 2), (2, 4), (4, 5)]
    with pytest.raises(AssertionError):
        C.chunks_within(lambda a, b: 10 * (b - a), 5, 9)


def test_table_shapes_follow_the_rules():
    assert 150 <= len(C.CASES) <= 300 and len(set(c.name for c in C.CASES)) == len(C.CASES)
    for c in C.CASES:
        p = c.plan
        assert (c.D == 32 or c.group == 'D') and (c.Ni <= 21 or c.group in ('Ni', 'nitems')), c          # small unless the seam is D or Ni
        assert c.P <= 1025 and len(c.LI) * len(c.LC) <= 5125 and sum(c.sub_lens) <= 700, c
        x = c.inputs()
        assert x['images'].shape == (c.Ni, 36, c.D) and x['words'].shape == (c.n_tok, c.D)
        # the plan is consistent: every short pair in exactly one item, items within the limits, slots a permutation
        assert sorted(p.pair_out + p.long_slots) == list(range(c.P)), c
        assert [q for v in p.items for q in v] == list(range(p.P)) and all(1 <= len(v) <= 16 for v in p.items), c
        assert all(r <= 64 for r in p.rows) and all(p.pair_img[q] == p.item_img[t] for t, v in enumerate(p.items) for q in v), c
        assert all(p.pair_col[q] == 64 * t + p.rbase[q] - k for t, v in enumerate(p.items) for k, q in enumerate(v)), c
        # sgr_group_meta_kernel's class, restated: small = at most 32 node rows and at most 12 softmax tiles (sum of ceil(n / 16)^2)
        for t, v in enumerate(p.items):
            tiles = sum(((p.pair_len[q] + 1 + 15) // 16) ** 2 for q in v)
            assert p.cls[t] == (0 if p.rows[t] <= 32 and tiles <= 12 else 1) and tiles <= 24, (c, t)
        assert p.chunks and p.chunks[0][0] == 0 and p.chunks[-1][1] == p.n_items and all(a[1] == b[0] for a, b in zip(p.chunks, p.chunks[1:])), c
        assert (len(p.chunks) > 1) == bool(c.budget_items) or p.n_items <= (c.budget_items or 0), c
        if p.budget:
            assert all(p.need(a, b) <= p.budget for a, b in p.chunks), c
            assert all(b == p.n_items or p.need(a, b + 1) > p.budget for a, b in p.chunks), c              # every chunk as long as fits
    # the facts the names claim
    by = lambda kernel, group, tag: [c for c in C.cases(kernel, group) if c.tag == tag]
    for kernel in C.KERNELS:
        for c in by(kernel, 'items', 'cap16'):
            assert [len(v) for v in c.plan.items[:3]] == [16, 2, 1] and c.plan.rows[:3] == [32, 43, 23] and c.plan.item_img[:4] == [0, 0, 0, 1], c
        for c in by(kernel, 'items', 'fill64'):
            assert c.plan.rows[0] == 64 and [c.plan.pair_len[q] for q in c.plan.items[0]] == [31, 31] and len(c.plan.items[2]) == 1, c
        for c in by(kernel, 'items', 'w63'):
            assert [c.plan.pair_len[q] for q in c.plan.items[0]] == [63] and c.plan.item_img[:3] == [0, 0, 0], c
        for c in by(kernel, 'items', 'rows'):
            assert (c.plan.rows, c.plan.na, c.plan.cls) == ([16, 17, 32, 33, 48, 49, 64], [1, 2, 2, 3, 3, 4, 4], [0, 0, 0, 1, 1, 1, 1]), c
        for c in by(kernel, 'items', 'percap'):
            assert [len(v) for v in c.plan.items] == [16, 4, 4, 4, 4, 5, 5, 5, 1], c
        for c in by(kernel, 'items', 'one'):
            assert c.P == 1 and c.plan.n_items == 1, c
        for c in C.cases(kernel, 'perchunk'):
            want = [c.K] if c.budget_items else [c.P]
            assert sorted(c.seams()['pairs_per_chunk']) == want and (c.P in (255, 256, 257) or len(c.plan.chunks) >= 3), c
        for c in by(kernel, 'cut', 'items9'):
            n = {1: 9, 2: 5, 4: 3}[c.budget_items]
            assert c.plan.n_items == 9 and len(c.plan.chunks) == n and c.plan.chunks[1][0] == c.budget_items, c
            assert 'inside_an_image' in c.seams()['cut'] and 'last_chunk_one_item' in c.seams()['cut'], c
        for c in by(kernel, 'cut', 'mixed'):
            assert any(c.plan.item_begin[a] != a for a, _ in c.plan.chunks[1:]), c                          # p0 != it0
        for c in C.cases(kernel, 'Ni'):
            assert c.plan.per == (c.Ni + 1023) // 1024 and {0, c.Ni - 1} <= set(c.LI) and len(c.LI) <= 11, c
            if c.Ni >= 1025:
                assert {1023, 1024} <= set(c.LI) and 5 in c.claims, c
        for c in C.cases(kernel, 'long'):
            assert len(c.plan.long_slots) == sum(1 for _, k in c.pairs if c.lens[k] > 63) >= 9, c
    for c in C.cases('scores', 'nitems'):
        assert c.plan.n_items == c.Ni == c.P and len(c.plan.chunks) == 1 and c.plan.cls.count(0) == c.Ni, c          # all in the 32-row class
        assert c.seams()['walk32'] == {{256: 'below', 257: 'below', 1024: 'above', 1025: 'twice'}[c.Ni]}, c      # 512 resident workgroups: 2 each | a third


@pytest.mark.parametrize("kernel", C.KERNELS)
def test_mirror_is_the_oracles_function_and_the_bound_is_tight(kernel):
    worst = 0.0
    for c in C.cases(kernel):
        ref = c.reference()
        n_w = sum(c.lens[k] for s, (_, k) in enumerate(c.pairs) if c.short(s))
        n_aux = sum((c.lens[k] + 1) if c.mod == 'SAF' else c.steps * (c.lens[k] + 1) ** 2 for s, (_, k) in enumerate(c.pairs) if c.short(s))
        assert ref['sharp'] >= C.MIN_SHARP, (c, ref['sharp'])
        want = ref['score'][0]
        assert c.P < 4 or float(want.max() - want.min()) >= C.MIN_SPAN, (c, float(want.max() - want.min()))
        for t in c.tensors:
            want, e_oracle, e_mirror, tol, agree = ref[t]
            assert want.shape == ({'score': c.P, 'attn': n_w * 36}.get(t, n_aux),), (c, t)
            assert bool(torch.isfinite(want).all()) and e_oracle == e_oracle and e_mirror == e_mirror, (c, t)
            assert agree <= C.MIRROR_AGREES, (c, t, agree)
            assert c.name not in C.FALLBACK and tol == C.FACTOR * max(e_oracle, e_mirror, C.U * float(want.abs().max())), (c, t)
            assert C.FACTOR * max(e_oracle, e_mirror) <= C.OLD[t], "%s %s: 16 x (e32 oracle %.3g, mirror %.3g) is looser than the older tests' %.3g" % (
                c, t, e_oracle, e_mirror, C.OLD[t])
            assert tol <= C.OLD[t], (c, t)
            worst = max(worst, tol / C.OLD[t])
        if kernel == 'attention':       # the float64 rows sum to 1: attn per word, node_w per pair, edge per querying node
            assert float((ref['attn'][0].view(-1, 36).sum(1) - 1.0).abs().max()) <= 1e-12, c
            o, aux = 0, ref[c.aux][0]
            for s, (_, k) in enumerate(c.pairs):
                if c.short(s):
                    n = c.lens[k] + 1
                    blk = aux[o:o + n].view(1, n) if c.mod == 'SAF' else aux[o:o + c.steps * n * n].view(-1, n)
                    assert float((blk.sum(1) - 1.0).abs().max()) <= (C.OLD_SUM if c.mod == 'SAF' else 1e-12), c     # (SAF: 1 - 1e-8 / sum of the sigmoids, l1norm's eps)
                    o += blk.numel()
    assert worst <= 1.0


def claims_restated(c):
    """The rules of the helper's docstring, from the plan's facts."""
    p, w = c.plan, []
    att, sgr = c.kernel == 'attention', c.mod == 'SGR'
    big = c.P > 300 or c.Ni > 1000
    several = any(len(v) > 1 for v in p.items)
    if not big:
        w += [1] if any(p.pair_cap[a] != p.pair_cap[b] for v in p.items for a, b in zip(v, v[1:])) else []
        if len(p.chunks) > 1:
            w += [3, 4] + ([2] if any(p.item_img[t - a] != p.item_img[t] for a, b in p.chunks[1:] for t in range(a, b)) else [])
        w += [6] if att or sgr or (c.S == 256 and any((n + 1) % 4 for n in p.pair_len)) else []
        w += ([7] if max(p.pair_len) > 1 else []) + [8, 9] + ([90] if c.D <= 96 else [])
        w += [11] if not att and any(n > 63 for n in c.sub_lens) else []
        if att:
            w += ([12 if sgr else 13] if several else []) + ([14] if sgr and c.steps > 1 else [])
    w += [5] if any(i >= 1024 for i in p.pair_img) else []
    w += [10] if not att and any(a != b for r in c.cand for a, b in zip(r, r[1:] + r[:1])) else []
    return w


@pytest.mark.parametrize("kernel", C.KERNELS)
def test_bound_sees_every_claimed_defect(kernel):
    claimed = {}
    for c in C.cases(kernel):
        ref, defects = c.reference(), c.defects()
        assert sorted(defects) == sorted(c.claims) == sorted(claims_restated(c)), (c, sorted(defects), c.claims, claims_restated(c))
        for n, res in defects.items():
            assert res, (c, n)
            best = 0.0
            for t, value in res.items():
                want, _, _, tol, _ = ref[t]
                assert value.shape == want.shape and value.dtype == torch.float64, (c, n, t)
                best = max(best, float((value - want).abs().max()) / tol)
            assert best >= C.SENSITIVITY, "%s defect %d moves no tensor by more than %.3g x its bound" % (c, n, best)
            claimed.setdefault(n, []).append(c)
    assert set(claimed) == set([1, 2, 3, 4, 5, 6, 7, 8, 9, 90] + ([10, 11] if kernel == 'scores' else [12, 13, 14]))
    assert all(len(v) >= 2 for v in claimed.values()), {n: len(v) for n, v in claimed.items()}
    # the chunk defects are claimed at every cut the table holds; the prefix stride at both per = 2 and 3
    assert set(v for c in claimed[3] for v in c.seams()['cut']) >= {'after_first_item', 'inside_an_image', 'last_chunk_one_item'}
    assert set(c.plan.per for c in claimed[5]) >= ({2, 3} if kernel == 'scores' else {2} | {3} & set(c.plan.per for c in C.cases(kernel, 'Ni')))
    assert set(c.route_name() for c in claimed[6]) >= ({'saf256', 'sgr_fused', 'sgr_chain'} if kernel == 'scores' else {'reason_saf', 'reason_sgr'})
    if kernel == 'attention':
        assert set(c.steps for c in claimed[14]) == {2, 3, 8}


def test_fallback_list():
    assert C.FALLBACK == {} and len(C.FALLBACK) <= C.FALLBACK_SHARE * len(C.CASES)
    assert C.FALLBACK_SHARE == 0.02 and C.FACTOR == P.FACTOR == 16 and C.U == P.U == 2.0 ** -24 and C.SENSITIVITY == P.SENSITIVITY == 10
    assert C.MIRROR_AGREES == 1e-11 and (C.MIN_SHARP, C.MIN_SPAN) == (E.MIN_SHARP, E.MIN_SPAN) == (2.0, 0.05)
    assert C.OLD == {'score': 5e-6, 'attn': 2e-5, 'node_w': 2e-5, 'edge': 2e-5} and C.OLD_SUM == 1e-5
    assert all(k.split('-seed')[0] in C.RESEED or '-seed' not in k for k in C._BY_NAME)
    # the sharpened weights, never the plain ones
    for c in C.CASES[::17]:
        plain = E.sgraf_weights.make(c.D, c.S, c.steps if c.mod == 'SGR' else 3)
        key = 'SAF_module.attn_sim_w.weight' if c.mod == 'SAF' else 'SGR_module.sgr0.graph_query_w.weight'
        assert c.weights is E.weights(c.mod, c.D, c.S, c.steps if c.mod == 'SGR' else 3) and not torch.equal(c.weights[key], plain[key]), c


def _src(*path):
    with open(os.path.join(PKG, *path)) as f:
        return re.sub(r"\s+", " ", f.read())


def test_constants_are_the_ones_of_the_source():
    """The mirrors' constants and index arithmetic, as the source text states them (whitespace folded)."""
    text = {n: _src("csrc", n) for n in ("sgraf_pairs.h", "sgraf_pairs.hip", "sgraf_attn.hip", "sgr_fused.hip", "itr_internal.h", "scan_common.h")}
    text["ops.py"] = _src("itr_amd", "ops.py")
    text["test_sgraf_attention_gpu.py"] = _src("..", "tests", "test_sgraf_attention_gpu.py")
    text["test_sgraf_candidates_gpu.py"] = _src("..", "tests", "test_sgraf_candidates_gpu.py")
    pins = {
        "scan_common.h": ("constexpr int SC_R = %d;" % C.SC_R,),
        "itr_internal.h": ("static inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }", "bytes += align256(n);"),
        "sgraf_pairs.h": (
            "constexpr int GP_PAIRS = %d;" % C.GP_PAIRS, "constexpr int GP_MAXW = %d;" % C.GP_MAXW, "constexpr int GP_ITEM = SC_NT;",
            "constexpr int GP_MAXCAP = %d;" % C.GP_MAXCAP, "static inline bool gp_fused(int module, int S) { return module == 1 && S == 256; }",
            "t.wt = c.take<float>((size_t)ncols * D * 4);", "if (S != 256) t.Aloc = c.take<float>((size_t)ncols * D * 4);",
            "if (module == 1 && with_steps) {", "t.fused_ws = c.take(sgr_fused_workspace_bytes(n_items, n_pairs, 0));", "t.fused_bad = c.take<int>(256);",
            "t.col_src = c.take<int64_t>((size_t)ncols * 8);", "t.grp_begin = c.take<int32_t>((size_t)(n_items + 1) * 4);",
        ),
        "sgraf_pairs.hip": (
            "__global__ __launch_bounds__(%d) void sgraf_pairs_plan_kernel(" % C.PLAN_THREADS, "const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;",
            "int len = (c >= 0 && c < Nc) ? cap_len[c] : 0;", "bool ok = len >= 1 && len <= GP_MAXW;",
            "if (ok) { const int64_t o = cap_off[c]; ok = o >= 0 && o + len <= n_rows; }", "if (!ok) len = 1;",
            "if (n == 0 || ncap == GP_MAXCAP || rows + len + 1 > GP_ITEM) {", "pair_col[p] = (int32_t)(item * GP_ITEM + (rows - ncap));",
            "pair_capok[p] = ok ? c : -1;", "rows += len + 1;",
            "__global__ __launch_bounds__(%d) void sgraf_pairs_prefix_kernel(" % C.PREFIX_THREADS, "const int64_t per = (n + 1023) / 1024;",
            "const int64_t b = t * per < n ? t * per : n, e = (b + per < n) ? b + per : n;", "item_begin[run] = (int32_t)P;",
            "hipLaunchKernelGGL(sgraf_pairs_prefix_kernel, dim3(1), dim3(%d), 0, st, img_items, Ni, P, item_begin, n_items_dev);" % C.PREFIX_THREADS,
            "__global__ __launch_bounds__(%d) void sgraf_pair_index_kernel(" % C.INDEX_THREADS, "cap_col[j] = (int32_t)(pair_col[p0 + j] - it0 * GP_ITEM);",
            "if (j <= n_items) grp_begin[j] = (int32_t)(item_begin[it0 + j] - p0);",
            "const int64_t j = (int64_t)blockIdx.x * GP_PAIRS + wave;", "const int ncb = (W + 15) >> 4;",
            "if (c < 0 || ii < 0 || ii >= g.Ni || W < 1 || W > GP_MAXW || col0 < 0 || col0 + W > g.ncols) return;",
            "for (int s = r; s < SC_R; ++s) t = fmaf(G[r * SC_R + s], e[s], t);", "g.cn[col] = 1.f / (sqrtf(fmaxf(q, 0.f)) + 1e-8f);",
            "const int64_t j = (int64_t)blockIdx.x * %d + (threadIdx.x >> 6);" % C.PER_WG, "const int64_t col = (int64_t)blockIdx.x * %d + (threadIdx.x >> 6);" % C.PER_WG,
            "for (int d = lane; d < D / 4; d += 64) dst[d] = s[d];", "for (int d = threadIdx.x; d < D; d += 256) {",
            "if (o >= 0 && o < out_len) out[o] = pair_cap[j] >= 0 ? sc[j] : __builtin_nanf(\"\");",
            "hipLaunchKernelGGL(gram_mfma_kernel, dim3((unsigned)Ni), dim3(256), 0, st, img, R, D, s.gram, 1);",
        ),
        "sgraf_attn.hip": (
            "constexpr int GR_THREADS = 256;", "constexpr int GR_WAVES = GR_THREADS / 64;", "constexpr int GR_LDE = GP_ITEM + 4;",
            "constexpr int GR_MAXS = %d;" % C.GR_MAXS, "if (o < 0 || o >= g.out_len) { o = -1; return false; }",
            "return ab >= 0 && ab + (int64_t)W * SC_R <= g.attn_len && xb >= 0 && xb + xn <= g.aux_len;",
            "const int na = (m.nrows + 15) >> 4;", "for (int nt = wave; nt < S / 16; nt += GR_WAVES) {", "for (int j = wave; j < ncap; j += GR_WAVES) {",
            "const float an = mine / (asum + 1e-8f);", "float vec[GR_MAXS / 64];", "const int row = a * 16 + (lane >> 2), q = lane & 3;",
            "for (int c = lo + q; c < hi; c += 4) mx = fmaxf(mx, er[c]);", "const int T = (n + 15) >> 4;",
            "const int64_t off = emit ? m.aux_base[cj] + ((int64_t)k * n + (row - lo)) * n : 0;",
            "const int64_t j = (int64_t)blockIdx.x * %d + (threadIdx.x >> 6);" % C.PER_WG,
            "if (((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 15) == 0) {",
        ),
        "sgr_fused.hip": ("w.meta = c.take<SgrGroupMeta>((size_t)n_groups * sizeof(SgrGroupMeta));", "w.glist = c.take<int32_t>((size_t)2 * n_groups * 4);",
                          "w.cap_bad = c.take<int32_t>((size_t)n_caps * 4);", "static_assert(sizeof(SgrGroupMeta) == %d" % C.GROUP_META_BYTES),
        "ops.py": ("SGRAF_MAX_WORDS = %d" % C.GP_MAXW, "SGRAF_COMPOSED_MAX_WORDS = %d" % C.MAX_COMPOSED, "SGRAF_ATTN_MAX_SIM_DIM = %d" % C.GR_MAXS,
                   "off, klen = _caption_tables(plan, dev, SGRAF_MAX_WORDS)", "img_ptr, imgs, caps, slot = _group_pairs(imgs, Ni, (caps, slot), grouped=by == 'image')",
                   "key, order = torch.sort(key, stable=True)", "mid = (lo + hi + 1) // 2", "chunks.append((it0, lo))"),
        "test_sgraf_attention_gpu.py": ("TOL_ATTN = 2e-5", "TOL_SCORE = 5e-6", "TOL_SUM = 1e-5"),
        "test_sgraf_candidates_gpu.py": ("TOL = 5e-6",),
    }
    for name, lines in pins.items():
        for line in lines:
            assert line in text[name], "%s no longer says: %s" % (name, line)
    assert (C.GP_ITEM, C.GR_LDE, C.GR_WAVES) == (E.SC_NT, E.SC_NT + 4, 4) and C.OLD_ATTN == 2e-5
