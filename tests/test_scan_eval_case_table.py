"""No GPU: the case table of the SCAN evaluation sweep (tests/helpers/scan_eval_cases.py) is fit for its purpose.

References: the float64 mirror of the kernel's algebra is the oracle's function (1e-11), so its float32 run measures that algebra's own
rounding.  Bounds: every case's tol is at most 2^-10 of its largest score and never looser than what the older tests hold the fused
kernel to.  Planner mirror: its bins are valid (every caption once, <= 64 words and <= 16 captions per bin, never more bins than best
fit decreasing), on the table's caption sets and on seeded random ones.  Coverage: every seam value of the launch code keeps a case
(stated here a second time), and taking the sole carrier of a value out of the table is noticed.  Sensitivity: each claimed defect
moves S by at least 10 x the bound the GPU sweep applies.  Pins: the constants and gates the mirrors copy are checked against the
source text of csrc/ and ops.py, so an edit to the kernel's geometry fails here instead of silently moving the seams."""
import os
import random
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import scan_eval_cases as E         # noqa: E402
import scan_train_cases as S        # noqa: E402
import train_prim_cases as P        # noqa: E402

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "image-text-retrieval_amd")

# what the table must hold, stated here a second time: an edit that shrinks SEAMS in the helper does not shrink the requirement
BOTH = {
    'norm,agg': [(n, a) for n in S.NORMS for a in S.AGGS],
    'D': (32, 64, 96, 128, 160, 192, 224, 256, 1024), 'nk': (1, 2, 3, 4, 5, 6, 7, 8, 32), 'mainloop': ('simple', 'pipelined'),
    'Ni': (1, 2, 3, 4, 5, 8, 31, 32, 33, 65), 'Ni%4': (0, 1, 2, 3), 'img_tiles': (8, 9),
    'n_tiles': (1, 7, 8, 9, 16, 17), 'PIxPJ': ((3, 3), (1, 16), (1, 17)), 'PI*PJ': (1, 2, 3, 9, 16, 17), 'rep': (0, 1), 'pgroup': (0, 1),
    'tile': ((1, 64, 1), (16, 64, 0), (16, 16, 0), (1, 1, 0), (2, 64, 0), (2, 64, 1), (3, 64, 1), (9, 45, 0)),
    'ncap': (1, 16), 'used': (1, 16, 64), 'far': (0, 1), 'far_from': ('first', 'later'), 'unroll_tile': (1,),
    'W': (1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64),
    'long': (65, 96), 'long_at': ('first', 'middle', 'last'), 'Nc_kernel': (0,), 'zero': (((0, 7), 8),),
}
REQUIRED = {
    't2i': dict(BOTH, cap_end=tuple(range(64))),
    'i2t': dict(BOTH, route=('mfma', 'scalar'), scalar_tile=('ncap16', 'far', 'W64'), per=(1, 2, 3), Nc_kernel=(0, 1023, 1024, 1025, 2049),
                **{'W*W': (256, 289, 4096),
                   'route,norm,ls': [(r, n, l) for n in ('clipped_l2norm', 'l2norm', 'softmax', 'l1norm')
                                     for r, l in (('mfma', 30.0), ('scalar', 30.5), ('scalar', 60.0), ('scalar', 60.5))] +
                   [('scalar', 'no_norm', 9.0), ('scalar', 'clipped', 9.0)]}),
}


def missing(cs, required):
    seen = {}
    for c in cs:
        for k, vs in c.seams().items():
            seen.setdefault(k, set()).update(str(v) for v in vs)
    return [(k, v) for k, vs in required.items() for v in vs if str(v) not in seen.get(k, ())]


@pytest.mark.parametrize("xa", E.DIRECTIONS)
def test_every_seam_value_has_a_case(xa):
    assert E.cases(xa)
    assert not missing(E.cases(xa), REQUIRED[xa])
    assert not missing(E.cases(xa), E.SEAMS[xa])
    for k, vs in REQUIRED[xa].items():          # the helper's own list asks for no less
        assert set(str(v) for v in vs) <= set(str(v) for v in E.SEAMS[xa][k]), k


@pytest.mark.parametrize("xa", E.DIRECTIONS)
def test_taking_out_a_sole_carrier_is_noticed(xa):
    """The mutation check: for every required value carried by exactly one case, the table without that case fails the coverage."""
    sole = {}
    for k, vs in REQUIRED[xa].items():
        for v in vs:
            carriers = [c for c in E.cases(xa) if str(v) in set(str(s) for s in c.seams().get(k, ()))]
            if len(carriers) == 1:
                sole.setdefault(carriers[0].name, []).append((k, v))
    assert len(sole) >= 8, sole         # (Ni = 65, n_tiles 7 .. 17, D = 32 .. 1024, every (route, norm, lambda) of the gate, ...)
    for name, what in sole.items():
        rest = [c for c in E.cases(xa) if c.name != name]
        assert set(what) <= set(missing(rest, REQUIRED[xa])), (name, what)


def test_table_shapes_follow_the_rules():
    assert 150 <= len(E.CASES) <= 300 and len(set(c.name for c in E.CASES)) == len(E.CASES)
    for c in E.CASES:
        assert c.R == E.SC_R == 36 and c.D % E.SC_BK == 0 and c.n_tok == sum(c.lens) and all(1 <= w <= S.ST_MAXW for w in c.lens), c
        assert c.Ni * c.n_tok * c.D <= 65 * 1088 * 32, c            # the largest: the 3 x 3 patch grid
        assert (c.ls == E.LAMBDA_SOFTMAX) == (c.group != 'gate' or c.norm in ('no_norm', 'clipped')), c
        x = c.inputs()
        assert x['images'].shape == (c.Ni, 36, c.D) and x['words'].shape == (c.n_tok, c.D)
        if c.zero:
            (zi, zr), zw = c.zero
            assert float(x['images'][zi, zr].abs().max()) == 0.0 and float(x['words'][zw].abs().max()) == 0.0
            assert zi == 0 and c.Ni % 4 and 0 < zw < c.n_tok - 1 and zw not in S._offsets(c.lens)
        assert (c.tied is not None) == (c.agg == 'Max')
    # the composition rows hold the tile they are there for, next to other tiles
    for xa in E.DIRECTIONS:
        for tag, (_, tile) in E.COMPOSITION.items():
            cs = [c for c in E.cases(xa, 'tile') if c.tag == tag]
            assert set(c.norm for c in cs) == {E.DEFAULT, 'softmax'} | ({'no_norm'} if xa == 'i2t' else set()), (xa, tag)
            assert all(tile in c.plan.summary and c.plan.n_tiles >= 2 for c in cs), (xa, tag)
        # every scalar-route case of the gate group meets a tile of 16 captions, a `far` tile and a caption of 64 words
        for c in E.cases(xa, 'gate'):
            if c.plan.route == 'scalar':
                assert c.seams()['scalar_tile'] == {'ncap16', 'far', 'W64'}, c
    # `far` set by a caption that is not the first of its tile: columns 31 .. 48 of (31, 18, 15)
    c = [c for c in E.cases('i2t', 'tile') if c.tag == '31.18.15'][0]
    t = [k for k, s in enumerate(c.plan.summary) if s == (3, 64, 1)][0]
    assert c.plan.layout[t][0] == [0, 31, 49, 64] and [c.plan.k_len[k] for k in c.plan.tiles[t]] == [31, 18, 15]


def test_planner_mirror():
    def by_size(lens):
        out = [[] for _ in range(65)]
        for c, w in enumerate(lens):
            out[w].append(c)
        return out

    rng = random.Random(5)
    sets = [c.plan.k_len for c in E.CASES if c.plan.k_len]
    sets += [[rng.choice((7, 13, 31, 32, 33, 64)) for _ in range(rng.randint(1, 80))] for _ in range(20)]
    sets += [[rng.randint(1, 64) for _ in range(rng.randint(1, 120))] for _ in range(20)]
    sets += [[rng.randint(1, 20) for _ in range(rng.randint(1, 300))] for _ in range(10)] + [[1] * 33, [64] * 3, [1], [63, 1, 1]]
    fewer = 0
    for lens in sets:
        tiles = E.pack_bins(lens)
        assert sorted(c for t in tiles for c in t) == list(range(len(lens))), lens
        for t in tiles:
            assert 1 <= len(t) <= 16 and sum(lens[c] for c in t) <= 64, (lens, t)
            assert [lens[c] for c in t] == sorted((lens[c] for c in t), reverse=True), (lens, t)       # largest first
            E.tile_layout(t, lens)
        bfd = E.pack_best_fit_decreasing(by_size(lens), 64, 16)
        assert len(tiles) <= len(bfd) and len(tiles) >= -(-sum(lens) // 64), lens
        fewer += len(E.pack_exact_fill(by_size(lens), 64, 16)) > len(bfd)
    assert fewer >= 1           # the fewer-bins choice is exercised: exact fill loses on some set
    # hand-checked plans
    assert E.pack_bins([1] * 17) == [list(range(16)), [16]]
    assert E.pack_bins([57, 7, 33, 31]) == [[0, 1], [2, 3]] and E.pack_bins([31, 18, 15, 57, 7]) == [[3, 4], [0, 1, 2]]
    assert E.tile_layout([0, 1, 2], [31, 18, 15]) == ([0, 31, 49, 64], [0] * 31 + [1] * 18 + [2] * 15, 1)
    assert E.tile_layout([0, 1], [32, 32])[2] == 0 and E.tile_layout([0, 1], [33, 31])[2] == 1 and E.tile_layout([0], [48])[2] == 1
    assert E.tile_layout([0, 1], [16, 32])[2] == 0 and E.tile_layout([0, 1], [15, 18])[2] == 1
    cs, cc, far = E.tile_layout([0, 1, 2], [3, 2, 1])
    assert cs == [0, 3, 5, 6] and cc[:7] == [0, 0, 0, 1, 1, 2, -1] and cc[7:] == [-1] * 57 and far == 0


def test_patch_walk_and_route_mirrors():
    assert E.patch_walk(5, 2)[:4] == (2, 1, 1, 512) and E.patch_walk(65, 17)[:3] == (17, 3, 3)
    assert E.patch_walk(65, 17)[4:] == ({0, 1}, {0}) and E.patch_walk(3, 128)[4:] == ({0, 1}, {0}) and E.patch_walk(3, 129)[4:] == ({0, 1}, {0, 1})
    assert E.patch_walk(33, 2)[:3] == (9, 2, 1) and E.patch_walk(32, 2)[:3] == (8, 1, 1) and E.patch_walk(5, 9)[4:] == ({0}, {0})
    assert E.patch_walk(3, 129)[3] == 2 * 512 and E.patch_walk(3, 128)[3] == 512
    assert [E.i2t_route(n, 9.0) for n in S.NORMS] == ['mfma', 'mfma', 'scalar', 'scalar', 'mfma', 'mfma', 'mfma']
    assert E.i2t_route('l2norm', 30.0) == E.i2t_route('l2norm', -30.0) == 'mfma' and E.i2t_route('l2norm', 30.5) == 'scalar'
    p = E.Plan(5, 96, (65, 5, 96, 7), 'i2t', 'l2norm', 9.0)
    assert (p.short_idx, p.long_idx, p.k_len, p.Nc_kernel, p.cap_col) == ([1, 3], [0, 2], [5, 7], 2, {3: (0, 0), 1: (0, 7)})
    assert [E.Plan(1, 32, [1] * n, 'i2t', 'l2norm', 9.0).per for n in (1023, 1024, 1025, 2049)] == [1, 1, 2, 3]
    assert (E.Plan(5, 64, (3,), 't2i', 'l2norm', 9.0).mainloop, E.Plan(5, 96, (3,), 't2i', 'l2norm', 9.0).mainloop) == ('simple', 'pipelined')


@pytest.mark.parametrize("xa", E.DIRECTIONS)
def test_mirror_is_the_oracles_function_and_the_bound_is_tight(xa):
    worst = 0.0
    for c in E.cases(xa):
        want, e_oracle, e_mirror, tol, agree = c.reference()
        m = float(want.abs().max())
        assert want.shape == (c.Ni, c.Nc) and bool(torch.isfinite(want).all()) and e_oracle == e_oracle and e_mirror == e_mirror, c
        assert agree <= E.MIRROR_AGREES * max(1.0, m), (c, agree)
        if not c.big:           # ... and the training table's mirror of the same pair (softmax of lambda * _first_norm), a third writing of it
            x = {k: v.double() for k, v in c.inputs().items()}
            train = (S.mirror_t2i if xa == 't2i' else S.mirror_i2t)(x, c.lens, c.norm, c.agg, lambda_softmax=c.ls)['S']
            assert float((train - c.evaluate(torch.float64, c.mirror)).abs().max()) <= E.MIRROR_AGREES * max(1.0, m), c
        if c.name not in E.FALLBACK:
            assert tol == E.FACTOR * max(e_oracle, e_mirror, E.U * m), c
        assert tol <= E.CAP * m, "%s: tol %.3g is %.3g of max|want| %.3g (e32 oracle %.3g, mirror %.3g)" % (c, tol, tol / m, m, e_oracle, e_mirror)
        assert tol <= c.old_bound(), "%s: tol %.3g is looser than the older tests' %.3g" % (c, tol, c.old_bound())
        assert tol < E.OLD_BOUND or c.agg == 'Sum', c
        worst = max(worst, tol / (E.CAP * m))
    assert worst <= 0.25        # (the issue's probes: 0.16 of the cap; this table: at most 0.02)


@pytest.mark.parametrize("xa", E.DIRECTIONS)
def test_bound_sees_every_claimed_defect(xa):
    claimed = {}
    for c in E.cases(xa):
        want, _, _, tol, _ = c.reference()
        for letter, value in c.defects().items():
            assert value.shape == want.shape, (c, letter)
            moved = float((value - want).abs().max())
            assert moved >= E.SENSITIVITY * tol, "%s defect %s moves S by %.3g, %.3g x its bound" % (c, letter, moved, moved / tol)
            claimed.setdefault(letter, []).append(c)
    assert set(claimed) == set('abcpsmt' if xa == 't2i' else 'abcsfto')
    # the claims follow the rules of the helper's docstring, restated
    for c in E.cases(xa):
        p = c.plan
        want = 'a' if c.big else 'ab' + ('c' if c.max_len > 1 else '') + ('p' if xa == 't2i' and c.agg in ('LogSumExp', 'Mean') else '') + \
            ('s' if any(len(t) > 1 and p.k_len[t[k]] > 1 for t in p.tiles for k in range(len(t) - 1)) else '')
        want += 'm' if xa == 't2i' and c.agg == 'Mean' and any(n > 1 for n, _, _ in p.summary) else ''
        want += 'f' if xa == 'i2t' and p.route == 'mfma' and any(f for _, _, f in p.summary) else ''
        want += 't' if c.Ni % 4 and c.Ni > 1 and p.n_tiles and (xa == 't2i' or c.zero) else ''
        want += 'o' if xa == 'i2t' and p.Nc_kernel > 1024 else ''
        assert c.claims == want, (c, c.claims, want)
    assert all(c.big == (c.group == 'prep' and c.Nc > 1000) for c in E.cases(xa))
    # Max: the dropped element carries the maximum (the tie), and every `far` tile composition is claimed on the matrix-core route
    assert any(c.agg == 'Max' for c in claimed['b']) and any(c.agg == 'Max' for c in claimed['c'])
    if xa == 'i2t':
        assert {'one64', 'blockseams', '33.31', '31.18.15'} <= set(c.tag for c in claimed['f'])
        assert set(c.plan.Nc_kernel for c in claimed['o']) == {1025, 2049}
        assert all(c.zero for c in claimed['t'])
    else:
        assert set(c.Ni for c in claimed['t']) >= {2, 3, 5, 31, 33, 65}


def test_a_zero_word_moves_no_i2t_score():
    """Why no i2t case claims the counted padding column (helper docstring): the oracle itself does not see it."""
    c = [c for c in E.cases('i2t', 'norm') if c.norm == 'l2norm' and c.agg == 'Sum'][0]
    x = {k: v.double() for k, v in c.inputs().items()}
    lens = (c.lens[0] + 1,) + c.lens[1:]
    x['words'] = torch.cat([x['words'][:c.lens[0]], torch.zeros(1, c.D, dtype=torch.float64), x['words'][c.lens[0]:]], 0)
    got = S.oracle(x, 'i2t', lens, c.norm, c.agg, c.ls)['S']
    assert float((got - c.reference()[0]).abs().max()) <= 1e-12


def test_fallback_list():
    assert set(E.FALLBACK) <= set(c.name for c in E.CASES)
    assert len(E.FALLBACK) <= E.FALLBACK_SHARE * len(E.CASES)
    assert E.FALLBACK_SHARE == 0.02 and E.FACTOR == P.FACTOR == 16 and E.U == P.U == 2.0 ** -24 and E.SENSITIVITY == P.SENSITIVITY == 10
    assert E.CAP == 2.0 ** -10 and E.MIRROR_AGREES == 1e-11 and (E.LAMBDA_LSE, E.LAMBDA_SOFTMAX) == (6.0, 9.0) and E.OLD_BOUND == 2e-5
    assert all(v <= E.OLD_BOUND for v in E.FALLBACK.values())


def test_the_training_references_kept_their_defaults():
    """lambda_softmax is an optional argument of the training table's references; its default is the value they had built in."""
    c = [c for c in S.cases('t2i') if c.max_len >= 5][0]         # (a one-word caption has one i2t weight, 1 at any lambda)
    x = {k: v.double() for k, v in c.inputs().items()}
    for fn in (lambda **kw: S.oracle(x, c.xa, c.lens, c.norm, c.agg, **kw), lambda **kw: S.mirror_t2i(x, c.lens, c.norm, c.agg, **kw),
               lambda **kw: S.mirror_i2t(x, c.lens, c.norm, c.agg, **kw)):
        assert torch.equal(fn()['S'], fn(lambda_softmax=9.0)['S']) and not torch.equal(fn()['S'], fn(lambda_softmax=4.0)['S'])


def _src(*path):
    with open(os.path.join(PKG, *path)) as f:
        return re.sub(r"\s+", " ", f.read())


def test_constants_are_the_ones_of_the_source():
    """The mirrors' constants and gates, as the source text states them (whitespace folded)."""
    text = {"scan_common.h": _src("csrc", "scan_common.h"), "scan_xattn.hip": _src("csrc", "scan_xattn.hip"), "pack_plan.h": _src("csrc", "pack_plan.h"),
            "scan_mainloop.inc": _src("csrc", "scan_mainloop.inc"), "ops.py": _src("itr_amd", "ops.py"),
            "itr_hip.h": _src("..", "include", "itr_hip.h")}
    pins = {
        "scan_common.h": ("constexpr int SC_R = %d;" % E.SC_R, "constexpr int SC_IMGS = %d;" % E.SC_IMGS, "constexpr int SC_NT = ITR_SCAN_NT;",
                          "constexpr int SC_MAXCAP = %d;" % E.SC_MAXCAP, "constexpr int SC_BK = %d," % E.SC_BK),
        "itr_hip.h": ("#define ITR_SCAN_NT %d" % E.SC_NT,),
        "pack_plan.h": (
            "constexpr int PACK_MAXN = %d;" % E.PACK_MAXN,
            # exact fill
            "for (int w = (L < rem ? L : rem); w >= 1; --w) {", "for (int s = 0; s + w <= rem; ++s) {",
            "for (int k = 1; k <= avail[w] && s + k * w <= rem && best[s] + k <= maxn - 1; ++k)", "if (best[s] + k < nb[s + k * w]) {",
            "while (best[s] == INF) --s;", "if (cnt[w] && avail[w] / cnt[w] < reps) reps = avail[w] / cnt[w];",
            "for (int w = L; w >= 1; --w) // largest first, as the kernels' unit tables expect nothing else",
            # best fit decreasing and the choice
            "while (r <= cap && open[r].empty()) ++r;", "if (B.n < maxn && r - w > 0) open[r - w].push_back(t);",
            "const std::vector<PackBin> &best = b.size() < a.size() ? b : a;",
        ),
        "scan_xattn.hip": (
            "itr::pack_bins(by_len, nt, itr::SC_MAXCAP, tiles);",
            # the column layout
            "if (w > 0 && ((pos + w - 1) >> 4) - (pos >> 4) >= 2) far = 1;", "for (int k = n; k <= SC_MAXCAP; ++k) m.cap_start[k] = pos;",
            # the patch walk, in the kernel and at the launch
            "const int64_t PI = (img_tiles + 7) / 8, PJ = (g.n_tiles + 7) / 8;", "const int64_t xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;",
            "const int64_t pgroup = slot >> 6;", "const int within = (int)(slot & 63);",
            "const int64_t patch = (pgroup * g.tpw + rep) * 8 + xcd;", "if (patch >= PI * PJ) break;",
            "const int64_t it = (patch / PJ) * 8 + (within & 7);", "const int64_t ct = (patch % PJ) * 8 + (within >> 3);",
            "if (it >= img_tiles || ct >= g.n_tiles) continue;", "a.tpw = %d;" % E.TPW,
            "const int64_t grid = ceil_div(ceil_div(PI * PJ, 8), (int64_t)a.tpw) * 64 * 8;",
            # the i2t route gate
            "const bool mfma_path = (norm == 0 || norm == 1 || norm == 2 || norm == 5 || norm == 6) && fabsf(ls) <= %d.f;" % E.I2T_MFMA_LS,
            # the preparation
            "__global__ __launch_bounds__(%d) void sq_prefix_kernel(" % E.PREFIX_THREADS, "const int64_t per = (n + %d) / %d;" % (E.PREFIX_THREADS - 1, E.PREFIX_THREADS),
            "hipLaunchKernelGGL(sq_prefix_kernel, dim3(1), dim3(%d), 0, st, cap_len, Nc, w.coff);" % E.PREFIX_THREADS,
            "float acc[%d]; // up to 64*64/256 pairs per thread" % E.GRAM_ACC, "for (int e = 0; e < %d; ++e) {" % E.GRAM_ACC,
            # the arithmetic the mirror copies
            "const float ls_log2e = ls * 1.44269504088896341f;", "e[r] = FOLDED ? __builtin_amdgcn_exp2f(e[r]) : fast_exp(e[r] - mx);",
            "const float w2 = fast_sqrt(fmaxf(q, 0.f));", "simv = num * fast_rcp(fmaxf(w1 * w2, 1e-8f));",
            "if (mfma_path && NORM != 2) na.s0 *= ls * 1.44269504088896341f;",
            "const float w2 = fast_sqrt(fmaxf(sq[j], 0.f)) * rden;", "rs_out[r2 * SC_MAXCAP + fi] = (snum[j] * rden) * fast_rcp(fmaxf(w1 * w2, 1e-8f));",
            "sm.rsim2[tid][k] = (num * rden) / fmaxf(w1 * w2, 1e-8f);",
        ),
        "scan_mainloop.inc": ("const int nk = g.D / SC_BK;", "if (nk >= %d) {" % E.PIPELINE_NK),
        "ops.py": ("long_mask = self.len_host > (SCAN_NT if max_kernel_len is None else max_kernel_len)",
                   "out[:, torch.from_numpy(plan.short_idx).to(dev)] = part"),
    }
    for name, lines in pins.items():
        for line in lines:
            assert line in text[name], "%s no longer says: %s" % (name, line)
    assert E.MFMA_NORMS == tuple(S.NORMS[k] for k in (0, 1, 4, 5, 6))          # norms 0, 1, 2, 5, 6 of the library's numbering
    ops_text = text["ops.py"]
    for k, name in ((0, 'clipped_l2norm'), (1, 'l2norm'), (2, 'softmax'), (5, 'l1norm'), (6, 'clipped_l1norm')):
        assert re.search(r"['\"]%s['\"]: %d\b" % (name, k), ops_text), name
