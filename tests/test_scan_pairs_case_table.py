"""No GPU: the case table of the SCAN candidate-list sweep (tests/helpers/scan_pairs_cases.py) is fit for its purpose.

References: the float64 mirror of the pair kernels' algebra is the oracle's function (1e-11) on every compared tensor, so its float32
run measures that algebra's own rounding.  Bounds: every tensor's tol is at most 2^-10 of its largest value, and for scores and cosines
never looser than what the older tests hold the kernels to.  Planning mirrors: block offsets, the bisection, the grid bound and the
attention pairs' units on hand-checked lists.  Coverage: every seam value keeps a case (stated here a second time), and taking the sole
carrier of a value out of the table is noticed.  Sensitivity: each claimed defect moves some compared tensor by at least 10 x the bound
the GPU sweep applies to it.  Pins: the constants the mirrors copy are checked against the source text of csrc/ and ops.py."""
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import scan_pairs_cases as C        # noqa: E402
import scan_train_cases as S        # noqa: E402
import train_prim_cases as P        # noqa: E402

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "image-text-retrieval_amd")
KD = [(k, xa) for k in C.KERNELS for xa in C.DIRECTIONS]
ZERO = ((0, 7), 8)

# what the table must hold, stated here a second time: an edit that shrinks SEAMS in the helper does not shrink the requirement
BOTH = {
    'norm,agg': [(n, a) for n in S.NORMS for a in S.AGGS],
    'D': (16, 32, 48, 64, 272), 'chunks': (1, 2, 3, 4, 17),
    'W': (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 22, 23), 'ncb': (1, 2, 3, 4),
    'Nc': (1, 2, 1023, 1024, 1025, 2049), 'Ni': (1, 9), 'listed_at': (0, 1022, 1023, 1024, 2048), 'image': ('last',),
    'ls': (4.0, 9.0), 'zero': (ZERO,), 'abi': (0, 1),
}
SCORES = dict(BOTH, n_c=(0, 1, 7, 8, 9, 16, 17), blocks=(0, 1, 2, 3), empty_at=('first', 'last', 'run', 'all_but_one'), per=(1, 2, 3),
              image=('last', 'block_of_one'), by=('caption', 'image', 'abi'), long_at=('first', 'middle', 'last'), only_long=(0, 1))
ATTENTION = dict(BOTH, W=BOTH['W'] + (65, 79, 80, 81, 95, 96), ncb=(1, 2, 3, 4, 5, 6), rounds=(1, 2), direct=(0, 1), P=(1, 3, 4, 5, 8, 9),
                 mixed_wg=(1,))
I2T = {'W*W': (484, 529, 4096), 'stage': ('<=512', '>512'), 'per': (1, 2, 3)}
REQUIRED = {('scores', 't2i'): SCORES, ('scores', 'i2t'): dict(SCORES, **I2T),
            ('attention', 't2i'): ATTENTION, ('attention', 'i2t'): dict(ATTENTION, **I2T)}


def missing(cs, required):
    seen = {}
    for c in cs:
        for k, vs in c.seams().items():
            seen.setdefault(k, set()).update(str(v) for v in vs)
    return [(k, v) for k, vs in required.items() for v in vs if str(v) not in seen.get(k, ())]


@pytest.mark.parametrize("kernel,xa", KD)
def test_every_seam_value_has_a_case(kernel, xa):
    assert C.cases(kernel, xa)
    assert not missing(C.cases(kernel, xa), REQUIRED[kernel, xa])
    assert not missing(C.cases(kernel, xa), C.SEAMS[kernel, xa])
    for k, vs in REQUIRED[kernel, xa].items():          # the helper's own list asks for no less
        assert set(str(v) for v in vs) <= set(str(v) for v in C.SEAMS[kernel, xa][k]), k


@pytest.mark.parametrize("kernel,xa", KD)
def test_taking_out_a_sole_carrier_is_noticed(kernel, xa):
    """The mutation check: for every required value carried by exactly one case, the table without that case fails the coverage."""
    sole, req = {}, REQUIRED[kernel, xa]
    for k, vs in req.items():
        for v in vs:
            carriers = [c for c in C.cases(kernel, xa) if str(v) in set(str(s) for s in c.seams().get(k, ()))]
            if len(carriers) == 1:
                sole.setdefault(carriers[0].name, []).append((k, v))
    assert len(sole) >= 6, sole         # (D = 16 .. 272, Nc = 1 .. 2049, lambda = 4, the direct call, ...)
    for name, what in sole.items():
        rest = [c for c in C.cases(kernel, xa) if c.name != name]
        assert set(what) <= set(missing(rest, req)), (name, what)


def test_table_shapes_follow_the_rules():
    assert 150 <= len(C.CASES) <= 300 and len(set(c.name for c in C.CASES)) == len(C.CASES)
    for c in C.CASES:
        assert c.R == 36 and c.D % C.SP_BK == 0 and c.n_tok == sum(c.lens) and all(1 <= w <= C.SA_MAXW for w in c.lens), c
        assert c.Ni <= 9 and c.n_tok <= 2049 * 4 and c.P <= 160 and c.n_tok * c.D <= 624 * 272, c        # small: a handful of images
        assert (c.ls == C.LAMBDA_SOFTMAX) == (c.group != 'ls') and c.ls in (4.0, 9.0), c
        assert c.Nc < 1000 or (max(c.lens) <= 4 and len(c.listed) <= 12), c
        x = c.inputs()
        assert x['images'].shape == (c.Ni, 36, c.D) and x['words'].shape == (c.n_tok, c.D)
        if c.zero:
            (zi, zr), zw = c.zero
            assert float(x['images'][zi, zr].abs().max()) == 0.0 and float(x['words'][zw].abs().max()) == 0.0
            assert 0 < zw < c.n_tok - 1 and zw not in c.off and any(i == zi for i, _ in c.pairs)
            assert any(c.off[k] < zw < c.off[k] + c.lens[k] for k in c.listed)
        assert (c.tied is not None) == (c.agg == 'Max')
        if c.tied:
            i, r, w = c.tied
            assert any(ii == i and c.off[cc] + c.lens[cc] - 1 == w for ii, cc in c.pairs), c        # the tie sits on a listed pair
        if c.kernel == 'scores':
            p = c.plan
            assert (c.cand is None) == c.abi and sorted(p.pair_out + p.long_pairs) == list(range(c.P)), c
            assert p.n_blocks == sum(C.blocks_of(n) for n in p.counts) <= p.grid == (C.grid_bound(p.P, c.Nc) if p.P else 0), c
            assert p.cap_ptr[-1] == p.P == len(p.pair_img) and all(c.lens[k] > 64 for _, k in (c.pairs[s] for s in p.long_pairs)), c
        else:
            assert c.cand is None and c.plan is None
    # the direct call's list is one no `by` produces: slots descend inside a caption; its blocks meet every count of the seam
    for xa in C.DIRECTIONS:
        c, = C.cases('scores', xa, 'abi')
        assert any(len(v) > 1 and [s for _, s in v] == sorted((s for _, s in v), reverse=True) for v in c.plan.per_cap)
        assert set(c.plan.counts) == {0, 1, 8, 9, 17}
        # the large caption sets list captions on both sides of the 1024-thread seam, over hundreds of captions listed by nobody
        for c in C.cases('scores', xa, 'Nc'):
            if c.Nc >= 1025:
                assert {0, 1023, 1024, c.Nc - 1} <= set(c.listed) and 'run' in c.seams()['empty_at'] and 'k' in c.claims, c
        # a caption of more than 64 words and one of fewer share a workgroup of the attention kernel
        assert all('mixed_wg' in c.seams() for c in C.cases('attention', xa, 'P') if c.P >= 3)


def test_planning_mirrors():
    assert [C.ncb(w) for w in (1, 16, 17, 32, 33, 48, 49, 64, 65, 80, 81, 96)] == [1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6]
    assert [C.chunks(d) for d in (16, 32, 48, 64, 272)] == [1, 2, 3, 4, 17]
    assert [C.blocks_of(n) for n in (0, 1, 7, 8, 9, 16, 17)] == [0, 1, 1, 1, 2, 2, 3]
    assert [C.prefix_per(n) for n in (1, 1023, 1024, 1025, 2048, 2049)] == [1, 1, 1, 2, 2, 3]
    assert C.blk_ptr_of([0, 9, 0, 0, 17, 8, 1, 0]) == [0, 0, 2, 2, 2, 5, 6, 7, 7]
    bp = C.blk_ptr_of([0, 9, 0, 0, 17, 8, 1, 0])
    assert [C.bisect_caption(bp, b, 8) for b in range(7)] == [1, 1, 4, 4, 4, 5, 6]          # over equal neighbours, never an empty caption
    assert C.bisect_caption([0, 3], 2, 1) == 0 and C.bisect_caption([0, 0, 1], 0, 2) == 1
    # per = 2, 3: the thread-by-thread scan is the plain prefix sum
    for n in (1025, 2049):
        counts = [(7 * k) % 19 if k % 5 == 0 else 0 for k in range(n)]
        want, run = [], 0
        for v in counts:
            want.append(run)
            run += C.blocks_of(v)
        assert C.blk_ptr_of(counts) == want + [run]
    assert C.grid_bound(35, 8) == 13 and C.grid_bound(3, 2049) == 4 and C.grid_bound(8, 1) == 3
    for counts in ([1] * 40, [8] * 5, [9] * 5, [0, 0, 17], [7, 1, 1, 1]):
        assert sum(C.blocks_of(n) for n in counts) <= C.grid_bound(sum(counts), len(counts))
    assert C.sq_offsets([2, 0, 3, 1]) == [0, 4, 4, 13]
    assert [C.attn_unit(p, w) for p, w in ((0, 1), (3, 64), (4, 65), (9, 96))] == [(0, 0, 1), (0, 3, 1), (1, 0, 2), (2, 1, 2)]
    p = C.ScoresPlan(9, (65, 5, 96, 7), [(0, 0), (1, 1), (2, 2), (3, 3), (4, 1)])
    assert (p.klen, p.long_pairs, p.counts, p.pair_img, p.pair_out, p.cap_ptr) == ([0, 5, 0, 7], [0, 2], [0, 2, 0, 1], [1, 4, 3], [1, 4, 3], [0, 0, 2, 2, 3])
    assert p.blocks == [(1, [(1, 1), (4, 4)]), (3, [(3, 3)])] and (p.n_blocks, p.grid) == (2, 0 + 3 + 1)
    assert C.lists_by_image((2, 0, 1), 3) == [[0], [0], [2]] and C.lists_by_caption(2, 9, 3, 1) == [[1, 3, 5], [2, 4, 6]]


@pytest.mark.parametrize("kernel,xa", KD)
def test_mirror_is_the_oracles_function_and_the_bound_is_tight(kernel, xa):
    worst = 0.0
    for c in C.cases(kernel, xa):
        ref = c.reference()
        assert tuple(ref) == C.TENSORS[kernel]
        n_words = sum(c.lens[k] for _, k in c.pairs)
        for t, (want, e_oracle, e_mirror, tol, agree) in ref.items():
            m = float(want.abs().max())
            assert want.shape == ({'score': c.P, 'attn': n_words * 36, 'row_sim': n_words if xa == 't2i' else c.P * 36}[t],), (c, t)
            assert bool(torch.isfinite(want).all()) and e_oracle == e_oracle and e_mirror == e_mirror, (c, t)
            assert agree <= C.MIRROR_AGREES * max(1.0, m), (c, t, agree)
            if c.name not in C.FALLBACK:
                assert tol == C.FACTOR * max(e_oracle, e_mirror, C.U * m), (c, t)
            assert tol <= C.CAP * m, "%s %s: tol %.3g is %.3g of max|want| %.3g (e32 oracle %.3g, mirror %.3g)" % (c, t, tol, tol / m, m, e_oracle, e_mirror)
            old = c.old_bound(t)
            assert (old is None) == (t == 'attn')
            if old is not None:
                assert tol <= old, "%s %s: tol %.3g is looser than the older tests' %.3g" % (c, t, tol, old)
                assert tol < C.OLD_BOUND or c.agg == 'Sum', (c, t)
            worst = max(worst, tol / (C.CAP * m))
        if kernel == 'attention':       # every t2i row and i2t column of the float64 matrices sums to 1
            o = 0
            for _, k in c.pairs:
                A = ref['attn'][0][o:o + c.lens[k] * 36].view(-1, 36)
                assert float((A.sum(1 if xa == 't2i' else 0) - 1.0).abs().max()) <= 1e-12, c
                o += A.numel()
    assert worst <= 0.25        # (the issue's probe of the oracle half: 0.03 of the cap; this table: at most 0.031)


@pytest.mark.parametrize("kernel,xa", KD)
def test_bound_sees_every_claimed_defect(kernel, xa):
    claimed = {}
    for c in C.cases(kernel, xa):
        ref, defects = c.reference(), c.defects()
        assert set(defects) == set(c.claims), c
        for letter, res in defects.items():
            assert res, (c, letter)
            best = 0.0
            for t, value in res.items():
                want, _, _, tol, _ = ref[t]
                assert value.shape == want.shape, (c, letter, t)
                best = max(best, float((value - want).abs().max()) / tol)
            assert best >= C.SENSITIVITY, "%s defect %s moves no tensor by more than %.3g x its bound" % (c, letter, best)
            claimed.setdefault(letter, []).append(c)
    want = 'abcrn' + ('k' if kernel == 'scores' else '2Td') + ('go' if xa == 'i2t' else 't') + ('l' if (kernel, xa) == ('attention', 't2i') else '')
    assert set(claimed) == set(want)
    # the claims follow the rules of the helper's docstring, restated
    for c in C.cases(kernel, xa):
        L = [c.lens[k] for k in c.listed]
        taken = [k for k in c.listed if kernel == 'attention' or c.lens[k] <= 64]
        short = [k for k in c.listed if c.lens[k] <= 64]
        w = 'ab' + ('c' if max(L) > 1 else '')
        if xa == 'i2t':
            w += 'r' if max(L) > 1 else ''
        elif c.agg in ('LogSumExp', 'Sum') or (max(L) > 1 and (c.agg == 'Mean' or c.norm not in ('no_norm', 'clipped'))):
            w += 'r'
        units = c.units()
        assert sorted(p for u in units for p in u) == sorted(p for p, (_, k) in enumerate(c.pairs) if k in taken), c
        assert all(len(u) <= (8 if kernel == 'scores' else 4) for u in units), c
        w += 'n' if any(c.pairs[u[j]][0] != c.pairs[u[j ^ 1]][0] for u in units for j in range(len(u)) if (j ^ 1) < len(u)) else ''
        if kernel == 'scores':
            nz = [k for k, n in enumerate(c.plan.counts) if n]
            w += 'k' if any(c.plan.counts[k] > 8 for k in nz[:-1]) else ''
        w += ('g' if len(short) >= 2 else '') + ('o' if any(k >= 1024 for k in short) else '') if xa == 'i2t' else ''
        w += 't' if xa == 't2i' and c.Ni > 1 and any(i == c.Ni - 1 and k in taken for i, k in c.pairs) else ''
        if kernel == 'attention':
            w += ('2' + ('l' if xa == 't2i' and c.agg != 'Max' else '') if max(L) > 64 else '') + ('T' if max(L) > 1 else '') + 'd'
        assert sorted(c.claims) == sorted(w), (c, c.claims, w)
    # Max: the dropped element carries the maximum (the tie); the bisection defect is claimed across a run of unlisted captions
    assert any(c.agg == 'Max' for c in claimed['b']) and any(c.agg == 'Max' for c in claimed['c'])
    if kernel == 'scores':
        assert any('run' in c.seams()['empty_at'] for c in claimed['k']) and any(c.abi for c in claimed['k'])
    if xa == 'i2t':
        assert set(c.Nc for c in claimed['o']) == {1025, 2049}
    else:
        assert len(claimed['t']) >= 40
    if kernel == 'attention':
        assert set(w for c in claimed['2'] for w in c.listed_lens if w > 64) >= {65, 79, 80, 81, 95, 96}


def test_fallback_list():
    assert set(C.FALLBACK) <= set(c.name for c in C.CASES)
    assert len(C.FALLBACK) <= C.FALLBACK_SHARE * len(C.CASES)
    assert C.FALLBACK_SHARE == 0.02 and C.FACTOR == P.FACTOR == 16 and C.U == P.U == 2.0 ** -24 and C.SENSITIVITY == P.SENSITIVITY == 10
    assert C.CAP == S.CAP == 2.0 ** -10 and C.MIRROR_AGREES == 1e-11 and (C.LAMBDA_LSE, C.LAMBDA_SOFTMAX) == (6.0, 9.0) and C.OLD_BOUND == 2e-5
    assert all(v <= C.OLD_BOUND for d in C.FALLBACK.values() for v in d.values())


def _src(*path):
    with open(os.path.join(PKG, *path)) as f:
        return re.sub(r"\s+", " ", f.read())


def test_constants_are_the_ones_of_the_source():
    """The mirrors' constants and index arithmetic, as the source text states them (whitespace folded)."""
    text = {"scan_pairs.hip": _src("csrc", "scan_pairs.hip"), "scan_attn.hip": _src("csrc", "scan_attn.hip"), "pair_mainloop.h": _src("csrc", "pair_mainloop.h"),
            "pair_epilogue.h": _src("csrc", "pair_epilogue.h"), "scan_xattn.hip": _src("csrc", "scan_xattn.hip"), "scan_common.h": _src("csrc", "scan_common.h"),
            "ops.py": _src("itr_amd", "ops.py")}
    pins = {
        "scan_common.h": ("constexpr int SC_R = %d;" % C.SC_R,),
        "pair_mainloop.h": (
            "constexpr int SP_LDP = SC_R + 1;", "constexpr int SP_BK = %d;" % C.SP_BK,
            "w = w < W ? w : W - 1;", "const int kn = (k0 + SP_BK < D) ? k0 + SP_BK : k0;", "for (int k0 = 0; k0 < D; k0 += SP_BK) {",
            "if (r < SC_R) pk[(nt * 16 + fi) * SP_LDP + r] = acc[mt][nt][q];",
        ),
        "pair_epilogue.h": (
            "constexpr int SP_MAXW = %d;" % C.SP_MAXW,
            "if (NORM == 0 || NORM == 1) s0 = 1.f / (sqrtf(s0) + 1e-8f);", "else if (NORM == 5 || NORM == 6) s0 = 1.f / (s0 + 1e-8f);",
            "else if (NORM == 2) s1 = 1.f / s1;", "if (NORM == 2) return fast_exp(a - t0) * t1;",
        ),
        "scan_pairs.hip": (
            "constexpr int SP_IMGS = %d;" % C.SP_IMGS, "constexpr int SP_THREADS = SP_IMGS * 64;",
            # the work units
            "if (b >= g.blk_ptr[Nc]) return;", "int lo = 0, hi = Nc;", "while (hi - lo > 1) {", "if (g.blk_ptr[mid] <= b) lo = mid; else hi = mid;",
            "const int64_t p = (int64_t)g.cap_ptr[c] + (int64_t)(b - g.blk_ptr[c]) * SP_IMGS + wave;",
            "const bool have = p >= 0 && p < g.P && p < (int64_t)g.cap_ptr[c + 1];", "const bool cap_ok = W >= 1 && W <= SP_MAXW;",
            "const bool slot_ok = have && oidx >= 0 && (int64_t)oidx < g.out_len;",
            "const bool run = slot_ok && cap_ok && ii >= 0 && (int64_t)ii < g.Ni;", "const int ncb = (W + 15) >> 4;",
            "if (slot_ok && lane == 0) g.out[oidx] = score;",
            # i2t: the staged Gram matrix
            "for (int idx = tid; idx < W * W; idx += SP_THREADS) hc[idx] = H[idx];",
            # the block plan and the grid bound
            "__global__ __launch_bounds__(%d) void pairs_blkptr_kernel(" % C.PREFIX_THREADS, "const int64_t per = (n + %d) / %d;" % (C.PREFIX_THREADS - 1, C.PREFIX_THREADS),
            "return cnt > 0 ? (cnt + SP_IMGS - 1) / SP_IMGS : 0;",
            "hipLaunchKernelGGL(pairs_blkptr_kernel, dim3(1), dim3(%d), 0, st, cap_ptr, Nc, w.blk_ptr);" % C.PREFIX_THREADS,
            "hipLaunchKernelGGL(sq_prefix_kernel, dim3(1), dim3(%d), 0, st, cap_len, Nc, w.coff);" % C.PREFIX_THREADS,
            "const int64_t grid = P / SP_IMGS + (Nc < P ? Nc : P) + 1;",
            # the arithmetic the mirror copies
            "e[r] = fast_exp(e[r] - mx);", "for (int s = r; s < SC_R; ++s) t = fmaf(G[r * SC_R + s], e[s], t);",
            "const float w2 = sqrtf(fmaxf(q, 0.f)) * rden;", "sim = (num * rden) / fmaxf(w1 * w2, 1e-8f);",
            "hipLaunchKernelGGL(gram_mfma_kernel, dim3((unsigned)Ni), dim3(256), 0, st, img, R, D, w.gram, 1);",
        ),
        "scan_attn.hip": (
            "constexpr int SA_WAVES = %d;" % C.SA_WAVES, "constexpr int SA_MAXW = %d;" % C.SA_MAXW,
            "const int64_t p = (int64_t)blockIdx.x * SA_WAVES + wave;", "if (p >= g.P) return;", "const int ncb = (W + 15) >> 4;",
            "if (ncb == 5) pair_mainloop<1>(vi, ec + (int64_t)64 * g.D, W - 64, g.D, lane, pk + 64 * SP_LDP);",
            "else if (ncb == 6) pair_mainloop<2>(vi, ec + (int64_t)64 * g.D, W - 64, g.D, lane, pk + 64 * SP_LDP);",
            "for (int wb = 0; wb < W; wb += 64) {", "if (W <= SP_MAXW) {", "for (int i = lane; i < n; i += 64) {",
            "const int w = i / SC_R, r = i - w * SC_R;", "const unsigned grid = (unsigned)ceil_div(P, SA_WAVES);",
            "const float w2 = sqrtf(fmaxf(q, 0.f)) * rden;", "sim = (num * rden) / fmaxf(w1 * w2, 1e-8f);",
        ),
        "scan_xattn.hip": (
            "__global__ __launch_bounds__(%d) void sq_prefix_kernel(" % C.PREFIX_THREADS, "const int64_t per = (n + %d) / %d;" % (C.PREFIX_THREADS - 1, C.PREFIX_THREADS),
            "if (upper2) v = s_ > r ? 2.f * v : (s_ == r ? v : 0.f);",
        ),
        "ops.py": ("off, klen = _caption_tables(plan, dev, SCAN_NT)", "lens = plan.len_host if max_words is None else np.where(plan.len_host > max_words, 0, plan.len_host)",
                   "cap_ptr, caps, imgs, slot = _group_pairs(caps, Nc, (imgs, slot), grouped=by == 'caption')", "key, order = torch.sort(key, stable=True)",
                   "SCAN_NT = %d" % C.SP_MAXW),
    }
    for name, lines in pins.items():
        for line in lines:
            assert line in text[name], "%s no longer says: %s" % (name, line)
    assert C.SP_LDP == C.SC_R + 1 and C.STAGE_THREADS == C.SP_IMGS * 64 == 512
    assert (22 * 22 <= C.STAGE_THREADS < 23 * 23) and 64 * 64 == 8 * C.STAGE_THREADS
