"""No GPU: the case table of the training-primitive sweep (tests/helpers/train_prim_cases.py) is fit for its purpose.

Sensitivity: for every case, the float64 result with the LAST index of its reduced / tiled axis left out differs from the reference
by at least 10 x the bound the GPU sweep will apply -- so a kernel that drops one row, column or element cannot pass.  Coverage:
every seam of the launch geometry keeps a case on both sides, so a later edit cannot quietly thin the table."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import train_prim_cases as T        # noqa: E402

_WITH_DEFECT = [c for c in T.CASES if c.defect is not None]
_DERIVED = {
    ('gate_apply', 'n'): lambda s: s['rows'] * s['dk'],
    ('gru_cell', 'n'): lambda s: s['B'] * s['H'],
    ('addattn_score', 'rows'): lambda s: s['B'] * s['N'],
}


@pytest.mark.parametrize("case", _WITH_DEFECT, ids=repr)
def test_bound_sees_a_dropped_last_element(case):
    ref, bad = case.reference(), case.defects()
    assert bad, case
    for name, d in bad.items():
        want, e32, tol, rule = ref[name]
        assert torch.isfinite(want).all()
        moved = float((d - want).abs().max())
        assert moved >= T.SENSITIVITY * tol, "%s %s: defect moves %.3g, bound %.3g (%s, e32 %.3g)" % (case, name, moved, tol, rule, e32)


def test_every_case_has_a_defect_or_is_exact():
    for c in T.CASES:
        assert c.defect is not None or c.exact, c
    assert len(set(c.name for c in T.CASES)) == len(T.CASES)


def test_references_are_finite_and_small():
    for c in T.CASES:
        for name, (want, e32, tol, rule) in c.reference().items():
            assert torch.isfinite(want).all(), (c, name)
            assert want.numel() * 8 < 4 << 20, (c, name)          # the widest tensor stays below a few MB
            assert e32 == e32 and e32 < float('inf'), (c, name)


@pytest.mark.parametrize("op", sorted(T.SEAMS))
def test_every_seam_has_a_case_on_both_sides(op):
    have = T.cases(op)
    assert have, op
    for param, values in T.SEAMS[op].items():
        get = _DERIVED.get((op, param), lambda s, p=param: s[p])
        seen = set(str(get(c.shape)) for c in have)
        missing = [v for v in values if str(v) not in seen]
        assert not missing, "%s: no case with %s in %s" % (op, param, missing)


def test_seam_lists_are_the_ones_of_the_launch_geometry():
    S = T.SEAMS
    for op in ('mul', 'act', 'gelu', 'gate_apply'):
        assert set(S[op]['n']) >= {1, 255, 256, 257, 513}
    assert set(S['gru_cell']['n']) >= {1, 256, 258, 259}
    for op, w in (('add_bcast_mid_act', 'H'), ('addattn_score', 'H'), ('l2norm_mid', 'D'), ('relu_maxpool', 'C'), ('mean_mid', 'F'),
                  ('group_max', 'Nc')):
        assert set(S[op][w]) >= {1, 255, 256, 257, 513}
        mid = [k for k in S[op] if k not in (w, 'B', 'Ni', 'kind', 'rows')]
        assert len(mid) == 1 and set(S[op][mid[0]]) == {1, 2, 37}
        assert set(S[op]['Ni' if op == 'group_max' else 'B']) == {1, 3}
    for op in ('add_layernorm', 'addattn_score'):
        assert set(S[op]['rows']) >= {1, 3, 4, 5} and set(S[op]['H']) >= {1, 63, 64, 65, 130, 257, 260}
    assert set(S['nll_logsoftmax']['V']) == {1, 63, 64, 65, 255, 256, 257, 513} and set(S['nll_logsoftmax']['B']) == {1, 7}
    assert set(zip(*[[c.shape[k] for c in T.cases('batch_norm_train')] for k in 'NC'])) >= \
        {(2, 1), (31, 64), (32, 65), (33, 63), (257, 65), (513, 3), (16385, 2)}
    assert set(tuple(c.shape[k] for k in 'BRKD') for c in T.cases('summarize')) >= \
        {(1, 1, 1, 1), (2, 36, 12, 257), (2, 37, 65, 64), (1, 96, 96, 70), (1, 192, 192, 8)}
    assert set(S['summarize']['D']) >= {1, 255, 256, 257, 513}
    assert set(c.extra for c in T.cases('mha')) >= {(1, 1, 1, 1), (2, 63, 3, 5), (1, 64, 2, 64), (3, 17, 1, 33)}
    for op in ('bmm_nn', 'bmm_nt'):
        assert set(tuple(c.shape[k] for k in ('batch', 'M', 'N', 'K')) for c in T.cases(op)) >= \
            {(1, 1, 1, 1), (3, 9, 11, 14), (2, 16, 17, 257), (1, 65, 65, 3)}
    assert set(S['l2norm_rows']['dim']) == {1, 63, 64, 65, 257, 1025}
    for op in ('transpose2d', 'colsum'):
        assert set(S[op]['cols']) == {1, 31, 32, 33, 63, 64, 65, 257} and set(S[op]['rows']) >= set(S[op]['cols'])
    assert 4097 in S['colsum']['rows'] and set(S['colsum']['acc']) == {0, 1}
    assert set(S['gather_rows']['E']) == {1, 127, 128, 129, 300}
    assert set(T.ADAM_SIZES) >= {1, 255, 256, 257, 1023, 1024, 1025, 65537, T.SQ_SUM_ELEMS_PER_BLOCK, T.SQ_SUM_ELEMS_PER_BLOCK + 1}
    assert T.ADAM_ONES == 40 and T.DROPOUT_N == (1, 255, 256, 257) and T.DROPOUT_P == (0.1, 0.5)


def test_batch_norm_cases_reach_the_row_slices():
    assert T.bn_slices(257, 65) == (2, [129, 128])
    assert T.bn_slices(513, 3) == (3, [171, 171, 171])
    s, rows = T.bn_slices(16385, 2)
    assert s == 64 and rows[-1] < rows[0] and rows[-1] > 0
    for n, c in ((2, 1), (31, 64), (32, 65), (33, 63)):
        assert T.bn_slices(n, c)[0] == 1
    # no N <= 20000 leaves a trailing slice empty, at any number of column blocks: nothing to add to the table for that
    for c in (1, 65, 64 * 16 + 1, 64 * 300):
        for n in range(1, 20001):
            assert T.bn_slices(n, c)[1][-1] > 0, (n, c)


def test_one_bmm_case_takes_a_second_grid_stride_pass():
    big = [c for c in T.cases('bmm_nt') if c.shape['M'] * c.shape['N'] > T.BMM_SMALL_MAX_GRID]
    assert big and all(c.shape['N'] > 64 for c in big)          # more than 64 output columns: the thread-per-output kernel


def test_decisive_inputs():
    for c in T.cases('nll_logsoftmax'):
        x = c.inputs()
        V = c.shape['V']
        assert int(x['logits'][0].argmax()) == V - 1
        assert int(x['target'][1 if c.shape['B'] > 1 else 0]) == V - 1
        if c.shape['B'] > 1:
            assert float(x['logits'][2].abs().min()) == 80.0 and (x['mask'] == 0).any()
    for c in T.cases('relu_maxpool'):
        x = c.inputs()['x']
        assert int(x[-1, :, -1].argmax()) == x.shape[1] - 1
        if c.shape['C'] > 1:
            assert float(x[:, :, 0].max()) < 0
    for c in T.cases('relu_maxpool', 'group_max'):
        t = c.inputs()['x' if c.op == 'relu_maxpool' else 'T']
        t = t.view(-1, c.extra, t.shape[-1]) if c.op == 'group_max' else torch.relu(t)
        top = t.topk(min(2, t.shape[1]), dim=1).values
        if top.shape[1] == 2:
            assert ((top[:, 0] > top[:, 1]) | (top[:, 0] == 0)).all(), c          # no ties in any maximum
    for c in T.cases('batch_norm_train'):
        x = c.inputs()['x']
        if x.shape[0] > 2:
            z = (x[-1] - x[:-1].mean(0)) / x[:-1].std(0)
            assert float((z - 3.0).abs().max()) < 1e-3
    for c in T.cases('mvm_scores'):                   # the arg-max view is the same in float32 and float64
        x = c.inputs()
        T32 = (x['img'].reshape(-1, T.MVM_D) @ x['cap'].t()).view(c.shape['Ni'], c.shape['k'], -1)
        T64 = (x['img'].double().reshape(-1, T.MVM_D) @ x['cap'].double().t()).view(c.shape['Ni'], c.shape['k'], -1)
        assert (T32.argmax(1) == T64.argmax(1)).all()
        top = T64.topk(2, dim=1).values
        assert float((top[:, 0] - top[:, 1]).min()) > 1e-4
    masks = [c.inputs()['mask'] for c in T.cases('mha') if c.shape['mask']]
    assert any((m.sum(1) == 1).any() and (m[:, 0] == 1).all() for m in masks if m.shape[1] > 1)
    for c in T.cases('gather_rows'):
        idx = c.inputs()['idx']
        assert idx.numel() == 513 and int(idx.min()) >= 0 and int(idx.max()) < T.GATHER_ROWS
        assert int(torch.bincount(idx).max()) >= 400


def test_adam_problem_clips_the_first_step_only():
    params, grads = T.adam_problem()
    sizes = [p.numel() for p in params]
    assert sorted(set(sizes)) == sorted(set(T.ADAM_SIZES) | {33}) and sizes.count(1) == T.ADAM_ONES + 1
    none = [i for i, g in enumerate(grads[0]) if g is None]
    assert len(none) == 1 and 0 < none[0] < len(sizes) - 1
    for step, gs in enumerate(grads):
        have = [g for g in gs if g is not None]
        assert all(float(g.abs().min()) >= 0.01 for g in have)
        norm = float(torch.sqrt(sum((g.double() ** 2).sum() for g in have)))
        assert (norm > 10 * T.ADAM_MAX_NORM) if step == 0 else (norm < 0.9 * T.ADAM_MAX_NORM), (step, norm)
    w64, w32, bad = T.adam_reference(torch.float64), T.adam_reference(torch.float32), T.adam_reference(torch.float64, drop_last=True)
    for s in range(T.ADAM_STEPS):
        e32, tol = T.tolerance(w64[s][3], w32[s][3])
        assert float((bad[s][3] - w64[s][3]).abs()) >= T.SENSITIVITY * tol, (s, e32, tol)


def test_adam_bounds_see_a_skipped_last_element():
    """An update that skips the last element of a tensor (the last thread of its last block) moves the parameter and both moments of
    that tensor by at least 10 x the bound the GPU test applies to it -- tensor by tensor, in every step the tensor has a gradient."""
    _, grads = T.adam_problem()
    w64, w32, bad = T.adam_reference(torch.float64), T.adam_reference(torch.float32), T.adam_reference(torch.float64, skip_last=True)
    checked = 0
    for s in range(T.ADAM_STEPS):
        for kind in range(3):
            for i, g in enumerate(grads[s]):
                if g is None:
                    continue
                want = w64[s][kind][i]
                e32, tol = T.tolerance(want, w32[s][kind][i])
                moved = float((bad[s][kind][i] - want).abs().max())
                assert moved >= T.SENSITIVITY * tol, (s, kind, i, want.numel(), moved, tol)
                checked += 1
    assert checked == 3 * (50 + 49 + 49)
