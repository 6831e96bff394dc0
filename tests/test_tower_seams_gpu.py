"""GPU: the glue kernels of the evaluation towers (csrc/transformer.hip, agsa_gate.hip, eltwise.hip, vsrn.hip, norm.hip through
itr_amd/ops.py) at every case of tests/helpers/tower_cases.py against the float64 reference.

Per case the WHOLE output is compared under 16 * max(e32, 2^-24 max|want|) (tests/helpers/tower_cases.py; tests/test_tower_case_table.py
proves on the CPU that the bound is at most 2^-12 of the tensor's largest value and that it sees every named defect at 10 x), every
compared value must be finite where the reference is, every guard element of a NaN-filled buffer wider than the result must still be NaN,
the library must be on the route the table lists (attention and norms: recomputed from the real pointers and strides), and a second
call on fresh tensors must give the same bits (none of these kernels has an atomic).  For attention, LayerNorm and the norms the bits of
one sequence or row run alone must equal its bits inside the batch: a wave's work does not depend on its neighbours, and an index mix-up
that a tolerance forgives shows here.  profiles/tower_seams/measured.txt is the record of one run (ITR_TOWER_SEAMS_RECORD=<file> appends
one line per case)."""
import os
import sys

import pytest
import torch

from itr_amd import _lib, ops

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import tower_cases as T        # noqa: E402

pytestmark = pytest.mark.gpu
RECORD = os.environ.get("ITR_TOWER_SEAMS_RECORD")
NAN = float('nan')


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _off(t):
    """Floats between the tensor's first element and the 16-byte boundary below it."""
    return (t.data_ptr() % 16) // 4


def _all_nan(t):
    return bool(torch.isnan(t).all())


# ---------------------------------------------------------------------------------------------------------------------
# one call of the case on fresh device tensors -> ({tensor: value}, [failure]); `only`: one sequence or row of the case alone
def run_attention(c, dev, only=None):
    e, x = c.extra, c.inputs()
    B, L, heads, dk = e['B'], e['L'], e['heads'], e['dk']
    A = heads * dk
    sel = slice(0, B * L) if only is None else slice(only * L, (only + 1) * L)
    mask = x.get('mask')
    if only is not None:
        B, mask = 1, None if mask is None else mask[only:only + 1]
    rows = B * L
    bufs, where = T.mha_placement(e['layout'], e['out'], A)
    flat, view = {}, {}
    for name, (lead, ld) in bufs.items():
        flat[name] = torch.full((lead + rows * ld + 4,), NAN, device=dev)
        view[name] = flat[name][lead:lead + rows * ld].view(rows, ld)
    t = {}
    for n in 'qkv':
        t[n] = view[where[n][0]][:, where[n][1]:where[n][1] + A]
        t[n].copy_(x[n][sel].to(dev))
    out = view['out'][:, where['out'][1]:where['out'][1] + A] if 'out' in where else None
    y = ops.mha_small(t['q'], t['k'], t['v'], None if mask is None else mask.to(dev), B, L, heads, dk, dk ** -0.5, out=out)
    fails = []
    route = T.mha_route(_off(t['q']), _off(t['k']), _off(t['v']), t['q'].stride(0), t['k'].stride(0), t['v'].stride(0), _off(y), y.stride(0), L)
    if route != c.route:
        fails.append("the pointers and strides give route %s, the table says %s" % (route, c.route))
    if out is not None:
        guard = torch.ones_like(flat['out'], dtype=torch.bool)
        guard[:rows * bufs['out'][1]].view(rows, -1)[:, where['out'][1]:where['out'][1] + A] = False
        if y.data_ptr() != out.data_ptr() or not _all_nan(flat['out'][guard]):
            fails.append("a guard element of the output buffer was written")
    return {'out': y}, fails


def run_add_layernorm(c, dev, only=None):
    x = c.inputs()
    sel = slice(None) if only is None else slice(only, only + 1)
    res = x['res'][sel].to(dev) if 'res' in x else None
    return {'y': ops.add_layernorm(x['x'][sel].to(dev), res, x['gamma'].to(dev), x['beta'].to(dev))}, []


def run_bert_embed_ln(c, dev, only=None):
    x = c.inputs()
    sel = slice(None) if only is None else slice(only, only + 1)
    ty = x['type_ids'][sel].to(dev) if 'type_ids' in x else None
    return {'y': ops.bert_embed_ln(x['ids'][sel].to(dev), ty, x['word'].to(dev), x['pos'].to(dev), x['type'].to(dev), x['gamma'].to(dev),
                                   x['beta'].to(dev))}, []


def run_relu_maxpool(c, dev):
    x = c.inputs()['x']
    B, _, Cc = x.shape
    buf = torch.full((B, Cc + 2), NAN, device=dev)
    y = ops.relu_maxpool(x.to(dev), c.extra['valid'], out=buf[:, 1:1 + Cc])
    ok = y.data_ptr() == buf[:, 1:].data_ptr() and _all_nan(buf[:, 0]) and _all_nan(buf[:, Cc + 1])
    return {'y': y}, [] if ok else ["a guard column of the output buffer was written"]


def run_mean_mid(c, dev):
    return {'y': ops.mean_mid(c.inputs()['x'].to(dev))}, []


def run_agsa_gate(c, dev):
    x = {k: v.to(dev) for k, v in c.inputs().items()}
    qo, ko = ops.agsa_gate(x['q'], x['k'], (x['Wq'], x['bq']), (x['Wk'], x['bk']), (x['Wg'], x['bg']))
    return {'qo': qo, 'ko': ko}, []


def run_gcn_relation(c, dev):
    e, tpg = c.extra, c.inputs()['tpg']
    n_img, N, D, ld, ldy = e['n_img'], e['N'], e['D'], e['ld'], e['ldy']
    if ld == 3 * D:
        return {'y': ops.gcn_relation(tpg.to(dev), n_img, N, D)}, []
    tbuf, ybuf = torch.full((n_img * N, ld), NAN, device=dev), torch.full((n_img * N, ldy), NAN, device=dev)
    tbuf[:, :3 * D] = tpg.to(dev)
    _lib.check(_lib.load().itr_gcn_relation(ops._p(tbuf), ld, ops._p(ybuf), ldy, n_img, N, D, ops._stream()))
    return {'y': ybuf[:, :D]}, [] if _all_nan(ybuf[:, D:]) else ["a guard column of the output buffer was written"]


def run_camera_summarize(c, dev):
    x = c.inputs()
    return {'out': ops.camera_summarize(x['smry'].to(dev), x['X'].to(dev))}, []


def run_camera_posenc(c, dev):
    x = c.inputs()
    return {'out': ops.camera_posenc(x['boxes'].to(dev), x['wh'].to(dev))}, []


def run_affine_cols(c, dev):
    x = {k: v.to(dev) for k, v in c.inputs().items()}
    return {'y': ops.affine_cols(x['x'], x.get('scale'), x.get('shift'), x.get('res'), c.extra['act'])}, []


def run_mul_rows(c, dev):
    x = c.inputs()
    Cc = x['a'].shape[1]
    return {'y': ops.mul_rows(x['a'].to(dev), x['bbuf'].to(dev)[:, T.MULROWS_COL:T.MULROWS_COL + Cc])}, []


def run_norm(c, dev, only=None):
    e, x = c.extra, c.inputs()['x']
    if only is not None:
        x = x[only:only + 1]
    rows, dim = x.shape
    fails = []
    if not e['lead']:
        xd = x.to(dev)
        y = ops._norm(xd, -1, T.NORM_EPS[e['kind']], e['kind'], bool(e['abs']))
        route = T.norm_route(dim, _off(xd) == 0 and _off(y) == 0)
    else:
        xbuf, ybuf = torch.full((e['lead'] + rows * dim + 3,), NAN, device=dev), torch.full((rows * dim + 4,), NAN, device=dev)
        xv = xbuf[e['lead']:e['lead'] + rows * dim]
        xv.copy_(x.reshape(-1).to(dev))
        _lib.check(_lib.load().itr_l2norm_rows(ops._p(xv), ops._p(ybuf), rows, dim, T.NORM_EPS[e['kind']], e['kind'], e['abs'], ops._stream()))
        y = ybuf[:rows * dim].view(rows, dim)
        route = T.norm_route(dim, _off(xv) == 0 and _off(ybuf) == 0)
        if not _all_nan(ybuf[rows * dim:]):
            fails.append("a guard element of the output buffer was written")
    if route != c.route:
        fails.append("the pointers give route %s, the table says %s" % (route, c.route))
    if only is None and rows > T.ZERO_ROW and e['kind'] != 3 and not bool((y[T.ZERO_ROW] == 0).all()):
        fails.append("the all-zero row does not give exact zeros")
    return {'y': y}, fails


RUN = {'attention': run_attention, 'add_layernorm': run_add_layernorm, 'bert_embed_ln': run_bert_embed_ln, 'relu_maxpool': run_relu_maxpool,
       'mean_mid': run_mean_mid, 'agsa_gate': run_agsa_gate, 'gcn_relation': run_gcn_relation, 'camera_summarize': run_camera_summarize,
       'camera_posenc': run_camera_posenc, 'affine_cols': run_affine_cols, 'mul_rows': run_mul_rows, 'norm': run_norm}


def _alone(c):
    """[(index run alone, {tensor: (first row, rows)} of the batch result it must reproduce)] for the families that have the check."""
    if c.family == 'attention':
        L = c.extra['L']
        return [(b, {'out': (b * L, L)}) for b in range(c.extra['B'])] if c.extra['B'] > 1 else []
    if c.family == 'add_layernorm':
        return [(r, {'y': (r, 1)}) for r in range(c.shape['rows'])] if c.shape['rows'] > 1 else []
    if c.family == 'bert_embed_ln':
        return [(b, {'y': (b, 1)}) for b in range(c.shape['B'])] if c.shape['B'] > 1 else []
    if c.family == 'norm' and not c.extra['lead']:
        return [(r, {'y': (r, 1)}) for r in range(c.shape['rows'])] if c.shape['rows'] > 1 else []
    return []


def sweep(c, dev):
    ref = c.reference()
    run = RUN[c.family]
    got, fails = run(c, dev)
    again, _ = run(c, dev)
    assert set(got) == set(ref), c
    ratios = {}
    for name, val in got.items():
        want, e32, tol, rule = ref[name]
        if tuple(val.shape) != tuple(want.shape):
            fails.append("%s has shape %s, not %s" % (name, tuple(val.shape), tuple(want.shape)))
            continue
        host = val.detach().cpu()
        if not bool((torch.isfinite(host) | torch.isnan(want)).all()):
            fails.append("%s is not finite where the reference is" % name)
        err = T.max_err(host, want)
        ratios[name] = err / tol
        print("%s %s: max err %.3e e32 %.3e tol %.3e ratio %.3f" % (c.name, name, err, e32, tol, ratios[name]))
        if not err <= tol:
            fails.append("%s: max err %.3e is %.3f x tol %.3e" % (name, err, ratios[name], tol))
        if not _bits_equal(val, again[name]):
            fails.append("%s: a second run gives other bits" % name)
    alone_ok = None
    for index, parts in _alone(c):
        one, _ = run(c, dev, only=index)
        for name, (r0, n) in parts.items():
            alone_ok = alone_ok is not False and _bits_equal(got[name][r0:r0 + n], one[name].reshape(got[name][r0:r0 + n].shape))
            if not alone_ok:
                fails.append("%s: row / sequence %d run alone gives other bits than inside the batch" % (name, index))
    if RECORD:
        cols = " ".join("%s: e32 %.3e tol %.3e ratio %.3f" % (k, ref[k][1], ref[k][2], r) for k, r in ratios.items())
        tail = "repeat %s" % ('DIFFERENT' if any('other bits' in m and 'alone' not in m for m in fails) else 'equal')
        if alone_ok is not None:
            tail += " alone %s" % ('equal' if alone_ok else 'DIFFERENT')
        with open(RECORD, "a") as f:
            f.write("%s %s route %s %s | %s | %s\n" % (c.family, c.name, c.route if c.route is not None else '-',
                                                       'fallback' if c.name in T.FALLBACK else 'primary', cols, tail))
    assert not fails, "%s: %s" % (c.name, "; ".join(fails))


def _param(*families):
    return pytest.mark.parametrize("case", T.cases(*families), ids=lambda c: c.name)


@_param('attention')
def test_attention_seams_vs_float64(dev, case):
    sweep(case, dev)


@_param('add_layernorm', 'bert_embed_ln')
def test_layernorm_seams_vs_float64(dev, case):
    sweep(case, dev)


@_param('relu_maxpool')
def test_relu_maxpool_seams_vs_float64(dev, case):
    sweep(case, dev)


@_param('mean_mid')
def test_mean_mid_seams_vs_float64(dev, case):
    sweep(case, dev)


@_param('agsa_gate')
def test_agsa_gate_seams_vs_float64(dev, case):
    sweep(case, dev)


@_param('gcn_relation')
def test_gcn_relation_seams_vs_float64(dev, case):
    sweep(case, dev)


@_param('camera_summarize', 'camera_posenc')
def test_camera_summary_and_posenc_seams_vs_float64(dev, case):
    sweep(case, dev)


@_param('affine_cols', 'mul_rows')
def test_eltwise_seams_vs_float64(dev, case):
    sweep(case, dev)


@_param('norm')
def test_norm_seams_vs_float64(dev, case):
    sweep(case, dev)


def _refuse(what, dev):
    r = lambda *s: torch.randn(*s, device=dev)        # noqa: E731
    if what == 'mha L=65':
        return ops.mha_small(r(65, 16), r(65, 16), r(65, 16), None, 1, 65, 1, 16, 0.25)
    if what == 'mha dk=8':
        return ops.mha_small(r(4, 8), r(4, 8), r(4, 8), None, 1, 4, 1, 8, 0.35)
    if what == 'layernorm H=4100':
        return ops.add_layernorm(r(2, 4100), None, r(4100), r(4100))
    if what == 'agsa dk=64':
        return ops.agsa_gate(r(4, 64), r(4, 64), (r(64, 64), r(64)), (r(64, 64), r(64)), (r(128, 64), r(128)))
    if what == 'gcn N=37':
        return ops.gcn_relation(r(37, 12), 1, 37, 4)
    if what == 'summarize R=65':
        return ops.camera_summarize(r(1, 65, 2), r(1, 65, 8))
    raise KeyError(what)


@pytest.mark.parametrize("what", T.REFUSALS)
def test_sizes_outside_the_kernels_are_refused(dev, what):
    with pytest.raises((NotImplementedError, RuntimeError)):
        _refuse(what, dev)
