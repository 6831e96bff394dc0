"""GPU: the fp32 GEMM family (csrc/gemm_f32.hip, gemm_stream.hip, gemm_skinny.hip, gemm_tn.hip) at every case of
tests/helpers/gemm_cases.py against the float64 reference of the same operation -- the WHOLE output, not sampled rows.

Every output (and every workspace) is NaN-filled before the call: an element the kernel leaves unwritten fails the comparison, and
the guard columns behind a wider leading dimension must still be NaN afterwards.  Tolerance per compared tensor: the primary rule
16 * max(e32, u max|want|), or, for the cases the table names in FALLBACK, the a-priori bound (K + 2) u (|A| |B|^T + |bias| + |C0|)
elementwise (tests/helpers/gemm_cases.py; tests/test_gemm_case_table.py proves on the CPU that either sees a dropped last k).
Bit-exact checks of what the code claims: tile == stream_plain == stream_xcd on every streaming case, the same bits on a second call
of every sliced route, a row's bits independent of the number of rows in the call, residual == accumulate on a copy.
The calls go to the C entry points that ops.linear / linear_strided / gemm_acc / gemm_residual / mvm_scores and autograd._gemm_tn / _bmm
forward to (itr_gemm_nt[_algo|_acc|_residual|_splitk], itr_mvm_scores, itr_gemm_tn[_batched]): the wrappers allocate their own outputs
and take no offset base, and the sweep needs NaN-filled wider outputs; the identity checks at the end go through the wrappers.
profiles/gemm_seams/measured.txt is the record of one run (ITR_GEMM_SEAMS_RECORD=<file> appends one line per case and tensor)."""
import ctypes as C
import os
import sys

import pytest
import torch

from itr_amd import _lib, ops

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import gemm_cases as G        # noqa: E402

pytestmark = pytest.mark.gpu
NAN = float('nan')
RECORD = os.environ.get("ITR_GEMM_SEAMS_RECORD")


def _p(t, off=0):
    return C.c_void_p(t.data_ptr() + 4 * off) if t is not None and t.numel() else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _nan(dev, *shape):
    return torch.full(shape, NAN, device=dev, dtype=torch.float32)


def _ws(dev, nbytes):
    """A workspace whose every float is NaN: a partial product that is not written shows in the sum."""
    return torch.full((max(int(nbytes), 4),), 255, device=dev, dtype=torch.uint8)


def _dummy(dev):
    return torch.zeros(4, device=dev)


def run(case, x, dev, algo=None):
    """-> {tensor: (valid region, guard region or None)} of one call of the case's entry point on freshly NaN-filled outputs."""
    lib = _lib.load()
    s = case.shape
    if case.kind == 'nt':
        M, N, K, lda, ldc = s['M'], s['N'], s['K'], s['lda'], s['ldc']
        a, b = x['abuf'].to(dev), (x['B'].to(dev) if K else _dummy(dev))
        bias = x['bias'].to(dev) if 'bias' in x else None
        out = _nan(dev, M, ldc)
        Ap, Bp, bp = _p(a, s['a_off']), C.c_void_p(b.data_ptr()), _p(bias)
        if case.entry == 'algo':
            _lib.check(lib.itr_gemm_nt_algo(Ap, lda, Bp, K, bp, _p(out), ldc, M, N, K, s['act'], G.ALGOS[algo or s['algo']], _stream()))
        elif case.entry == 'nt':
            _lib.check(lib.itr_gemm_nt(Ap, lda, Bp, K, bp, _p(out), ldc, M, N, K, s['act'], _stream()))
        elif case.entry == 'acc':
            out[:, :N] = x['C0'].to(dev)
            _lib.check(lib.itr_gemm_nt_acc(Ap, lda, Bp, K, bp, _p(out), ldc, M, N, K, s['act'], _stream()))
        elif case.entry == 'residual':
            r = _nan(dev, M, s['ldr'])
            r[:, :N] = x['C0'].to(dev)
            _lib.check(lib.itr_gemm_nt_residual(Ap, lda, Bp, K, bp, _p(r), s['ldr'], _p(out), ldc, M, N, K, s['act'], _stream()))
        else:
            wsb = lib.itr_gemm_nt_splitk_workspace_bytes(M, N, K)
            ws = _ws(dev, wsb)
            _lib.check(lib.itr_gemm_nt_splitk(Ap, lda, Bp, K, bp, _p(out), ldc, M, N, K, s['act'], _p(ws), wsb, _stream()))
        return {'C': (out[:, :N], out[:, N:])}
    if case.kind == 'groupmax':
        img, cap = x['img'].to(dev), x['cap'].to(dev)
        out = _nan(dev, s['Ni'], s['ldc'])
        _lib.check(lib.itr_mvm_scores(_p(img), _p(cap), _p(out), s['Ni'], s['Nc'], s['k'], s['D'], s['ldc'], _stream()))
        return {'C': (out[:, :s['Nc']], out[:, s['Nc']:])}
    if case.kind == 'tn':
        R, P, Q = s['R'], s['P'], s['Q']
        a, b = x['A'].to(dev), x['B'].to(dev)
        out = _nan(dev, P, s['ldc'])
        if s['acc']:
            out[:, :Q] = x['C0'].to(dev)
        cs = _nan(dev, P + 3) if s['colsum'] else None
        wsb = lib.itr_gemm_tn_workspace_bytes(R, P, Q)
        ws = _ws(dev, wsb)
        _lib.check(lib.itr_gemm_tn(_p(a, s['a_off']), s['lda'], _p(b, s['b_off']), s['ldb'], _p(out), s['ldc'], R, P, Q, s['acc'], _p(cs),
                                   _p(ws), wsb, _stream()))
        res = {'C': (out[:, :Q], out[:, Q:])}
        if cs is not None:
            res['colsum'] = (cs[:P], cs[P:])
        return res
    Bn, R, P, Q = s['batch'], s['R'], s['P'], s['Q']
    a, b = x['A'].to(dev), x['B'].to(dev)
    out = _nan(dev, Bn, P * Q + 3)
    _lib.check(lib.itr_gemm_tn_batched(_p(a), P, s['batch_a'], _p(b), Q, s['batch_b'], _p(out), Q, P * Q + 3, R, P, Q, Bn, _stream()))
    return {'C': (out[:, :P * Q].reshape(Bn, P, Q), out[:, P * Q:])}


def _ratio(err, tol):
    """max err / tol with 0 / 0 = 0 and a NaN (an unwritten or poisoned element) = inf."""
    r = torch.where(err == 0, torch.zeros_like(err), err / tol)
    r = torch.where(torch.isnan(r), torch.full_like(r, float('inf')), r)
    return float(r.max()) if r.numel() else 0.0


def sweep(cases, dev, repeat=False, algos=None):
    """Runs the cases; -> the list of failures.  repeat: a second call must give the same bits; algos: every algo of the list is
    run, the first is compared with the reference and the others with the first, bit for bit."""
    bad, lines = [], []
    for c in cases:
        x = c.inputs()
        ref = c.reference(x)
        got = run(c, x, dev, algos[0] if algos else None)
        bits = []
        if repeat:
            again = run(c, x, dev)
            bits.append(('repeat', all(torch.equal(got[k][0], again[k][0]) for k in got)))
        for other in (algos or ())[1:]:
            o = run(c, x, dev, other)
            bits.append(('%s==%s' % (algos[0], other), torch.equal(got['C'][0], o['C'][0]) and bool(torch.isnan(o['C'][1]).all())))
        bound = c.fallback(x) if c.rule == 'fallback' else None
        for name, (want, e32, tol) in ref.items():
            val, guard = got[name]
            err = (val.double() - want.to(dev)).abs()
            worst = float(torch.nan_to_num(err, nan=float('inf')).max()) if err.numel() else 0.0
            ratio = _ratio(err, tol if bound is None else bound[name].to(dev))
            guards = guard is None or bool(torch.isnan(guard).all())
            note = ""
            if bound is None and ratio > 1.0:           # for the record: what the a-priori bound would say
                note = " (fallback ratio %.3g)" % _ratio(err, c.fallback(x)[name].to(dev))
            lines.append("%-14s %-16s %s %s: max err %.3e tol %.3e rule %s ratio %.3f guards %s%s%s" % (
                c.group, c.route, c.name, name, worst, tol if bound is None else float(bound[name].max()), c.rule, ratio,
                'nan' if guards else 'TOUCHED', "".join(" %s %s" % (k, 'equal' if v else 'DIFFERENT') for k, v in bits), note))
            if not (ratio <= 1.0 and guards and all(v for _, v in bits)):
                bad.append(lines[-1])
    if RECORD:
        with open(RECORD, "a") as f:
            f.write("\n".join(lines) + "\n")
    return bad


def _chunks(group, n):
    cs = G.cases(group)
    per = -(-len(cs) // n)
    return [pytest.param(cs[i * per:(i + 1) * per], id="%s%d" % (group, i)) for i in range(n)]


@pytest.mark.parametrize("cases", _chunks('tile_fast', 2) + _chunks('tile_aligned', 1) + _chunks('tile_scalar', 1) + _chunks('tile_count', 1) +
                         _chunks('epilogue', 1) + _chunks('strides', 1) + _chunks('groupmax', 2) + _chunks('skinny_direct', 1) +
                         _chunks('tn_batched', 1))
def test_single_pass_routes_vs_float64(dev, cases):
    bad = sweep(cases, dev)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("cases", _chunks('splitk', 1) + _chunks('skinny_sliced', 2) + _chunks('tn', 2))
def test_sliced_routes_vs_float64_and_repeatable(dev, cases):
    bad = sweep(cases, dev, repeat=True)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("tiles_n", G.STREAM_TN)
def test_streaming_vs_float64_and_bit_equal_to_the_tile_kernel(dev, tiles_n):
    """Both maps of the streaming kernel and the tile kernel, bit for bit (the gemm_stream.hip header's claim)."""
    cases = [c for c in G.cases('stream') if c.shape['N'] == tiles_n * 128]
    resident = 2 * torch.cuda.get_device_properties(dev).multi_processor_count
    for c in cases:         # the device admits what the table planned for
        s = c.shape
        assert G.stream_plan(s['M'], s['N'], s['K'], s['act'], s['lda'], s['K'], s['ldc'], 3, resident, s['a_off']), (c, resident)
    bad = sweep(cases, dev, algos=('stream_xcd', 'stream_plain', 'tile'))
    assert not bad, "\n".join(bad)


def _record(line):
    if RECORD:
        with open(RECORD, "a") as f:
            f.write(line + "\n")


@pytest.mark.parametrize("K,kernel", [(64, 'fast'), (36, 'aligned'), (37, 'scalar')])
def test_a_rows_bits_do_not_depend_on_the_row_count(dev, K, kernel):
    """The sharded evaluation's guarantee (gemm_nt_algo): linear(a)[:m] == linear(a[:m]) on the automatic route."""
    assert G.nt_kernel(300, 200, K, K, K) == kernel
    g = torch.Generator().manual_seed(K)
    a, w, b = (torch.randn(*s, generator=g).to(dev) for s in ((300, K), (200, K), (200,)))
    full = ops.linear(a, w, b, act='relu')
    for m in (1, 127, 128, 129):
        same = torch.equal(full[:m], ops.linear(a[:m], w, b, act='relu'))
        _record("row_count      %-16s K%d m%d: %s" % (kernel, K, m, 'equal' if same else 'DIFFERENT'))
        assert same, (kernel, m)


def test_a_rows_bits_do_not_depend_on_the_row_count_streaming(dev):
    """The same across the streaming kernel's admission: M rows on the automatic route stream (two rounds of the resident
    workgroups), fewer rows run on the tile kernel."""
    resident = 2 * torch.cuda.get_device_properties(dev).multi_processor_count
    N, K = 1024, 128
    Ms = 2 * resident // (N // 128) * 128
    assert G.nt_algo_route(Ms, N, K, 0, K, K, N, 0, resident).startswith('stream') and G.nt_algo_route(Ms - 128, N, K, 0, K, K, N, 0, resident) == 'fast'
    g = torch.Generator().manual_seed(5)
    a, w, b = (torch.randn(*s, generator=g).to(dev) for s in ((Ms + 129, K), (N, K), (N,)))
    full = ops.linear(a, w, b)
    assert bool(torch.isfinite(full).all())
    for m in (1, 127, 128, 129, Ms - 128, Ms, Ms + 128):
        same = torch.equal(full[:m], ops.linear(a[:m], w, b))
        _record("row_count      %-16s K%d m%d of %d: %s" % (G.nt_algo_route(m, N, K, 0, K, K, N, 0, resident), K, m, Ms + 129, 'equal' if same else 'DIFFERENT'))
        assert same, m


@pytest.mark.parametrize("K", [64, 36, 37])
def test_residual_equals_accumulate_on_a_copy(dev, K):
    g = torch.Generator().manual_seed(K)
    a, w, b, r = (torch.randn(*s, generator=g).to(dev) for s in ((129, K), (130, K), (130,), (129, 130)))
    for act in (None, 'relu', 'tanh'):
        res = ops.gemm_residual(a, w, b, r, act=act)
        acc = ops.gemm_acc(a, K, 129, K, w, b, r.clone(), act=act)
        same = torch.equal(res, acc)
        _record("residual==acc  %-16s K%d act %s: %s" % (G.nt_kernel(129, 130, K, K, K), K, act, 'equal' if same else 'DIFFERENT'))
        assert same and bool(torch.isfinite(res).all()), (K, act)
