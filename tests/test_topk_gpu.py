"""GPU: top-K retrieval lists (csrc/topk.hip; ops.topk_lists / topk_merge_cols, evaluation.topk, the evalrank_* `topk`
keyword) against the numpy oracle np.argsort(canon(x), kind='stable')[::-1][:K] (tests/helpers/topk_oracle.py):
indices and score bits exactly equal."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import rank_matrices as RM        # noqa: E402
import topk_oracle as T           # noqa: E402

from itr_amd import ops                          # noqa: E402
from itr_amd.metricmodule import evaluation      # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _check_rows(S_dev, S_host, k):
    ri, rv, _ = ops.topk_lists(S_dev, k, cols=False)
    wi, wv = T.topk_rows(S_host, k)
    assert (ri.cpu().numpy() == wi).all()
    assert (_bits(rv.cpu().numpy()) == _bits(wv)).all()


def _check_cols(S_dev, S_host, k):
    _, _, part = ops.topk_lists(S_dev, k, rows=False)
    ci, cv = ops.topk_merge_cols([part], k)
    wi, wv = T.topk_cols(S_host, k)
    assert (ci.cpu().numpy() == wi).all()
    assert (_bits(cv.cpu().numpy()) == _bits(wv)).all()


def _check_both(S_dev, S_host, k):
    ri, rv, part = ops.topk_lists(S_dev, k)
    ci, cv = ops.topk_merge_cols([part], k)
    want = T.topk_all(S_host, k)
    assert (ri.cpu().numpy() == want['i2t_topk']).all() and (ci.cpu().numpy() == want['t2i_topk']).all()
    assert (_bits(rv.cpu().numpy()) == _bits(want['i2t_topk_scores'])).all()
    assert (_bits(cv.cpu().numpy()) == _bits(want['t2i_topk_scores'])).all()


def test_topk_shapes_strides_alignment(dev):
    rng = np.random.RandomState(0)
    one = np.array([[-0.0]], np.float32)
    _check_both(torch.from_numpy(one).to(dev), one, 1)
    s = rng.randn(7, 35).astype(np.float32)
    _check_rows(torch.from_numpy(s).to(dev), s, 35)             # K = the row's length
    _check_cols(torch.from_numpy(s).to(dev), s, 7)              # K = the column's length
    for k in (1, 10, 100, 128):
        s = rng.randn(37, 1001).astype(np.float32)              # Nc not a multiple of 4
        _check_rows(torch.from_numpy(s).to(dev), s, k)
        _check_cols(torch.from_numpy(s).to(dev), s, min(k, 37))
    for width in (1100, 1101):                                  # strided views: ldS % 4 == 0 and not
        big = rng.randn(40, width).astype(np.float32)
        v = torch.from_numpy(big).to(dev)[:, :1001]
        assert v.stride(0) == width
        _check_both(v, big[:, :1001], 10)
    flat = torch.from_numpy(rng.randn(40 * 1004 + 1).astype(np.float32)).to(dev)
    mis = flat[1:].view(40, 1004)                               # storage offset of 4 bytes: not 16-byte aligned
    assert mis.data_ptr() % 16 != 0
    _check_both(mis, mis.cpu().numpy(), 10)


def _special_rows(n, rng):
    rows = [np.arange(n, dtype=np.float32),                                         # ascending: every element beats the threshold
            np.arange(n, dtype=np.float32)[::-1].copy(),                            # descending
            np.full(n, 0.25, np.float32),                                           # all equal
            np.full(n, np.nan, np.float32),                                         # all NaN
            rng.choice(np.array([np.inf, -np.inf, np.nan, 1.0, -1.0], np.float32), n),
            rng.choice(np.array([0.0, -0.0], np.float32), n),
            (rng.randint(-3, 4, n) * np.float32(1e-45)).astype(np.float32),         # subnormals (and zeros of both signs)
            rng.randint(0, 3, n).astype(np.float32),                                # many exact ties
            rng.randn(n).astype(np.float32)]
    return np.stack(rows)


def test_topk_special_values_both_directions(dev):
    rng = np.random.RandomState(1)
    for n in (2100, 5000):                                       # several chunks (threshold merges) per row
        s = _special_rows(n, rng)
        for k in (1, 9, 100, 128):
            _check_rows(torch.from_numpy(s).to(dev), s, k)
            st = np.ascontiguousarray(s.T)                       # the same lines as columns
            _check_cols(torch.from_numpy(st).to(dev), st, k)
        _check_cols(torch.from_numpy(s).to(dev), s, 9)


def test_topk1_equals_rank_counts_top1(dev):
    for name, make in RM.CASES.items():
        m = make()
        S64 = torch.from_numpy(m).to(dev)
        ri, _, part = ops.topk_lists(S64, 1)
        ci, _ = ops.topk_merge_cols([part], 1)
        _, i_top, _, t_top = ops.rank_counts_f64(S64, 5)
        assert (ri[:, 0] == i_top).all() and (ci[:, 0] == t_top).all(), name
        S32 = torch.from_numpy(m.astype(np.float32)).to(dev)
        ri, _, part = ops.topk_lists(S32, 1)
        ci, _ = ops.topk_merge_cols([part], 1)
        _, i_top, _, t_best, _ = ops.rank_counts(S32, 5)
        assert (ri[:, 0] == i_top).all() and (ci[:, 0].long() == (t_best & 0xffffffff)).all(), name


@pytest.mark.parametrize("k", [10, 100])
def test_topk_row_blocks_merge_to_the_whole_matrix(dev, k):
    rng = np.random.RandomState(2)
    s = rng.randn(300, 777).astype(np.float32)
    s[:, ::5] = np.round(s[:, ::5])                              # exact ties across blocks
    s[::7] = np.round(s[::7] * 2) / 2
    S = torch.from_numpy(s).to(dev)
    wi, wv, part = ops.topk_lists(S, k)
    whole = ops.topk_merge_cols([part], k)
    want = T.topk_all(s, k)
    assert (whole[0].cpu().numpy() == want['t2i_topk']).all()
    for cuts in ([300], [13, 287], [100, 50, 150], [1, 2, 3, 5, 8, 13, 21, 247]):
        bounds = np.concatenate([[0], np.cumsum(cuts)])
        parts, rows_i, rows_v = [], [], []
        for a, b in zip(bounds[:-1], bounds[1:]):
            ri, rv, p = ops.topk_lists(S[a:b], k, row0=int(a))
            parts.append(p)
            rows_i.append(ri)
            rows_v.append(rv)
        ci, cv = ops.topk_merge_cols(parts, k)
        assert torch.equal(ci, whole[0]) and torch.equal(cv.view(torch.int32), whole[1].view(torch.int32)), cuts
        assert torch.equal(torch.cat(rows_i), wi) and torch.equal(torch.cat(rows_v).view(torch.int32), wv.view(torch.int32))


def test_topk_float64(dev):
    m = RM.half_ulp_matrix()
    got = evaluation.topk(m, 10)
    want = T.topk_all(m, 10)
    for key in want:
        assert got[key].dtype == want[key].dtype and (got[key] == want[key]).all(), key
    # selecting in fp32 would not do: the neighbours 2m / 2m+1 of every row collapse there
    assert not (T.topk_rows(m.astype(np.float32), 10)[0] == want['i2t_topk']).all()
    m = RM.ensemble_sigmoid_matrix(35)
    got = evaluation.topk(torch.from_numpy(m), 25)
    want = T.topk_all(m, 25)
    for key in want:
        assert (got[key] == want[key]).all(), key
    # fp32 input is selected in fp32
    got32 = evaluation.topk(m.astype(np.float32), 5)
    assert got32['i2t_topk_scores'].dtype == np.float32
    assert (got32['t2i_topk'] == T.topk_cols(m.astype(np.float32), 5)[0]).all()


@pytest.mark.parametrize("k", [10, 100])
def test_topk_full_size(dev, k):
    rng = np.random.RandomState(7)
    s = rng.randn(5000, 25000).astype(np.float32)
    s[:, ::11] = np.round(s[:, ::11], 1)                         # ties
    S = torch.from_numpy(s).to(dev)
    ri, rv, part = ops.topk_lists(S, k)
    ci, cv = ops.topk_merge_cols([part], k)
    wri, wrv, wci, wcv = T.topk_exact_large(s, k)
    assert (ri.cpu().numpy() == wri).all() and (ci.cpu().numpy() == wci).all()
    assert (_bits(rv.cpu().numpy()) == _bits(wrv)).all() and (_bits(cv.cpu().numpy()) == _bits(wcv)).all()


def test_topk_family_agrees_at_power_of_two_seams(dev):
    """K = L and K = L +- 1 of the shared sorting network (csrc/select.h): the row, slab, column and fold kernels and the two
    re-sorts give one list per query, equal to the numpy order in indices and score bits."""
    rng = np.random.RandomState(11)
    q = rng.randn(5, 36).astype(np.float32)
    g = rng.randn(300, 36).astype(np.float32)
    g[10:20] = g[3]                                              # exact score ties
    queries, gallery = torch.from_numpy(q).to(dev), torch.from_numpy(g).to(dev)
    # the same values as column slices of 37-wide buffers: rows not 16-byte aligned, leading dimension % 4 != 0
    q_odd = torch.zeros(5, 37, device=dev)[:, 1:].copy_(queries)
    g_odd = torch.zeros(300, 37, device=dev)[:, 1:].copy_(gallery)
    assert g_odd.data_ptr() % 16 != 0 and g_odd.stride(0) == 37
    S = ops.cosine_scores(queries, gallery)
    S_host = S.cpu().numpy()
    St = S.t().contiguous()
    for k in (1, 2, 63, 64, 65, 127, 128):
        wi, wv = T.topk_rows(S_host, k)
        ri, rv, _ = ops.topk_lists(S, k, cols=False)
        got = {"rows": (ri, rv)}
        for n_slabs in (0, 1, 3):
            got["search %d" % n_slabs] = ops.search_topk(queries, gallery, k, n_slabs=n_slabs)[:2]
            got["search %d, unaligned" % n_slabs] = ops.search_topk(q_odd, g_odd, k, n_slabs=n_slabs)[:2]
        got["cols"] = ops.topk_merge_cols([ops.topk_lists(St, k, rows=False)[2]], k)
        lo_hi = ops.topk_fold_cols(St[170:], k, row0=170, state=ops.topk_fold_cols(St[:170], k, row0=0))
        hi_lo = ops.topk_fold_cols(St[:170], k, row0=0, state=ops.topk_fold_cols(St[170:], k, row0=170))
        got["fold"], got["fold, reversed"] = ops.topk_merge_cols([lo_hi], k), ops.topk_merge_cols([hi_lo], k)
        got["rerank"] = ops.rerank_lists(ri.flip(1).contiguous(), rv.flip(1).contiguous())[:2]
        fi, fused, fv, _ = ops.rerank_fused_lists(ri.flip(1).contiguous(), [rv.flip(1).contiguous()])
        got["rerank_fused"] = (fi, fv[0])
        assert (fused.cpu().numpy() == wv.astype(np.float64)).all(), k
        for name, (i, v) in got.items():
            assert i.shape == (5, k) and (i.cpu().numpy() == wi).all(), (name, k)
            assert (_bits(v.cpu().numpy()) == _bits(wv)).all(), (name, k)


# ---- end to end: evalrank_single / _ensemble / _fast with topk
def _toy_checkpoints(golden, tmp_path, seeds=(1, 2)):
    from test_evalrank_gpu import _materialise, _scan_cfg
    from itr_amd import utils
    from itr_amd.modalmodule import get_model
    g = golden("g14_data_layer")
    name, data_path, vdir = _materialise(g, tmp_path)
    paths = []
    for seed in seeds:
        save_dir = str(tmp_path / ('run%d' % seed))
        os.makedirs(save_dir)
        cfg = _scan_cfg(name, data_path, vdir, save_dir, seed)
        cfg['vocab_size'] = int(g["vocab_len"])
        torch.manual_seed(seed)
        model = get_model(cfg)
        utils.save_checkpoint({'epoch': 3, 'model': model.state_dict(), 'best_rsum': 12.5, 'best_r1': 1.5, '_config': cfg,
                               'Eiters': 77}, True, prefix=save_dir)
        paths.append(os.path.join(save_dir, 'model_best.pth.tar'))
    return name, paths


def test_evalrank_topk_npz(golden, dev, tmp_path, monkeypatch):
    import yaml
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    name, paths = _toy_checkpoints(golden, tmp_path)
    d0 = os.path.dirname(paths[0])
    yml = os.path.join(d0, '%s_single_result.yaml' % name)
    evaluation.evalrank_single(paths[0], split='test')
    plain = open(yml, 'rb').read()
    evaluation.evalrank_single(paths[0], split='test', topk=0)
    assert open(yml, 'rb').read() == plain
    assert not [f for f in os.listdir(d0) if f.endswith('.npz')]
    # topk = 5: the npz, against the oracle on the float64 matrix the ranks were computed from
    mats = []
    real = evaluation.cal_sims

    def spy(*a, **kw):
        mats.append(real(*a, **kw))
        return mats[-1]
    monkeypatch.setattr(evaluation, 'cal_sims', spy)
    res = evaluation.evalrank_single(paths[0], split='test', topk=5)
    assert open(yml, 'rb').read() == plain                        # the YAML does not change with the lists
    z = np.load(os.path.join(d0, '%s_single_top5.npz' % name))
    assert mats[0].dtype == np.float64
    want = T.topk_all(mats[0], 5)
    for key in want:
        assert z[key].dtype == want[key].dtype and (z[key] == want[key]).all(), key
    y = yaml.safe_load(open(yml))
    assert (z['i2t_topk'][:, 0] == np.asarray(y['i2t_top1'])).all() and (z['t2i_topk'][:, 0] == np.asarray(y['t2i_top1'])).all()
    assert (z['i2t_topk'][:, 0] == res['i2t_top1']).all()
    # ensemble: the lists of the float64 average
    mats.clear()
    res2 = evaluation.evalrank_ensemble(paths[0], paths[1], split='test', topk=5)
    z2 = np.load(os.path.join(d0, '%s_ensemble_top5.npz' % name))
    avg = (mats[0] + mats[1]) / 2
    want2 = T.topk_all(avg, 5)
    for key in want2:
        assert (z2[key] == want2[key]).all(), key
    assert (z2['t2i_topk'][:, 0] == res2['t2i_top1']).all()
    # fast path (fp32 matrix on the device): first column = its top1, lists = the oracle on ITS matrix
    monkeypatch.setattr(evaluation, 'cal_sims', real)
    fast_plain = evaluation.evalrank_fast(paths[0], split='test')
    yml_plain = open(yml, 'rb').read()
    fast = evaluation.evalrank_fast(paths[0], split='test', topk=5)
    assert open(yml, 'rb').read() == yml_plain
    zf = np.load(os.path.join(d0, '%s_single_top5.npz' % name))
    assert zf['i2t_topk_scores'].dtype == np.float32
    assert (zf['i2t_topk'][:, 0] == fast['i2t_top1']).all() and (zf['t2i_topk'][:, 0] == fast['t2i_top1']).all()
    assert (np.asarray(fast_plain['i2t_top1']) == fast['i2t_top1']).all()
    # the fp32 scores of the fast path agree with the reference-shaped path's float64 matrix to fp32 accuracy, same indices
    assert (zf['i2t_topk'] == want['i2t_topk']).all()
    np.testing.assert_allclose(zf['i2t_topk_scores'], want['i2t_topk_scores'], rtol=0, atol=1e-5)
    # 2 ranks over gloo, both on this GPU: the same npz
    single = {k: zf[k].copy() for k in zf.files}
    os.remove(os.path.join(d0, '%s_single_top5.npz' % name))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29641", os.path.join(ROOT, "tests", "helpers", "topk_fast_worker.py"), paths[0]]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    z2r = np.load(os.path.join(d0, '%s_single_top5.npz' % name))
    assert sorted(z2r.files) == sorted(single)
    for key in single:
        assert (_bits(z2r[key]) == _bits(single[key])).all() if z2r[key].dtype.kind == 'f' else (z2r[key] == single[key]).all(), key
