"""GPU: evalrank_rerank(..., explain_sgraf=M) and `python test.py COARSE FINE --rerank K --explain-sgraf M` on the toy precomp
dataset and tiny checkpoints of test_evalrank_rerank_gpu.py (VSE++ coarse, SGRAF SAF / SGR fine): the file holds the first M columns
of the reranked lists with what ops.sgraf_pair_attention gives for those pairs (bit for bit), its scores are the fine scores the
lists were ordered by, and its blocks are the restated oracle's (tests/helpers/sgraf_explain_oracle.py) within the bounds of
test_sgraf_attention_gpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import sgraf_explain_oracle as X                                                    # noqa: E402
from itr_amd import ops                                                              # noqa: E402
from itr_amd.metricmodule import evaluation                                         # noqa: E402
from test_evalrank_explain_gpu import _fine_operands                                # noqa: E402
from test_evalrank_rerank_gpu import K, N_IMG, _checkpoint, _dataset, _run          # noqa: E402

pytestmark = pytest.mark.gpu

M = 3
TOL_ATTN, TOL_SCORE = 2e-5, 5e-6
COMMON = ['idx', 'scores', 'attn', 'attn_ptr', 'cap_len', 'explained']


@pytest.mark.parametrize("mod", ['SAF', 'SGR'])
def test_explain_sgraf_file_and_command_line(golden, dev, tmp_path, mod):
    g = golden("g14_data_layer")
    name, data_path, vdir = _dataset(g, tmp_path)
    coarse = _checkpoint(g, tmp_path, 'coarse', 'VSE_PP', [], name, data_path, vdir, 3)
    fine = _checkpoint(g, tmp_path, 'fine', 'SGRAF', ['module_name=%s' % mod], name, data_path, vdir, 5)
    cdir = os.path.dirname(coarse)
    before = sorted(os.listdir(cdir))
    res = evaluation.evalrank_rerank(coarse, fine, K, split='test', explain_sgraf=M)
    path = os.path.join(cdir, '%s_rerank%d_explain%d_sgraf.npz' % (name, K, M))
    assert sorted(os.listdir(cdir)) == sorted(before + ['%s_rerank%d_result.yaml' % (name, K), '%s_rerank%d.npz' % (name, K), os.path.basename(path)])
    assert res['k'] == K
    lists = np.load(os.path.join(cdir, '%s_rerank%d.npz' % (name, K)))
    z = {k_: v for k_, v in np.load(path).items()}
    aux = ['node_w', 'node_ptr'] if mod == 'SAF' else ['edge', 'edge_ptr']
    assert sorted(z) == sorted(d + '_' + k_ for d in ('i2t', 't2i') for k_ in COMMON + aux)
    cfg, images, words, plan, img_h, cap_h, lens = _fine_operands(fine, dev)
    model, _ = evaluation._load_for_eval(fine, None)
    enc = model.sim_enc
    steps = int(enc.sgr_step)
    w_d = {k_: v.detach() for k_, v in enc.state_dict().items()}
    w_h = {k_: v.detach().cpu().float() for k_, v in w_d.items()}
    L = [int(x) for x in lens]
    S_ref, parts = X.sgraf_similarity_explained(w_h, img_h.float(), cap_h.float(), L, mod, steps)
    X.assert_restates_oracle(S_ref, w_h, img_h.float(), cap_h.float(), L, mod, steps)
    for d, n in (('i2t', N_IMG), ('t2i', 5 * N_IMG)):
        idx = z[d + '_idx']
        assert idx.shape == (n, M) and np.array_equal(idx, lists[d + '_topk'][:, :M])
        q = np.repeat(np.arange(n), M)
        pairs = np.stack([q, idx.reshape(-1)] if d == 'i2t' else [idx.reshape(-1), q], 1).astype(np.int32)
        got = ops.sgraf_pair_attention(images, words, plan, w_d, torch.from_numpy(pairs).to(dev), module_name=mod, sgr_step=steps)
        for k_, t in (('attn', got.attn), ('scores', got.score), (aux[0], got.node_w if mod == 'SAF' else got.edge)):
            assert np.array_equal(z[d + '_' + k_].reshape(-1).view(np.uint32), t.cpu().numpy().view(np.uint32)), (d, k_)
        assert np.array_equal(z[d + '_attn_ptr'], got.attn_ptr.cpu().numpy())
        assert np.array_equal(z[d + '_' + aux[1]], (got.node_ptr if mod == 'SAF' else got.edge_ptr).cpu().numpy())
        assert np.array_equal(z[d + '_cap_len'], lens[pairs[:, 1]]) and bool(z[d + '_explained'].all())
        # the fine scores the lists were ordered by (the score path's; the explaining kernel's own arithmetic: within the score bound)
        e = float(np.abs(z[d + '_scores'].astype(np.float64) - lists[d + '_topk_scores'][:, :M]).max())
        print("%s %s: explained scores vs reranked list scores: max|d| = %.3g" % (mod, d, e))
        assert e <= TOL_SCORE
        # every block against the restated oracle
        pl = [(int(i), int(c)) for i, c in pairs]
        e_attn = float(np.abs(z[d + '_attn'] - X.flat_blocks(parts, pl, 'attn')).max())
        want = X.flat_blocks(parts, pl, aux[0])
        assert want.shape == z[d + '_' + aux[0]].shape
        e_aux = float(np.abs(z[d + '_' + aux[0]] - want).max())
        e_sc = float(np.abs(z[d + '_scores'].reshape(-1) - S_ref.double().numpy()[pairs[:, 0], pairs[:, 1]]).max())
        print("%s %s vs oracle: max|d| attn %.3g, %s %.3g, score %.3g" % (mod, d, e_attn, aux[0], e_aux, e_sc))
        assert e_attn <= TOL_ATTN and e_aux <= TOL_ATTN and e_sc <= TOL_SCORE
    # the command line writes the same file
    os.remove(path)
    r = _run([coarse, fine, "--rerank", str(K), "--explain-sgraf", str(M), "--split", "test"])
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    z2 = np.load(path)
    assert sorted(z2.keys()) == sorted(z) and all(np.array_equal(z2[k_], z[k_]) for k_ in z)


def test_explain_sgraf_refusals(golden, dev, tmp_path):
    g = golden("g14_data_layer")
    name, data_path, vdir = _dataset(g, tmp_path)
    coarse = _checkpoint(g, tmp_path, 'coarse', 'VSE_PP', [], name, data_path, vdir, 3)
    scan = _checkpoint(g, tmp_path, 'scan', 'SCAN', [], name, data_path, vdir, 4)
    sgraf = _checkpoint(g, tmp_path, 'sgraf', 'SGRAF', ['module_name=SAF'], name, data_path, vdir, 5)
    cdir = os.path.dirname(coarse)
    before = sorted(os.listdir(cdir))
    with pytest.raises(NotImplementedError, match="SGRAF"):
        evaluation.evalrank_rerank(coarse, scan, K, split='test', explain_sgraf=M)
    with pytest.raises(NotImplementedError, match="explain_sgraf"):
        evaluation.evalrank_rerank(coarse, sgraf, K, split='test', explain=M)
    with pytest.raises(ValueError):
        evaluation.evalrank_rerank(coarse, sgraf, K, split='test', fold5=True, explain_sgraf=M)
    for bad in (0, -1, K + 1):
        with pytest.raises(ValueError):
            evaluation.evalrank_rerank(coarse, sgraf, K, split='test', explain_sgraf=bad)
    r = _run([coarse, "--explain-sgraf", "3", "--split", "test"])
    assert r.returncode == 2 and "--rerank" in r.stderr
    assert sorted(os.listdir(cdir)) == before, "a refused call wrote a file"
    # the scorer can reason, and still cannot `explain`
    fn = evaluation._sgraf_score_fn
    assert "reasoning" in fn.__doc__
    with pytest.raises(NotImplementedError):
        evaluation.explain({}, lambda cand, by: None, M)
    with pytest.raises(NotImplementedError):
        evaluation.explain_sgraf({}, lambda cand, by: None, M)
