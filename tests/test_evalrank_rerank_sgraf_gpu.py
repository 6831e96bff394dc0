"""GPU: evaluation.evalrank_rerank and `python test.py COARSE FINE --rerank 10` with an SGRAF fine checkpoint (SAF and SGR) on a toy precomp
dataset built from tests/golden/g14_data_layer.npz like test_evalrank_rerank_gpu.py's, and the fold5 form -- five folds of 1000 images,
the coarse and rerank blocks averaged as evalrank_single's fold5 does, the npz holding every fold's lists -- for an SGRAF and for a SCAN
fine model."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from itr_amd import config as C, utils
from itr_amd.metricmodule import evaluation
from itr_amd.modalmodule import get_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEST_PY = os.path.join(ROOT, "image-text-retrieval_amd", "test.py")
K = 10


def _dataset(g, tmp_path, n_img):
    name = 'toy_precomp'
    d = tmp_path / 'data' / name
    d.mkdir(parents=True)
    caps = bytes(g["caps_blob"]).split(b"\n")[:-1]
    rng = np.random.RandomState(0)
    np.save(d / 'test_ims.npy', rng.randn(n_img, 36, 8).astype(np.float32))
    # the fixture has 30 lines: later passes get another line appended, so that neighbouring captions differ
    lines = [caps[i % len(caps)] + (b"" if i < len(caps) else b" " + caps[(7 * i + 3 + i // len(caps)) % len(caps)]) for i in range(5 * n_img)]
    (d / 'test_caps.txt').write_bytes(b"\n".join(lines) + b"\n")
    vdir = tmp_path / 'vocab'
    vdir.mkdir()
    (vdir / ('%s_vocab.json' % name)).write_text(bytes(g["vocab_json"]).decode())
    return name, str(tmp_path / 'data'), str(vdir)


def _checkpoint(g, tmp_path, tag, model_name, extra, name, data_path, vdir, seed, batch_size=7):
    save_dir = str(tmp_path / tag)
    os.makedirs(save_dir)
    cfg = C.build_config(['with', model_name, 'data_name=%s' % name, 'bi_gru=True', 'seed=%d' % seed] + extra)
    cfg.update(img_dim=8, embed_size=32, word_dim=16, vocab_size=int(g["vocab_len"]), data_path=data_path, vocab_path=vdir,
               batch_size=batch_size, workers=0, save_dir=save_dir, word_tokenize=None, sim_dim=16, vocab_type='json')
    torch.manual_seed(seed)
    model = get_model(cfg)
    utils.save_checkpoint({'epoch': 0, 'model': model.state_dict(), 'best_rsum': 0.0, 'best_r1': 0.0, '_config': cfg, 'Eiters': 1},
                          True, prefix=save_dir)
    return os.path.join(save_dir, 'model_best.pth.tar')


def _check_lists(z, top, y, single, prefix=''):
    for d in ('i2t', 't2i'):
        lists, scores = z[prefix + d + '_topk'], z[prefix + d + '_topk_scores']
        assert np.array_equal(np.sort(lists, 1), np.sort(top[prefix + d + '_topk'], 1)), d       # exactly the coarse model's K best
        assert (np.diff(scores, axis=1) <= 0).all(), d                                               # in descending fine order
        assert np.isfinite(scores).all(), d
        want = evaluation.rerank_rank_vector(lists, np.asarray(single[d + '_ranks']), d)
        assert list(y['rerank'][d + '_ranks']) == [float(v) for v in want], d


@pytest.mark.parametrize("mod", ['SAF', 'SGR'])
def test_rerank_with_an_sgraf_fine_model(golden, dev, tmp_path, mod):
    g = golden("g14_data_layer")
    n_img = 12
    name, data_path, vdir = _dataset(g, tmp_path, n_img)
    coarse = _checkpoint(g, tmp_path, 'coarse', 'VSE_PP', [], name, data_path, vdir, 3)
    fine = _checkpoint(g, tmp_path, 'fine', 'SGRAF', ['module_name=%s' % mod], name, data_path, vdir, 4)
    r = subprocess.run([sys.executable, TEST_PY, coarse, fine, "--rerank", str(K), "--split", "test"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    cdir = os.path.dirname(coarse)
    y = yaml.safe_load(open(os.path.join(cdir, '%s_rerank%d_result.yaml' % (name, K))))
    z = dict(np.load(os.path.join(cdir, '%s_rerank%d.npz' % (name, K))))
    assert y['data_name'] == name and y['k'] == K
    assert sorted(z) == ['i2t_topk', 'i2t_topk_scores', 't2i_topk', 't2i_topk_scores']
    assert z['i2t_topk'].shape == (n_img, K) and z['t2i_topk'].shape == (5 * n_img, K)
    single = evaluation.evalrank_single(coarse, split='test', topk=K)
    for key in ('i2t_ranks', 't2i_ranks'):
        assert list(y['coarse'][key]) == [float(v) for v in np.asarray(single[key])], key
    top = np.load(os.path.join(cdir, '%s_single_top%d.npz' % (name, K)))
    _check_lists(z, top, y, single)
    assert not np.array_equal(z['t2i_topk'], top['t2i_topk']), "the fine model re-orders at least one list"
    # the listed scores are the fine model's own dense scores of those pairs
    # (its t2i lists at topk = n_img hold every image of every caption: the whole matrix)
    evaluation.evalrank_single(fine, split='test', topk=n_img)
    dtop = np.load(os.path.join(os.path.dirname(fine), '%s_single_top%d.npz' % (name, n_img)))
    S = np.zeros((n_img, 5 * n_img))
    for c in range(5 * n_img):
        S[dtop['t2i_topk'][c], c] = dtop['t2i_topk_scores'][c]
    worst = max(float(np.abs(np.take_along_axis(S, z['i2t_topk'], 1) - z['i2t_topk_scores']).max()),
                float(np.abs(np.take_along_axis(S.T, z['t2i_topk'], 1) - z['t2i_topk_scores']).max()))
    print("reranked scores against the fine model's dense scores (%s): max|d| = %.3g" % (mod, worst))
    assert worst <= 2e-5
    # the same through the function, and a VSE++ fine model is still refused
    res = evaluation.evalrank_rerank(coarse, fine, K, split='test')
    assert list(res['rerank']['t2i_ranks']) == list(y['rerank']['t2i_ranks'])
    with pytest.raises(NotImplementedError, match="SCAN or SGRAF"):
        evaluation.evalrank_rerank(fine, coarse, K, split='test')


@pytest.mark.parametrize("fine_model,extra", [('SGRAF', ['module_name=SGR']), ('SCAN', [])])
def test_rerank_fold5(golden, dev, tmp_path, fine_model, extra):
    """fold5=True: five folds of 1000 images x 5000 captions; the yaml averages the folds like evalrank_single's fold5, the npz holds the
    lists of every fold under PART_<n>_ keys."""
    g = golden("g14_data_layer")
    n_img = 5000
    name, data_path, vdir = _dataset(g, tmp_path, n_img)
    coarse = _checkpoint(g, tmp_path, 'coarse', 'VSE_PP', [], name, data_path, vdir, 3, batch_size=500)
    fine = _checkpoint(g, tmp_path, 'fine', fine_model, extra, name, data_path, vdir, 4, batch_size=500)
    res = evaluation.evalrank_rerank(coarse, fine, K, split='test', fold5=True)
    cdir = os.path.dirname(coarse)
    y = yaml.safe_load(open(os.path.join(cdir, '%s_5fold_rerank%d_result.yaml' % (name, K))))
    z = np.load(os.path.join(cdir, '%s_5fold_rerank%d.npz' % (name, K)))
    assert y['data_name'] == name + '_5fold' and y['k'] == K
    single = evaluation.evalrank_single(coarse, split='test', fold5=True, topk=K)
    top = np.load(os.path.join(cdir, '%s_5fold_single_top%d.npz' % (name, K)))
    for block in ('coarse', 'rerank'):
        parts = [y[block]['PART_%d' % (i + 1)] for i in range(5)]
        # Mean_metrics: evalrank_single's fold5 averaging applied to the five folds' `result` rows
        rows = []
        for p_ in parts:
            rows += p_['result']
        want = evaluation._mean_metrics({'sum_result': rows})
        assert set(y[block]['Mean_metrics']) == set(want), block
        for key, v in want.items():
            assert y[block]['Mean_metrics'][key] == pytest.approx(float(v)), (block, key)
    for key, v in single['Mean_metrics'].items():
        assert y['coarse']['Mean_metrics'][key] == pytest.approx(float(v)), key
    for i in range(5):
        pre = 'PART_%d_' % (i + 1)
        assert z[pre + 'i2t_topk'].shape == (1000, K) and z[pre + 't2i_topk'].shape == (5000, K)
        part_single = single['PART_%d' % (i + 1)]
        assert list(y['coarse']['PART_%d' % (i + 1)]['i2t_ranks']) == [float(v) for v in np.asarray(part_single['i2t_ranks'])]
        _check_lists(z, top, {'rerank': y['rerank']['PART_%d' % (i + 1)], 'fine': fine_model}, part_single, prefix=pre)
    assert list(res['rerank']['PART_3']['t2i_ranks']) == list(y['rerank']['PART_3']['t2i_ranks'])
