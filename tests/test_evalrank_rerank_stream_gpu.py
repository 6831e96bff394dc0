"""GPU: evaluation.evalrank_rerank / evalrank_rerank_ensemble with stream_coarse=True and `python test.py COARSE FINE --rerank 10
--stream-coarse` on the toy precomp dataset and tiny checkpoints of tests/helpers/ensemble_toy.py (VSE++ coarse model, SCAN or
SAF + SGR fine models): the coarse matrix is never built, and the files are the plain call's -- the same YAML rank vectors and Recall
numbers, the same .npz lists, byte for byte."""
import os
import subprocess
import sys

import numpy as np
import pytest
import yaml

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from ensemble_toy import checkpoint, dataset                                         # noqa: E402
from itr_amd.metricmodule import evaluation                                          # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEST_PY = os.path.join(ROOT, "image-text-retrieval_amd", "test.py")
K, N_IMG = 10, 12
RANK_KEYS = ('i2t_ranks', 't2i_ranks', 'i2t_top1', 't2i_top1')
NUM_KEYS = ('i2t_r1', 'i2t_r5', 'i2t_r10', 'i2t_medr', 'i2t_meanr', 't2i_r1', 't2i_r5', 't2i_r10', 't2i_medr', 't2i_meanr', 'rsum',
            'i2t_ave_r', 't2i_ave_r', 'result')


def _setup(golden, tmp_path, coarse, fines):
    g = golden("g14_data_layer")
    name, data_path, vdir = dataset(g, tmp_path, N_IMG)
    c = checkpoint(g, tmp_path, 'coarse', coarse[0], coarse[1], name, data_path, vdir, 3)
    f = [checkpoint(g, tmp_path, 'fine%d' % (j + 1), fam, extra, name, data_path, vdir, 4 + j) for j, (fam, extra) in enumerate(fines)]
    return name, c, f


def _read(cdir, stem):
    y = yaml.safe_load(open(os.path.join(cdir, stem + '_result.yaml')))
    z = dict(np.load(os.path.join(cdir, stem + '.npz')))
    os.remove(os.path.join(cdir, stem + '_result.yaml'))
    os.remove(os.path.join(cdir, stem + '.npz'))
    return y, z


def _assert_same_files(plain, streamed):
    (y0, z0), (y1, z1) = plain, streamed
    assert sorted(y0) == sorted(y1)
    for block in ('coarse', 'rerank'):
        assert sorted(y0[block]) == sorted(y1[block]), block
        for key in RANK_KEYS + NUM_KEYS:
            assert y0[block][key] == y1[block][key], (block, key)
    for key in y0:
        if key not in ('coarse', 'rerank'):
            assert y0[key] == y1[key], key
    assert sorted(z0) == sorted(z1)
    for key in z0:
        assert z0[key].dtype == z1[key].dtype and z0[key].shape == z1[key].shape and z0[key].tobytes() == z1[key].tobytes(), key


def test_stream_coarse_writes_the_plain_calls_files(golden, dev, tmp_path):
    name, coarse, (fine,) = _setup(golden, tmp_path, ('VSE_PP', []), [('SCAN', ['cross_attn=t2i'])])
    cdir, stem = os.path.dirname(coarse), '%s_rerank%d' % (name, K)
    evaluation.evalrank_rerank(coarse, fine, K, split='test')
    plain = _read(cdir, stem)
    assert plain[1]['i2t_topk'].shape == (N_IMG, K) and plain[1]['t2i_topk'].shape == (5 * N_IMG, K)
    evaluation.evalrank_rerank(coarse, fine, K, split='test', stream_coarse=True)
    _assert_same_files(plain, _read(cdir, stem))
    # explain keeps working on the streamed lists
    evaluation.evalrank_rerank(coarse, fine, K, split='test', stream_coarse=True, explain=2)
    assert os.path.exists(os.path.join(cdir, stem + '_explain2.npz'))
    _assert_same_files(plain, _read(cdir, stem))


def test_stream_coarse_ensemble(golden, dev, tmp_path):
    name, coarse, fines = _setup(golden, tmp_path, ('VSE_PP', []), [('SGRAF', ['module_name=SAF']), ('SGRAF', ['module_name=SGR'])])
    cdir, stem = os.path.dirname(coarse), '%s_rerank%d_ensemble' % (name, K)
    evaluation.evalrank_rerank_ensemble(coarse, fines, K, split='test')
    plain = _read(cdir, stem)
    assert plain[1]['i2t_topk_member_scores'].shape == (2, N_IMG, K)
    evaluation.evalrank_rerank_ensemble(coarse, fines, K, split='test', stream_coarse=True)
    _assert_same_files(plain, _read(cdir, stem))


def test_stream_coarse_command_line(golden, dev, tmp_path):
    name, coarse, (fine,) = _setup(golden, tmp_path, ('VSE_PP', []), [('SCAN', ['cross_attn=i2t'])])
    cdir, stem = os.path.dirname(coarse), '%s_rerank%d' % (name, K)
    evaluation.evalrank_rerank(coarse, fine, K, split='test')
    plain = _read(cdir, stem)
    r = subprocess.run([sys.executable, TEST_PY, coarse, fine, "--rerank", str(K), "--split", "test", "--stream-coarse"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    _assert_same_files(plain, _read(cdir, stem))
    r = subprocess.run([sys.executable, TEST_PY, coarse, "--stream-coarse"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--stream-coarse needs --rerank" in r.stderr


def test_a_dense_coarse_model_is_refused(golden, dev, tmp_path):
    name, coarse, (fine,) = _setup(golden, tmp_path, ('SCAN', ['cross_attn=t2i']), [('SCAN', ['cross_attn=i2t'])])
    with pytest.raises(NotImplementedError, match="stream_coarse"):
        evaluation.evalrank_rerank(coarse, fine, K, split='test', stream_coarse=True)
    with pytest.raises(NotImplementedError, match="stream_coarse"):
        evaluation.evalrank_rerank_ensemble(coarse, [fine], K, split='test', stream_coarse=True)
    left = [f for f in os.listdir(os.path.dirname(coarse)) if 'rerank' in f]
    assert left == [], left


def test_stream_coarse_explain_sgraf(golden, dev, tmp_path):
    """explain_sgraf keeps working: the streamed call writes the plain call's lists and the plain call's explanation file"""
    name, coarse, (fine,) = _setup(golden, tmp_path, ('VSE_PP', []), [('SGRAF', ['module_name=SAF'])])
    cdir, stem = os.path.dirname(coarse), '%s_rerank%d' % (name, K)
    ex = os.path.join(cdir, stem + '_explain2_sgraf.npz')
    evaluation.evalrank_rerank(coarse, fine, K, split='test', explain_sgraf=2)
    plain, plain_ex = _read(cdir, stem), dict(np.load(ex))
    os.remove(ex)
    evaluation.evalrank_rerank(coarse, fine, K, split='test', stream_coarse=True, explain_sgraf=2)
    _assert_same_files(plain, _read(cdir, stem))
    got_ex = dict(np.load(ex))
    assert sorted(got_ex) == sorted(plain_ex)
    for key in plain_ex:
        assert got_ex[key].dtype == plain_ex[key].dtype and got_ex[key].tobytes() == plain_ex[key].tobytes(), key


def test_stream_coarse_fold5(golden, dev, tmp_path):
    """fold5 keeps working: five folds of 1000 images x 5000 captions (strided image rows, per-fold caption slices).  The plain call
    scores each fold in (5 x 500)^2 tiles, the streamed one in full-width row blocks: the same lists and ranks in every fold."""
    g = golden("g14_data_layer")
    name, data_path, vdir = dataset(g, tmp_path, 5000)
    coarse = checkpoint(g, tmp_path, 'coarse', 'VSE_PP', [], name, data_path, vdir, 3, batch_size=500)
    fine = checkpoint(g, tmp_path, 'fine1', 'SCAN', ['cross_attn=t2i'], name, data_path, vdir, 4, batch_size=500)
    cdir, stem = os.path.dirname(coarse), '%s_5fold_rerank%d' % (name, K)

    evaluation.evalrank_rerank(coarse, fine, K, split='test', fold5=True)
    y0, z0 = _read(cdir, stem)
    evaluation.evalrank_rerank(coarse, fine, K, split='test', fold5=True, stream_coarse=True)
    y1, z1 = _read(cdir, stem)
    assert sorted(z0) == sorted(z1) == sorted('PART_%d_%s' % (i + 1, s) for i in range(5)
                                              for s in ('i2t_topk', 'i2t_topk_scores', 't2i_topk', 't2i_topk_scores'))
    for key in z0:
        assert z0[key].shape == z1[key].shape and z0[key].tobytes() == z1[key].tobytes(), key
    assert z0['PART_2_t2i_topk'].shape == (5000, K)
    for block in ('coarse', 'rerank'):
        assert y0[block]['Mean_metrics'] == y1[block]['Mean_metrics'], block
        for i in range(5):
            for key in RANK_KEYS + NUM_KEYS:
                assert y0[block]['PART_%d' % (i + 1)][key] == y1[block]['PART_%d' % (i + 1)][key], (block, i, key)
