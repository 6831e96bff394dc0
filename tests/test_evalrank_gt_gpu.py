"""GPU: `test.py --gt FILE.npz` / evalrank_single(gt=...) on the toy precomp dataset of tests/golden/g14_data_layer.npz: the two new
files hold gt_metrics of cal_sims' matrix, and everything written without --gt stays byte for byte what it was."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from itr_amd import config as C, ops, utils
from itr_amd.datamodule import data_loader as dl
from itr_amd.metricmodule import evaluation
from itr_amd.modalmodule import get_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEST_PY = os.path.join(ROOT, "image-text-retrieval_amd", "test.py")


def _toy(golden, tmp_path, seed):
    g = golden("g14_data_layer")
    name = 'toy_precomp'
    d = tmp_path / 'data' / name
    if not d.exists():
        d.mkdir(parents=True)
        for split in ('train', 'dev', 'test'):
            np.save(d / ('%s_ims.npy' % split), g["ims"])
            (d / ('%s_caps.txt' % split)).write_bytes(bytes(g["caps_blob"]))
        (tmp_path / 'vocab').mkdir()
        (tmp_path / 'vocab' / ('%s_vocab.json' % name)).write_text(bytes(g["vocab_json"]).decode())
    save_dir = str(tmp_path / ('run%d' % seed))
    os.makedirs(save_dir)
    cfg = C.build_config(['with', 'SCAN', 'data_name=%s' % name, 'bi_gru=True', 'max_violation=True', 'seed=%d' % seed])
    cfg.update(img_dim=8, embed_size=32, word_dim=16, vocab_size=int(g["vocab_len"]), data_path=str(tmp_path / 'data'),
               vocab_path=str(tmp_path / 'vocab'), batch_size=7, workers=0, save_dir=save_dir, word_tokenize=None)
    torch.manual_seed(seed)
    model = get_model(cfg)
    utils.save_checkpoint({'epoch': 3, 'model': model.state_dict(), 'best_rsum': 12.5, 'best_r1': 1.5, '_config': cfg, 'Eiters': 77}, True,
                          prefix=save_dir)
    return name, cfg, os.path.join(save_dir, 'model_best.pth.tar')


def _sims(path):
    """The float64 matrix evalrank_single ranks: the checkpoint through the loader, encode_data and cal_sims."""
    model, cfg = evaluation._load_for_eval(path, None)
    loader, _ = dl.get_test_loader('test', cfg['data_name'], cfg['batch_size'], cfg['workers'], cfg)
    img, cap, lens = evaluation.encode_data(model, loader, islength=True)
    return evaluation.cal_sims(model, img[::5], cap, lengths=lens, shard_size=cfg['batch_size'] * 5)


def _relation(n_img, n_cap, seed):
    rng = np.random.RandomState(seed)
    rel = rng.rand(n_img, n_cap) < 0.2
    rel[np.arange(n_cap) // 5, np.arange(n_cap)] = True          # the layout pairs included
    rel[:, 7] = False                                            # a caption without positives
    return np.argwhere(rel)


def _check_files(run_dir, name, tag, want):
    y = yaml.safe_load(open(os.path.join(run_dir, '%s_%s_gt_result.yaml' % (name, tag))))
    z = np.load(os.path.join(run_dir, '%s_%s_gt_positions.npz' % (name, tag)))
    assert y['data_name'] == name
    for d in ('i2t', 't2i'):
        scalars = {k: v for k, v in want[d].items() if not isinstance(v, np.ndarray)}
        assert set(y[d]) == set(scalars) >= {'r@1', 'r@5', 'r@10', 'medr', 'meanr', 'rprecision', 'map_at_r', 'n_queries', 'n_without_positives'}
        for k, v in scalars.items():
            assert y[d][k] == v, (d, k)
        for k in ('positions', 'best', 'rprecision_q', 'ap_q'):
            assert np.array_equal(z['%s_%s' % (d, k)], want[d][k], equal_nan=True), (d, k)
    assert want['t2i']['n_without_positives'] == 1
    return z


def test_test_py_gt_writes_the_metrics_of_the_relation(golden, dev, tmp_path):
    name, cfg, path = _toy(golden, tmp_path, 1)
    run_dir = os.path.dirname(path)
    sims = _sims(path)
    n_img, n_cap = sims.shape
    pairs = _relation(n_img, n_cap, 0)
    gt_file = str(tmp_path / 'relation.npz')
    np.savez(gt_file, pairs=pairs, n_images=n_img, n_captions=n_cap)
    # without --gt: the result file, and no new file
    evaluation.evalrank_single(path, split='test')
    plain = open(os.path.join(run_dir, '%s_single_result.yaml' % name), 'rb').read()
    assert not [f for f in os.listdir(run_dir) if '_gt_' in f]
    # the command line with --gt: the same result file byte for byte, and the two new files
    r = subprocess.run([sys.executable, TEST_PY, path, "--split", "test", "--gt", gt_file], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert open(os.path.join(run_dir, '%s_single_result.yaml' % name), 'rb').read() == plain
    gt = ops.GroundTruth(pairs, n_img, n_cap, dev)
    want = evaluation.gt_metrics(sims, gt)
    z = _check_files(run_dir, name, 'single', want)
    assert np.array_equal(z['img_ptr'], gt.img_ptr_host) and np.array_equal(z['cap_img'], gt.cap_img.cpu().numpy())
    # --gt with --rerank is refused before anything runs
    r = subprocess.run([sys.executable, TEST_PY, path, path, "--rerank", "4", "--gt", gt_file], capture_output=True, text=True, timeout=600)
    assert r.returncode == 2 and "--gt does not combine with --rerank" in r.stderr


def test_evalrank_gt_ensemble_and_refusals(golden, dev, tmp_path):
    name, cfg, p1 = _toy(golden, tmp_path, 1)
    _, _, p2 = _toy(golden, tmp_path, 2)
    sims = (_sims(p1) + _sims(p2)) / 2
    n_img, n_cap = sims.shape
    pairs = _relation(n_img, n_cap, 1)
    gt_file = str(tmp_path / 'relation.npz')
    np.savez(gt_file, pairs=pairs)
    res = evaluation.evalrank_ensemble(p1, p2, split='test', gt=gt_file)
    assert 'i2t_ranks' in res and not any('gt' in k for k in res)          # the return value is the one without gt
    _check_files(os.path.dirname(p1), name, 'ensemble', evaluation.gt_metrics(sims, ops.GroundTruth(pairs, n_img, n_cap, dev)))
    with pytest.raises(ValueError, match="fold5"):
        evaluation.evalrank_single(p1, split='test', fold5=True, gt=gt_file)
    bad = str(tmp_path / 'bad.npz')
    np.savez(bad, pairs=pairs, n_images=n_img + 1)
    with pytest.raises(ValueError, match="n_images"):
        evaluation.evalrank_single(p1, split='test', gt=bad)
    np.savez(bad, pairs=np.concatenate([pairs, [[n_img, 0]]]))
    with pytest.raises(ValueError, match="out of range"):
        evaluation.evalrank_single(p1, split='test', gt=bad)
