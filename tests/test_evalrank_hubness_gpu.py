"""GPU: `test.py --hubness ...` / evalrank_single(hubness=...) on the toy precomp dataset of tests/golden/g14_data_layer.npz: the hub
files hold cal_recall of the oracle-adjusted cal_sims matrix, and everything written without the flag stays byte for byte what it was."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import hubness_oracle as H        # noqa: E402

from itr_amd import config as C, utils                    # noqa: E402
from itr_amd.datamodule import data_loader as dl           # noqa: E402
from itr_amd.metricmodule import evaluation                # noqa: E402
from itr_amd.modalmodule import get_model                  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEST_PY = os.path.join(ROOT, "image-text-retrieval_amd", "test.py")
TOL = 1e-10


def _toy(golden, tmp_path, seed, big_dev=False):
    """big_dev: the loader fixes the length of every `dev` split at 5 000 captions (the reference's rule for COCO's), so a dev split
    that can be encoded holds 1 000 images: the toy's 6 images and 30 captions in a cycle, the images with seeded noise."""
    g = golden("g14_data_layer")
    name = 'toy_precomp'
    d = tmp_path / 'data' / name
    if not d.exists():
        d.mkdir(parents=True)
        for split in ('train', 'dev', 'test'):
            np.save(d / ('%s_ims.npy' % split), g["ims"])
            (d / ('%s_caps.txt' % split)).write_bytes(bytes(g["caps_blob"]))
        if big_dev:
            lines = bytes(g["caps_blob"]).splitlines()
            assert len(lines) == 30 and g["ims"].shape[0] == 6
            rng = np.random.default_rng(0)
            ims = g["ims"][np.arange(1000) % 6]
            np.save(d / 'dev_ims.npy', (ims + 0.05 * rng.standard_normal(ims.shape)).astype(g["ims"].dtype))
            (d / 'dev_caps.txt').write_bytes(b"\n".join(lines[c % 30] for c in range(5000)) + b"\n")
        (tmp_path / 'vocab').mkdir()
        (tmp_path / 'vocab' / ('%s_vocab.json' % name)).write_text(bytes(g["vocab_json"]).decode())
    save_dir = str(tmp_path / ('run%d' % seed))
    os.makedirs(save_dir)
    cfg = C.build_config(['with', 'SCAN', 'data_name=%s' % name, 'bi_gru=True', 'max_violation=True', 'seed=%d' % seed])
    cfg.update(img_dim=8, embed_size=32, word_dim=16, vocab_size=int(g["vocab_len"]), data_path=str(tmp_path / 'data'),
               vocab_path=str(tmp_path / 'vocab'), batch_size=64 if big_dev else 7, workers=0, save_dir=save_dir, word_tokenize=None)
    torch.manual_seed(seed)
    model = get_model(cfg)
    utils.save_checkpoint({'epoch': 3, 'model': model.state_dict(), 'best_rsum': 12.5, 'best_r1': 1.5, '_config': cfg, 'Eiters': 77}, True,
                          prefix=save_dir)
    return name, cfg, os.path.join(save_dir, 'model_best.pth.tar')


def _encoded(path, split):
    model, cfg = evaluation._load_for_eval(path, None)
    loader, _ = dl.get_test_loader(split, cfg['data_name'], cfg['batch_size'], cfg['workers'], cfg)
    return (model, cfg) + tuple(evaluation.encode_data(model, loader, islength=True))


def _sims(model, cfg, img, cap, lens):
    """A float64 matrix as evalrank_single scores it: images img[::5] against the captions through cal_sims."""
    return evaluation.cal_sims(model, img[::5], cap, lengths=lens, shard_size=cfg['batch_size'] * 5)


def _close(got, want, what):
    assert got.dtype == np.float64 and got.shape == want.shape, what
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print("%s: max error %.3g" % (what, err.max()))
    assert np.isfinite(got).all() and err.max() <= TOL, (what, err.max())


def _check_hub_files(run_dir, name, method, sims, want_a, want_b, extra):
    y = yaml.safe_load(open(os.path.join(run_dir, '%s_single_hub_%s_result.yaml' % (name, method))))
    z = np.load(os.path.join(run_dir, '%s_single_hub_%s.npz' % (name, method)))
    assert sorted(z.files) == ['a', 'b']
    _close(z['a'], want_a, method + " a")
    _close(z['b'], want_b, method + " b")
    # ranks: exactly those of the numpy-adjusted matrix under the vectors the run wrote
    i_rank, i_top, t_rank, t_top = H.ranks(H.adjust(sims, z['a'], z['b']))
    assert y['i2t_ranks'] == i_rank.tolist() and y['i2t_top1'] == i_top.tolist()
    assert y['t2i_ranks'] == t_rank.tolist() and y['t2i_top1'] == t_top.tolist()
    want = evaluation.cal_recall(H.adjust(sims, z['a'], z['b']))
    for k in ('rsum', 'i2t_r1', 'i2t_r5', 'i2t_r10', 'i2t_medr', 'i2t_meanr', 't2i_r1', 't2i_r5', 't2i_r10', 't2i_medr', 't2i_meanr'):
        assert y[k] == float(want[k]), k
    assert y['data_name'] == name and y['hubness'] == method
    for k, v in extra.items():
        assert y[k] == v, k
    return y


def test_test_py_hubness_writes_the_corrected_results(golden, dev, tmp_path):
    name, cfg, path = _toy(golden, tmp_path, 1, big_dev=True)
    run_dir = os.path.dirname(path)
    model, cfg, img, cap, lens = _encoded(path, 'test')
    sims = _sims(model, cfg, img, cap, lens)
    # without the flag: the result file, and no hub file
    evaluation.evalrank_single(path, split='test')
    plain_file = os.path.join(run_dir, '%s_single_result.yaml' % name)
    plain = open(plain_file, 'rb').read()
    assert not [f for f in os.listdir(run_dir) if '_hub_' in f]

    # inverted softmax, the bank `self`
    r = subprocess.run([sys.executable, TEST_PY, path, "--split", "test", "--hubness", "invsoftmax"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert open(plain_file, 'rb').read() == plain
    a, b = H.vectors(sims, 'invsoftmax', beta=20.0)
    y = _check_hub_files(run_dir, name, 'invsoftmax', sims, a, b, {'hub_beta': 20.0, 'querybank': 'self'})
    assert 'transductive' in y['comment'] and 'hub_k' not in y

    # CSLS with the dev split as the bank: a from test images x dev captions, b from dev images x test captions
    r = subprocess.run([sys.executable, TEST_PY, path, "--split", "test", "--hubness", "csls", "--hub-k", "3", "--querybank", "dev"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert open(plain_file, 'rb').read() == plain
    _, _, q_img, q_cap, q_lens = _encoded(path, 'dev')
    S_a = _sims(model, cfg, img, q_cap, q_lens)
    S_b = _sims(model, cfg, q_img, cap, lens)
    a, b = H.vectors(sims, 'csls', k=3, S_a=S_a, S_b=S_b)
    y = _check_hub_files(run_dir, name, 'csls', sims, a, b, {'hub_k': 3, 'querybank': 'dev'})
    assert 'comment' not in y and 'hub_beta' not in y

    # refused before anything runs
    for args, msg in (((path, "--hubness", "csls", "--fast"), "--hubness does not combine with --fast"),
                      ((path, path, "--hubness", "csls", "--rerank", "4"), "--hubness does not combine with --rerank")):
        r = subprocess.run([sys.executable, TEST_PY] + list(args), capture_output=True, text=True, timeout=600)
        assert r.returncode == 2 and msg in r.stderr


def test_evalrank_hubness_topk_gt_and_ensemble(golden, dev, tmp_path):
    name, cfg, p1 = _toy(golden, tmp_path, 1)
    _, _, p2 = _toy(golden, tmp_path, 2)
    run_dir = os.path.dirname(p1)
    m1 = _encoded(p1, 'test')
    m2 = _encoded(p2, 'test')
    sims = (_sims(*m1) + _sims(*m2)) / 2
    n_img, n_cap = sims.shape
    pairs = np.argwhere(np.arange(n_cap)[None, :] // 5 == np.arange(n_img)[:, None])
    gt_file = str(tmp_path / 'relation.npz')
    np.savez(gt_file, pairs=pairs)
    res = evaluation.evalrank_ensemble(p1, p2, split='test', topk=4, gt=gt_file, hubness='invsoftmax', hub_beta=5.0)
    assert 'i2t_ranks' in res and not any('hub' in k for k in res)           # the return value is the one without the flag
    a, b = H.vectors(sims, 'invsoftmax', beta=5.0)
    z = np.load(os.path.join(run_dir, '%s_ensemble_hub_invsoftmax.npz' % name))
    _close(z['a'], a, "ensemble a")
    _close(z['b'], b, "ensemble b")
    adj = H.adjust(sims, z['a'], z['b'])
    y = yaml.safe_load(open(os.path.join(run_dir, '%s_ensemble_hub_invsoftmax_result.yaml' % name)))
    i_rank, _, t_rank, _ = H.ranks(adj)
    assert y['i2t_ranks'] == i_rank.tolist() and y['t2i_ranks'] == t_rank.tolist() and y['hub_beta'] == 5.0
    # the hub-tagged counterparts of topk and gt come from the adjusted matrix
    lists = np.load(os.path.join(run_dir, '%s_ensemble_hub_invsoftmax_top4.npz' % name))
    want = evaluation.topk(adj, 4)
    for k, v in want.items():
        assert np.array_equal(lists[k], v), k
    yg = yaml.safe_load(open(os.path.join(run_dir, '%s_ensemble_hub_invsoftmax_gt_result.yaml' % name)))
    assert yg['i2t']['r@1'] == y['i2t_r1'] and yg['t2i']['r@1'] == y['t2i_r1']      # the layout relation: the same numbers
    assert os.path.exists(os.path.join(run_dir, '%s_ensemble_hub_invsoftmax_gt_positions.npz' % name))
    # and the plain files are those of a run without the flag
    keep = {f: open(os.path.join(run_dir, f), 'rb').read() for f in os.listdir(run_dir) if '_hub_' not in f and f.endswith('.yaml')}
    evaluation.evalrank_ensemble(p1, p2, split='test', topk=4, gt=gt_file)
    for f, data in keep.items():
        assert open(os.path.join(run_dir, f), 'rb').read() == data, f
