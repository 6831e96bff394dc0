"""GPU: itr_amd.search.GalleryIndex and `python search.py` on the toy precomp dataset and tiny checkpoints of
tests/helpers/ensemble_toy.py (12 images / 60 captions; VSE++ coarse model, SCAN t2i or SGRAF SAF fine model).  The answers of the
index are the rows of the split-sized evaluation for the same queries -- evaluation.topk on the fp32 cosine matrix, evaluation.rerank
with the evaluation's own fine scorer -- index for index and byte for byte."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from ensemble_toy import checkpoint, dataset                                         # noqa: E402
from itr_amd import ops                                                              # noqa: E402
from itr_amd.datamodule import data_loader as data                                   # noqa: E402
from itr_amd.metricmodule import evaluation                                          # noqa: E402
from itr_amd.search import GalleryIndex, Query                                       # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEARCH_PY = os.path.join(ROOT, "image-text-retrieval_amd", "search.py")
K, N_IMG = 10, 12
FINES = {'scan': ('SCAN', ['cross_attn=t2i']), 'saf': ('SGRAF', ['module_name=SAF'])}


@pytest.fixture(scope="module")
def toy(golden, dev, tmp_path_factory):
    """the dataset, one VSE++ coarse checkpoint, the fine checkpoints, a second VSE++ checkpoint, and every model's encode_data arrays"""
    tmp = tmp_path_factory.mktemp("search_index")
    g = golden("g14_data_layer")
    name, data_path, vdir = dataset(g, tmp, N_IMG)
    paths = {'coarse': checkpoint(g, tmp, 'coarse', 'VSE_PP', [], name, data_path, vdir, 3),
             'other': checkpoint(g, tmp, 'other', 'VSE_PP', [], name, data_path, vdir, 11),
             'scan_coarse': checkpoint(g, tmp, 'scanc', 'SCAN', ['cross_attn=i2t'], name, data_path, vdir, 12)}
    for j, (tag, (fam, extra)) in enumerate(sorted(FINES.items())):
        paths[tag] = checkpoint(g, tmp, tag, fam, extra, name, data_path, vdir, 4 + j)
    models, embs = {}, {}
    for tag in ('coarse',) + tuple(sorted(FINES)):
        model, cfg = evaluation._load_for_eval(paths[tag], None)
        loader, _ = data.get_test_loader('test', cfg['data_name'], cfg['batch_size'], cfg['workers'], cfg)
        models[tag] = model
        embs[tag] = evaluation.encode_data(model, loader, islength=cfg['name'] in ('SGRAF', 'SCAN'))
    lines = open(os.path.join(data_path, name, 'test_caps.txt'), 'rb').read().split(b"\n")[:-1]
    return {'tmp': tmp, 'paths': paths, 'models': models, 'embs': embs, 'lines': lines, 'data_dir': os.path.join(data_path, name)}


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_from_embeddings_gives_the_rows_of_the_evaluation(toy):
    img, cap, _ = toy['embs']['coarse']
    index = GalleryIndex.from_embeddings(coarse=(img, cap))
    S = ops.cosine_scores(torch.from_numpy(img[::5].copy()).cuda(), torch.from_numpy(cap).cuda()).cpu().numpy()
    want = evaluation.topk(S, K)
    t2i = index.search_embedded(cap, 't2i', K)
    i2t = index.search_embedded(img[::5], 'i2t', K)
    assert t2i.idx.shape == (5 * N_IMG, K) and i2t.idx.shape == (N_IMG, K)
    assert same(t2i.idx, want['t2i_topk']) and same(t2i.scores, want['t2i_topk_scores'])
    assert same(i2t.idx, want['i2t_topk']) and same(i2t.scores, want['i2t_topk_scores'])
    assert same(t2i.coarse_idx, t2i.idx) and same(t2i.coarse_scores, t2i.scores)
    # the fused pass and the matrix path (what `route = 'auto'` picks between by gallery size): the same bytes
    assert index.route == 'auto'
    for route in ('fused', 'matrix'):
        index.route = route
        r = index.search_embedded(cap, 't2i', K)
        assert same(r.idx, t2i.idx) and same(r.scores, t2i.scores), route
        r = index.search_embedded(img[::5], 'i2t', K)
        assert same(r.idx, i2t.idx) and same(r.scores, i2t.scores), route
    index.route = 'fused'
    # one query at a time, and a tensor on the device: the same rows
    one = index.search_embedded(torch.from_numpy(cap[7:8]).cuda(), 't2i', K)
    assert same(one.idx, want['t2i_topk'][7:8]) and same(one.scores, want['t2i_topk_scores'][7:8])


@pytest.mark.parametrize("tag", sorted(FINES))
def test_rerank_gives_the_lists_of_evaluation_rerank(toy, tag):
    img, cap, _ = toy['embs']['coarse']
    f_img, f_cap, f_len = toy['embs'][tag]
    model = toy['models'][tag]
    index = GalleryIndex.from_embeddings(coarse=(img, cap), fine=(f_img, f_cap, f_len), fine_model=model)
    index.route = 'fused'
    make = evaluation._scan_score_fn if model.config['name'] == 'SCAN' else evaluation._sgraf_score_fn
    S = ops.cosine_scores(torch.from_numpy(img[::5].copy()).cuda(), torch.from_numpy(cap).cuda()).cpu().numpy()
    _, _, _, want = evaluation.rerank(S, make(model, f_img[::5], f_cap, f_len), K)
    t2i = index.search_embedded(Query('text', cap, f_cap, f_len), 't2i', K, rerank=K)
    i2t = index.search_embedded(Query('images', img[::5], f_img[::5]), 'i2t', K, rerank=K)
    assert same(t2i.idx, want['t2i_topk']) and same(t2i.scores, want['t2i_topk_scores'])
    assert same(i2t.idx, want['i2t_topk']) and same(i2t.scores, want['i2t_topk_scores'])
    coarse = evaluation.topk(S, K)
    assert same(t2i.coarse_idx, coarse['t2i_topk']) and same(i2t.coarse_scores, coarse['i2t_topk_scores'])
    # k < rerank: the head of the reranked lists
    head = index.search_embedded(Query('text', cap, f_cap, f_len), 't2i', 3, rerank=K)
    assert same(head.idx, want['t2i_topk'][:, :3]) and same(head.scores, want['t2i_topk_scores'][:, :3])
    with pytest.raises(ValueError, match="rerank"):
        index.search_embedded(Query('text', cap, f_cap, f_len), 't2i', K, rerank=K - 1)


@pytest.fixture(scope="module")
def built(toy):
    index = GalleryIndex.build(toy['paths']['coarse'], toy['paths']['scan'], split='test')
    index.route = 'fused'                  # (the command line below runs 'auto': the matrix path at this size, the same bytes)
    return index


def test_build_keeps_the_evaluations_embeddings(toy, built):
    img, cap, _ = toy['embs']['coarse']
    f_img, f_cap, f_len = toy['embs']['scan']
    h = built._host
    assert same(h['coarse_img'], img[::5]) and same(h['coarse_cap'], cap)
    assert same(h['fine_img'], f_img[::5]) and same(h['fine_cap'], f_cap) and same(h['fine_lens'], f_len)


def test_save_load_round_trip(toy, built):
    path = str(toy['tmp'] / 'index.npz')
    built.save(path)
    again = GalleryIndex.load(path, toy['paths']['coarse'], toy['paths']['scan'])
    assert sorted(again._host) == sorted(built._host) and all(same(again._host[k], built._host[k]) for k in built._host)
    assert again.meta == built.meta and again.meta['split'] == 'test' and again.meta['im_div'] == 5 and len(again.meta['sha256_coarse']) == 64
    lines = toy['lines'][:9]
    a, b = built.search_text(lines, 5, rerank=K), again.search_text(lines, 5, rerank=K)
    assert all(same(x, y) for x, y in zip(a.arrays().values(), b.arrays().values()))
    with pytest.raises(ValueError, match="different coarse checkpoint"):
        GalleryIndex.load(path, toy['paths']['other'], toy['paths']['scan'])
    with pytest.raises(ValueError, match="different fine checkpoint"):
        GalleryIndex.load(path, toy['paths']['coarse'], toy['paths']['saf'])
    with pytest.raises(ValueError, match="different fine checkpoint"):
        GalleryIndex.load(path, toy['paths']['coarse'])


def test_text_encoding(toy, built):
    lines = toy['lines']
    assert len(lines) == 5 * N_IMG
    q = built.encode_text(lines)
    assert q.token_ids == [built.dataset.token_ids(i) for i in range(len(lines))]
    assert q.token_ids == built.encode_text([l.decode() for l in lines]).token_ids
    # one by one, in batches of 7, all at once: bit-identical embeddings
    for step in (1, 7):
        for i in range(0, len(lines), step):
            part = built.encode_text(lines[i:i + step])
            assert same(part.coarse, q.coarse[i:i + step])
            for j in range(len(part)):
                n = int(part.lens[j])
                assert n == int(q.lens[i + j]) and same(part.fine[j, :n], q.fine[i + j, :n])
    a, b = built.search_text(lines, K, rerank=K), built.search_embedded(q, 't2i', K, rerank=K)
    assert all(same(x, y) for x, y in zip(a.arrays().values(), b.arrays().values()))
    # image queries answer with captions
    feats = np.load(os.path.join(toy['data_dir'], 'test_ims.npy'))
    r = built.search_images(feats[:3], 4)
    assert r.idx.shape == (3, 4) and (r.idx >= 0).all() and (r.idx < 5 * N_IMG).all()


def test_command_line(toy, built):
    tmp = toy['tmp']
    qfile, ifile, ofile = str(tmp / 'queries.txt'), str(tmp / 'cli_index.npz'), str(tmp / 'cli_out.npz')
    lines = toy['lines'][3:11]
    with open(qfile, 'wb') as f:
        f.write(b"\n".join(lines) + b"\n")
    want = built.search_text(lines, 5, rerank=K)
    cmd = [sys.executable, SEARCH_PY, toy['paths']['coarse'], toy['paths']['scan'], "--split", "test", "--queries", qfile, "-k", "5",
           "--rerank", str(K), "--index", ifile, "--out", ofile]
    for run, word in enumerate(("saved", "loaded")):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
        assert "index %s" % word in r.stdout and os.path.exists(ifile)
        z = np.load(ofile)
        assert same(z['idx'], want.idx) and same(z['scores'], want.scores)
        assert [s for s in z['queries']] == [l.decode() for l in lines]
        assert r.stdout.count("query ") == len(lines)
        os.remove(ofile)


def test_refusals(toy):
    with pytest.raises(NotImplementedError, match="cannot be the coarse model"):
        GalleryIndex.build(toy['paths']['scan_coarse'], split='test')
    with pytest.raises(NotImplementedError, match="must be SCAN or SGRAF"):
        GalleryIndex.build(toy['paths']['coarse'], toy['paths']['other'], split='test')
