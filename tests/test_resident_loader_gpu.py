"""GPU: the device-resident training loader (datamodule/resident.py) hands out the batches of the DataLoader path, member by
member and bit for bit, refuses a split that does not fit, and trains to what the DataLoader path trains to -- in process,
from the command line and on two data-parallel ranks.  The toy split is tests/golden/g14_data_layer.npz as precomp files."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from itr_amd.datamodule import data_loader as dl, tokenization as tok
from itr_amd.datamodule.resident import ResidentLoader, ResidentTrainSet

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "helpers", "resident_train_worker.py")
NAME = 'toy_precomp'


def _materialise(g, root, per_caption=False):
    """train / dev files of the toy split: 6 images x 5 captions (im_div 5), or the feature rows repeated per caption (im_div 1).
    Boxes are the fixture's; the image sizes are drawn here as INTEGERS, so the float32 cast of __getitem__ has work to do."""
    d = root / 'data' / NAME
    d.mkdir(parents=True)
    rep = 5 if per_caption else 1
    rng = np.random.RandomState(5)
    for split in ('train', 'dev'):
        np.save(d / ('%s_ims.npy' % split), np.repeat(g["ims"], rep, axis=0))
        np.save(d / ('%s_boxes.npy' % split), np.repeat(g["boxes"], rep, axis=0))
        np.save(d / ('%s_img_sizes.npy' % split), np.repeat(rng.randint(200, 640, size=(6, 2)), rep, axis=0))
        (d / ('%s_caps.txt' % split)).write_bytes(bytes(g["caps_blob"]))
    vdir = root / 'vocab'
    vdir.mkdir()
    (vdir / ('%s_vocab.json' % NAME)).write_text(bytes(g["vocab_json"]).decode())
    vfile = root / 'bert_vocab.txt'
    vfile.write_bytes(bytes(g["bert_vocab"]))
    return str(d), str(root / 'data'), str(vdir), str(vfile)


@pytest.fixture(scope="module")
def toy(golden, tmp_path_factory):
    g = golden("g14_data_layer")
    return {pc: _materialise(g, tmp_path_factory.mktemp("resident_pc%d" % pc), per_caption=bool(pc)) for pc in (0, 1)}


def _layout_cfg(layout, vdir, vfile, seed):
    base = {'data_name': NAME, 'vocab_path': vdir, 'vocab_type': 'json', 'word_tokenize': tok.regex_word_tokenize, 'seed': seed}
    return dict(base, **{
        'SCAN': {'name': 'SCAN', 'text_encoder': 'gru', 'use_bbox': False},
        'VSRN': {'name': 'VSRN', 'text_encoder': 'gru', 'use_bbox': False, 'max_len': 9},       # 9: some captions are cut, some padded
        'SAEM': {'name': 'SAEM', 'text_encoder': 'bert', 'use_bbox': False, 'max_words': 12, 'vocab_file': vfile},
        'CAMERA': {'name': 'CAMERA', 'text_encoder': 'bert', 'use_bbox': True, 'max_words': 12, 'vocab_file': vfile},
    }[layout])


def _same_member(k, got, want):
    if torch.is_tensor(want):
        assert torch.is_tensor(got) and got.is_cuda and not want.is_cuda, k
        assert got.dtype == want.dtype and got.shape == want.shape, (k, got.dtype, want.dtype, got.shape, want.shape)
        assert np.array_equal(got.cpu().numpy().view(np.uint8), want.numpy().view(np.uint8)), k
    else:
        assert type(got) is type(want), (k, type(got), type(want))
        assert len(got) == len(want), k
        for a, b in zip(got, want):
            if b is None:
                assert a is None, k
            else:
                assert type(a) is type(b) and int(a) == int(b), (k, a, b)
                if torch.is_tensor(b):
                    assert a.dtype == b.dtype and a.shape == b.shape and not a.is_cuda, k
        if isinstance(want, np.ndarray):
            assert got.dtype == want.dtype and got.shape == want.shape, k


@pytest.mark.parametrize("layout,per_caption", [("SCAN", 0), ("SCAN", 1), ("VSRN", 0), ("SAEM", 0), ("CAMERA", 0)])
def test_batches_equal_the_loaders(dev, toy, layout, per_caption):
    d, _, vdir, vfile = toy[per_caption]
    cfg = _layout_cfg(layout, vdir, vfile, seed=4)
    loader, _ = dl.get_precomp_loader(d, 'train', cfg, batch_size=7, shuffle=True, num_workers=0)
    assert loader.dataset.im_div == (1 if per_caption else 5)
    rs = ResidentTrainSet(dl.PrecompDataset(d, 'train', cfg), dev)
    res = ResidentLoader(rs, 7, True, cfg['seed'])
    assert len(res) == len(loader) == 5 and isinstance(res.dataset, dl.PrecompDataset)
    assert rs.bytes_held == rs.bytes_needed
    n_batches = 0
    for epoch in range(2):
        for got, want in zip(res, loader):
            assert isinstance(got, tuple) and len(got) == len(want) == 8
            for k in range(8):
                _same_member(k, got[k], want[k])
            n_batches += 1
    assert n_batches == 10
    assert int(rs.bad_flag.item()) == 0


def test_memory_refusal_allocates_nothing(dev, toy):
    d, _, vdir, vfile = toy[0]
    dset = dl.PrecompDataset(d, 'train', _layout_cfg('SCAN', vdir, vfile, 0))
    need = 6 * 36 * 8 * 4 + (int(dset.token_ids_range(0, 30)[1].sum()) + 31) * 8
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(dev)
    with pytest.raises(MemoryError) as e:
        ResidentTrainSet(dset, dev, max_bytes=1)
    assert "%d bytes" % need in str(e.value) and "only 1 bytes" in str(e.value)
    assert torch.cuda.memory_allocated(dev) == before
    with pytest.raises(MemoryError):
        ResidentTrainSet(dset, dev, max_bytes=need - 1)
    assert torch.cuda.memory_allocated(dev) == before
    assert ResidentTrainSet(dset, dev, max_bytes=need).bytes_held == need           # exactly what it asked for
    assert ResidentTrainSet(dset, dev).bytes_held == need                           # the default allowance holds a toy split
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ResidentTrainSet(dset, 'cpu')


def _differ(a, b):
    """(largest per-step loss difference, largest parameter difference) of two runs"""
    assert a[0].shape == b[0].shape and a[1].shape == b[1].shape
    return float(np.abs(a[0] - b[0]).max()), float(np.abs(a[1] - b[1]).max())


def _check_parity(loader_1, loader_2, resident):
    """The yardstick is the DataLoader path run twice from one seed: the resident run may differ from the first of them by no
    more than the second does -- bit for bit where those two agree bit for bit.

    The batches of the two paths are bit-identical (test_batches_equal_the_loaders) and the training step is deterministic -- the
    embedding gradient, once an atomic scatter whose last bits changed from run to run, adds the rows of a token in row order
    (csrc/train.hip) -- so the two DataLoader runs agree bit for bit, which is asserted, and the resident run has to as well.

    Record of the atomic scatter (MI355X, toy epoch of 5 steps, largest |difference| of the per-step losses / of the final
    parameters): two DataLoader runs differed by 0 .. 4.8e-07 / 3.0e-08 .. 1.64e-07 and the resident run by as much from either, so
    this comparison, which puts no factor on the yardstick, missed by rounding noise about as often as it was met."""
    assert str(loader_1[2]) == str(loader_2[2]) == 'DataLoader' and str(resident[2]) == 'ResidentLoader'
    assert len(loader_1[0]) == 5 and np.isfinite(loader_1[0]).all() and np.isfinite(resident[1]).all()
    d_loss, d_par = _differ(loader_1, loader_2)
    r_loss, r_par = _differ(loader_1, resident)
    print("loader vs loader: dloss %.3e dparam %.3e; resident vs loader: dloss %.3e dparam %.3e" % (d_loss, d_par, r_loss, r_par))
    assert d_loss == 0 and d_par == 0, (d_loss, d_par)          # the step is deterministic
    assert r_loss <= d_loss and r_par <= d_par, (r_loss, d_loss, r_par, d_par)
    if d_loss == 0 and d_par == 0:
        assert np.array_equal(loader_1[0], resident[0]) and np.array_equal(loader_1[1].view(np.uint32), resident[1].view(np.uint32))


@pytest.mark.parametrize("model_name", ["VSE_PP", "SCAN"])
def test_training_parity(dev, toy, model_name):
    from resident_train_worker import run_epoch
    _, data_path, vdir, _ = toy[0]
    runs = [run_epoch(model_name, NAME, data_path, vdir, resident) for resident in (0, 0, 1)]
    _check_parity(*runs)


def _big_dev_split(toy_paths, root, n_img=40):
    """A split train.py can validate on: the 'dev' split is cut to 5000 captions by the data layer, so it must hold as many."""
    g_caps = open(os.path.join(toy_paths[0], 'train_caps.txt'), 'rb').read().split(b"\n")[:-1]
    d = root / 'data' / NAME
    d.mkdir(parents=True)
    rng = np.random.RandomState(0)
    for split, n in (('train', n_img), ('dev', 1000)):
        np.save(d / ('%s_ims.npy' % split), rng.randn(n, 36, 8).astype(np.float32))
        (d / ('%s_caps.txt' % split)).write_bytes(b"\n".join(g_caps[i % len(g_caps)] for i in range(5 * n)) + b"\n")
    return str(root / 'data')


@pytest.mark.parametrize("resident", [True, False])
def test_train_command_line(toy, tmp_path, resident):
    """`python train.py with SCAN ... resident_data=True num_epochs=1` trains and writes its best checkpoint; so does the default"""
    data_path = _big_dev_split(toy[0], tmp_path)
    runs = str(tmp_path / 'runs')
    args = [sys.executable, os.path.join(ROOT, "image-text-retrieval_amd", "train.py"), "with", "SCAN", "data_name=%s" % NAME,
            "data_path=%s" % data_path, "vocab_path=%s" % toy[0][2], "save_path=%s" % runs, "num_epochs=1", "batch_size=20", "val_step=100",
            "log_step=5", "workers=0", "img_dim=8", "embed_size=32", "word_dim=16", "max_violation=True", "seed=3", "learning_rate=0.002",
            "bi_gru=True"] + (["resident_data=True"] if resident else [])
    r = subprocess.run(args, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    run_dirs = glob.glob(os.path.join(runs, "SCAN", "toy_3_*"))
    assert len(run_dirs) == 1, run_dirs
    assert os.path.exists(os.path.join(run_dirs[0], 'model_best.pth.tar'))
    ck = torch.load(os.path.join(run_dirs[0], 'epo0_checkpoint.pth.tar'), map_location='cpu', weights_only=False)
    assert ck['Eiters'] == 10 and ck['_config']['resident_data'] is resident
    assert ("Data " in r.stderr) or ("Data " in r.stdout)          # the loop's data-time meter is logged


def _dp_run(tmp_path, toy_paths, tag, resident, port):
    out = str(tmp_path / ("%s.npz" % tag))
    env = dict(os.environ, ITR_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), WORKER, "--model", "SCAN", "--data-name", NAME, "--data-path", toy_paths[1], "--vocab-path", toy_paths[2],
           "--resident", str(int(resident)), "--out", out]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    z = np.load(out)
    assert int(z["world"]) == 2
    return z["losses"], z["params"], str(z["loader"])


def test_data_parallel_two_ranks(toy, tmp_path):
    """two gloo ranks on this GPU: every rank holds the whole split, draws the same global batches and shards them in train_emb"""
    runs = [_dp_run(tmp_path, toy[0], tag, resident, 29671 + k) for k, (tag, resident) in enumerate((("loader_1", 0), ("loader_2", 0), ("resident", 1)))]
    _check_parity(*runs)
