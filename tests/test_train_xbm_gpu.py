"""GPU: `memory_bank=M` through `train_emb` of the three families that have a cross-batch memory (VSE++, SAEM, VSRN; the tiny
configurations of tests/helpers/mask_train_worker.py), for both losses, and through the command line.

Four steps under spies with memory_bank=32, memory_start=0 and batches of 10-12: the first step finds the memory empty and calls the
plain loss; steps 2-4 call the xbm op with n = B, 2B, min(3B, 32) memory slots.  The captured (S, R, C, groups) give the float64
helper's loss (tests/helpers/xbm_oracle.py) within 1e-4 * max(1, loss64), the sibling tests' bound for the same quantity
(test_train_infonce_gpu.py); the memory holds the operands of the pair function in ring order; the parameters move."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import mask_train_worker as W  # noqa: E402
import xbm_oracle as X  # noqa: E402
from itr_amd import ops  # noqa: E402
from itr_amd.modalmodule import Models  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = [("VSE_PP", 12), ("SAEM", 11), ("VSRN", 10)]
M = 32
NAMES = ("hinge_loss", "infonce_loss", "xbm_hinge_loss", "xbm_infonce_loss")


class Spies(object):
    """the four loss ops replaced by recording wrappers, and the operands every step hands to base_module._hinge_memory"""

    def __init__(self, model):
        self.model = model

    def __enter__(self):
        self.calls, self.operands = [], []
        self._ops = {k: getattr(ops, k) for k in NAMES}
        for name in NAMES:
            setattr(ops, name, self._wrap(name))
        inner = self.model._hinge_memory

        def hinge_memory(img, cap, scores, ids, pair_fn, *a, **k):
            self.operands.append((img.detach().clone(), cap.detach().clone(), np.asarray(ids)))
            return inner(img, cap, scores, ids, pair_fn, *a, **k)
        self.model._hinge_memory = hinge_memory
        return self

    def _wrap(self, name):
        def spy(*a, **k):
            loss = self._ops[name](*a, **k)
            tensors = [t.detach().double().cpu() for t in a if torch.is_tensor(t) and t.is_floating_point()]
            ints = [t.detach().cpu().clone() for t in a if torch.is_tensor(t) and not t.is_floating_point()]      # (views of the memory: copied now)
            self.calls.append(dict(op=name, tensors=tensors, ints=ints, args=a, kwargs=dict(k), loss=float(loss.detach())))
            return loss
        return spy

    def __exit__(self, *exc):
        for name in NAMES:
            setattr(ops, name, self._ops[name])
        del self.model._hinge_memory


def build(name, tmp_path, loss, memory_bank=M, memory_start=0):
    cfg, model = W.build_model(name, str(tmp_path / "files"), False)
    assert cfg['memory_bank'] == 0 and cfg['memory_start'] == 0
    model.config.update(loss=loss, memory_bank=memory_bank, memory_start=memory_start)          # read at call time
    return cfg, model


def steps(name, cfg, model, B, count, seed=5):
    rng = np.random.RandomState(seed)
    all_ids = []
    for _ in range(count):
        ids = W.distinct_ids(B, rng)
        all_ids.append(ids)
        model.train_emb(W.make_batch(name, cfg, rng, B, ids))
    torch.cuda.synchronize()
    return all_ids


def want_loss(call, loss, cfg):
    S, R, C = (t.float() for t in call['tensors'][:3])
    groups, bank_groups = np.asarray(call['args'][3]), call['ints'][0].numpy()
    mask_batch = call['kwargs']['mask_batch']
    if loss == 'infonce':
        return float(X.infonce_parts(S, R, C, groups, bank_groups, X.scale_of(0.05), mask_batch)[0]), groups, bank_groups
    return float(X.hinge_loss(S, R, C, groups, bank_groups, cfg['margin'], True, mask_batch)), groups, bank_groups


@pytest.mark.parametrize("loss", ["hinge", "infonce"])
@pytest.mark.parametrize("name,B", FAMILIES, ids=[n for n, _ in FAMILIES])
def test_four_steps(tmp_path, dev, name, B, loss):
    cfg, model = build(name, tmp_path, loss)
    before = W.flat_params(model).clone()
    with Spies(model) as spy:
        all_ids = steps(name, cfg, model, B, 4)
    plain, xbm = ('infonce_loss', 'xbm_infonce_loss') if loss == 'infonce' else ('hinge_loss', 'xbm_hinge_loss')
    assert [c['op'] for c in spy.calls] == [plain, xbm, xbm, xbm]
    assert tuple(spy.calls[0]['tensors'][0].shape) == (B, B)
    dropped = 0
    for step, call in enumerate(spy.calls[1:], start=2):
        n = min((step - 1) * B, M)
        S, R, C = call['tensors'][:3]
        assert tuple(S.shape) == (B, B) and tuple(R.shape) == (B, n) and tuple(C.shape) == (n, B)
        want, groups, bank_groups = want_loss(call, loss, cfg)
        assert groups.tolist() == (np.asarray(all_ids[step - 1]) // W.IM_DIV).tolist() and call['kwargs'] == {'mask_batch': False}
        assert call['args'][5:] == ((0.05,) if loss == 'infonce' else (cfg['margin'], True))
        print("\n%s %s step %d: n = %d, loss %.6f, float64 on the captured matrices %.6f" % (name, loss, step, n, call['loss'], want))
        assert abs(call['loss'] - want) <= 1e-4 * max(1.0, want)
        dropped += int((groups[:, None] == bank_groups[None, :]).sum())
    assert dropped >= 1          # some stored caption was of a query's own image, and was no negative
    logged = float(model.logger.meters[W.LOSS_KEY.get(name, 'Loss')].val)
    assert logged == spy.calls[-1]['loss']
    # the memory: the operands of the pair function, in ring order
    slots = [None] * M
    head = 0
    for img, cap, ids in spy.operands:
        for r in range(B):
            slots[(head + r) % M] = (img[r], cap[r], int(ids[r]) // W.IM_DIV)
        head = (head + B) % M
    v_img, v_cap, v_group = model.memory.view()
    assert len(model.memory) == M and model.memory.pushed == 4 * B and model.memory.head == head
    assert torch.equal(v_img, torch.stack([s[0] for s in slots])) and torch.equal(v_cap, torch.stack([s[1] for s in slots]))
    assert v_group.cpu().tolist() == [s[2] for s in slots]
    if name == 'SAEM':          # the renormalised rows that enter the cosine, not the towers' outputs
        assert float((v_img.norm(dim=1) - 1).abs().max()) < 1e-5 and float((v_cap.norm(dim=1) - 1).abs().max()) < 1e-5
    after = W.flat_params(model)
    assert torch.isfinite(after).all() and float((after - before).abs().max()) > 0.0
    del model
    torch.cuda.empty_cache()


def test_memory_start_delays_the_use_and_a_loaded_state_empties_the_memory(tmp_path, dev):
    name, B = "VSE_PP", 12
    cfg, model = build(name, tmp_path, 'hinge', memory_start=2)
    with Spies(model) as spy:
        steps(name, cfg, model, B, 3)
    assert [c['op'] for c in spy.calls] == ['hinge_loss', 'hinge_loss', 'xbm_hinge_loss']          # Eiters = 3 > memory_start
    assert tuple(spy.calls[2]['tensors'][1].shape) == (B, 2 * B)                                     # pushed from the first step on
    assert len(model.memory) == M
    model.load_state_dict(model.state_dict())
    assert len(model.memory) == 0 and model.memory.pushed == 0
    with Spies(model) as spy:
        steps(name, cfg, model, B, 2, seed=6)
    assert [c['op'] for c in spy.calls] == ['hinge_loss', 'xbm_hinge_loss'] and tuple(spy.calls[1]['tensors'][1].shape) == (B, B)
    # mask_same_image reaches the op as mask_batch
    model.config['mask_same_image'] = True
    with Spies(model) as spy:
        steps(name, cfg, model, B, 1, seed=7)
    assert spy.calls[0]['op'] == 'xbm_hinge_loss' and spy.calls[0]['kwargs'] == {'mask_batch': True}
    # switched off again: the step as it was
    model.config.update(memory_bank=0, mask_same_image=False)
    with Spies(model) as spy:
        steps(name, cfg, model, B, 1, seed=8)
    assert [c['op'] for c in spy.calls] == ['hinge_loss'] and spy.calls[0]['args'][1:] == (cfg['margin'], True) and spy.calls[0]['kwargs'] == {}
    del model
    torch.cuda.empty_cache()


def test_refusals(tmp_path, dev):
    for cls in (Models.SCAN, Models.SGRAF, Models.CAMERA):
        with pytest.raises(ValueError, match="has no cross-batch memory"):
            cls(dict(memory_bank=32))
    for bad in (dict(memory_bank=-1), dict(memory_start=-1)):
        with pytest.raises(ValueError, match="non-negative integer"):
            Models.VSE_PP(bad)
    with pytest.raises(ValueError, match="smaller than batch_size"):
        Models.VSE_PP(dict(memory_bank=64, batch_size=128))
    name, B = "VSE_PP", 12
    cfg, model = build(name, tmp_path, 'hinge', memory_bank=8)
    with pytest.raises(ValueError, match="smaller than the batch"):
        steps(name, cfg, model, B, 1)
    model.config['memory_bank'] = M
    model.train_im_div = None
    with pytest.raises(ValueError, match="train_im_div"):
        steps(name, cfg, model, B, 1)
    model.train_im_div = W.IM_DIV

    class LiveComm(object):
        on, world, rank = True, 2, 0
    t = torch.zeros(B, B, device=dev)
    with pytest.raises(ValueError, match="data parallelism"):
        model._hinge_memory(t, t, t, list(range(B)), None, None, LiveComm())
    del model
    torch.cuda.empty_cache()


def test_train_and_test_command_line(golden, tmp_path):
    """`python train.py with VSE_PP memory_bank=64 memory_start=2 num_epochs=1 ...` on a synthetic precomp directory trains and
    writes its best checkpoint with the keys in its configuration; `python test.py` evaluates that checkpoint."""
    g = golden("g14_data_layer")
    name = 'toy_precomp'
    d = tmp_path / 'data' / name
    d.mkdir(parents=True)
    caps = bytes(g["caps_blob"]).split(b"\n")[:-1]
    rng = np.random.RandomState(0)
    for split, n_img in (('train', 40), ('dev', 1000)):
        np.save(d / ('%s_ims.npy' % split), rng.randn(n_img, 36, 8).astype(np.float32))
        (d / ('%s_caps.txt' % split)).write_bytes(b"\n".join(caps[i % len(caps)] for i in range(5 * n_img)) + b"\n")
    vdir = tmp_path / 'vocab'
    vdir.mkdir()
    (vdir / ('%s_vocab.json' % name)).write_text(bytes(g["vocab_json"]).decode())
    runs = str(tmp_path / 'runs')
    pkg = os.path.join(ROOT, "image-text-retrieval_amd")
    args = [sys.executable, os.path.join(pkg, "train.py"), "with", "VSE_PP", "memory_bank=64", "memory_start=2", "num_epochs=1",
            "data_name=%s" % name, "data_path=%s" % (tmp_path / 'data'), "vocab_path=%s" % vdir, "vocab_type=json", "save_path=%s" % runs,
            "batch_size=20", "val_step=100", "log_step=5", "workers=0", "img_dim=8", "embed_size=32", "word_dim=16", "seed=3",
            "learning_rate=0.002"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    run_dirs = glob.glob(os.path.join(runs, "VSE_PP", "toy_3_*"))
    assert len(run_dirs) == 1, run_dirs
    best = os.path.join(run_dirs[0], 'model_best.pth.tar')
    ck = torch.load(best, map_location='cpu', weights_only=False)
    assert ck['_config']['memory_bank'] == 64 and ck['_config']['memory_start'] == 2 and ck['Eiters'] == 10
    r = subprocess.run([sys.executable, os.path.join(pkg, "test.py"), best, "--split", "dev", "--data-path", str(tmp_path / 'data')],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert os.path.exists(os.path.join(run_dirs[0], '%s_single_result.yaml' % name))
