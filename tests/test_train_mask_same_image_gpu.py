"""GPU: `mask_same_image=True` through one `train_emb` step of each of the six model families (tiny configurations, shaped like
tests/helpers/dp_train_worker.py builds them), and through the data-parallel step.

One process, with a spy on ops.hinge_loss (as test_train_fullshape_gpu.py does): the groups that reach the hinge are ids // 5 in the
row order of the captured score matrix; the step's loss is the float64 helper's on that matrix (1e-4 * max(1, loss64), the bound of
test_kernels_gpu.py::test_hinge_random); with the switch off the hinge is called exactly as before; with the switch on and no two
captions of one image in the batch the parameters after the step are those of the switch-off step, bit for bit; the switch without
`train_im_div` is refused.

Data parallel (the gloo harness of test_dp_train_gpu.py: 2 and 3 ranks on the one GPU): first-step gradients, losses and gradient
norms of the masked step agree with the single-process run under that file's tolerances for the same quantities (2e-5 relative
gradient norm, rtol 2e-5 losses, rtol 1e-4 norms) -- and the single-process run differs from a switch-off run of the same batches,
so the comparison cannot pass with the mask dropped on both sides."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import hinge_groups_oracle as H  # noqa: E402
import mask_train_worker as W  # noqa: E402
from itr_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "helpers", "mask_train_worker.py")
FAMILIES = [("VSE_PP", {}, 12), ("SCAN", {"cross_attn": "t2i"}, 12), ("SCAN", {"cross_attn": "i2t"}, 12), ("SGRAF", {"module_name": "SAF"}, 10),
            ("SGRAF", {"module_name": "SGR"}, 10), ("SAEM", {}, 11), ("CAMERA", {}, 10), ("VSRN", {}, 10)]


def one_step(name, kw, B, files, mask, ids, im_div=W.IM_DIV):
    cfg, model = W.build_model(name, files, mask, im_div=im_div, **kw)
    batch = W.make_batch(name, cfg, np.random.RandomState(11), B, ids)
    seen, hinge = [], ops.hinge_loss

    def spy(scores, *a, **k):
        loss = hinge(scores, *a, **k)
        seen.append(dict(scores=scores.detach().double().cpu(), args=a, kwargs=dict(k), loss=float(loss.detach())))
        return loss
    ops.hinge_loss = spy
    try:
        model.train_emb(batch)
    finally:
        ops.hinge_loss = hinge
    torch.cuda.synchronize()
    out = dict(cfg=cfg, seen=seen, hinge=float(model.logger.meters[W.LOSS_KEY.get(name, 'Loss')].val), params=W.flat_params(model).cpu())
    del model
    torch.cuda.empty_cache()
    return out


@pytest.mark.parametrize("name,kw,B", FAMILIES, ids=["%s%s" % (n, "".join("-" + v for v in k.values())) for n, k, _ in FAMILIES])
def test_one_step(tmp_path, dev, name, kw, B):
    files = str(tmp_path / "files")
    ids, sets = W.colliding_ids(B, np.random.RandomState(5))
    groups = np.asarray(ids) // W.IM_DIV
    assert len(sets) == 3 and all(len(set(groups[s])) == 1 for s in sets) and len(set(groups)) == B - 4
    assert all(abs(a - b) > 1 for s in sets for a in s for b in s if a != b)            # not next to each other in the sorted batch

    on = one_step(name, kw, B, files, True, ids)
    assert len(on['seen']) == 1
    call = on['seen'][0]
    assert call['args'] == (on['cfg']['margin'], True) and list(call['kwargs']) == ['groups']
    assert np.asarray(call['kwargs']['groups']).tolist() == groups.tolist()              # one process: the batch order
    assert tuple(call['scores'].shape) == (B, B)
    want, _ = H.hinge_groups_loss_and_grad(call['scores'], groups, on['cfg']['margin'], True)
    unmasked = float(H.hinge_groups_loss(call['scores'], np.arange(B), on['cfg']['margin'], True))
    print("\n%s %s: hinge %.6f, float64 on the captured matrix %.6f (unmasked %.6f)" % (name, kw, call['loss'], float(want), unmasked))
    assert abs(call['loss'] - float(want)) <= 1e-4 * max(1.0, float(want))
    assert on['hinge'] == call['loss']

    distinct = W.distinct_ids(B, np.random.RandomState(5))
    assert len(set(np.asarray(distinct) // W.IM_DIV)) == B
    off = one_step(name, kw, B, files, False, distinct)
    assert len(off['seen']) == 1 and off['seen'][0]['kwargs'] == {} and off['seen'][0]['args'] == (off['cfg']['margin'], True)
    on_distinct = one_step(name, kw, B, files, True, distinct)
    assert list(on_distinct['seen'][0]['kwargs']) == ['groups']
    assert torch.equal(on_distinct['params'].view(torch.int32), off['params'].view(torch.int32))
    assert on_distinct['seen'][0]['loss'] == off['seen'][0]['loss']

    with pytest.raises(ValueError, match="train_im_div"):
        one_step(name, kw, B, files, True, ids, im_div=None)


# ------------------------------------------------------------------------------------------ data parallel
def _run(tmp_path, tag, world, extra):
    out = str(tmp_path / ("%s_%d.npz" % (tag, world)))
    args = [WORKER, "--out", out] + extra
    if world == 1:
        cmd, env = [sys.executable] + args, dict(os.environ)
    else:
        env = dict(os.environ, ITR_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
               "--master-addr", "127.0.0.1", "--master-port", str(29710 + world)] + args
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return np.load(out)


@pytest.mark.parametrize("extra,world", [
    (["--model", "VSE_PP"], 2),
    (["--model", "SCAN", "--cross-attn", "t2i", "--batch", "25"], 3),      # ragged shards: 9 / 8 / 8 rows
    (["--model", "SAEM", "--batch", "11"], 2),                             # the family that reorders ids for its own use
])
def test_dp_masked_step_equals_single_process(tmp_path, extra, world):
    one = _run(tmp_path, "one", 1, extra)
    off = _run(tmp_path, "off", 1, extra + ["--no-mask"])
    dp = _run(tmp_path, "dp", world, extra)
    assert int(one["dp_world"]) == 1 and int(dp["dp_world"]) == world
    # the mask is live: the same batches without it give another hinge and another gradient
    assert abs(float(one["hinges"][0]) - float(off["hinges"][0])) > 1e-3 * abs(float(off["hinges"][0])), (one["hinges"], off["hinges"])
    assert np.linalg.norm(one["grads1"] - off["grads1"]) > 1e-3 * np.linalg.norm(off["grads1"])
    g1, g2 = one["grads1"], dp["grads1"]
    rel = np.linalg.norm(g1 - g2) / np.linalg.norm(g1)
    print("\n%s on %d ranks: first-step gradient differs by %.2e (relative), losses %s vs %s, norms %s vs %s" % (
        extra, world, rel, dp["losses"][:1], one["losses"][:1], dp["gnorms"][:1], one["gnorms"][:1]))
    assert g1.shape == g2.shape and rel <= 2e-5, rel
    np.testing.assert_allclose(dp["losses"][:1], one["losses"][:1], rtol=2e-5)
    np.testing.assert_allclose(dp["hinges"][:1], one["hinges"][:1], rtol=2e-5)
    np.testing.assert_allclose(dp["gnorms"][:1], one["gnorms"][:1], rtol=1e-4)
