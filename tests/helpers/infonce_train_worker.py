#!/usr/bin/env python3
"""`loss=infonce` through `model.train_emb`: the tiny configurations, batches and ids of tests/helpers/mask_train_worker.py with the
ranking loss switched.

Imported (tests/test_train_infonce_gpu.py): build_model_with_loss -- a model built from a configuration that carries the loss keys
from the start, so that its criterion is the InfoNCE one.
Run as a script (the data-parallel test): `model.train_emb` steps on seeded global batches with colliding ids (dense_ids) and
mask_same_image on, alone or as one rank of a torch.distributed job (backend from ITR_DIST_BACKEND; gloo = several ranks on ONE GPU);
rank 0 writes the per-step losses, gradient norms, the first step's gradient and the final parameters to --out (npz)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mask_train_worker as W  # noqa: E402  (puts the package on sys.path)
import numpy as np  # noqa: E402
import torch  # noqa: E402


def build_model_with_loss(name, files_dir, mask, loss, temperature=None, **kw):
    """mask_train_worker.build_model with `loss=<loss>` (and `temperature=...`) among the configuration's command-line updates, i.e.
    in the configuration before the model and its criterion are built."""
    from itr_amd import config as C
    extra = ['loss=%s' % loss] + ([] if temperature is None else ['temperature=%r' % temperature])
    build_config = C.build_config
    C.build_config = lambda argv: build_config(list(argv) + extra)
    try:
        return W.build_model(name, files_dir, mask, **kw)
    finally:
        C.build_config = build_config


def main():
    import torch.distributed as dist
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="SCAN")
    ap.add_argument("--cross-attn", default="t2i")
    ap.add_argument("--batch", type=int, default=24)
    ap.add_argument("--steps", type=int, default=1)
    ap.add_argument("--loss", default="infonce", choices=["hinge", "infonce"])
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    backend = os.environ.get("ITR_DIST_BACKEND", "nccl")
    torch.cuda.set_device(0 if backend == "gloo" else int(os.environ.get("LOCAL_RANK", "0")))
    if world > 1:
        dist.init_process_group(backend)
    cfg, model = build_model_with_loss(a.model, a.out + ".files_rank%s" % os.environ.get("RANK", "0"), True, a.loss, cross_attn=a.cross_attn)
    assert model.config['loss'] == a.loss
    rng = np.random.RandomState(7)
    losses, retrieval, gnorms, grads1 = [], [], [], []
    for _ in range(a.steps):
        ids = W.dense_ids(a.batch, rng)
        model.train_emb(W.make_batch(a.model, cfg, rng, a.batch, ids))
        meters = model.logger.meters
        losses.append(float(meters['Loss1'].val) + float(meters['Loss2'].val) if a.model == 'SAEM' else float(meters['Loss'].val))
        retrieval.append(float(meters[W.LOSS_KEY.get(a.model, 'Loss')].val))
        gnorms.append(float(model.optimizer.last_grad_norm[0]))
        if not grads1:     # the (summed, unclipped) gradient of the first step, as Adam.step saw it
            grads1.append(torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).detach().reshape(-1) for p in model.params
                                     if p.requires_grad]).cpu().numpy())
    torch.cuda.synchronize()
    if world == 1 or dist.get_rank() == 0:
        comm = model.optimizer.comm
        np.savez(a.out, dp_world=(comm.world if comm is not None else 1), params=W.flat_params(model).cpu().numpy(), grads1=grads1[0],
                 losses=np.asarray(losses), retrieval=np.asarray(retrieval), gnorms=np.asarray(gnorms), lr=cfg['learning_rate'])
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
