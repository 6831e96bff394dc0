#!/usr/bin/env python3
"""Worker of tests/test_resident_loader_gpu.py: one epoch of `utils.train_step` over `data_loader.get_loaders`' train loader
(the DataLoader path, or the device-resident one with --resident 1), alone or as one rank of a torch.distributed job
(backend from ITR_DIST_BACKEND; gloo = several ranks on ONE GPU).  Rank 0 writes the per-step losses and the final
parameters to --out (npz)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "image-text-retrieval_amd"))
import numpy as np
import torch
import torch.distributed as dist


def run_epoch(model_name, data_name, data_path, vocab_path, resident, seed=3, batch_size=7):
    """-> (per-step losses, flat final parameters, type name of the train loader)"""
    from itr_amd import config as C, utils
    from itr_amd.datamodule import data_loader as dl
    from itr_amd.modalmodule import get_model
    cfg = C.build_config(['with', model_name, 'data_name=%s' % data_name, 'data_path=%s' % data_path, 'vocab_path=%s' % vocab_path,
                          'vocab_type=json', 'bi_gru=True', 'max_violation=True', 'seed=%d' % seed, 'batch_size=%d' % batch_size, 'workers=0',
                          'img_dim=8', 'embed_size=32', 'word_dim=16', 'learning_rate=0.002', 'val_step=1000000', 'log_step=1000000',
                          'resident_data=%s' % bool(resident)])
    utils.setup_seed(cfg['seed'])
    train_loader, val_loader, cfg['vocab_size'] = dl.get_loaders(cfg['data_name'], cfg['batch_size'], cfg['workers'], cfg)
    model = get_model(cfg).cuda()
    losses, step = [], model.train_emb

    def recording_step(batch, *a, **k):
        step(batch, *a, **k)
        losses.append(float(model.logger.meters['Loss'].val))
    model.train_emb = recording_step
    utils.train_step(cfg, train_loader, model, 0, val_loader)
    torch.cuda.synchronize()
    flat = torch.cat([p.detach().reshape(-1) for p in model.params if p.requires_grad]).cpu().numpy()
    return np.asarray(losses, dtype=np.float64), flat, type(train_loader).__name__


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="SCAN")
    ap.add_argument("--data-name", required=True)
    ap.add_argument("--data-path", required=True)
    ap.add_argument("--vocab-path", required=True)
    ap.add_argument("--resident", type=int, default=0)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    torch.cuda.set_device(0)
    if world > 1:
        dist.init_process_group(os.environ.get("ITR_DIST_BACKEND", "nccl"))
    losses, flat, kind = run_epoch(a.model, a.data_name, a.data_path, a.vocab_path, a.resident)
    if world == 1 or dist.get_rank() == 0:
        np.savez(a.out, losses=losses, params=flat, loader=kind, world=world)
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()
