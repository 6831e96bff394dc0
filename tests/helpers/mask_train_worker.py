#!/usr/bin/env python3
"""Tiny configurations of the six model families (shaped like tests/helpers/dp_train_worker.py builds them) and batches whose `ids`
put two or three captions of one image into a batch, for the mask_same_image tests.

Imported (tests/test_train_mask_same_image_gpu.py): build_model / make_batch / colliding_ids / distinct_ids.
Run as a script (the data-parallel test): `model.train_emb` steps on seeded global batches with colliding ids (dense_ids), alone or as one rank of a
torch.distributed job (backend from ITR_DIST_BACKEND; gloo = several ranks on ONE GPU); rank 0 writes the per-step losses, gradient
norms, the first step's gradient and the final parameters to --out (npz)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if os.path.join(ROOT, "image-text-retrieval_amd") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "image-text-retrieval_amd"))
import numpy as np
import torch

IM_DIV = 5
LOSS_KEY = {'SAEM': 'Loss1', 'CAMERA': 'Rank_Loss', 'VSRN': 'Loss_retrieval'}      # the meter that holds the retrieval hinge alone


def build_model(name, files_dir, mask, cross_attn='t2i', module_name='SAF', im_div=IM_DIV):
    """-> (cfg, model) in training mode, seeded, every dropout site at p = 0 (two steps from the same seed are comparable bit for bit)."""
    from itr_amd import config as C
    from itr_amd.modalmodule import get_model
    from itr_amd.metricmodule.evaluation import LogCollector
    over = ['with', name, 'data_name=coco_precomp', 'bi_gru=True', 'max_violation=True', 'embed_size=256', 'word_dim=64',
            'mask_same_image=%s' % bool(mask)]
    if name == 'SCAN':
        over.append('cross_attn=' + cross_attn)
    if name == 'SGRAF':
        over.append('module_name=' + module_name)
    cfg = C.build_config(over)
    cfg['vocab_size'] = 500
    cfg['img_dim'] = 128
    if name == 'SGRAF':
        cfg.update(embed_size=32, word_dim=16, sim_dim=16, sgr_step=3, learning_rate=2e-3)
    if name in ('SAEM', 'CAMERA'):
        from itr_amd.modalmodule import bert
        os.makedirs(files_dir, exist_ok=True)
        bc = dict(vocab_size=500, hidden_size=32, num_hidden_layers=2, num_attention_heads=2, intermediate_size=64, max_position_embeddings=40,
                  type_vocab_size=2, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
        with open(os.path.join(files_dir, 'bert_config.json'), 'w') as f:
            json.dump(bc, f)
        with open(os.path.join(files_dir, 'trans_cfg.json'), 'w') as f:
            json.dump(dict(bc, num_hidden_layers=1, vocab_size=10), f)
        torch.manual_seed(99)
        bm = bert.BertModel(bert.BertConfig.from_dict(bc))
        for p_ in bm.parameters():
            p_.data.normal_(0, 0.05)
        torch.save(bm.state_dict(), os.path.join(files_dir, 'pytorch_model.bin'))
        cfg.update(bert_config_file=os.path.join(files_dir, 'bert_config.json'), init_checkpoint=os.path.join(files_dir, 'pytorch_model.bin'),
                   trans_cfg=os.path.join(files_dir, 'trans_cfg.json'), final_dims=32, embed_size=32, learning_rate=1e-3)
        if name == 'CAMERA':
            cfg.update(img_dim=24, head=2, smry_k=12, drop=0.0, smry_lamda=0.01)
    if name == 'VSRN':
        cfg.update(img_dim=20, embed_size=32, word_dim=12, vocab_size=40, dim_vid=32, dim_hidden=16, dim_word=10, max_len=8, input_dropout_p=0.0,
                   rnn_dropout_p=0.0, learning_rate=2e-3)
    torch.manual_seed(1234)
    model = get_model(cfg)
    if name == 'VSRN':
        model.caption_model.cuda()
    if name == 'SGRAF':
        model.txt_enc.dropout_p = 0.0
        for m_ in model.sim_enc.modules():
            if isinstance(m_, torch.nn.Dropout):
                m_.p = 0.0
    model.train_im_div = im_div
    model.train_start()
    model.logger = LogCollector()
    return cfg, model


def distinct_ids(B, rng):
    """caption ids of B different images"""
    return [int(5 * i + c) for i, c in zip(rng.permutation(4 * B)[:B], rng.randint(0, IM_DIV, size=B))]


def colliding_ids(B, rng):
    """distinct_ids, then two pairs and one triple of batch positions, no two of them adjacent, get captions of one image each.
    -> (ids, [positions of each group])"""
    ids = distinct_ids(B, rng)
    while True:
        at = [int(x) for x in rng.permutation(B)[:7]]
        sets = [at[0:2], at[2:4], at[4:7]]
        if all(abs(a - b) > 1 for s in sets for a in s for b in s if a != b):
            break
    for s in sets:
        img = ids[s[0]] // IM_DIV
        for k, pos in enumerate(s):
            ids[pos] = IM_DIV * img + (ids[s[0]] % IM_DIV + k) % IM_DIV
    return ids, sets


def dense_ids(B, rng):
    """B different captions of only B // 5 + 1 images: about an eighth of every row of the score matrix is masked, so that some
    row's or column's hardest negative is certainly among the masked entries (the data-parallel test needs the mask to matter)."""
    return [int(x) for x in rng.permutation(IM_DIV * (B // IM_DIV + 1))[:B]]


def make_batch(name, cfg, rng, B, ids):
    """One length-sorted global batch in the loaders' 8-tuple layout (host tensors; `ids` at position 5)."""
    lens = sorted([int(x) for x in rng.randint(3, 15, size=B)], reverse=True)
    if name == 'VSRN':      # the VSRN loader's layout: every caption padded to max_len + 1 ids, all "lengths" equal
        L = cfg['max_len'] + 1
        tok = torch.zeros(B, L, dtype=torch.long)
        mask = torch.zeros(B, L, dtype=torch.long)
        for b in range(B):
            l = int(rng.randint(3, L))
            tok[b, :l] = torch.from_numpy(rng.randint(1, 40, size=l))
            mask[b, :l] = 1
        feats = torch.from_numpy(rng.randn(B, 36, 20).astype(np.float32))
        return (feats, None, None, tok, [L] * B, list(ids), mask, None)
    if name in ('SAEM', 'CAMERA'):
        L = 14
        tok = torch.from_numpy(rng.randint(1, 500, size=(B, L)))
        mask = torch.zeros(B, L, dtype=torch.long)
        for b, l in enumerate(lens):
            mask[b, :l] = 1
            tok[b, l:] = 0
        types = torch.zeros(B, L, dtype=torch.long)
        if name == 'SAEM':
            feats = torch.from_numpy(rng.randn(B, 36, 128).astype(np.float32))
            feats = feats / feats.norm(dim=-1, keepdim=True)
            return (feats, None, None, tok, lens, list(ids), mask, types)
        feats = torch.from_numpy(rng.randn(B, 36, 24).astype(np.float32))
        wh = torch.from_numpy(rng.randint(200, 640, size=(B, 2)).astype(np.float32))
        xy = rng.rand(B, 36, 2, 2).astype(np.float32)
        xy.sort(axis=2)
        boxes = torch.from_numpy(np.concatenate([xy[:, :, 0], xy[:, :, 1]], -1)) * torch.cat([wh, wh], 1)[:, None, :]
        return (feats, boxes, wh, tok, lens, list(ids), mask, types)
    tok = torch.zeros(B, max(lens), dtype=torch.long)
    for b, l in enumerate(lens):
        tok[b, :l] = torch.from_numpy(rng.randint(4, 500, size=l))
    feats = torch.from_numpy(rng.randn(B, 36, 128).astype(np.float32))
    feats = feats / feats.norm(dim=-1, keepdim=True)
    return (feats, None, None, tok, lens, list(ids), None, None)


def flat_params(model):
    return torch.cat([p.detach().reshape(-1) for p in model.params if p.requires_grad])


def main():
    import torch.distributed as dist
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="SCAN")
    ap.add_argument("--cross-attn", default="t2i")
    ap.add_argument("--batch", type=int, default=24)
    ap.add_argument("--steps", type=int, default=1)
    ap.add_argument("--no-mask", action="store_true")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    backend = os.environ.get("ITR_DIST_BACKEND", "nccl")
    torch.cuda.set_device(0 if backend == "gloo" else int(os.environ.get("LOCAL_RANK", "0")))
    if world > 1:
        dist.init_process_group(backend)
    cfg, model = build_model(a.model, a.out + ".files_rank%s" % os.environ.get("RANK", "0"), not a.no_mask, cross_attn=a.cross_attn)
    rng = np.random.RandomState(7)
    losses, hinges, gnorms, grads1 = [], [], [], []
    for _ in range(a.steps):
        ids = dense_ids(a.batch, rng)
        model.train_emb(make_batch(a.model, cfg, rng, a.batch, ids))
        meters = model.logger.meters
        losses.append(float(meters['Loss1'].val) + float(meters['Loss2'].val) if a.model == 'SAEM' else float(meters['Loss'].val))
        hinges.append(float(meters[LOSS_KEY.get(a.model, 'Loss')].val))
        gnorms.append(float(model.optimizer.last_grad_norm[0]))
        if not grads1:     # the (summed, unclipped) gradient of the first step, as Adam.step saw it
            grads1.append(torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).detach().reshape(-1) for p in model.params
                                     if p.requires_grad]).cpu().numpy())
    torch.cuda.synchronize()
    if world == 1 or dist.get_rank() == 0:
        comm = model.optimizer.comm
        np.savez(a.out, dp_world=(comm.world if comm is not None else 1), params=flat_params(model).cpu().numpy(), grads1=grads1[0],
                 losses=np.asarray(losses), hinges=np.asarray(hinges), gnorms=np.asarray(gnorms), lr=cfg['learning_rate'])
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
