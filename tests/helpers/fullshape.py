"""Weights, batches and the oracle's training step at the benchmarked training shapes (tools/train_bench.py): batch 128, 36 x 2048
region features, the COCO vocabulary, word_dim 300, embed 1024, a bi-GRU, sim_dim 256.  Everything is generated on the host from a
fixed seed, so the oracle side of tests/test_train_fullshape_gpu.py can be prepared without a GPU."""
import math

import numpy as np
import torch

import itr_oracle as O

V_COCO, WORD_DIM, EMBED, IMG_DIM, REGIONS, SIM_DIM, BATCH = 11353, 300, 1024, 2048, 36, 256, 128

# (model, options) as the test names them; every one also gets data_name=coco_precomp, bi_gru=True, max_violation=True
CONFIGS = {
    'VSEPP': ('VSE_PP', []),
    'SCAN-t2i': ('SCAN', []),       # the named config: clipped_l2norm, LogSumExp, lambda_lse 6, lambda_softmax 9
    'SCAN-i2t': ('SCAN', ['cross_attn=i2t', 'agg_func=Mean', 'lambda_softmax=4']),
    'SGRAF-SAF': ('SGRAF', ['module_name=SAF']),
    'SGRAF-SGR': ('SGRAF', ['module_name=SGR', 'sgr_step=3']),
}


def config(name):
    from itr_amd import config as C
    model, opts = CONFIGS[name]
    cfg = C.build_config(['with', model, 'data_name=coco_precomp', 'bi_gru=True', 'max_violation=True'] + opts)
    cfg['vocab_size'] = V_COCO
    cfg['img_dim'] = IMG_DIM
    return cfg


def make_batch(kind, seed, B=BATCH):
    """kind 'A': train_bench.make_batches' shape -- 6..20 words, ids in [4, V), l2-normalised N(0, 1) 36 x 2048 features.
    kind 'B': the same with 12 captions of 33..64 words and two of 70 and 82 (the longest Flickr30k caption).
    -> (feats (B, 36, 2048) fp32, ids (B, max len) int64, lens sorted longest first)."""
    rng = np.random.RandomState(seed)
    lens = [int(x) for x in rng.randint(6, 21, size=B)]
    if kind == 'B':
        lens[:12] = [int(x) for x in rng.randint(33, 65, size=12)]
        lens[12:14] = [70, 82]
    elif kind != 'A':
        raise ValueError(kind)
    lens = sorted(lens, reverse=True)
    ids = torch.zeros(B, max(lens), dtype=torch.long)
    for b, l in enumerate(lens):
        ids[b, :l] = torch.from_numpy(rng.randint(4, V_COCO, size=l))
    g = torch.Generator().manual_seed(seed)
    feats = O.l2norm(torch.randn(B, REGIONS, IMG_DIM, generator=g), -1)
    return feats, ids, lens


def make_weights(cfg, seed):
    """The reference's initial scales: Xavier-uniform fc with zero bias, embedding U(+-0.1), GRU U(+-1/sqrt(D)), and for SGRAF the
    similarity module of tests/helpers/sgraf_weights.  -> [img_enc, txt_enc(, sim_enc)] state dicts (fp32)."""
    g = torch.Generator().manual_seed(seed)
    u = lambda shape, r: (torch.rand(*shape, generator=g) * 2 - 1) * r
    r = math.sqrt(6.0 / (IMG_DIM + EMBED))
    wi = {'fc.weight': u((EMBED, IMG_DIM), r), 'fc.bias': torch.zeros(EMBED)}
    wt = {'embed.weight': u((V_COCO, WORD_DIM), 0.1)}
    k = 1.0 / math.sqrt(EMBED)
    for suf in ('', '_reverse'):
        wt['rnn.weight_ih_l0' + suf] = u((3 * EMBED, WORD_DIM), k)
        wt['rnn.weight_hh_l0' + suf] = u((3 * EMBED, EMBED), k)
        wt['rnn.bias_ih_l0' + suf] = u((3 * EMBED,), k)
        wt['rnn.bias_hh_l0' + suf] = u((3 * EMBED,), k)
    if cfg['name'] != 'SGRAF':
        return [wi, wt]
    import sgraf_weights
    drop = 'SGR_module.' if cfg['module_name'] == 'SAF' else 'SAF_module.'
    ws = {k: v for k, v in sgraf_weights.make(EMBED, SIM_DIM, cfg['sgr_step'], seed=seed + 1).items() if not k.startswith(drop)}
    for k in [k for k in ws if k.endswith('.running_mean')]:
        ws[k[:-len('running_mean')] + 'num_batches_tracked'] = torch.tensor(0)
    return [wi, wt, ws]


def oracle_step(cfg, weights, batch, dtype):
    """The oracle's train_emb restatement in `dtype` on the host: gru_model_train_step (VSE++, SCAN) or sgraf_model_train_grads.
    -> dict(loss, grads {'txt.<k>' | 'img.<k>' | 'sim.<k>': clipped gradient}, grad_norm (before clipping), scores, bn_stats)."""
    feats, ids, lens = batch
    cast = lambda d: {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in d.items()}
    out = {}
    model = cfg['name']
    if model == 'SGRAF':
        wi, wt, ws = [cast(d) for d in weights]
        loss, grads = O.sgraf_model_train_grads(wi, wt, ws, feats.to(dtype), ids, lens, cfg, out=out)
    else:
        wi, wt = [cast(d) for d in weights]
        loss, grads, _, _, _ = O.gru_model_train_step(model, wi, wt, feats.to(dtype), ids, lens, cfg, out=out)
    return dict(loss=float(loss), grads=grads, grad_norm=float(out['grad_norm']), scores=out['scores'], bn_stats=out.get('bn_stats'))


def replay_bn(buffers, bn_stats, momentum=0.1):
    """torch BatchNorm's running-statistic updates, one per recorded call in call order, in the dtype of `bn_stats`:
    running = (1 - momentum) running + momentum batch, the variance unbiased by N / (N - 1).  -> {'<bn>.running_mean' | ... : tensor}."""
    out = {k: v.to(bn_stats[0][1].dtype).clone() if v.is_floating_point() else int(v) for k, v in buffers.items()}
    for p, mean, var, n in bn_stats:
        out[p + '.running_mean'] = (1 - momentum) * out[p + '.running_mean'] + momentum * mean
        out[p + '.running_var'] = (1 - momentum) * out[p + '.running_var'] + momentum * var * (n / (n - 1.0))
        out[p + '.num_batches_tracked'] += 1
    return out


def flip_margin(scores, margin=0.2):
    """Distance of the max-violation hinge from a discrete change: per row and per column of `scores`, the gap between the two
    hardest negatives, and |margin + hardest negative - positive| (the hinge's kink).  -> the smallest over all 2B of them."""
    S = scores.double()
    n = S.shape[0]
    off = S.masked_fill(torch.eye(n, dtype=torch.bool), float('-inf'))
    d = S.diag()
    worst = float('inf')
    for M in (off, off.t()):           # rows: an image against its captions; columns (as rows of the transpose): a caption's images
        top = M.topk(2, dim=1).values
        worst = min(worst, float((top[:, 0] - top[:, 1]).min()), float((margin + top[:, 0] - d).abs().min()))
    return worst
