"""Weights, batches and the oracle's training step at the benchmarked training shapes (tools/train_bench.py): batch 128, 36 x 2048
region features, the COCO vocabulary, word_dim 300, embed 1024, a bi-GRU, sim_dim 256; VSRN with its own configuration (embed 2048,
a one-way text GRU, the captioning model with dim_hidden 512 and 61-id captions).  Everything is generated on the host from a
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
    'VSRN': ('VSRN', ['input_dropout_p=0.0', 'rnn_dropout_p=0.0']),     # embed 2048, dim_hidden 512, max_len 60; bi_gru is not read
}
VSRN_IDS = 61           # the loader's VSRN captions: max_len + 1 ids (data_loader.py:117-125)


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
    kind 'VSRN': train_bench's VSRN layout -- kind A's words in front of zeros, VSRN_IDS ids per caption, the mask on the first 60.
    -> (feats (B, 36, 2048) fp32, ids (B, max len) int64, lens sorted longest first[, mask (B, VSRN_IDS) fp32 for 'VSRN'])."""
    if kind == 'VSRN':
        feats, ids, lens = make_batch('A', seed, B)
        vid = torch.zeros(B, VSRN_IDS, dtype=torch.long)
        vid[:, :ids.shape[1]] = ids
        mask = torch.zeros(B, VSRN_IDS)
        mask[:, :VSRN_IDS - 1] = 1
        return feats, vid, [VSRN_IDS] * B, mask
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
    similarity module of tests/helpers/sgraf_weights.  -> [img_enc, txt_enc(, sim_enc)] state dicts (fp32).  VSRN: vsrn_weights."""
    g = torch.Generator().manual_seed(seed)
    u = lambda shape, r: (torch.rand(*shape, generator=g) * 2 - 1) * r
    if cfg['name'] == 'VSRN':
        return vsrn_weights(cfg, g, u)
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


def _gru(w, pre, n_in, H, u):
    k = 1.0 / math.sqrt(H)
    w.update({pre + 'weight_ih_l0': u((3 * H, n_in), k), pre + 'weight_hh_l0': u((3 * H, H), k), pre + 'bias_ih_l0': u((3 * H,), k),
              pre + 'bias_hh_l0': u((3 * H,), k)})


def vsrn_weights(cfg, g, u):
    """VSRN's initial scales (ImgEncoder.py:166-197, vsrn_.py, TextEncoder.py, Fusionmodule.py:147-365): fc Xavier-uniform with zero
    bias; Conv1d / Linear weights and biases U(+-1/sqrt(fan_in)) (torch's defaults); GRUs U(+-1/sqrt(H)); text embedding U(+-0.1),
    decoder embedding N(0, 1); vid2hid and decoder.out Xavier-normal.  The GCN BatchNorms start at gamma = beta = 0 in the reference,
    which makes every Rs_GCN an identity with no gradient into it: they get trained-like values instead, as in G16 / G21.
    -> [img_enc, txt_enc, caption_model] state dicts (fp32)."""
    D, Dv, H, Wd, E, V = cfg['embed_size'], cfg['dim_vid'], cfg['dim_hidden'], cfg['dim_word'], cfg['word_dim'], cfg['vocab_size']
    xn = lambda n_out, n_in: torch.randn(n_out, n_in, generator=g) * math.sqrt(2.0 / (n_in + n_out))
    wi = {'fc.weight': u((D, IMG_DIM), math.sqrt(6.0 / (IMG_DIM + D))), 'fc.bias': torch.zeros(D)}
    _gru(wi, 'img_rnn.', D, D, u)
    for i in (1, 2, 3, 4):
        p = 'Rs_GCN_%d.' % i
        for conv in ('g', 'W.0', 'theta', 'phi'):
            wi[p + conv + '.weight'] = u((D, D, 1), 1.0 / math.sqrt(D))
            wi[p + conv + '.bias'] = u((D,), 1.0 / math.sqrt(D))
        wi[p + 'W.1.weight'] = torch.rand(D, generator=g) * 0.6 + 0.2
        wi[p + 'W.1.bias'] = torch.randn(D, generator=g) * 0.05
        wi[p + 'W.1.running_mean'] = torch.randn(D, generator=g) * 0.1
        wi[p + 'W.1.running_var'] = torch.rand(D, generator=g) + 0.5
        wi[p + 'W.1.num_batches_tracked'] = torch.tensor(0)
    wt = {'embed.weight': u((V, E), 0.1)}
    _gru(wt, 'rnn.', E, D, u)
    wc = {'encoder.vid2hid.weight': xn(H, Dv), 'encoder.vid2hid.bias': u((H,), 1.0 / math.sqrt(Dv))}
    _gru(wc, 'encoder.rnn.', H, H, u)
    wc.update({'decoder.embedding.weight': torch.randn(V, Wd, generator=g),
               'decoder.attention.linear1.weight': u((H, 2 * H), 1.0 / math.sqrt(2 * H)),
               'decoder.attention.linear1.bias': u((H,), 1.0 / math.sqrt(2 * H)),
               'decoder.attention.linear2.weight': u((1, H), 1.0 / math.sqrt(H))})
    _gru(wc, 'decoder.rnn.', H + Wd, H, u)
    wc.update({'decoder.out.weight': xn(V, H), 'decoder.out.bias': u((V,), 1.0 / math.sqrt(H))})
    return [wi, wt, wc]


def oracle_step(cfg, weights, batch, dtype):
    """The oracle's train_emb restatement in `dtype` on the host: gru_model_train_step (VSE++, SCAN), sgraf_model_train_grads or
    vsrn_model_train_grads.  -> dict(loss, grads {'txt.<k>' | 'img.<k>' | 'sim.<k>' | 'cap.<k>': clipped gradient}, grad_norm (before
    clipping), scores, bn_stats, terms {logged loss term: value} (VSRN's Loss_caption / Loss_retrieval))."""
    feats, ids, lens = batch[:3]
    cast = lambda d: {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in d.items()}
    out = {}
    model = cfg['name']
    if model == 'VSRN':
        wi, wt, wc = [cast(d) for d in weights]
        loss, grads = O.vsrn_model_train_grads(wi, wt, wc, feats.to(dtype), ids, lens, batch[3], cfg, out=out)
        out['terms'] = {'Loss_caption': float(out['loss_caption']), 'Loss_retrieval': float(out['loss_retrieval'])}
    elif model == 'SGRAF':
        wi, wt, ws = [cast(d) for d in weights]
        loss, grads = O.sgraf_model_train_grads(wi, wt, ws, feats.to(dtype), ids, lens, cfg, out=out)
    else:
        wi, wt = [cast(d) for d in weights]
        loss, grads, _, _, _ = O.gru_model_train_step(model, wi, wt, feats.to(dtype), ids, lens, cfg, out=out)
    return dict(loss=float(loss), grads=grads, grad_norm=float(out['grad_norm']), scores=out['scores'], bn_stats=out.get('bn_stats'),
                terms=out.get('terms', {}))


def replay_bn(buffers, bn_stats, momentum=0.1):
    """torch BatchNorm's running-statistic updates, one per recorded call in call order, in the dtype of `bn_stats`:
    running = (1 - momentum) running + momentum batch, the variance unbiased by N / (N - 1).  -> {'<bn>.running_mean' | ... : tensor}."""
    out = {k: v.to(bn_stats[0][1].dtype).clone() if v.is_floating_point() else int(v) for k, v in buffers.items()}
    for p, mean, var, n in bn_stats:
        out[p + '.running_mean'] = (1 - momentum) * out[p + '.running_mean'] + momentum * mean
        out[p + '.running_var'] = (1 - momentum) * out[p + '.running_var'] + momentum * var * (n / (n - 1.0))
        out[p + '.num_batches_tracked'] += 1
    return out


def flip_margin(scores, margin=0.2, row_gaps=True):
    """Distance of the max-violation hinge from a discrete change: per row and per column of `scores`, the gap between the two
    hardest negatives, and |margin + hardest negative - positive| (the hinge's kink).  -> the smallest over all 2B of them.
    row_gaps=False leaves out the rows' top-2 gaps (for captions that coincide: see caption_spread)."""
    S = scores.double()
    n = S.shape[0]
    off = S.masked_fill(torch.eye(n, dtype=torch.bool), float('-inf'))
    d = S.diag()
    worst = float('inf')
    for M in (off, off.t()):           # rows: an image against its captions; columns (as rows of the transpose): a caption's images
        top = M.topk(2, dim=1).values
        worst = min(worst, float((margin + top[:, 0] - d).abs().min()))
        if row_gaps or M is not off:
            worst = min(worst, float((top[:, 0] - top[:, 1]).min()))
    return worst


def caption_spread(scores):
    """max |S[i, j] - S[i, k]| over all images i and captions j, k: how far the captions are from one vector, as the images see it."""
    S = scores.double()
    return float((S.max(1).values - S.min(1).values).max())
