"""Evaluation harness with the reference's signatures (itr/metricmodule/evaluation.py:75-259):
encode_data, cal_sims, i2t, t2i, cal_recall -- scoring and ranking on the HIP kernels.

Differences that are deliberate (DESIGN.md "reference quirks"):
  * cal_sims slices `lengths` per caption shard.  The reference passes the un-sliced array, so every caption
    shard j > 0 is scored with the lengths of shard 0 (evaluation.py:149);
    `ref_quirk_unsliced_lengths=True` reproduces that bit of behaviour.
  * i2t / t2i count instead of sorting; ranks are identical except on exact score ties, where numpy's
    unstable argsort makes the reference implementation-defined.
"""
import time
from collections import OrderedDict

import numpy as np
import torch

from .. import ops


class AverageMeter(object):
    """Computes and stores the average and current value (evaluation.py:15-40)."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.val = 0
        self.avg = 0
        self.sum = 0
        self.count = 0

    def update(self, val, n=0):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / (.0001 + self.count)

    def __str__(self):
        if self.count == 0:
            return str(self.val)
        return '%.4f (%.4f)' % (self.val, self.avg)


class LogCollector(object):
    """A collection of logging objects that can change from train to val (evaluation.py:43-72)."""

    def __init__(self):
        self.meters = OrderedDict()

    def update(self, k, v, n=0):
        if k not in self.meters:
            self.meters[k] = AverageMeter()
        self.meters[k].update(v, n)

    def __str__(self):
        s = ''
        for i, (k, v) in enumerate(self.meters.items()):
            if i > 0:
                s += '  '
            if k == 'lr':
                v = '{:.3e}'.format(v.val)
            s += k + ' ' + str(v)
        return s

    def tb_log(self, tb_logger, prefix='', step=None):
        for k, v in self.meters.items():
            tb_logger.log_value(prefix + k, v.val, step=step)


def encode_data(model, data_loader, islength=False):
    """Encode all images and captions loadable by `data_loader` -> (img_embs, cap_embs, cap_lens) numpy arrays,
    exactly the reference's layout (evaluation.py:75-121): row `ids[k]` of every array belongs to dataset
    item ids[k]; word-level caption embeddings are zero-padded to the longest caption."""
    val_logger = LogCollector()
    model.val_start()
    max_n_word = 0
    no_init = True
    if islength:
        for (_, _, _, _, lengths_, _, _, _) in data_loader:
            max_n_word = max(max_n_word, int(lengths_[0]))
    img_embs = cap_embs = cap_lens = None
    for batch_data in data_loader:
        model.logger = val_logger
        images, boxes, imgs_wh, captions, lengths, ids, captions_mask, captions_type_ids = batch_data
        with torch.no_grad():
            emd_list = model.forward_emb(images=images, boxes=boxes, imgs_wh=imgs_wh, captions=captions,
                                         lengths=lengths, ids=ids, captions_mask=captions_mask,
                                         captions_type_ids=captions_type_ids)
        img_emb, cap_emb = emd_list[0], emd_list[1]
        if no_init:
            no_init = False
            n = len(data_loader.dataset)
            ima_size = [n] + list(img_emb.size()[1:])
            cap_size = [n] + list(cap_emb.size()[1:])
            if islength:
                cap_size[1] = max_n_word
            img_embs = np.zeros(ima_size, dtype=np.float32)
            cap_embs = np.zeros(cap_size, dtype=np.float32)
            cap_lens = np.zeros(n, dtype=np.int32)
        ids = list(ids)
        img_embs[ids] = img_emb.detach().cpu().numpy()
        if cap_emb.dim() == 3:
            cap_embs[ids, :cap_emb.size(1)] = cap_emb.detach().cpu().numpy()
        else:
            cap_embs[ids] = cap_emb.detach().cpu().numpy()
        cap_lens[ids] = [int(l) for l in lengths]
    return img_embs, cap_embs, cap_lens


def _cal_fun(model):
    if model.config['name'] in ['CAMERA']:
        return model.mvm
    return model.sim_enc if model.sim_enc is not None else model.criterion.sim


def cal_sims(model, img_embs, cap_embs, lengths=None, shard_size=128, ref_quirk_unsliced_lengths=False):
    """(n_img, n_cap) float64 similarity matrix (evaluation.py:124-153).  Same tiling loop as the reference
    so that `shard_size` keeps its meaning; each tile is one kernel launch on device-resident blocks."""
    cal_fun = _cal_fun(model)
    n_img, n_cap = len(img_embs), len(cap_embs)
    t0 = time.time()
    dev = torch.device('cuda', torch.cuda.current_device())
    img_all = torch.from_numpy(np.ascontiguousarray(img_embs)).to(dev)
    cap_all = torch.from_numpy(np.ascontiguousarray(cap_embs)).to(dev)
    d = np.zeros((n_img, n_cap))
    for i0 in range(0, n_img, shard_size):
        i1 = min(i0 + shard_size, n_img)
        for j0 in range(0, n_cap, shard_size):
            j1 = min(j0 + shard_size, n_cap)
            lens = lengths
            if lengths is not None and not ref_quirk_unsliced_lengths:
                lens = lengths[j0:j1]
            with torch.no_grad():
                sim = cal_fun(img_all[i0:i1], cap_all[j0:j1], lens, model.config)
            d[i0:i1, j0:j1] = sim.detach().cpu().numpy()
    print('Calculate similarity matrix elapses: {:.3f}s'.format(time.time() - t0))
    return d


def _device_matrix(sims):
    """numpy array or tensor -> contiguous device tensor: float32 stays float32, anything else becomes float64."""
    if torch.is_tensor(sims):
        S = sims.detach()
        if S.dtype not in (torch.float32, torch.float64):
            S = S.to(torch.float64)
        return S.contiguous().cuda()
    a = np.asarray(sims)
    if a.dtype != np.float32:
        a = a.astype(np.float64, copy=False)
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ranks(sims):
    """Rank vectors of a similarity matrix in the arithmetic the caller holds it in: float64 input (cal_sims' output,
    an ensemble average -- what the reference argsorts, evaluation.py:169, :209, :380) is counted in float64, so the
    indices equal the reference's even where two scores differ by less than an fp32 ulp; float32 input is counted in
    float32; anything else is widened to float64 (exact for every narrower type)."""
    S = _device_matrix(sims)
    if S.dtype == torch.float64:
        i_rank, i_top, t_rank, t_top = ops.rank_counts_f64(S, 5)
    else:
        i_rank, i_top, t_rank, t_best, _ = ops.rank_counts(S, 5)
        t_top = t_best & 0xffffffff
    return (i_rank.cpu().numpy().astype(np.float64), i_top.cpu().numpy().astype(np.float64),
            t_rank.cpu().numpy().astype(np.float64), t_top.cpu().numpy().astype(np.float64))


def topk(sims, k=10):
    """The first k entries of the reference's ranked lists inds = np.argsort(sims[index])[::-1] (evaluation.py:169 for i2t,
    :209 for t2i), selected on the GPU in the arithmetic the caller holds the matrix in (as _ranks: float64 input is selected
    in float64).  Order: larger score first, the higher index on exact ties, -0.0 == +0.0, NaN as +inf (column 0 is the
    ranker's top1).  -> {'i2t_topk': int64 (Ni, k), 'i2t_topk_scores': (Ni, k), 't2i_topk': int64 (Nc, k),
    't2i_topk_scores': (Nc, k)}, scores in the matrix's dtype with their original bits."""
    S = _device_matrix(sims)
    r_idx, r_val, part = ops.topk_lists(S, k)
    c_idx, c_val = ops.topk_merge_cols([part], k)
    return {'i2t_topk': r_idx.cpu().numpy().astype(np.int64), 'i2t_topk_scores': r_val.cpu().numpy(),
            't2i_topk': c_idx.cpu().numpy().astype(np.int64), 't2i_topk_scores': c_val.cpu().numpy()}


def _save_topk(save_dir, data_name, tag, k, lists):
    """`<save_dir>/<data_name>_<tag>_top<k>.npz` next to the result YAML (fold5: PART_<i>_-prefixed arrays)."""
    import os
    path = os.path.join(save_dir, f'{data_name}_{tag}_top{k}.npz')
    np.savez(path, **lists)
    return path


def i2t(sims, return_ranks=False):
    """Images->Text (evaluation.py:156-189): sims (N, 5N)."""
    ranks, top1, _, _ = _ranks(sims)
    out = ops.recall_from_ranks(ranks)
    return (out, (ranks, top1)) if return_ranks else out


def t2i(sims, return_ranks=False):
    """Text->Images (evaluation.py:192-222)."""
    _, _, ranks, top1 = _ranks(sims)
    out = ops.recall_from_ranks(ranks)
    return (out, (ranks, top1)) if return_ranks else out


def cal_recall(sims):
    """Result dict of evaluation.py:225-259."""
    r, rt = i2t(sims, return_ranks=True)
    ri, rti = t2i(sims, return_ranks=True)
    ar = (r[0] + r[1] + r[2]) / 3
    ari = (ri[0] + ri[1] + ri[2]) / 3
    rsum = r[0] + r[1] + r[2] + ri[0] + ri[1] + ri[2]
    print("rsum: %.1f" % rsum)
    print("Average i2t Recall: %.1f" % ar)
    print("Image to text: r1 %.1f; r5 %.1f; r10 %.1f; medr %.1f; meanr %.1f" % r)
    print("Average t2i Recall: %.1f" % ari)
    print("Text to image: r1 %.1f; r5 %.1f; r10 %.1f; medr %.1f; meanr %.1f" % ri)
    res = {'result': [list(r) + list(ri) + [ar, ari, rsum]], 'rsum': rsum, 'i2t_ave_r': ar, 'i2t_r1': r[0],
           'i2t_r5': r[1], 'i2t_r10': r[2], 'i2t_medr': r[3], 'i2t_meanr': r[4], 'i2t_ranks': rt[0],
           'i2t_top1': rt[1], 't2i_ave_r': ari, 't2i_r1': ri[0], 't2i_r5': ri[1], 't2i_r10': ri[2],
           't2i_medr': ri[3], 't2i_meanr': ri[4], 't2i_ranks': rti[0], 't2i_top1': rti[1]}
    return res


# ---------------------------------------------------------------------------------------------------------
# Metrics under ANY ground-truth relation (ops.GroundTruth): several positives per query, or none.
_GT_SCALARS = ('medr', 'meanr', 'rprecision', 'map_at_r', 'n_queries', 'n_without_positives')


def metrics_from_positions(ptr, pos, ks=(1, 5, 10)):
    """Host numpy, float64.  ptr [n + 1]: CSR pointer of the queries; pos [nnz]: the 0-based position of every positive in its
    query's ranked list (ops.rank_positions).  Over the queries with at least one positive, R_q their number of positives and
    p_1 < ... < p_R their positions:
      r@k        = 100 mean[p_1 < k]
      medr       = floor(median(p_1)) + 1,  meanr = mean(p_1) + 1          (the reference's formulas, on the best positive)
      rprecision = 100 mean[#{p_j < R_q} / R_q]
      map_at_r   = 100 mean[(1 / R_q) sum_{j : p_j < R_q} j / (p_j + 1)]
    plus n_queries (those with a positive), n_without_positives, and per query (NaN / -1 where it has no positive) the arrays
    best (p_1), rprecision_q and ap_q."""
    ptr = np.asarray(ptr, dtype=np.int64)
    pos = np.asarray(pos, dtype=np.int64)
    if ptr.ndim != 1 or len(ptr) < 1 or ptr[0] != 0 or ptr[-1] != len(pos) or (np.diff(ptr) < 0).any():
        raise ValueError("metrics_from_positions: ptr must rise from 0 to len(pos) = %d" % len(pos))
    R = np.diff(ptr)
    nq = len(R)
    has = R > 0
    n = int(has.sum())
    seg = np.repeat(np.arange(nq), R)
    p = pos[np.lexsort((pos, seg))]                      # ascending inside every query
    j = np.arange(len(p)) - ptr[seg] + 1                 # 1-based index among the query's positives
    Rq = R[seg].astype(np.float64)
    hit = p < R[seg]
    best = np.full(nq, -1, dtype=np.int64)
    best[has] = p[ptr[:-1][has]]
    rprec_q = np.full(nq, np.nan)
    ap_q = np.full(nq, np.nan)
    rprec_q[has] = (np.bincount(seg, weights=hit / Rq, minlength=nq))[has]
    ap_q[has] = (np.bincount(seg, weights=np.where(hit, j / (p + 1.0), 0.0) / Rq, minlength=nq))[has]
    out = OrderedDict()
    b = best[has]
    for k in ks:
        out['r@%d' % k] = 100.0 * int((b < k).sum()) / n if n else float('nan')
    out['medr'] = float(np.floor(np.median(b)) + 1) if n else float('nan')
    out['meanr'] = float(int(b.sum())) / n + 1.0 if n else float('nan')
    out['rprecision'] = 100.0 * float(rprec_q[has].mean()) if n else float('nan')
    out['map_at_r'] = 100.0 * float(ap_q[has].mean()) if n else float('nan')
    out['n_queries'] = n
    out['n_without_positives'] = nq - n
    out['best'], out['rprecision_q'], out['ap_q'] = best, rprec_q, ap_q
    return out


def gt_metrics(sims, gt, ks=(1, 5, 10)):
    """`metrics_from_positions` of both directions under the relation `gt` (ops.GroundTruth), the positions counted on the GPU in
    the arithmetic the caller holds the matrix in (as _ranks: a float64 matrix is ranked in float64).
    -> {'i2t': {...metrics, 'positions': int64 [nnz] in image-CSR order}, 't2i': {... in caption-CSR order}}."""
    S = _device_matrix(sims)
    i_pos, t_pos, _ = ops.rank_positions(S, gt)
    out = {}
    for name, ptr, pos in (('i2t', gt.img_ptr_host, i_pos), ('t2i', gt.cap_ptr_host, t_pos)):
        pos = pos.cpu().numpy().astype(np.int64)
        out[name] = metrics_from_positions(ptr, pos, ks)
        out[name]['positions'] = pos
    return out


def _load_gt(path, n_images, n_captions):
    """`.npz` holding `pairs` [nnz, 2] (image, caption) and optionally n_images / n_captions -> ops.GroundTruth over the gallery."""
    with np.load(path) as z:
        if 'pairs' not in z.files:
            raise ValueError("%s holds no `pairs` array" % path)
        pairs = z['pairs']
        for key, have in (('n_images', n_images), ('n_captions', n_captions)):
            if key in z.files and int(z[key]) != have:
                raise ValueError("%s: %s = %d, the gallery has %d" % (path, key, int(z[key]), have))
    return ops.GroundTruth(pairs, n_images, n_captions, torch.device('cuda', torch.cuda.current_device()))


def _save_gt(save_dir, data_name, tag, res, gt):
    import os
    import yaml
    scalars = {d: {k: (int(v) if isinstance(v, (int, np.integer)) else float(v)) for k, v in res[d].items() if not isinstance(v, np.ndarray)}
               for d in ('i2t', 't2i')}
    scalars['data_name'] = data_name
    with open(os.path.join(save_dir, f'{data_name}_{tag}_gt_result.yaml'), 'w') as f:
        yaml.safe_dump(scalars, f)
    arrays = {f'{d}_{k}': v for d in ('i2t', 't2i') for k, v in res[d].items() if isinstance(v, np.ndarray)}
    arrays.update(img_ptr=gt.img_ptr_host, cap_ptr=gt.cap_ptr_host, img_cap=gt.img_cap.cpu().numpy(), cap_img=gt.cap_img.cpu().numpy())
    np.savez(os.path.join(save_dir, f'{data_name}_{tag}_gt_positions.npz'), **arrays)


# ---------------------------------------------------------------------------------------------------------
# Hubness correction before ranking: S'[i, j] = S[i, j] - a[i] - b[j].  a is constant along a row, so the i2t order
# is corrected by b alone (it penalises hub captions), and b along a column, so the t2i order by a alone: ONE adjusted matrix serves
# both directions and every consumer of a similarity matrix (cal_recall, topk, gt_metrics, rerank) works on it unchanged.
HUBNESS_METHODS = ('csls', 'invsoftmax')


def _check_hubness(who, method, k, beta):
    if method not in HUBNESS_METHODS:
        raise ValueError("%s: hubness must be one of %s, got %r" % (who, HUBNESS_METHODS, method))
    if method == 'csls' and (int(k) != k or k < 1):
        raise ValueError("%s: hub_k = %r must be an integer >= 1" % (who, k))
    if method == 'invsoftmax' and not (float(beta) > 0.0 and np.isfinite(float(beta))):
        raise ValueError("%s: hub_beta = %r must be finite and positive" % (who, beta))


def hubness_vectors(sims, method, k=10, beta=20.0):
    """The correction vectors of the query bank `self`: the statistics of the evaluated matrix sims [Ni, Nc] itself (transductive).
    method 'invsoftmax' (Smith et al. 2017): a[i] = (1 / beta) log sum_q exp(beta sims[i, q]), b[j] the same down column j -- ONE
    `ops.hub_lse_fold` over the matrix.  method 'csls' (Conneau et al. 2018): a[i] = 0.5 * mean of the k largest of row i, b[j] of
    column j, the k largest in the ranker's order (`ops.topk_lists` + `ops.topk_merge_cols`, then `ops.hub_list_mean`).  float32
    input is reduced as float32 widened to double, anything else in float64 (as `_ranks`).  -> (a [Ni], b [Nc]) float64 numpy."""
    _check_hubness("hubness_vectors", method, k, beta)
    S = _device_matrix(sims)
    if method == 'invsoftmax':
        a, state = ops.hub_lse_fold(S, beta)
        b = ops.hub_lse_cols(state, beta)
    else:
        k = int(k)
        if k > min(S.shape):
            raise ValueError("hubness_vectors: k = %d is larger than a side of the %d x %d matrix" % (k, S.shape[0], S.shape[1]))
        _, r_val, part = ops.topk_lists(S, k)
        _, c_val = ops.topk_merge_cols([part], k)
        a, b = ops.hub_list_mean(r_val, k), ops.hub_list_mean(c_val, k)
    return a.cpu().numpy(), b.cpu().numpy()


def _hub_block_scorer(members, n_cols, shard_sizes):
    """-> f(i0, i1): the device matrix [i1 - i0, n_cols] of image rows i0 .. i1 - 1 against ALL caption columns, scored with every
    member's own cal_fun in cal_sims' tiles (shard x shard, so a block that starts on a shard boundary holds the very scores cal_sims
    would); one member: its scores as they are, several: their float64 mean, summed in member order and divided once, as
    `_score_blocks` averages whole matrices.  members: (model, img_dev, cap_dev, lens)."""
    def block(i0, i1):
        acc = None
        for (model, img, cap, lens), shard in zip(members, shard_sizes):
            cal_fun = _cal_fun(model)
            out = None
            for r0 in range(i0, i1, shard):
                r1 = min(r0 + shard, i1)
                for j0 in range(0, n_cols, shard):
                    j1 = min(j0 + shard, n_cols)
                    with torch.no_grad():
                        sim = cal_fun(img[r0:r1], cap[j0:j1], None if lens is None else lens[j0:j1], model.config).detach()
                    if (r0, r1, j0, j1) == (i0, i1, 0, n_cols):
                        out = sim
                    else:
                        if out is None:
                            out = torch.empty(i1 - i0, n_cols, device=sim.device, dtype=sim.dtype)
                        out[r0 - i0:r1 - i0, j0:j1] = sim
            if len(members) == 1:
                return out
            acc = out.double() if acc is None else acc + out.double()
        return acc / len(members)
    return block


def _hub_rows_per_block(rows, shard):
    """Whole shards per block where a block holds at least one (the tiles are then cal_sims' own)."""
    rows = max(1, int(rows))
    return rows if rows < shard else rows // shard * shard


class _RunningColumnLists(object):
    """The k largest entries of every column over the row blocks folded so far, for CSLS' b.  fp32 blocks: `ops.topk_fold_cols`.
    float64 blocks (ensemble means): the block's own final lists (`ops.topk_lists`) are put beside the running ones and the k
    largest of the two taken again; only the VALUES reach the mean, so which of two equal scores is kept does not matter."""
    def __init__(self, k):
        self.k, self.state, self.vals, self.row0 = k, None, None, 0

    def fold(self, S):
        n = S.shape[0]
        if S.dtype == torch.float32:
            self.state = ops.topk_fold_cols(S, self.k, row0=self.row0, state=self.state)
        else:
            kb = min(self.k, n)
            _, _, (_, val) = ops.topk_lists(S, kb, rows=False)
            if self.vals is None:
                self.vals = torch.full((S.shape[1], self.k), float('-inf'), device=S.device, dtype=torch.float64)
            both = torch.cat([self.vals, val], 1)
            _, self.vals, _ = ops.topk_lists(both, self.k, cols=False)
        self.row0 += n

    def mean(self):
        if self.vals is not None:
            return ops.hub_list_mean(self.vals, self.k)
        _, val = ops.topk_merge_cols([self.state], self.k)
        return ops.hub_list_mean(val, self.k)


def hubness_bank_vectors(models_embs, bank_embs, method, k=10, beta=20.0, sl_img=slice(0, None, 5), sl_cap=slice(None), block_rows=640):
    """The correction vectors from an EXTERNAL query bank (the usual choice: the train or dev split), whose score matrices may be
    several times the gallery's and are never stored.  models_embs: list of (model, img_embs, cap_embs, cap_lens, shard_size) of
    the gallery, as `_score_blocks` takes them (sl_img / sl_cap select the gallery's images and captions: a fold); bank_embs: list
    of (img_embs, cap_embs, cap_lens) of the bank per model, in encode_data's layout (bank images = img_embs[::5]).
      a [Ni]: from gallery-image x bank-caption scores -- rows are complete in a block: the fold's row_lse, or
              `ops.topk_lists(rows=True)` then `ops.hub_list_mean`;
      b [Nc]: from bank-image x gallery-caption scores -- row blocks go through `ops.hub_lse_fold`, or through
              `ops.topk_fold_cols`, `ops.topk_merge_cols` and `ops.hub_list_mean`.
    Both are scored in image-row blocks with the model's own cal_fun, ONE block on the device at a time: block_rows bank images for
    b, and for a as many gallery images as give a block of the same number of scores (whole shards of the first model where a block
    holds at least one: the tiles are then cal_sims' own).  Several models: the members' blocks are
    averaged in float64 on the device before folding.  -> (a, b) float64 numpy."""
    who = "hubness_bank_vectors"
    _check_hubness(who, method, k, beta)
    if len(bank_embs) != len(models_embs):
        raise ValueError("%s: %d bank encodings for %d models" % (who, len(bank_embs), len(models_embs)))
    dev = torch.device('cuda', torch.cuda.current_device())

    def to_dev(x):
        return torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    shards = [m[4] for m in models_embs]
    g_img = [to_dev(m[1][sl_img]) for m in models_embs]
    g_cap = [to_dev(m[2][sl_cap]) for m in models_embs]
    g_len = [None if m[3] is None else m[3][sl_cap] for m in models_embs]
    q_img = [to_dev(q[0][::5]) for q in bank_embs]
    q_cap = [to_dev(q[1]) for q in bank_embs]
    q_len = [q[2] for q in bank_embs]
    models = [m[0] for m in models_embs]
    Ni, Nc, Qi, Qc = len(g_img[0]), len(g_cap[0]), len(q_img[0]), len(q_cap[0])
    k = int(k)
    if method == 'csls' and k > min(Qi, Qc):
        raise ValueError("%s: k = %d is larger than a side of the bank (%d images, %d captions)" % (who, k, Qi, Qc))
    block_rows = int(block_rows)
    if block_rows < 1:
        raise ValueError("%s: block_rows = %d < 1" % (who, block_rows))

    # b: bank images x gallery captions, folded down the columns
    score = _hub_block_scorer(list(zip(models, q_img, g_cap, g_len)), Nc, shards)
    state, lists = None, _RunningColumnLists(k)
    rows_b = _hub_rows_per_block(block_rows, shards[0])
    for i0 in range(0, Qi, rows_b):
        S = score(i0, min(i0 + rows_b, Qi))
        if method == 'invsoftmax':
            _, state = ops.hub_lse_fold(S, beta, state=state, rows=False)
        else:
            lists.fold(S)
        del S
    b = ops.hub_lse_cols(state, beta) if method == 'invsoftmax' else lists.mean()

    # a: gallery images x bank captions, whole rows per block
    score = _hub_block_scorer(list(zip(models, g_img, q_cap, q_len)), Qc, shards)
    rows_a = _hub_rows_per_block(block_rows * Nc // max(Qc, 1), shards[0])
    parts = []
    for i0 in range(0, Ni, rows_a):
        S = score(i0, min(i0 + rows_a, Ni))
        if method == 'invsoftmax':
            parts.append(ops.hub_lse_fold(S, beta, cols=False)[0])
        else:
            parts.append(ops.hub_list_mean(ops.topk_lists(S, k, cols=False)[1], k))
        del S
    a = torch.cat(parts)
    return a.cpu().numpy(), b.cpu().numpy()


def hubness_adjust(sims, a, b):
    """S' = dtype((double(sims[i, j]) - a[i]) - b[j]) on the GPU (`ops.hub_adjust`), in the dtype of sims (float32 stays float32,
    anything else is float64 as in `_ranks`); a / b: float64 vectors (numpy or tensors), None = zeros.  numpy's
    ((sims.astype(float64) - a[:, None]) - b[None, :]).astype(dtype) is the same matrix bit for bit.  -> numpy array for numpy input,
    a device tensor for a tensor."""
    S = _device_matrix(sims)

    def vec(v):
        if v is None or torch.is_tensor(v):
            return v if v is None else v.to(device=S.device, dtype=torch.float64)
        return torch.from_numpy(np.ascontiguousarray(np.asarray(v, dtype=np.float64))).to(S.device)
    out = ops.hub_adjust(S, vec(a), vec(b))
    return out if torch.is_tensor(sims) else out.cpu().numpy()


def _hub_part(hub, sims, models_embs, sl_img, sl_cap, k, gt, prefix):
    """One gallery (the whole split, or a fold): vectors -> adjusted matrix -> cal_recall, with the hub-tagged top-k lists and
    ground-truth metrics beside it."""
    method = hub['method']
    if hub['bank'] is None:
        a, b = hubness_vectors(sims, method, hub['k'], hub['beta'])
    else:
        a, b = hubness_bank_vectors(models_embs, hub['bank'], method, hub['k'], hub['beta'], sl_img, sl_cap)
    adj = hubness_adjust(sims, a, b)
    hub['vectors'][prefix + 'a'], hub['vectors'][prefix + 'b'] = a, b
    if k > 0:
        hub['lists'].update({prefix + key: v for key, v in topk(adj, k).items()})
    if gt is not None:
        hub['gt_result'] = gt_metrics(adj, gt['relation'])
    print("--------------------- hubness-corrected (%s) ---------------------" % method)
    return cal_recall(adj)


# ---------------------------------------------------------------------------------------------------------
# evalrank_single / evalrank_ensemble (evaluation.py:262-435): checkpoint -> loader -> encode -> score -> rank ->
# `<save_dir>/<data_name>[_5fold]_{single,ensemble}_result.yaml`.
_MEAN_KEYS = ('i2t_r1', 'i2t_r5', 'i2t_r10', 'i2t_medr', 'i2t_meanr', 't2i_r1', 't2i_r5', 't2i_r10', 't2i_medr', 't2i_meanr')


def _plain(res):
    """YAML-portable copy: numpy scalars / arrays -> python floats / lists (the reference dumps numpy objects,
    which needs yaml's unsafe loader to read back)."""
    out = {}
    for k, v in res.items():
        if isinstance(v, dict):
            out[k] = _plain(v)
        elif isinstance(v, np.ndarray):
            out[k] = [float(x) for x in v.tolist()]
        elif isinstance(v, (list, tuple)):
            out[k] = [[float(x) for x in row] if isinstance(row, (list, tuple, np.ndarray)) else
                      (float(row) if isinstance(row, (float, int, np.floating, np.integer)) else row) for row in v]
        elif isinstance(v, (np.floating, np.integer)):
            out[k] = float(v)
        else:
            out[k] = v
    return out


def _mean_metrics(res_dic):
    """fold5 averaging (evaluation.py:307-333).  The reference writes the means INTO the last fold's dict (the same
    object as PART_5), so its PART_5 entry shows the averages; here PART_5 keeps its own numbers and
    `Mean_metrics` is a dict of its own."""
    mean = tuple(np.array(res_dic['sum_result']).mean(axis=0).flatten())
    print("---------------------------------------------------------")
    print("--------------------- Mean metrics: ---------------------")
    print("rsum: %.1f" % (mean[10] * 6))
    print("Average i2t Recall: %.1f" % mean[11])
    print("Image to text: r1 %.1f; r5 %.1f; r10 %.1f; medr %.1f; meanr %.1f" % mean[:5])
    print("Average t2i Recall: %.1f" % mean[12])
    print("Text to image: r1 %.1f; r5 %.1f; r10 %.1f; medr %.1f; meanr %.1f" % mean[5:10])
    out = {'rsum': mean[10] * 6, 'i2t_ave_r': mean[11], 't2i_ave_r': mean[12]}
    out.update({k: mean[i] for i, k in enumerate(_MEAN_KEYS)})
    return out


def _load_for_eval(model_path, data_path):
    from ..modalmodule import get_model
    from ..utils import load_checkpoint
    checkpoint = load_checkpoint(model_path)
    _config = checkpoint['_config']
    print('Best model: Epoch = {}, Eiters = {}, Rsum = {:.2f}, R1 = {:.2f}'.format(
        checkpoint['epoch'], checkpoint['Eiters'], checkpoint['best_rsum'], checkpoint.get('best_r1', checkpoint.get('best_rl', 0.0))))
    if data_path is not None:
        _config['data_path'] = data_path
    model = get_model(_config)
    model.load_state_dict(checkpoint['model'])
    return model, _config


def _score_blocks(models_embs, fold5, k=0, lists=None, gt=None, hub=None):
    """models_embs: list of (model, img_embs, cap_embs, cap_lens, shard_size); the similarity matrices of the
    models are averaged (ensemble, evaluation.py:377-381).  k > 0: the top-k lists of every (float64) matrix go into
    `lists` (fold5: keys PART_<i>_..., indices local to the part's matrix).  gt: {'path': FILE.npz} (not with fold5): the metrics
    of that relation on the same matrix go into gt['result'], the relation into gt['relation'].  hub: the state of a hubness
    correction (`_evalrank`): the plain results are computed exactly as without it, and the corrected results of every gallery go
    into hub['res'] (fold5: per fold, with vectors derived per fold)."""
    def sims_of(sl_img, sl_cap):
        acc = None
        for model, img, cap, lens, shard in models_embs:
            s = cal_sims(model, img[sl_img], cap[sl_cap], lengths=lens[sl_cap], shard_size=shard)
            acc = s if acc is None else acc + s
        return acc / len(models_embs)

    n = len(models_embs[0][1])
    if not fold5:
        sims = sims_of(slice(0, n, 5), slice(None))
        if k > 0:
            lists.update(topk(sims, k))
        if gt is not None:
            gt['relation'] = _load_gt(gt['path'], sims.shape[0], sims.shape[1])
            gt['result'] = gt_metrics(sims, gt['relation'])
        res = cal_recall(sims)
        if hub is not None:
            hub['res'] = _hub_part(hub, sims, models_embs, slice(0, n, 5), slice(None), k, gt, '')
        return res
    res_dic = {'sum_result': []}
    if hub is not None:
        hub['res'] = {'sum_result': []}
    for i in range(5):
        print(f"--------------------- The {i + 1} part ---------------------")
        sl_img, sl_cap = slice(i * 5000, (i + 1) * 5000, 5), slice(i * 5000, (i + 1) * 5000)
        sims = sims_of(sl_img, sl_cap)
        if k > 0:
            lists.update({f'PART_{i + 1}_{key}': v for key, v in topk(sims, k).items()})
        part = cal_recall(sims)
        res_dic[f'PART_{i + 1}'] = part
        res_dic['sum_result'] += part['result']
        if hub is not None:
            part = _hub_part(hub, sims, models_embs, sl_img, sl_cap, k, None, f'PART_{i + 1}_')
            hub['res'][f'PART_{i + 1}'] = part
            hub['res']['sum_result'] += part['result']
    res_dic['Mean_metrics'] = _mean_metrics(res_dic)
    if hub is not None:
        print("--------------------- hubness-corrected (%s) ---------------------" % hub['method'])
        hub['res']['Mean_metrics'] = _mean_metrics(hub['res'])
    return res_dic


def _evalrank(model_paths, data_path, split, fold5, tag, topk=0, gt=None, hubness=None, hub_k=10, hub_beta=20.0, querybank='self'):
    import os
    import yaml
    if hubness is not None:
        _check_hubness("evalrank_" + tag, hubness, hub_k, hub_beta)
        if not isinstance(querybank, str) or not querybank:
            raise ValueError("evalrank_%s: querybank must be 'self' or the name of a split, got %r" % (tag, querybank))
    elif querybank != 'self' or hub_k != 10 or hub_beta != 20.0:
        raise ValueError("evalrank_%s: hub_k / hub_beta / querybank need hubness='csls' or 'invsoftmax'" % tag)
    if gt is not None and fold5:
        raise ValueError("gt does not combine with fold5: a ground-truth relation indexes ONE gallery, fold5 ranks five")
    gt = None if gt is None else {'path': gt}
    from ..datamodule import data_loader as data
    loaded = [_load_for_eval(p, data_path) for p in model_paths]
    _config = loaded[0][1]
    print(f'Loading dataset : {_config["data_name"]} ......')
    data_loader, _ = data.get_test_loader(split, _config['data_name'], _config['batch_size'], _config['workers'], _config)
    print('Computing results...')
    # the reference asks for max-length sizing only for SGRAF (evaluation.py:284), which breaks SCAN whenever a later
    # batch holds a longer caption than the first; word-level models all need it
    islength = _config['name'] in ['SGRAF', 'SCAN']
    embs = []
    for model, cfg in loaded:
        img, cap, lens = encode_data(model, data_loader, islength=islength)
        embs.append((model, img, cap, lens, cfg['batch_size'] * 5))
    print('#Images: %d, #Captions: %d' % (embs[0][1].shape[0] / 5, embs[0][2].shape[0]))
    lists = {}
    hub = None
    if hubness is not None:
        hub = {'method': hubness, 'k': int(hub_k), 'beta': float(hub_beta), 'bank': None, 'vectors': {}, 'lists': {}}
        if querybank != 'self':                # the bank split through the same loader path, encoded by every model
            print(f'Encoding the query bank : {querybank} ......')
            bank_loader, _ = data.get_test_loader(querybank, _config['data_name'], _config['batch_size'], _config['workers'], _config)
            hub['bank'] = [encode_data(model, bank_loader, islength=islength) for model, _ in loaded]
    res_dic = _score_blocks(embs, fold5, topk, lists, gt, hub)
    res_dic['data_name'] = _config['data_name'] + ('_5fold' if fold5 else '')
    if len(model_paths) > 1 and fold5:
        res_dic['modal_path_1'], res_dic['modal_path_2'] = model_paths[0], model_paths[1]
    save_dir = os.path.dirname(model_paths[0])
    out_file = os.path.join(save_dir, f'{res_dic["data_name"]}_{tag}_result.yaml')
    with open(out_file, 'w') as yaml_file:
        yaml.safe_dump(_plain(res_dic), yaml_file)
    if topk > 0:
        _save_topk(save_dir, res_dic['data_name'], tag, topk, lists)
    if gt is not None:
        _save_gt(save_dir, res_dic['data_name'], tag, gt['result'], gt['relation'])
    if hub is not None:
        _save_hub(save_dir, res_dic['data_name'], tag, hub, querybank, topk, gt)
    return res_dic


def _save_hub(save_dir, data_name, tag, hub, querybank, topk, gt):
    """`<data_name>_<tag>_hub_<method>_result.yaml` (cal_recall of the adjusted matrix and how it was corrected),
    `..._hub_<method>.npz` (the vectors a and b; fold5: PART_<i>_-prefixed) and the hub-tagged counterparts of topk and gt."""
    import os
    import yaml
    htag = f'{tag}_hub_{hub["method"]}'
    out = dict(hub['res'])
    out['data_name'] = data_name
    out['hubness'] = hub['method']
    out['hub_k' if hub['method'] == 'csls' else 'hub_beta'] = hub['k'] if hub['method'] == 'csls' else hub['beta']
    out['querybank'] = querybank
    if querybank == 'self':
        out['comment'] = ('querybank self: the correction is derived from the evaluated queries themselves, so these numbers are '
                          'transductive; name a held-out split (--querybank dev / train) for inductive ones')
    with open(os.path.join(save_dir, f'{data_name}_{htag}_result.yaml'), 'w') as f:
        yaml.safe_dump(_plain(out), f)
    np.savez(os.path.join(save_dir, f'{data_name}_{htag}.npz'), **hub['vectors'])
    if topk > 0:
        _save_topk(save_dir, data_name, htag, topk, hub['lists'])
    if gt is not None:
        _save_gt(save_dir, data_name, htag, hub['gt_result'], gt['relation'])


def _recall_dict(ranks):
    """cal_recall's dict (evaluation.py:225-259) from rank vectors."""
    i_rank, i_top, t_rank, t_top = [np.asarray(x, dtype=np.float64) for x in ranks]
    r, ri = ops.recall_from_ranks(i_rank), ops.recall_from_ranks(t_rank)
    ar, ari = (r[0] + r[1] + r[2]) / 3, (ri[0] + ri[1] + ri[2]) / 3
    rsum = r[0] + r[1] + r[2] + ri[0] + ri[1] + ri[2]
    return {'result': [list(r) + list(ri) + [ar, ari, rsum]], 'rsum': rsum, 'i2t_ave_r': ar, 'i2t_r1': r[0], 'i2t_r5': r[1],
            'i2t_r10': r[2], 'i2t_medr': r[3], 'i2t_meanr': r[4], 'i2t_ranks': i_rank, 'i2t_top1': i_top, 't2i_ave_r': ari,
            't2i_r1': ri[0], 't2i_r5': ri[1], 't2i_r10': ri[2], 't2i_medr': ri[3], 't2i_meanr': ri[4], 't2i_ranks': t_rank,
            't2i_top1': t_top}


def evalrank_fast(model_path, data_path=None, split='dev', fold5=False, comm=None, topk=0):
    """Same result dict / YAML as evalrank_single through the sharded device-resident pipeline
    (itr_amd.evalpipe.evaluate_precomp): launch one process per GPU with torch.distributed.run; rank 0 writes
    `<run dir>/<data_name>[_5fold]_single_result.yaml`, and with topk > 0 also `..._single_top<topk>.npz` (the top-k lists of
    the fp32 matrix the pipeline ranks; evalpipe.finalize_topk)."""
    import os
    import yaml
    from .. import evalpipe
    from ..datamodule import data_loader as data
    model, _config = _load_for_eval(model_path, data_path)
    dset = data.PrecompDataset(os.path.join(_config['data_path'], _config['data_name']), split, _config)
    comm = comm or evalpipe.Comm()
    lists = {}

    def run(fold, prefix):
        if topk <= 0:
            return evalpipe.evaluate_precomp(model, dset, comm, fold=fold)
        ranks, tl = evalpipe.evaluate_precomp(model, dset, comm, fold=fold, topk=topk)
        lists.update({prefix + key: v for key, v in zip(('i2t_topk', 'i2t_topk_scores', 't2i_topk', 't2i_topk_scores'), tl)})
        return ranks
    if not fold5:
        res_dic = _recall_dict(run(None, ''))
    else:
        res_dic = {'sum_result': []}
        for i in range(5):
            part = _recall_dict(run((i, 5000), f'PART_{i + 1}_'))
            res_dic[f'PART_{i + 1}'] = part
            res_dic['sum_result'] += part['result']
        res_dic['Mean_metrics'] = _mean_metrics(res_dic)
    res_dic['data_name'] = _config['data_name'] + ('_5fold' if fold5 else '')
    if comm.rank == 0:
        with open(os.path.join(os.path.dirname(model_path), f'{res_dic["data_name"]}_single_result.yaml'), 'w') as f:
            yaml.safe_dump(_plain(res_dic), f)
        if topk > 0:
            _save_topk(os.path.dirname(model_path), res_dic['data_name'], 'single', topk, lists)
    return res_dic


def evalrank_single(model_path, data_path=None, split='dev', fold5=False, topk=0, gt=None, hubness=None, hub_k=10, hub_beta=20.0,
                    querybank='self'):
    """evaluation.py:262-335.  topk > 0: also `<data_name>[_5fold]_single_top<topk>.npz` next to the YAML (`topk`).
    gt: path of an `.npz` holding `pairs` [nnz, 2] (image, caption) and optionally n_images / n_captions, a ground-truth relation
    over the gallery (not with fold5): besides everything above, `<data_name>_single_gt_result.yaml` gets R@K, medr, meanr,
    R-Precision and mAP@R of both directions under it and `<data_name>_single_gt_positions.npz` the arrays (`gt_metrics`).
    hubness: 'csls' (hub_k) or 'invsoftmax' (hub_beta): everything above is computed and written exactly as without it, and in
    addition `<data_name>[_5fold]_single_hub_<method>_result.yaml` gets cal_recall of the hubness-corrected matrix
    (`hubness_adjust`) with the method, its parameter and the query bank, and `..._single_hub_<method>.npz` the vectors a and b;
    topk / gt also write `..._single_hub_<method>_top<topk>.npz` / `..._single_hub_<method>_gt_*` from the corrected matrix.
    querybank: 'self' (the evaluated matrix itself: transductive) or a split ('dev', 'train') encoded through the same loader
    (`hubness_bank_vectors`).  fold5 derives the vectors per fold."""
    return _evalrank([model_path], data_path, split, fold5, 'single', topk, gt, hubness, hub_k, hub_beta, querybank)


def evalrank_ensemble(model_path, model_path2, data_path=None, split='dev', fold5=False, topk=0, gt=None, hubness=None, hub_k=10,
                      hub_beta=20.0, querybank='self'):
    """evaluation.py:338-435: the two models' similarity matrices are averaged before ranking.  topk > 0: the top-k lists
    of the float64 average go to `<data_name>[_5fold]_ensemble_top<topk>.npz`.  gt: as evalrank_single, on the float64 average
    -> `<data_name>_ensemble_gt_result.yaml` / `..._ensemble_gt_positions.npz`.  hubness / hub_k / hub_beta / querybank: as
    evalrank_single, on the float64 average -> `<data_name>[_5fold]_ensemble_hub_<method>_result.yaml` / `..._ensemble_hub_<method>.npz`."""
    return _evalrank([model_path, model_path2], data_path, split, fold5, 'ensemble', topk, gt, hubness, hub_k, hub_beta, querybank)


# ---------------------------------------------------------------------------------------------------------
# Coarse-to-fine retrieval: a cheap model shortlists k candidates per query, the cross-attention model scores only those pairs
# (ops.scan_candidate_scores / ops.sgraf_candidate_scores) and re-orders the shortlist (ops.rerank_lists).
def rerank_rank_vector(lists, coarse_ranks, direction, im_div=5):
    """Rank vector of the RERANKED ranking (host arithmetic, numpy only).  The reranked ranking of a query is its k shortlisted
    candidates in fine order followed by all other candidates in coarse order; the rank of a query is the best position of a
    ground-truth candidate in it (evaluation.py:156-222: i2t the best of the image's `im_div` captions, t2i the caption's image).
    A ground truth inside the shortlist therefore has its position in the reranked list; with none inside, the best ground truth
    keeps its coarse rank (the k shortlisted and the same others still stand before it).
    lists: int [n, k] reranked shortlists; coarse_ranks: [n] ranks under the coarse matrix; direction 'i2t' | 't2i'."""
    lists = np.asarray(lists)
    n = lists.shape[0]
    q = np.arange(n)[:, None]
    if direction == 'i2t':
        hit = (lists // im_div) == q
    elif direction == 't2i':
        hit = lists == (q // im_div)
    else:
        raise ValueError("direction must be 'i2t' or 't2i', got %r" % (direction,))
    inside = hit.any(axis=1)
    return np.where(inside, hit.argmax(axis=1), np.asarray(coarse_ranks)).astype(np.float64)


def rerank(sims_coarse, score_fn, k, im_div=5):
    """Both directions of coarse-to-fine retrieval on one (n_img, n_cap) coarse matrix (device float32, or anything
    `_device_matrix` can turn into it): the k-lists of every image (over captions) and of every caption (over images) come from
    the top-k path, `score_fn(cand, by)` (cand int32 device [n, k]; by = 'image' for lists of caption indices per image, 'caption'
    for lists of image indices per caption) returns their fine scores [n, k], and ops.rerank_lists re-orders them.
    -> ((r1, r5, r10, medr, meanr) i2t, the same for t2i, (i2t_ranks, t2i_ranks), lists) with lists = {'i2t_topk', 'i2t_topk_scores',
    't2i_topk', 't2i_topk_scores'} (the reranked lists and their fine scores) as `topk` lays them out."""
    k = _rerank_args("rerank", k)
    r_idx, c_idx, i_rank, t_rank = _materialised_coarse(sims_coarse, k, im_div)
    return _rerank_tail(r_idx, c_idx, i_rank, t_rank, score_fn, None, im_div)


def _rerank_args(who, k, score_fns=None):
    """The argument rules of rerank / rerank_ensemble and their streamed forms -> int(k)."""
    k = int(k)
    if k < 10:
        raise ValueError("%s: k = %d < 10: R@10 would not be defined by the shortlist" % (who, k))
    if score_fns is not None and not 1 <= len(score_fns) <= 4:
        raise ValueError("%s: 1 to 4 fine members, got %d" % (who, len(score_fns)))
    return k


def _rerank_tail(r_idx, c_idx, i_rank, t_rank, score_fn, score_fns, im_div):
    """What follows the coarse stage, whichever way it produced the shortlists (r_idx / c_idx int32 device [n, k]) and the coarse
    ranks (host [n]): fine scores, ops.rerank_lists (score_fn) or ops.rerank_fused_lists (score_fns, the ensemble), the reranked
    rank vectors.  -> `rerank`'s / `rerank_ensemble`'s tuple.  The materialised and the streamed forms both end here."""
    if score_fns is None:
        fine_i = score_fn(r_idx, 'image')
        fine_t = score_fn(c_idx, 'caption')
        ri, rv, _ = ops.rerank_lists(r_idx, fine_i)
        ci, cv, _ = ops.rerank_lists(c_idx, fine_t)
        lists = {'i2t_topk': ri.cpu().numpy().astype(np.int64), 'i2t_topk_scores': rv.cpu().numpy(),
                 't2i_topk': ci.cpu().numpy().astype(np.int64), 't2i_topk_scores': cv.cpu().numpy()}
    else:
        fine_i, fine_t = [], []
        for f in score_fns:
            fn = f() if _is_factory(f) else f
            fine_i.append(fn(r_idx, 'image'))
            fine_t.append(fn(c_idx, 'caption'))
            del fn                                # a factory's state goes before the next member's is built
        ri, rf, rv, _ = ops.rerank_fused_lists(r_idx, fine_i)
        ci, cf, cv, _ = ops.rerank_fused_lists(c_idx, fine_t)
        lists = {'i2t_topk': ri.cpu().numpy().astype(np.int64), 'i2t_topk_scores': rf.cpu().numpy(),
                 'i2t_topk_member_scores': rv.cpu().numpy(),
                 't2i_topk': ci.cpu().numpy().astype(np.int64), 't2i_topk_scores': cf.cpu().numpy(),
                 't2i_topk_member_scores': cv.cpu().numpy()}
    i_ranks = rerank_rank_vector(lists['i2t_topk'], i_rank, 'i2t', im_div)
    t_ranks = rerank_rank_vector(lists['t2i_topk'], t_rank, 't2i', im_div)
    return ops.recall_from_ranks(i_ranks), ops.recall_from_ranks(t_ranks), (i_ranks, t_ranks), lists


def _materialised_coarse(sims_coarse, k, im_div):
    """The coarse stage of `rerank` / `rerank_ensemble` on a stored matrix: the k-lists of both directions from the top-k path
    (int32, on the device) and the coarse rank vectors (host) -> (r_idx, c_idx, i_rank, t_rank)."""
    S = _device_matrix(sims_coarse)
    if S.dtype != torch.float32:
        S = S.to(torch.float32)
    r_idx, _, part = ops.topk_lists(S, k)
    c_idx, _ = ops.topk_merge_cols([part], k)
    i_rank, _, t_rank, _, _ = ops.rank_counts(S, im_div)
    return r_idx, c_idx, i_rank.cpu().numpy(), t_rank.cpu().numpy()


def _streamed_coarse(img_emb, cap_emb, coarse_score_fn, k, im_div):
    """The coarse stage of `rerank_streamed` / `rerank_ensemble_streamed`: evalpipe.score_topk_streamed -> the shortlists back on
    the device (int32, what the fine scorers take) and the streamed coarse rank tuple."""
    from .. import evalpipe
    dev = torch.device('cuda', torch.cuda.current_device())
    img = img_emb if torch.is_tensor(img_emb) else torch.from_numpy(np.ascontiguousarray(img_emb))
    cap = cap_emb if torch.is_tensor(cap_emb) else torch.from_numpy(np.ascontiguousarray(cap_emb))
    (i_idx, _, t_idx, _), ranks = evalpipe.score_topk_streamed(img.to(dev), cap.to(dev), coarse_score_fn, k, im_div)
    r_idx = torch.from_numpy(i_idx.astype(np.int32)).to(dev)
    c_idx = torch.from_numpy(t_idx.astype(np.int32)).to(dev)
    return r_idx, c_idx, ranks


def rerank_streamed(img_emb, cap_emb, coarse_score_fn, score_fn, k, im_div=5, return_coarse_ranks=False):
    """`rerank` for a gallery whose coarse matrix does not fit: the shortlists and the coarse ranks come from
    evalpipe.score_topk_streamed(img_emb, cap_emb, coarse_score_fn, k) -- the matrix is scored in cache-sized row blocks and never
    stored, neither on the device nor on the host -- and everything after the coarse stage is `rerank`'s own code (_rerank_tail).
    coarse_score_fn(img_rows, cap, out=) is a pooled scorer (ops.cosine_scores, ops.order_scores, ops.pdist_cos, ops.mvm_scores).
    -> `rerank`'s tuple, entry for entry that of rerank(coarse_score_fn(img_emb, cap_emb), score_fn, k); with
    return_coarse_ranks=True also the streamed coarse rank tuple (i2t_rank, i2t_top1, t2i_rank, t2i_top1)."""
    k = _rerank_args("rerank_streamed", k)
    r_idx, c_idx, ranks = _streamed_coarse(img_emb, cap_emb, coarse_score_fn, k, im_div)
    out = _rerank_tail(r_idx, c_idx, ranks[0], ranks[2], score_fn, None, im_div)
    return (out, ranks) if return_coarse_ranks else out


def rerank_ensemble_streamed(img_emb, cap_emb, coarse_score_fn, score_fns, k, im_div=5, return_coarse_ranks=False):
    """`rerank_ensemble` with `rerank_streamed`'s coarse stage (the coarse matrix is never stored).  -> `rerank_ensemble`'s tuple."""
    score_fns = list(score_fns)
    k = _rerank_args("rerank_ensemble_streamed", k, score_fns)
    r_idx, c_idx, ranks = _streamed_coarse(img_emb, cap_emb, coarse_score_fn, k, im_div)
    out = _rerank_tail(r_idx, c_idx, ranks[0], ranks[2], None, score_fns, im_div)
    return (out, ranks) if return_coarse_ranks else out


def _streamed_coarse_scorer(name, cfg, who):
    """The pooled op cal_sims reaches for a coarse family (evalpipe.PooledModelEval._score has the same mapping), in its out= form."""
    if name in ('SCAN', 'SGRAF'):
        raise NotImplementedError("%s: stream_coarse needs a pooled coarse model (one vector per caption); the dense scorer of %s is not "
                                  "streamed" % (who, name))
    if name == 'CAMERA':
        return ops.mvm_scores
    if name == 'SAEM':
        if cfg.get('measure') == 'order':
            raise NotImplementedError("%s: stream_coarse has no streamed form of SAEM's euclidean pdist (measure = order)" % who)
        return ops.pdist_cos
    return ops.order_scores if cfg.get('measure') == 'order' else ops.cosine_scores


def explain(lists, score_fn, m):
    """Why the fine model preferred a result: the word-by-region attention of the best `m` results of every query in both
    directions.  lists: `rerank`'s (reranked) lists; score_fn: a fine scorer that can explain (`_scan_score_fn`'s: SCAN); 1 <= m <= k.
    -> dict of host arrays, per direction d in ('i2t', 't2i'): d_idx int64 [n, m] (query-major: the first m columns of d_topk),
    d_scores float32 [n, m] (fine scores), d_attn float32 (flat; pair q * m + j holds its [W, 36] word-major block at d_attn_ptr),
    d_attn_ptr int64 [n m + 1], d_row_sim (t2i model: one cosine per word at d_row_ptr; i2t model: 36 per pair), d_row_ptr int64
    [n m + 1], d_cap_len int32 [n m].  With the data layer's `boxes`, region r of d_attn's column r is the box to draw."""
    attention = getattr(score_fn, 'attention', None)
    if attention is None:
        raise NotImplementedError("explain: attention maps exist for a SCAN fine model only (an SGRAF scorer explains itself through explain_sgraf)")
    return _explain_both("explain", lists, attention, m, lambda a: ('row_sim', 'row_ptr', 'cap_len'))


def _explain_both(who, lists, explainer, m, own):
    """The two directions of `explain` / `explain_sgraf`: the first m columns of each direction's lists go to the device,
    explainer(cand, by, m) -> ops.ScanPairAttention / ops.SgrafPairAttention `a`, and its arrays come back under 'i2t_' / 't2i_':
    idx, scores, attn, attn_ptr, then the attributes own(a) names."""
    m = int(m)
    out = {}
    for d, by in (('i2t', 'image'), ('t2i', 'caption')):
        idx = np.asarray(lists[d + '_topk'])
        if m < 1 or m > idx.shape[1]:
            raise ValueError("%s: m = %d outside [1, %d]" % (who, m, idx.shape[1]))
        dev = torch.device('cuda', torch.cuda.current_device())
        cand = torch.from_numpy(np.ascontiguousarray(idx[:, :m]).astype(np.int32)).to(dev)
        a = explainer(cand, by, m)
        n = idx.shape[0]
        out.update({d + '_idx': idx[:, :m].astype(np.int64), d + '_scores': a.score.cpu().numpy().reshape(n, m),
                    d + '_attn': a.attn.cpu().numpy(), d + '_attn_ptr': a.attn_ptr.cpu().numpy()})
        out.update({d + '_' + name: getattr(a, name).cpu().numpy() for name in own(a)})
    return out


_explain_lists = explain          # evalrank_rerank's keyword `explain` hides the function there


def explain_sgraf(lists, score_fn, m):
    """Why an SGRAF fine model preferred a result: for the best `m` results of every query in both directions, the word-by-region
    attention, SAF's filtration weights over the alignment nodes or SGR's graph edges at every step, and the score.
    lists: `rerank`'s (reranked) lists; score_fn: `_sgraf_score_fn`'s (it carries `reasoning`); 1 <= m <= k.
    -> dict of host arrays, per direction d in ('i2t', 't2i'): d_idx int64 [n, m], d_scores float32 [n, m], d_attn float32 (flat;
    pair q * m + j holds its [W, 36] word-major block at d_attn_ptr), d_attn_ptr int64 [n m + 1], then for SAF d_node_w /
    d_node_ptr (W + 1 weights per pair, node 0 = the global node) or for SGR d_edge / d_edge_ptr ([sgr_step, W + 1, W + 1] per
    pair), d_cap_len int32 [n m] and d_explained bool [n m] (False: a caption of more than 63 words, scored but with empty blocks)."""
    reasoning = getattr(score_fn, 'reasoning', None)
    if reasoning is None:
        raise NotImplementedError("explain_sgraf: reasoning maps exist for an SGRAF fine model only (SCAN: explain)")
    return _explain_both("explain_sgraf", lists, reasoning, m,
                         lambda a: ('cap_len', 'explained') + (('node_w', 'node_ptr') if a.node_w is not None else ('edge', 'edge_ptr')))


_explain_sgraf_lists = explain_sgraf


def _packed_words(img_embs, cap_embs, cap_lens):
    """encode_data's padded word-level embeddings -> (images, packed words, ScanPlan) on the current device"""
    dev = torch.device('cuda', torch.cuda.current_device())
    lens = np.asarray(cap_lens, dtype=np.int64)
    images = torch.from_numpy(np.ascontiguousarray(img_embs)).to(dev)
    caps = torch.from_numpy(np.ascontiguousarray(cap_embs)).to(dev)
    L = caps.shape[1]
    keep = (torch.arange(L, device=dev)[None, :] < torch.from_numpy(lens).to(dev)[:, None]).reshape(-1)
    words = caps.reshape(-1, caps.shape[2])[keep].contiguous()
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    return images, words, ops.ScanPlan(off, lens.astype(np.int32), words.shape[0], dev)


def _sgraf_score_fn(model, img_embs, cap_embs, cap_lens):
    """score_fn of `rerank` for an SGRAF model (SAF or SGR): the captions packed once, the per-image / per-caption state (global
    vectors, Gram matrices, SGR's folded weights) prepared once and used for both list directions.
    Its attribute `reasoning(cand, by, m)` is ops.sgraf_candidate_attention on the same operands and state (`explain_sgraf`)."""
    images, words, plan = _packed_words(img_embs, cap_embs, cap_lens)
    enc = model.sim_enc
    weights = {k_: v.detach() for k_, v in enc.state_dict().items()}
    state = ops.sgraf_pairs_prepare(images, words, plan, weights, enc.module_name, enc.sgr_step)
    kw = dict(module_name=enc.module_name, sgr_step=enc.sgr_step, state=state)

    def fn(cand, by):
        return ops.sgraf_candidate_scores(images, words, plan, weights, cand, by, **kw)
    fn.reasoning = lambda cand, by, m: ops.sgraf_candidate_attention(images, words, plan, weights, cand, by, m=m, **kw)
    return fn


def _scan_score_fn(model, img_embs, cap_embs, cap_lens):
    """score_fn of `rerank` for a SCAN model: its word-level caption embeddings packed once, the pair workspace prepared once.
    Its attribute `attention(cand, by, m)` is ops.scan_candidate_attention on the same operands and workspace (`explain`)."""
    cfg = model.config
    images, words, plan = _packed_words(img_embs, cap_embs, cap_lens)
    kw = dict(cross_attn=cfg['cross_attn'], raw_feature_norm=cfg['raw_feature_norm'], agg_func=cfg['agg_func'],
              lambda_lse=cfg['lambda_lse'], lambda_softmax=cfg['lambda_softmax'])
    ws = ops.scan_pairs_prepare(images, words, plan, cfg['cross_attn'])

    def fn(cand, by):
        return ops.scan_candidate_scores(images, words, plan, cand, by, workspace=ws, **kw)
    fn.attention = lambda cand, by, m: ops.scan_candidate_attention(images, words, plan, cand, by, m=m, workspace=ws, **kw)
    return fn


def evalrank_rerank(model_path_coarse, model_path_fine, k, data_path=None, split='dev', fold5=False, explain=None, explain_sgraf=None,
                    stream_coarse=False):
    """Coarse-to-fine evaluation: the coarse model (any family evalrank_single scores) shortlists k candidates per query in both
    directions, the fine model -- SCAN (either cross_attn) or SGRAF (SAF or SGR) -- scores only those pairs, Recall@K is that of the reranked ranking
    (`rerank`).  Writes `<data_name>[_5fold]_rerank<k>_result.yaml` (the coarse-only numbers under 'coarse', the reranked ones
    under 'rerank') and the reranked lists `<data_name>[_5fold]_rerank<k>.npz` next to the coarse checkpoint.
    explain=M (1 <= M <= k, SCAN fine model, not with fold5): after re-ordering, the best M results of every query in both
    directions are explained (`explain`) and written to `<data_name>_rerank<k>_explain<M>.npz` next to the other files.
    explain_sgraf=M (the same rules, SGRAF fine model): `explain_sgraf`'s arrays go to `<data_name>_rerank<k>_explain<M>_sgraf.npz`.
    stream_coarse=True (pooled coarse models: VSE++ cosine / order, SAEM cosine, CAMERA; SCAN / SGRAF -> NotImplementedError): the
    coarse embeddings go to the device once and the coarse stage is `rerank_streamed`'s -- neither the fp32 nor the float64 coarse
    matrix is ever built; the 'coarse' block comes from the streamed ranks.  Same files, same keys."""
    return _evalrank_rerank("evalrank_rerank", False, model_path_coarse, [model_path_fine], k, data_path, split, fold5, explain, explain_sgraf,
                            stream_coarse)


def _evalrank_rerank(who, ensemble, model_path_coarse, model_paths_fine, k, data_path, split, fold5, explain, explain_sgraf, stream_coarse):
    """The driver of `evalrank_rerank` (ensemble=False: one fine checkpoint, its float32 scores re-order the lists through `rerank`)
    and `evalrank_rerank_ensemble` (ensemble=True: 1 to 4, fused in float64 through `rerank_ensemble`, also when there is one: the
    two forms write different scores and files).  The forms differ in the fine stage of a block, the file stem, the YAML key of
    the fine path(s), the printed lines and the explanation files' names; everything else is here once."""
    import os
    import yaml
    from ..datamodule import data_loader as data
    k = int(k)
    if k < 10:
        raise ValueError("%s: k = %d < 10: R@10 would not be defined by the shortlist" % (who, k))
    if ensemble and not 1 <= len(model_paths_fine) <= 4:
        raise ValueError("%s: 1 to 4 fine checkpoints, got %d" % (who, len(model_paths_fine)))
    one = 'member' if ensemble else 'fine model'
    wanted = {}
    for name, m in (('explain', explain), ('explain_sgraf', explain_sgraf)):
        if m is None:
            continue
        if fold5:
            raise ValueError("%s: %s does not combine with fold5" % (who, name))
        if int(m) < 1 or int(m) > k:
            raise ValueError("%s: %s = %d outside [1, k = %d]" % (who, name, int(m), k))
        wanted[name] = int(m)
    coarse, c_cfg = _load_for_eval(model_path_coarse, data_path)
    fines = [_load_for_eval(p, data_path) for p in model_paths_fine]
    families = [f_cfg['name'] for _, f_cfg in fines]
    for family in families:
        if family not in ('SCAN', 'SGRAF'):
            raise NotImplementedError("%s: %s fine model must be SCAN or SGRAF (candidate-list scoring exists for these only), got %s"
                                      % (who, 'every' if ensemble else 'the', family))

    def coarse_scorer():
        return _streamed_coarse_scorer(c_cfg['name'], c_cfg, who) if stream_coarse else None
    if ensemble:               # (the ensemble refuses an unstreamable coarse model before the explain rules, the single form after: kept)
        coarse_fn = coarse_scorer()
    if 'explain' in wanted and 'SCAN' not in families:
        raise NotImplementedError("%s: explain needs a SCAN %s (attention maps exist for SCAN only; an SGRAF %s explains itself through "
                                  "explain_sgraf), got %s" % (who, one, one, ', '.join(families)))
    if 'explain_sgraf' in wanted and 'SGRAF' not in families:
        raise NotImplementedError("%s: explain_sgraf needs an SGRAF %s (a SCAN %s explains itself through explain), got %s"
                                  % (who, one, one, ', '.join(families)))
    if not ensemble:
        coarse_fn = coarse_scorer()
    for _, f_cfg in fines:
        if f_cfg['data_name'] != c_cfg['data_name']:
            raise ValueError("%s: the checkpoints name different datasets (%s, %s): their lists would not index the same items"
                             % (who, c_cfg['data_name'], f_cfg['data_name']))
    embs = []
    for model, cfg in [(coarse, c_cfg)] + fines:
        loader, _ = data.get_test_loader(split, cfg['data_name'], cfg['batch_size'], cfg['workers'], cfg)
        embs.append(encode_data(model, loader, islength=cfg['name'] in ['SGRAF', 'SCAN']))
    (c_img, c_cap, c_len), f_embs = embs[0], embs[1:]
    for f_img, f_cap, _ in f_embs:
        if len(c_img) != len(f_img) or len(c_cap) != len(f_cap):
            raise ValueError("%s: the models' loaders hold different item counts (%d / %d images, %d / %d captions)"
                             % (who, len(c_img), len(f_img), len(c_cap), len(f_cap)))
    lists = {}
    explained = {}             # file suffix -> arrays

    if stream_coarse:                          # the coarse embeddings go to the device once; blocks below are views of them
        dev = torch.device('cuda', torch.cuda.current_device())
        c_img_dev = torch.from_numpy(np.ascontiguousarray(c_img)).to(dev)
        c_cap_dev = torch.from_numpy(np.ascontiguousarray(c_cap)).to(dev)

    def block(sl_img, sl_cap, prefix):
        def factory(j):
            make = _scan_score_fn if families[j] == 'SCAN' else _sgraf_score_fn
            f_img, f_cap, f_len = f_embs[j]
            return lambda: make(fines[j][0], f_img[sl_img], f_cap[sl_cap], f_len[sl_cap])
        factories = [factory(j) for j in range(len(fines))]
        # the ensemble hands the factories on: one member's device state at a time.  The single form builds its scorer here, where it
        # always did (before a streamed coarse stage, after a stored one), and keeps it for the explanation.
        fn = None
        if stream_coarse:
            img, cap = c_img_dev[sl_img].contiguous(), c_cap_dev[sl_cap]
            if ensemble:
                fine, c_ranks = rerank_ensemble_streamed(img, cap, coarse_fn, factories, k, return_coarse_ranks=True)
            else:
                fn = factories[0]()
                fine, c_ranks = rerank_streamed(img, cap, coarse_fn, fn, k, return_coarse_ranks=True)
            res_c = _recall_dict(c_ranks)
        else:
            sims = cal_sims(coarse, c_img[sl_img], c_cap[sl_cap], lengths=c_len[sl_cap], shard_size=c_cfg['batch_size'] * 5)
            res_c = cal_recall(sims)
            if ensemble:
                fine = rerank_ensemble(sims.astype(np.float32), factories, k)
            else:
                fn = factories[0]()
                fine = rerank(sims.astype(np.float32), fn, k)
        r, ri, (i_ranks, t_ranks), tl = fine
        lists.update({prefix + key: v for key, v in tl.items()})
        for j, family in enumerate(families):          # (ensemble: one member's state at a time, rebuilt for the explanation)
            member = '_member%d' % (j + 1) if ensemble else ''
            if family == 'SCAN' and 'explain' in wanted:
                explained['explain%d%s' % (wanted['explain'], member)] = _explain_lists(tl, fn or factories[j](), wanted['explain'])
            if family == 'SGRAF' and 'explain_sgraf' in wanted:
                explained['explain%d%s_sgraf' % (wanted['explain_sgraf'], member)] = _explain_sgraf_lists(tl, fn or factories[j](),
                                                                                                         wanted['explain_sgraf'])
        res_r = _recall_dict((i_ranks, tl['i2t_topk'][:, 0], t_ranks, tl['t2i_topk'][:, 0]))
        what = "Ensemble of %d reranked" % len(fines) if ensemble else "Reranked"
        print("%s (k = %d) image to text: r1 %.1f; r5 %.1f; r10 %.1f; medr %.1f; meanr %.1f" % ((what, k) + tuple(r)))
        print("%s (k = %d) text to image: r1 %.1f; r5 %.1f; r10 %.1f; medr %.1f; meanr %.1f" % ((what, k) + tuple(ri)))
        return res_c, res_r

    n = len(c_img)
    if not fold5:
        res_c, res_r = block(slice(0, n, 5), slice(None), '')
        res_dic = {'coarse': res_c, 'rerank': res_r}
    else:
        res_dic = {'coarse': {'sum_result': []}, 'rerank': {'sum_result': []}}
        for i in range(5):
            res_c, res_r = block(slice(i * 5000, (i + 1) * 5000, 5), slice(i * 5000, (i + 1) * 5000), f'PART_{i + 1}_')
            for key, part in (('coarse', res_c), ('rerank', res_r)):
                res_dic[key][f'PART_{i + 1}'] = part
                res_dic[key]['sum_result'] += part['result']
        for key in ('coarse', 'rerank'):
            res_dic[key]['Mean_metrics'] = _mean_metrics(res_dic[key])
    res_dic['data_name'] = c_cfg['data_name'] + ('_5fold' if fold5 else '')
    res_dic['k'] = k
    res_dic['modal_path_coarse'] = model_path_coarse
    if ensemble:
        res_dic['modal_paths_fine'] = list(model_paths_fine)
    else:
        res_dic['modal_path_fine'] = model_paths_fine[0]
    stem = os.path.join(os.path.dirname(model_path_coarse), f'{res_dic["data_name"]}_rerank{k}' + ('_ensemble' if ensemble else ''))
    with open(stem + '_result.yaml', 'w') as f:
        yaml.safe_dump(_plain(res_dic), f)
    np.savez(stem + '.npz', **lists)
    for suffix, arrays in explained.items():
        np.savez(stem + '_' + suffix + '.npz', **arrays)
    return res_dic


# ---------------------------------------------------------------------------------------------------------
# Ensemble reranking: several fine models score the same shortlists, the lists are re-ordered by the float64 mean of their scores
# (ops.rerank_fused_lists) -- evalrank_ensemble's average (evaluation.py:377-381) restricted to the listed pairs.
def _is_factory(f):
    """A zero-argument factory of a score_fn (as opposed to a score_fn, which takes (cand, by))"""
    import inspect
    try:
        params = inspect.signature(f).parameters.values()
    except (TypeError, ValueError):
        return False
    return not any(p.default is p.empty and p.kind in (p.POSITIONAL_ONLY, p.POSITIONAL_OR_KEYWORD) for p in params)


def rerank_ensemble(sims_coarse, score_fns, k, im_div=5):
    """`rerank` with an ensemble of 1 to 4 fine models: the k-lists of both directions come from the coarse matrix exactly as in
    `rerank`, every member scores the same two lists, and ops.rerank_fused_lists re-orders them by the fused score -- the float64
    sum of the members' scores in the order given, divided by their number (evalrank_ensemble's average on the listed pairs).
    score_fns: a sequence of `score_fn(cand, by)` as `rerank` takes them, or of zero-argument factories returning one: a member's
    device state is then built, used for both directions and released before the next member's is built.
    -> `rerank`'s tuple; in lists, 'i2t_topk_scores' / 't2i_topk_scores' are the float64 fused scores and 'i2t_topk_member_scores'
    / 't2i_topk_member_scores' (float32 [M, n, k]) what each member gave the entries, in the reranked order."""
    score_fns = list(score_fns)
    k = _rerank_args("rerank_ensemble", k, score_fns)
    r_idx, c_idx, i_rank, t_rank = _materialised_coarse(sims_coarse, k, im_div)
    return _rerank_tail(r_idx, c_idx, i_rank, t_rank, None, score_fns, im_div)


def evalrank_rerank_ensemble(model_path_coarse, model_paths_fine, k, data_path=None, split='dev', fold5=False, explain=None,
                             explain_sgraf=None, stream_coarse=False):
    """`evalrank_rerank` with an ensemble of 1 to 4 fine checkpoints, each SCAN (either cross_attn) or SGRAF (SAF or SGR), in any
    mix: the coarse model shortlists k candidates per query in both directions, every fine model scores those pairs, the lists are
    re-ordered by the float64 mean of the members' scores (`rerank_ensemble`; SAF + SGR is the published SGRAF, SCAN t2i + i2t the
    published SCAN).  One member's device state exists at a time.  Writes `<data_name>[_5fold]_rerank<k>_ensemble_result.yaml`
    ('coarse', 'rerank', 'k', 'data_name', 'modal_path_coarse', 'modal_paths_fine') and `<data_name>[_5fold]_rerank<k>_ensemble.npz`
    (the reranked lists, their fused scores and every member's scores) next to the coarse checkpoint; evalrank_rerank's files
    are not touched.
    explain=M / explain_sgraf=M (1 <= M <= k, not with fold5): the fused best M results of every query are explained by every SCAN /
    every SGRAF member (`explain` / `explain_sgraf` on the fused lists, one member at a time), member j (1-based position among
    the fine checkpoints) in `<data_name>_rerank<k>_ensemble_explain<M>_member<j>.npz` / `..._member<j>_sgraf.npz`.
    stream_coarse=True: as in `evalrank_rerank` -- the coarse matrix is never built (`rerank_ensemble_streamed`)."""
    model_paths_fine = [model_paths_fine] if isinstance(model_paths_fine, str) else list(model_paths_fine)
    return _evalrank_rerank("evalrank_rerank_ensemble", True, model_path_coarse, model_paths_fine, k, data_path, split, fold5, explain,
                            explain_sgraf, stream_coarse)
