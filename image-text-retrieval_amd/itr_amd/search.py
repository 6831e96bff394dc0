"""Query-time search: an encoded gallery that stays on the device and answers "here is a sentence (or an image), give me the k
best gallery items".

The evaluation (metricmodule/evaluation.py) ranks a whole split against itself; `GalleryIndex` holds what that evaluation encodes --
the pooled embeddings of a coarse model, optionally the region / word embeddings of a fine model -- and scores a handful of queries
against them: the coarse lists come from `ops.search_topk` (csrc/search.hip: one pass over the gallery, the score matrix is never
written), a fine model re-scores the shortlisted pairs only (`ops.scan_candidate_scores` / `ops.sgraf_candidate_scores`) and
`ops.rerank_lists` re-orders them.  The lists are, bit for bit, the rows of `evaluation.topk` / `evaluation.rerank` for the same
queries."""
import hashlib
import os

import numpy as np
import torch

from . import ops
from .metricmodule import evaluation


def fused_wins(n_queries, n_gallery, k):
    """Where ops.search_topk was measured faster than ops.cosine_scores + ops.topk_lists (tools/search_bench.py, D = 1 024, one
    MI355X): large galleries, and the fewer queries and the shorter the lists the earlier.  Both routes give the
    same bytes, so this routing is invisible to results."""
    if n_gallery < 100000:                 # 5 000 rows: the matrix path wins or ties in every cell; 113 287: see below
        return False
    big = n_gallery >= 500000
    if n_queries <= 4:
        return True
    if n_queries <= 16:
        return k <= 10 or big
    return big and k <= 10


def _sha256(path):
    h = hashlib.sha256()
    with open(path, 'rb') as f:
        for block in iter(lambda: f.read(1 << 20), b''):
            h.update(block)
    return h.hexdigest()


def _check_coarse(cfg):
    """The coarse families whose evaluation score is ops.cosine_scores of pooled embeddings (evaluation._streamed_coarse_scorer is the
    mapping); every other family is refused with the reason."""
    name = cfg['name']
    if name in ('SCAN', 'SGRAF'):
        raise NotImplementedError("GalleryIndex: %s cannot be the coarse model: it has no pooled embedding, every pair needs its "
                                  "cross-attention score; use it as the fine model behind a VSE++ or VSRN coarse model" % name)
    if name == 'CAMERA':
        raise NotImplementedError("GalleryIndex: a CAMERA coarse model scores the max over its views (ops.mvm_scores), not a cosine "
                                  "of one vector per item")
    if name == 'SAEM':
        raise NotImplementedError("GalleryIndex: a SAEM coarse model scores through pdist_cos, whose NaN -> 0 rule is not the "
                                  "fused search's cosine")
    if cfg.get('measure') == 'order':
        raise NotImplementedError("GalleryIndex: measure=order scores the order-embedding violation, not a cosine")
    if evaluation._streamed_coarse_scorer(name, cfg, "GalleryIndex") is not ops.cosine_scores:
        raise NotImplementedError("GalleryIndex: the coarse family %s is not scored by ops.cosine_scores" % name)


def _check_fine(cfg):
    if cfg['name'] not in ('SCAN', 'SGRAF'):
        raise NotImplementedError("GalleryIndex: the fine model must be SCAN or SGRAF (candidate-list scoring exists for these only), "
                                  "got %s" % cfg['name'])


def _dev():
    return torch.device('cuda', torch.cuda.current_device())


def _to_dev(a):
    return a.to(_dev()) if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


class Query(object):
    """Encoded queries: `coarse` float32 [n, D]; with a fine model `fine` (captions: word embeddings zero-padded to [n, L, D] with
    `lens`; images: regions [n, 36, D]); `token_ids` for sentences."""

    def __init__(self, kind, coarse, fine=None, lens=None, token_ids=None):
        self.kind, self.coarse, self.fine, self.lens, self.token_ids = kind, coarse, fine, lens, token_ids

    def __len__(self):
        return len(self.coarse)


class SearchResult(object):
    """`idx` int64 [n, k] (distinct images of the split for 't2i', captions for 'i2t'; -1 past the gallery), `scores` float32 [n, k]
    (the fine model's when reranked, else the coarse cosines), `coarse_idx` / `coarse_scores` [n, K'] the coarse shortlist."""

    def __init__(self, direction, idx, scores, coarse_idx, coarse_scores):
        self.direction, self.idx, self.scores, self.coarse_idx, self.coarse_scores = direction, idx, scores, coarse_idx, coarse_scores

    def arrays(self):
        return {'idx': self.idx, 'scores': self.scores, 'coarse_idx': self.coarse_idx, 'coarse_scores': self.coarse_scores}


class GalleryIndex(object):
    """An encoded gallery (the distinct images and all captions of a split) resident on the device.

    Coarse model: a family whose evaluation score is the cosine of pooled embeddings (VSE++ with measure=cosine, VSRN); order
    embeddings, SAEM, CAMERA and SCAN / SGRAF are refused with the reason.  Fine model (optional): SCAN (either cross_attn) or SGRAF
    (SAF / SGR), which re-scores the coarse shortlist."""

    def __init__(self):
        self.coarse_model = self.fine_model = self.dataset = None
        self.meta = {'data_name': '', 'split': '', 'im_div': 5, 'sha256_coarse': '', 'sha256_fine': ''}
        self.route = 'auto'                # 'fused' / 'matrix' pin the coarse route (`fused_wins` decides otherwise); same bytes either way
        self._host = {}

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_embeddings(cls, coarse, fine=None, fine_model=None, im_div=5, coarse_model=None, dataset=None):
        """An index over arrays the caller already holds, in `evaluation.encode_data`'s layout (one row per caption; image rows
        repeated im_div times): coarse = (img_embs [n, D], cap_embs [n, D]); fine = (img_embs [n, 36, D], cap_embs [n, L, D] padded
        word embeddings, cap_lens [n]) with fine_model, the SCAN / SGRAF model that scores them.  Distinct images are
        img_embs[::im_div], as in the evaluation.  coarse_model / dataset are needed only by `encode_text` / `encode_images`."""
        self = cls()
        if coarse_model is not None:
            _check_coarse(coarse_model.config)
        if (fine is None) != (fine_model is None):
            raise ValueError("GalleryIndex.from_embeddings: pass fine embeddings and fine_model together, or neither")
        if fine_model is not None:
            _check_fine(fine_model.config)
        self.coarse_model, self.fine_model, self.dataset = coarse_model, fine_model, dataset
        self.meta['im_div'] = int(im_div)
        c_img, c_cap = coarse
        self._host = {'coarse_img': np.ascontiguousarray(np.asarray(c_img, np.float32)[::im_div]),
                      'coarse_cap': np.ascontiguousarray(np.asarray(c_cap, np.float32))}
        if fine is not None:
            f_img, f_cap, f_len = fine
            self._host.update(fine_img=np.ascontiguousarray(np.asarray(f_img, np.float32)[::im_div]),
                              fine_cap=np.ascontiguousarray(np.asarray(f_cap, np.float32)), fine_lens=np.asarray(f_len, np.int32))
        self._upload()
        return self

    @classmethod
    def build(cls, coarse_path, fine_path=None, data_path=None, split='test', sides=('images', 'captions')):
        """Load the checkpoints (`evaluation._load_for_eval`), encode `split` once (`evaluation.encode_data`) and keep its distinct
        images and all its captions on the device.  sides: which galleries to keep ('images' answers sentences, 'captions' images)."""
        from .datamodule import data_loader as data
        coarse, c_cfg = evaluation._load_for_eval(coarse_path, data_path)
        _check_coarse(c_cfg)
        fine = f_cfg = None
        if fine_path is not None:
            fine, f_cfg = evaluation._load_for_eval(fine_path, data_path)
            _check_fine(f_cfg)
            if f_cfg['data_name'] != c_cfg['data_name']:
                raise ValueError("GalleryIndex.build: the checkpoints name different datasets (%s, %s)" % (c_cfg['data_name'], f_cfg['data_name']))
        embs = []
        for model, cfg in ((coarse, c_cfg), (fine, f_cfg)):
            if model is None:
                continue
            loader, _ = data.get_test_loader(split, cfg['data_name'], cfg['batch_size'], cfg['workers'], cfg)
            embs.append(evaluation.encode_data(model, loader, islength=cfg['name'] in ('SGRAF', 'SCAN')))
            dataset = loader.dataset
            im_div = 5                         # encode_data repeats an image row for each of its captions (evaluation.py: [::5])
        self = cls.from_embeddings(embs[0][:2], embs[1] if fine is not None else None, fine, im_div, coarse, dataset)
        self._drop_sides(sides)
        self.meta.update(data_name=c_cfg['data_name'], split=split, sha256_coarse=_sha256(coarse_path),
                         sha256_fine=_sha256(fine_path) if fine_path is not None else '')
        return self

    def save(self, path):
        """One .npz: the embeddings, lengths, data_name, split, im_div and the sha256 of each checkpoint file."""
        arrays = dict(self._host)
        arrays.update({k: np.asarray(v) for k, v in self.meta.items()})
        with open(path, 'wb') as f:
            np.savez(f, **arrays)
        return path

    @classmethod
    def load(cls, path, coarse_path, fine_path=None, data_path=None):
        """An index saved by `save`, with the checkpoints it was built from (needed to encode queries).  Raises ValueError if a
        checkpoint file's sha256 differs from the recorded one.  No encoding is performed."""
        from .datamodule import data_loader as data
        with np.load(path, allow_pickle=False) as z:
            arrays = {k: z[k] for k in z.files}
        self = cls()
        for k in self.meta:
            v = arrays.pop(k)
            self.meta[k] = int(v) if k == 'im_div' else str(v)
        for what, p, key in (('coarse', coarse_path, 'sha256_coarse'), ('fine', fine_path, 'sha256_fine')):
            have = _sha256(p) if p is not None else ''
            if have != self.meta[key]:
                raise ValueError("GalleryIndex.load: %s was built from a different %s checkpoint (sha256 %s..., %s has %s...)"
                                 % (path, what, self.meta[key][:12] or 'none', p, have[:12] or 'none'))
        self._host = arrays
        self.coarse_model, c_cfg = evaluation._load_for_eval(coarse_path, data_path)
        _check_coarse(c_cfg)
        if fine_path is not None:
            self.fine_model, f_cfg = evaluation._load_for_eval(fine_path, data_path)
            _check_fine(f_cfg)
        self.dataset = data.PrecompDataset(os.path.join(c_cfg['data_path'], c_cfg['data_name']), self.meta['split'], c_cfg)
        self._upload()
        return self

    def _drop_sides(self, sides):
        sides = tuple(sides)
        if not sides or any(s not in ('images', 'captions') for s in sides):
            raise ValueError("GalleryIndex: sides must name 'images' and / or 'captions', got %r" % (sides,))
        drop = [k for k in self._host if ('images' not in sides and k.endswith('_img')) or
                ('captions' not in sides and (k.endswith('_cap') or k == 'fine_lens'))]
        for k in drop:
            del self._host[k]
        self._upload()

    def _upload(self):
        h = self._host
        self.coarse = {side: _to_dev(h[key]) for side, key in (('images', 'coarse_img'), ('captions', 'coarse_cap')) if key in h}
        self.fine = {}
        if 'fine_img' in h:
            self.fine['images'] = _to_dev(h['fine_img'])
        if 'fine_cap' in h:
            _, words, plan = evaluation._packed_words(np.zeros((1, 1, 1), np.float32), h['fine_cap'], h['fine_lens'])
            self.fine['captions'] = (words, plan)

    # ------------------------------------------------------------------ queries
    def token_ids(self, sentence):
        """<start> w1 ... wn <end> of a raw sentence through the dataset's own path (PrecompDataset.caption_text, its word_tokenize and
        vocabulary): for a caption of the split, `dataset.token_ids(i)`."""
        if self.dataset is None:
            raise ValueError("GalleryIndex: raw text needs the dataset's tokeniser and vocabulary (an index built or loaded from "
                             "checkpoints has them); pass token-id lists instead")
        d = self.dataset
        if isinstance(sentence, bytes):
            sentence = sentence.strip()
        else:
            sentence = str(sentence).strip()
        tokens = d.word_tokenize(d.caption_text(sentence).lower())
        return [d.vocab('<start>')] + [d.vocab(t) for t in tokens] + [d.vocab('<end>')]

    @staticmethod
    def _gru_text(model, ids):
        """The GRU text tower of `model` on token-id lists -> (embeddings in the input order, lengths).  Last-state families give
        [n, D]; word-level families (SCAN, SGRAF) the packed rows scattered to [n, L, D]."""
        from .modalmodule.TextEncoder import EncoderText
        enc, cfg = model.txt_enc, model.config
        if not isinstance(enc, EncoderText) or enc.num_layers != 1:
            raise NotImplementedError("GalleryIndex.encode_text: a single-layer GRU text tower is needed, %s has %s"
                                      % (cfg['name'], type(enc).__name__))
        if cfg['name'] == 'VSRN':              # PrecompDataset.vsrn_ids: cut to max_len, then <pad> up to max_len + 1 ids
            max_len, rows = int(cfg['max_len']), []
            for r in ids:
                r = list(r)
                if len(r) > max_len:
                    r[max_len] = r[-1]
                    r = r[:max_len]
                rows.append(r + [0] * (max_len + 1 - len(r)))
            ids = rows
        lens = np.asarray([len(r) for r in ids], np.int64)
        order = np.argsort(-lens, kind='stable')                       # the kernels take captions by descending length
        dev = _dev()
        toks = ops.h2d(np.concatenate([np.asarray(ids[i], np.int64) for i in order]) if len(order) else np.zeros(0, np.int64), dev)
        ls = lens[order]
        off = ops.h2d(np.concatenate([[0], np.cumsum(ls)[:-1]]).astype(np.int64), dev)
        last = enc.method_name in ('VSE++', 'VSRN')
        with torch.no_grad():
            out = ops.gru_encode(toks, off, [int(l) for l in ls], enc._weights(), enc.use_bi_gru, no_txtnorm=enc.no_txtnorm,
                                 use_abs=enc.use_abs, gather_last=last, batch_invariant=True)
        out = out.cpu().numpy()
        if last:
            res = np.empty_like(out)
            res[order] = out
            return res, lens
        res = np.zeros((len(ids), int(lens.max()) if len(ids) else 0, out.shape[1]), np.float32)
        o = 0
        for i, l in zip(order, ls):
            res[i, :l] = out[o:o + l]
            o += l
        return res, lens

    def encode_text(self, sentences):
        """Sentences (str / bytes, tokenised as the dataset tokenises its captions) or token-id lists -> `Query` with the coarse and,
        when the index has a fine model, the fine (word-level) embeddings.  The GRU towers run with batch_invariant=True, as the
        sharded evaluation does (GruModelEval.encode_captions): a query's embedding, and therefore its answer, does not depend bit
        for bit on what else is in the batch -- one sentence at a time, seven at a time or all at once give the same bytes."""
        if isinstance(sentences, (str, bytes)):
            sentences = [sentences]
        ids = [self.token_ids(s) if isinstance(s, (str, bytes)) else [int(t) for t in s] for s in sentences]
        if self.coarse_model is None:
            raise ValueError("GalleryIndex.encode_text: the index holds no coarse model (from_embeddings without coarse_model)")
        coarse, _ = self._gru_text(self.coarse_model, ids)
        fine = lens = None
        if self.fine_model is not None:
            fine, lens = self._gru_text(self.fine_model, ids)
        return Query('text', coarse, fine, lens, ids)

    def encode_images(self, features):
        """Region features [n, 36, F] (what `<split>_ims.npy` holds) -> `Query` through the models' image towers."""
        if self.coarse_model is None:
            raise ValueError("GalleryIndex.encode_images: the index holds no coarse model (from_embeddings without coarse_model)")
        feats = torch.as_tensor(np.ascontiguousarray(np.asarray(features, np.float32)))
        if feats.dim() != 3:
            raise ValueError("GalleryIndex.encode_images: features must be [n, regions, F], got %s" % (tuple(feats.shape),))

        def tower(model):
            model.val_start()
            with torch.no_grad():
                out = model.img_enc(model._dev(feats))
            return (out[0] if isinstance(out, tuple) else out).detach().cpu().numpy()
        return Query('images', tower(self.coarse_model), tower(self.fine_model) if self.fine_model is not None else None)

    # ------------------------------------------------------------------ search
    def _coarse_lists(self, q, gallery, k):
        """-> (idx int32 device [n, k], val float32 device [n, k])"""
        n, N = q.shape[0], gallery.shape[0]
        if self.route not in ('auto', 'fused', 'matrix'):
            raise ValueError("GalleryIndex.route must be 'auto', 'fused' or 'matrix', got %r" % (self.route,))
        fused = self.route == 'fused' or (self.route == 'auto' and fused_wins(min(n, ops.SEARCH_MAX_QUERIES), N, k))
        if not fused and 0 < n and k <= N:          # the matrix path lists at most N entries per query; same bytes
            idx, val, _ = ops.topk_lists(ops.cosine_scores(q, gallery), k, cols=False)
            return idx, val
        out = [ops.search_topk(q[i:i + ops.SEARCH_MAX_QUERIES], gallery, k)[:2] for i in range(0, n, ops.SEARCH_MAX_QUERIES)]
        if not out:
            return (torch.empty(0, k, device=gallery.device, dtype=torch.int32), torch.empty(0, k, device=gallery.device))
        return torch.cat([o[0] for o in out], 0), torch.cat([o[1] for o in out], 0)

    def _fine_scores(self, q, direction, cand):
        """Fine scores [n, K'] of the shortlisted pairs; the query side is packed on its own plan."""
        model = self.fine_model
        if direction == 't2i':
            images = self.fine['images']
            _, words, plan = evaluation._packed_words(np.zeros((1, 1, 1), np.float32), q.fine, q.lens)
            by = 'caption'
        else:
            images = _to_dev(q.fine)
            words, plan = self.fine['captions']
            by = 'image'
        if model.config['name'] == 'SCAN':
            cfg = model.config
            return ops.scan_candidate_scores(images, words, plan, cand, by, cross_attn=cfg['cross_attn'],
                                             raw_feature_norm=cfg['raw_feature_norm'], agg_func=cfg['agg_func'],
                                             lambda_lse=cfg['lambda_lse'], lambda_softmax=cfg['lambda_softmax'])
        enc = model.sim_enc
        weights = {k_: v.detach() for k_, v in enc.state_dict().items()}
        return ops.sgraf_candidate_scores(images, words, plan, weights, cand, by, module_name=enc.module_name, sgr_step=enc.sgr_step)

    def search_embedded(self, q, direction, k, rerank=None):
        """The core: encoded queries against the resident gallery.  q: a `Query`, or just coarse embeddings [n, D] (array or tensor)
        when no reranking is asked for; direction 't2i' (caption queries, image gallery) or 'i2t'; 1 <= k <= 128.
        The coarse lists come from ops.search_topk, ops.SEARCH_MAX_QUERIES queries per call -- or, where that was measured slower
        (`fused_wins`; `route` pins it), from ops.cosine_scores + ops.topk_lists, which give the same bytes.  rerank=K' >= k: the fine model scores
        the K' shortlisted pairs of every query, ops.rerank_lists re-orders them and the first k are returned.  -> `SearchResult`."""
        if direction not in ('t2i', 'i2t'):
            raise ValueError("direction must be 't2i' or 'i2t', got %r" % (direction,))
        side = 'images' if direction == 't2i' else 'captions'
        if side not in self.coarse:
            raise ValueError("GalleryIndex: the index keeps no %s gallery (sides)" % side)
        if not isinstance(q, Query):
            q = Query('embedded', q)
        k = int(k)
        gallery = self.coarse[side]
        qc = _to_dev(q.coarse).to(torch.float32)
        if qc.dim() != 2 or qc.shape[1] != gallery.shape[1]:
            raise ValueError("GalleryIndex: query embeddings must be [n, %d], got %s" % (gallery.shape[1], tuple(qc.shape)))
        kc = k
        if rerank is not None:
            kc = int(rerank)
            if kc < k:
                raise ValueError("GalleryIndex: rerank = %d < k = %d" % (kc, k))
            if self.fine_model is None or q.fine is None:
                raise ValueError("GalleryIndex: rerank needs an index with a fine model and queries encoded by it")
            if kc > gallery.shape[0]:
                raise ValueError("GalleryIndex: rerank = %d exceeds the gallery's %d items" % (kc, gallery.shape[0]))
        c_idx, c_val = self._coarse_lists(qc, gallery, kc)
        if rerank is None or len(q) == 0:
            idx, val = c_idx[:, :k], c_val[:, :k]
        else:
            fine = self._fine_scores(q, direction, c_idx)
            ri, rv, _ = ops.rerank_lists(c_idx, fine)
            idx, val = ri[:, :k], rv[:, :k]
        return SearchResult(direction, idx.cpu().numpy().astype(np.int64), val.cpu().numpy(), c_idx.cpu().numpy().astype(np.int64),
                            c_val.cpu().numpy())

    def search_text(self, sentences, k, rerank=None):
        """The k best images for every sentence: search_embedded(encode_text(sentences), 't2i', k, rerank)."""
        return self.search_embedded(self.encode_text(sentences), 't2i', k, rerank)

    def search_images(self, features, k, rerank=None):
        """The k best captions for every image: search_embedded(encode_images(features), 'i2t', k, rerank)."""
        return self.search_embedded(self.encode_images(features), 'i2t', k, rerank)
