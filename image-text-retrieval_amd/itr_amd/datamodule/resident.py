"""Device-resident training split: the whole `{split}_ims.npy` (coco_precomp train: 113 287 x 36 x 2048 fp32 = 33.4 GB of the
MI355X's 288 GB) and the tokenised captions are uploaded ONCE, and every batch is assembled from HBM by one gather launch
(ops.collate_batch -> itr_collate_batch).  Per step the host draws the sample indices, sorts them the way collate_fn does and
uploads one small index vector; nothing else crosses the PCIe link and nothing synchronises.

    rs = ResidentTrainSet(PrecompDataset(path, 'train', config), device)
    for images, boxes, imgs_wh, captions_ids, lengths, ids, captions_mask, captions_type_ids in ResidentLoader(rs, 128, True, seed):
        ...

The batches are those of `get_precomp_loader(...)`'s DataLoader for the same seed, member by member, bit for bit (values,
shapes, dtypes, container types), epoch after epoch; the tensors live on the device, `lengths` and `ids` on the host.
Opt-in (`resident_data=True`); a split that does not fit is refused with MemoryError, never streamed and never handed to the
loader path silently."""
import time

import numpy as np
import torch
import torch.utils.data as data


class _IndexDataset(data.Dataset):
    """Sample i is the number i: a DataLoader over it hands out the sampler's index batches."""

    def __init__(self, n):
        self.n = int(n)

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return i


class BatchOrder(object):
    """The sample indices of every batch, in collate order, of a DataLoader(dataset of n samples, batch_size, shuffle,
    generator seeded as get_precomp_loader seeds it).  The sampler is not re-implemented: a DataLoader over an index-only
    dataset is iterated, so the generator is consumed exactly as the real loader consumes it, one `iter()` per epoch.
    sort_key (host int array [n], or None): collate_fn's `sorted(batch, key=len(caption ids), reverse=True)` -- descending and
    stable, equal keys keep the sampler's order; None when every caption has the same number of ids (BERT families, VSRN).
    Needs no GPU."""

    def __init__(self, n, batch_size, shuffle, seed, sort_key=None):
        gen = None
        if shuffle and seed is not None:
            gen = torch.Generator()
            gen.manual_seed(int(seed))
        self.loader = data.DataLoader(dataset=_IndexDataset(n), batch_size=batch_size, shuffle=shuffle, collate_fn=list, num_workers=0,
                                      generator=gen)
        self.sort_key = None if sort_key is None else np.asarray(sort_key, dtype=np.int64)
        if self.sort_key is not None and self.sort_key.shape != (int(n),):
            raise ValueError("BatchOrder: sort_key must hold one length per sample (%d), got %s" % (n, self.sort_key.shape))

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for batch in self.loader:
            idx = np.asarray(batch, dtype=np.int64)
            if self.sort_key is not None:
                idx = idx[np.argsort(-self.sort_key[idx], kind='stable')]
            yield idx


def _layout(config):
    if config.get('text_encoder') == 'bert':
        return 'bert'
    return 'vsrn' if config.get('name') == 'VSRN' else 'gru'


def _vsrn_tables(dataset, n):
    """PrecompDataset.vsrn_ids of captions 0 .. n-1 at once -> (ids int64 [n, max_len + 1], mask float32 [n, max_len + 1]): the
    first min(len, max_len) token ids, then zeros; the mask is computed after the padding, so it is the same row for every caption."""
    max_len = int(dataset.config['max_len'])
    packed, lens = dataset.token_ids_range(0, n)
    keep = np.minimum(lens, max_len)
    start = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), keep)
    cols = np.arange(int(keep.sum()), dtype=np.int64) - np.repeat(np.cumsum(keep) - keep, keep)
    ids = np.zeros((n, max_len + 1), dtype=np.int64)
    ids[rows, cols] = packed[np.repeat(start, keep) + cols]
    mask_row = np.asarray(dataset.vsrn_ids(0)[1], dtype=np.float32) if n else np.zeros(max_len + 1, np.float32)
    return ids, np.ascontiguousarray(np.broadcast_to(mask_row, ids.shape))


class ResidentTrainSet(object):
    """The tables of one PrecompDataset in device memory.

    Features (and, with config['use_bbox'], boxes and image sizes) go up from the memory map in row blocks through pinned
    staging buffers; the file is never held in host memory.  The captions are tokenised once on the host: packed ids +
    offsets (GRU families), [N, max_len + 1] ids and masks (VSRN), or the three [N, max_words] BERT feature tables.
    `lengths` (host int64 [N]) is what collate_fn would report per caption.

    max_bytes: the most device memory the tables may take; default 60 % of what the process can still have (free device
    memory + what torch holds in its cache).  The figure is a policy, not a measurement: it leaves room for the activations
    of the largest training steps (SGRAF: 872 MB-class workspaces) and a resident validation split.  More than that
    -> MemoryError before anything is allocated."""

    def __init__(self, dataset, device, max_bytes=None):
        from .. import ops
        self.dataset, self.device = dataset, torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError("ResidentTrainSet keeps the split in GPU memory: no CPU fallback")
        cfg = dataset.config
        self.layout = _layout(cfg)
        self.use_bbox = bool(cfg.get('use_bbox'))
        if self.use_bbox and self.layout != 'bert':
            raise NotImplementedError("use_bbox with a GRU text encoder: collate_fn itself cannot build such a batch")
        n = self.n = len(dataset)
        self.im_div = int(dataset.im_div)
        n_img = self.n_img = min(dataset.images.shape[0], (n - 1) // self.im_div + 1) if n else 0
        if n == 0:
            raise ValueError("ResidentTrainSet: the split has no captions")
        self.row_shape = tuple(dataset.images.shape[1:])
        need = n_img * int(np.prod(self.row_shape)) * 4
        if self.use_bbox:
            need += n_img * (int(np.prod(dataset.boxes.shape[1:])) + 2) * 4
        packed = None
        if self.layout == 'gru':
            packed, lens = dataset.token_ids_range(0, n)
            need += (packed.shape[0] + n + 1) * 8
        elif self.layout == 'vsrn':
            need += n * (int(cfg['max_len']) + 1) * (8 + 4)
        else:
            need += 3 * n * int(dataset.max_words) * 8
        if max_bytes is None:
            free, _ = torch.cuda.mem_get_info(self.device)
            cached = torch.cuda.memory_reserved(self.device) - torch.cuda.memory_allocated(self.device)
            max_bytes = int(0.6 * (free + cached))
        if need > max_bytes:
            raise MemoryError("ResidentTrainSet: the split needs %d bytes of device memory (%d image rows, %d captions) but only %d bytes "
                              "are allowed; train with resident_data=False" % (need, n_img, n, max_bytes))
        t0 = time.time()
        from ..evalpipe import _features_to_device
        self.feat = _features_to_device(dataset.images, 0, n_img, self.device)
        self.boxes = self.img_wh = None
        if self.use_bbox:
            self.boxes, self.img_wh = self._small_rows(dataset.boxes, n_img), self._small_rows(dataset.img_wh, n_img)
        self.packed = self.off = self.float_table = None
        self.tables = ()
        if self.layout == 'gru':
            self.lengths = np.asarray(lens, dtype=np.int64)
            off = np.concatenate([[0], np.cumsum(self.lengths)]).astype(np.int64)
            self.packed, self.off = ops.h2d(packed, self.device, torch.int64), ops.h2d(off, self.device, torch.int64)
        elif self.layout == 'vsrn':
            ids, mask = _vsrn_tables(dataset, n)
            self.lengths = np.full(n, ids.shape[1], dtype=np.int64)
            self.tables, self.float_table = (ops.h2d(ids, self.device),), ops.h2d(mask, self.device)
        else:
            ids, mask, types = dataset.bert_features_range(0, n)
            # collate_fn: the token count of the mask with boxes (CAMERA), len(caption ids) = max_words without (SAEM)
            self.lengths = mask.sum(1).astype(np.int64) if self.use_bbox else np.full(n, ids.shape[1], dtype=np.int64)
            self.tables = tuple(ops.h2d(t, self.device) for t in (ids, mask, types))
        self.bad_flag = torch.zeros(1, device=self.device, dtype=torch.int32)
        torch.cuda.synchronize(self.device)
        self.upload_seconds = time.time() - t0
        self.bytes_needed = need
        self.bytes_held = sum(t.numel() * t.element_size() for t in
                              (self.feat, self.boxes, self.img_wh, self.packed, self.off, self.float_table) + self.tables if t is not None)

    def _small_rows(self, arr, n_rows, chunk=8192):
        """boxes / image sizes as float32 (the cast of __getitem__: np.array(row, dtype=np.float32)), in row blocks."""
        from .. import ops
        out = torch.empty((n_rows,) + tuple(arr.shape[1:]), device=self.device, dtype=torch.float32)
        for c0 in range(0, n_rows, chunk):
            c1 = min(n_rows, c0 + chunk)
            out[c0:c1].copy_(ops.h2d(np.array(arr[c0:c1], dtype=np.float32), self.device), non_blocking=True)
        return out

    def sort_key(self):
        """collate_fn sorts by len(caption ids): the token count for the GRU families, one constant for every other layout."""
        return self.lengths if self.layout == 'gru' else None

    def batch(self, idx, check=False):
        """The reference's 8-tuple for the samples `idx` (host int64, already in collate order)."""
        from .. import ops
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        B = idx.shape[0]
        both = ops.h2d(np.concatenate([idx, idx // self.im_div]), self.device, torch.int64)       # ONE small upload per step
        cap_idx, img_idx = both[:B], both[B:]
        lens = self.lengths[idx]
        none = (None,) * B
        if self.layout == 'gru':
            out = ops.collate_batch(self.feat, img_idx, cap_idx=cap_idx, packed=self.packed, off=self.off, lmax=int(lens.max()),
                                    bad_flag=self.bad_flag, check=check)
            return out.images, none, none, out.ids, lens.tolist(), idx.tolist(), none, none
        out = ops.collate_batch(self.feat, img_idx, boxes=self.boxes, img_wh=self.img_wh, cap_idx=cap_idx, tables=self.tables,
                                float_table=self.float_table, bad_flag=self.bad_flag, check=check)
        if self.layout == 'vsrn':
            return out.images, none, none, out.tables[0], lens.tolist(), idx.tolist(), out.float_table, none
        ids, mask, types = out.tables
        if self.use_bbox:
            return out.images, out.boxes, out.img_wh, ids, list(torch.from_numpy(lens)), idx.copy(), mask, types
        return out.images, none, none, ids, lens.tolist(), idx.tolist(), mask, types


class ResidentLoader(object):
    """Iterable over the batches of a ResidentTrainSet in the order, and with the contents, of get_precomp_loader's DataLoader
    for the same batch_size / shuffle / seed (default drop_last: the partial last batch is kept).  `.dataset` is the
    PrecompDataset (validate_step looks at it)."""

    def __init__(self, resident_set, batch_size, shuffle, seed):
        self.resident_set, self.dataset = resident_set, resident_set.dataset
        self.batch_size = batch_size
        self.order = BatchOrder(resident_set.n, batch_size, shuffle, seed, resident_set.sort_key())

    def __len__(self):
        return len(self.order)

    def __iter__(self):
        for idx in self.order:
            yield self.resident_set.batch(idx)
