"""GPU: ops.collate_batch (itr_collate_batch, csrc/collate.hip) against numpy fancy indexing, bit for bit: a pure copy has no
tolerance.  Shapes cover the 16-byte path, the element-wise path (odd row length; a base that is not 16-byte aligned), rows of
one and of several 1024-unit chunks, one and several workgroup rows, and every job kind in one launch."""
import numpy as np
import pytest
import torch

from itr_amd import ops

pytestmark = pytest.mark.gpu


def _indices(rng, B, n):
    """index 0, index n - 1 and repeats are always there (B permitting)"""
    idx = rng.randint(0, n, size=B)
    idx[0] = n - 1
    if B > 1:
        idx[-1] = 0
    if B > 3:
        idx[2] = idx[1]
    return idx.astype(np.int64)


@pytest.mark.parametrize("B", [1, 7, 128])
@pytest.mark.parametrize("row_elems", [15, 288, 2051, 36 * 2048])      # 15, 2051: element-wise (2051: 3 chunks); 36 * 2048: 18 chunks of 16 B units
def test_feature_rows(dev, B, row_elems):
    rng = np.random.RandomState(B * 7 + row_elems % 97)
    n = 11
    feat = rng.randn(n, row_elems).astype(np.float32)
    idx = _indices(rng, B, n)
    out = ops.collate_batch(torch.from_numpy(feat).to(dev), torch.from_numpy(idx).to(dev), check=True)
    assert out.images.shape == (B, row_elems) and out.images.dtype == torch.float32
    assert out.boxes is None and out.img_wh is None and out.ids is None and out.tables == () and out.float_table is None
    assert np.array_equal(out.images.cpu().numpy().view(np.uint32), feat[idx].view(np.uint32))


def test_feature_rows_keep_their_trailing_shape(dev):
    rng = np.random.RandomState(1)
    feat = rng.randn(9, 36, 8).astype(np.float32)
    idx = _indices(rng, 7, 9)
    out = ops.collate_batch(torch.from_numpy(feat).to(dev), torch.from_numpy(idx).to(dev))
    assert out.images.shape == (7, 36, 8) and np.array_equal(out.images.cpu().numpy(), feat[idx])


@pytest.mark.parametrize("B", [1, 7, 128])
def test_unaligned_table_takes_the_elementwise_path(dev, B):
    """a feature table that starts 4 bytes into a larger buffer: rows of 288 floats, but no 16-byte alignment"""
    rng = np.random.RandomState(B)
    n, row = 13, 288
    buf = rng.randn(n * row + 1).astype(np.float32)
    big = torch.from_numpy(buf).to(dev)
    view = big[1:].view(n, row)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    idx = _indices(rng, B, n)
    out = ops.collate_batch(view, torch.from_numpy(idx).to(dev), check=True)
    assert np.array_equal(out.images.cpu().numpy().view(np.uint32), buf[1:].reshape(n, row)[idx].view(np.uint32))


def _ragged_want(rows, idx, lmax):
    want = np.zeros((len(idx), lmax), np.int64)
    for b, c in enumerate(idx):
        want[b, :len(rows[c])] = rows[c][:lmax]
    return want


@pytest.mark.parametrize("lens", [
    list(range(1, 14)),                      # lengths 1 .. Lmax
    [1] * 9,                                 # Lmax = 1
    [6] * 9,                                 # a batch whose captions are all of one length
    [1500, 3, 1024, 1025, 7],                # rows of two 1024-id chunks
], ids=["1..13", "all-1", "all-6", "long"])
@pytest.mark.parametrize("B", [1, 7, 128])
def test_ragged_ids(dev, lens, B):
    rng = np.random.RandomState(len(lens) + B)
    rows = [rng.randint(1, 10000, size=l).astype(np.int64) for l in lens]
    packed = np.concatenate(rows)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n_cap = len(lens)
    idx = _indices(rng, B, n_cap)
    idx = idx[np.argsort(-np.asarray(lens)[idx], kind='stable')]          # collate order; the kernel does not depend on it
    lmax = int(np.asarray(lens)[idx].max())
    feat = rng.randn(n_cap, 15).astype(np.float32)
    t = lambda a: torch.from_numpy(a).to(dev)
    out = ops.collate_batch(t(feat), t(idx), cap_idx=t(idx), packed=t(packed), off=t(off), lmax=lmax, check=True)
    assert out.ids.shape == (B, lmax) and out.ids.dtype == torch.int64
    assert np.array_equal(out.ids.cpu().numpy(), _ragged_want(rows, idx, lmax))
    assert np.array_equal(out.images.cpu().numpy(), feat[idx])
    # a shorter Lmax than the longest caption cuts the row, as a slice would
    if lmax > 1:
        out = ops.collate_batch(t(feat), t(idx), cap_idx=t(idx), packed=t(packed), off=t(off), lmax=lmax - 1)
        assert np.array_equal(out.ids.cpu().numpy(), _ragged_want(rows, idx, lmax)[:, :lmax - 1])


@pytest.mark.parametrize("W", [1, 32])
@pytest.mark.parametrize("B", [1, 7, 128])
def test_fixed_width_tables_with_boxes_and_sizes(dev, W, B):
    """every row job of a CAMERA batch in one launch: features, boxes, sizes, three int64 tables, one float table; the caption
    and the image index differ (five captions per image)"""
    rng = np.random.RandomState(W + B)
    n_img, n_cap = 6, 30
    feat = rng.randn(n_img, 36, 8).astype(np.float32)
    boxes = rng.rand(n_img, 36, 4).astype(np.float32)
    wh = rng.randint(200, 640, size=(n_img, 2)).astype(np.float32)
    tabs = [rng.randint(0, 30000, size=(n_cap, W)).astype(np.int64) for _ in range(3)]
    ftab = rng.rand(n_cap, W).astype(np.float32)
    cap = _indices(rng, B, n_cap)
    img = cap // 5
    t = lambda a: torch.from_numpy(a).to(dev)
    out = ops.collate_batch(t(feat), t(img), boxes=t(boxes), img_wh=t(wh), cap_idx=t(cap), tables=[t(x) for x in tabs], float_table=t(ftab),
                            check=True)
    assert np.array_equal(out.images.cpu().numpy(), feat[img])
    assert np.array_equal(out.boxes.cpu().numpy(), boxes[img]) and out.boxes.shape == (B, 36, 4)
    assert np.array_equal(out.img_wh.cpu().numpy(), wh[img]) and out.img_wh.shape == (B, 2)
    assert len(out.tables) == 3
    for got, want in zip(out.tables, tabs):
        assert got.dtype == torch.int64 and got.shape == (B, W) and np.array_equal(got.cpu().numpy(), want[cap])
    assert out.float_table.dtype == torch.float32 and np.array_equal(out.float_table.cpu().numpy(), ftab[cap])
    # a subset of the tables (VSRN: ids + float mask)
    out = ops.collate_batch(t(feat), t(img), cap_idx=t(cap), tables=[t(tabs[0])], float_table=t(ftab))
    assert np.array_equal(out.tables[0].cpu().numpy(), tabs[0][cap]) and np.array_equal(out.float_table.cpu().numpy(), ftab[cap])
    assert out.boxes is None and out.img_wh is None


def test_out_of_range_index_sets_the_flag(dev):
    rng = np.random.RandomState(3)
    feat = rng.randn(5, 288).astype(np.float32)
    tab = rng.randint(0, 100, size=(10, 4)).astype(np.int64)
    t = lambda a: torch.from_numpy(a).to(dev)
    for img, cap in (([1, 5, 2], [0, 1, 2]), ([1, -1, 2], [0, 1, 2]), ([1, 0, 2], [0, 10, 2]), ([1, 0, 2], [0, -7, 2])):
        img, cap = np.asarray(img, np.int64), np.asarray(cap, np.int64)
        out = ops.collate_batch(t(feat), t(img), cap_idx=t(cap), tables=[t(tab)])
        assert int(out.bad_flag.item()) == 1
        ok_img, ok_cap = np.where((img < 0) | (img >= 5), 0, img), np.where((cap < 0) | (cap >= 10), 0, cap)      # a bad index reads row 0
        assert np.array_equal(out.images.cpu().numpy(), feat[ok_img]) and np.array_equal(out.tables[0].cpu().numpy(), tab[ok_cap])
        with pytest.raises(IndexError, match="outside its table"):
            ops.collate_batch(t(feat), t(img), cap_idx=t(cap), tables=[t(tab)], check=True)
    # good indices leave a caller's flag alone, and the flag is reused over calls
    flag = torch.zeros(1, device=dev, dtype=torch.int32)
    out = ops.collate_batch(t(feat), t(np.asarray([4, 0], np.int64)), bad_flag=flag, check=True)
    assert out.bad_flag is flag and int(flag.item()) == 0
    # ragged: an index past the captions
    packed, off = np.arange(1, 7, dtype=np.int64), np.asarray([0, 2, 6], np.int64)
    out = ops.collate_batch(t(feat), t(np.asarray([0, 1], np.int64)), cap_idx=t(np.asarray([2, 1], np.int64)), packed=t(packed), off=t(off), lmax=4)
    assert int(out.bad_flag.item()) == 1 and out.ids.cpu().tolist() == [[1, 2, 0, 0], [3, 4, 5, 6]]


def test_empty_batch(dev):
    feat = torch.zeros(3, 8, device=dev)
    out = ops.collate_batch(feat, torch.zeros(0, dtype=torch.int64, device=dev), check=True)
    assert out.images.shape == (0, 8)


def test_cpu_tensors_are_rejected(dev):
    feat, idx = torch.zeros(3, 8), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.collate_batch(feat, idx.to(dev))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.collate_batch(feat.to(dev), idx)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.collate_batch(feat.to(dev), idx.to(dev), cap_idx=idx.to(dev), tables=[torch.zeros(3, 4, dtype=torch.int64)])
    with pytest.raises(TypeError):
        ops.collate_batch(feat.to(dev), idx.to(dev).int())
