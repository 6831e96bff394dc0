"""CPU: the sample order of the device-resident training loader (datamodule/resident.py::BatchOrder) is the order of
get_precomp_loader's DataLoader -- same seed, same batches, same collate order inside a batch, epoch after epoch."""
import numpy as np
import pytest

from itr_amd.datamodule import data_loader as dl, tokenization as tok
from itr_amd.datamodule.resident import BatchOrder


def _materialise(g, tmp_path, n_rep):
    """The data-layer golden fixture as a precomp directory; n_rep > 1 repeats images and captions, so every caption length
    occurs n_rep times at least (a sort that is not stable would reorder them)."""
    name = 'toy_precomp'
    d = tmp_path / ('data%d' % n_rep) / name
    d.mkdir(parents=True)
    caps = bytes(g["caps_blob"]).split(b"\n")[:-1]
    np.save(d / 'train_ims.npy', np.concatenate([g["ims"]] * n_rep))
    (d / 'train_caps.txt').write_bytes(b"\n".join(caps * n_rep) + b"\n")
    vdir = tmp_path / ('vocab%d' % n_rep)
    vdir.mkdir()
    (vdir / ('%s_vocab.json' % name)).write_text(bytes(g["vocab_json"]).decode())
    return name, str(d), str(vdir)


def _cfg(name, vdir, seed):
    return {'use_bbox': False, 'text_encoder': 'gru', 'vocab_path': vdir, 'data_name': name, 'vocab_type': 'json', 'name': 'SCAN',
            'word_tokenize': tok.regex_word_tokenize, 'seed': seed}


@pytest.fixture(scope="module")
def splits(golden, tmp_path_factory):
    g = golden("g14_data_layer")
    root = tmp_path_factory.mktemp("resident_order")
    return {n_rep: _materialise(g, root, n_rep) for n_rep in (1, 3)}


@pytest.mark.parametrize("n_rep", [1, 3])
@pytest.mark.parametrize("seed", [0, 11])
@pytest.mark.parametrize("batch_size", [1, 7, None])          # None: the whole split in one batch; 7 divides neither 30 nor 90
@pytest.mark.parametrize("shuffle", [True, False])
def test_order_is_the_loaders(splits, n_rep, seed, batch_size, shuffle):
    name, d, vdir = splits[n_rep]
    cfg = _cfg(name, vdir, seed)
    loader, _ = dl.get_precomp_loader(d, 'train', cfg, batch_size=batch_size or 30 * n_rep, shuffle=shuffle, num_workers=0)
    dset = loader.dataset
    n = len(dset)
    assert n == 30 * n_rep
    _, lens = dset.token_ids_range(0, n)
    if n_rep > 1:
        assert np.bincount(lens).max() >= n_rep          # several captions of one length
    order = BatchOrder(n, batch_size or n, shuffle, cfg['seed'], sort_key=lens)
    assert len(order) == len(loader)
    first = None
    for epoch in range(3):
        want = [(list(b[5]), list(b[4])) for b in loader]
        got = list(order)
        assert len(got) == len(want) == len(loader)
        for idx, (ids, lengths) in zip(got, want):
            assert idx.dtype == np.int64 and idx.tolist() == ids, (epoch, idx, ids)
            assert lens[idx].tolist() == lengths
        assert sorted(np.concatenate(got).tolist()) == list(range(n))
        flat = np.concatenate(got).tolist()
        if epoch == 0:
            first = flat
        elif shuffle and (batch_size or n) < n:
            assert flat != first                          # a new permutation every epoch, as the loader draws one
    if batch_size == 7:
        assert len(got[-1]) == n % 7                      # the partial last batch is kept (drop_last=False)


def test_constant_key_keeps_the_sampler_order(splits):
    """BERT families and VSRN: every caption has the same number of ids, collate_fn's stable sort changes nothing."""
    a = [b.tolist() for b in BatchOrder(30, 7, True, 5, sort_key=None)]
    b = [b.tolist() for b in BatchOrder(30, 7, True, 5, sort_key=np.full(30, 32))]
    assert a == b and sorted(sum(a, [])) == list(range(30))
    # and another seed gives another order
    assert a != [b.tolist() for b in BatchOrder(30, 7, True, 6, sort_key=None)]
