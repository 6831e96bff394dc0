"""CPU: the two helpers of the candidate ops (itr_amd/ops.py) that are pure host logic -- `_chunks_within`, which cuts the SGRAF
item plan into workspace-sized chunks, against a linear scan, and `_group_pairs`, the CSR grouping of listed pairs, on host tensors
against numpy's stable argsort and bincount.  No device is used."""
import numpy as np
import pytest
import torch

from itr_amd import ops


# ------------------------------------------------------------------------------------------ _chunks_within
def _need_of(sizes, c0, c1, c2):
    begin = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return lambda a, b: c0 + c1 * int(begin[b] - begin[a]) + c2 * (b - a)


def _linear_chunks(need, n_items, budget):
    """the definition: from each start, take items one by one while the chunk still fits"""
    chunks, a = [], 0
    while a < n_items:
        b = a + 1
        assert need(a, b) <= budget
        while b < n_items and need(a, b + 1) <= budget:
            b += 1
        chunks.append((a, b))
        a = b
    return chunks


@pytest.mark.parametrize("seed,n_items", [(0, 1), (1, 2), (2, 37), (3, 200)])
def test_chunks_within_are_contiguous_fit_and_are_maximal(seed, n_items):
    rng = np.random.RandomState(seed)
    sizes = rng.randint(1, 65, size=n_items)
    need = _need_of(sizes, c0=4096, c1=int(rng.randint(100, 3000)), c2=int(rng.randint(1, 500)))
    one = max(need(i, i + 1) for i in range(n_items))              # exactly the largest single item's need
    whole = need(0, n_items)
    between = [int(one + f * (whole - one)) for f in (0.03, 0.25, 0.5, 0.9)]
    for budget in [one, whole, whole - 1] + between:
        if budget < one:                                           # (n_items == 1: whole - 1 does not hold the item)
            continue
        chunks = ops._chunks_within("caller_name", need, n_items, budget)
        assert chunks[0][0] == 0 and chunks[-1][1] == n_items
        for (a, b), (a2, _) in zip(chunks, chunks[1:]):
            assert b == a2                                         # contiguous
        for a, b in chunks:
            assert a < b and need(a, b) <= budget                  # whole items, within the budget
            assert b == n_items or need(a, b + 1) > budget         # maximal: one more item would not fit
        assert chunks == _linear_chunks(need, n_items, budget)
    assert ops._chunks_within("caller_name", need, n_items, whole) == [(0, n_items)]
    if n_items > 1:
        assert len(ops._chunks_within("caller_name", need, n_items, whole - 1)) == 2


def test_chunks_within_no_items_and_an_item_that_does_not_fit():
    need = _need_of(np.asarray([3, 64, 5]), c0=10, c1=7, c2=2)
    assert ops._chunks_within("caller_name", need, 0, 1) == []
    assert ops._chunks_within("caller_name", need, 0, 0) == []
    largest = need(1, 2)
    assert ops._chunks_within("caller_name", need, 3, largest) == [(0, 1), (1, 2), (2, 3)]
    with pytest.raises(torch.cuda.OutOfMemoryError, match="caller_name") as e:
        ops._chunks_within("caller_name", need, 3, largest - 1)
    assert "one item needs %d bytes" % largest in str(e.value) and "%d allowed" % (largest - 1) in str(e.value)


# ------------------------------------------------------------------------------------------ _group_pairs
def _check_grouping(key, n_keys, grouped=False):
    key = np.asarray(key, dtype=np.int64)
    P = key.shape[0]
    col_a = np.arange(P, dtype=np.int64)                           # the incoming position: shows the order inside a group
    col_b = 1000 + 7 * key + np.arange(P) % 5                      # a column that depends on the key: shows that columns travel
    got = ops._group_pairs(torch.from_numpy(key), n_keys, (torch.from_numpy(col_a), torch.from_numpy(col_b)), grouped)
    ptr, gkey, ga, gb = got
    assert len(got) == 4 and ptr.dtype == torch.int32 and tuple(ptr.shape) == (n_keys + 1,)
    assert gkey.dtype == torch.int64 and ga.dtype == torch.int64
    ptr, gkey, ga, gb = (t.numpy() for t in got)
    order = np.argsort(key, kind='stable')
    assert np.array_equal(ptr, np.concatenate([[0], np.cumsum(np.bincount(key, minlength=n_keys))]))
    assert ptr[0] == 0 and ptr[-1] == P and np.all(np.diff(ptr) >= 0)
    assert np.array_equal(gkey, key[order]) and np.array_equal(ga, col_a[order]) and np.array_equal(gb, col_b[order])
    for j in range(n_keys):
        seg = slice(ptr[j], ptr[j + 1])
        assert np.all(gkey[seg] == j)
        assert np.all(np.diff(ga[seg]) > 0)                        # the pairs of a key keep their incoming order
        assert np.array_equal(ga[seg], np.nonzero(key == j)[0])
    assert np.array_equal(gb, 1000 + 7 * gkey + ga % 5)            # every column entry is still with its key
    if grouped:
        assert np.array_equal(ga, col_a)                           # nothing was permuted


def test_group_pairs_empty_and_single():
    _check_grouping([], 0)
    _check_grouping([], 6)
    _check_grouping([], 6, grouped=True)
    _check_grouping([0], 1)
    _check_grouping([4], 9)
    _check_grouping([4], 9, grouped=True)


def test_group_pairs_one_key_empty_groups_and_duplicates():
    _check_grouping([3] * 17, 4)                                   # all pairs under one key, the last
    _check_grouping([0] * 5, 8)                                    # ... under the first, empty groups behind it
    # empty groups at the front (0, 1), in the middle (4, 5, 7) and at the end (10 .. 13); n_keys > largest key + 1; duplicates
    _check_grouping([9, 2, 6, 2, 3, 9, 9, 8, 2, 6, 3, 2], 14)
    rng = np.random.RandomState(5)
    for n_keys, P in ((1, 40), (13, 300), (64, 65), (500, 257)):
        _check_grouping(rng.randint(0, n_keys, size=P), n_keys)
        _check_grouping(rng.randint(n_keys // 3, max(n_keys // 2, n_keys // 3 + 1), size=P), n_keys)


def test_group_pairs_already_grouped_input_is_not_permuted():
    rng = np.random.RandomState(6)
    _check_grouping(np.repeat(np.arange(21), 10), 21, grouped=True)          # lists flattened by their own query: K pairs per key
    key = np.sort(rng.randint(2, 30, size=200))
    _check_grouping(key, 37, grouped=True)                                   # ragged groups, empty ones at both ends
    _check_grouping(key, 37, grouped=False)                                  # the sorting path gives the same on such input
