"""CPU: the candidate-list entry points exist in every layer (library, header, binding, ops, evaluation), and the host arithmetic
that turns reranked lists + coarse ranks into rank vectors equals the definition of the reranked ranking stated in numpy."""
import os
import re

import numpy as np
import pytest

from itr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["itr_scan_pairs_workspace_bytes", "itr_scan_pairs_prepare", "itr_scan_pair_scores", "itr_rerank_lists"]


def header_decl(name):
    src = open(os.path.join(ROOT, "include", "itr_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, src)
    assert m, "include/itr_hip.h does not declare %s" % name
    return [a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"]


def test_new_symbols_exported_declared_and_bound():
    lib = _lib.load()
    for s in NEW:
        assert hasattr(lib, s), "libitr_hip.so does not export %s" % s
        assert s in _lib.SIGNATURES
        assert len(header_decl(s)) == len(_lib.SIGNATURES[s][1]), s
    assert lib.itr_abi_version() == _lib.ABI_VERSION
    assert _lib.ABI_VERSION > 32          # the parent's library returned 32
    src = open(os.path.join(ROOT, "include", "itr_hip.h")).read()
    assert int(re.search(r"#define\s+ITR_ABI_VERSION\s+(\d+)", src).group(1)) == _lib.ABI_VERSION


def test_python_entry_points_exist():
    from itr_amd import ops
    from itr_amd.metricmodule import evaluation
    for mod, name in ((ops, "scan_candidate_scores"), (ops, "rerank_lists"), (evaluation, "rerank"), (evaluation, "evalrank_rerank")):
        assert callable(getattr(mod, name))


def test_host_argument_checks():
    """no kernel is launched: the calls are refused on their arguments"""
    lib = _lib.load()
    assert lib.itr_rerank_lists(None, None, 4, 0, None, None, None, None) == -1
    assert lib.itr_rerank_lists(None, None, 4, 129, None, None, None, None) == -2
    assert lib.itr_rerank_lists(None, None, 0, 10, None, None, None, None) == 0
    assert lib.itr_scan_pairs_workspace_bytes(5000, 36, 325000, 25000, 0) > 5000 * 36 * 36 * 4
    one = 16                                                    # any non-null, 16-byte aligned value: refused before any use
    assert lib.itr_scan_pair_scores(one, one, one, one, one, one, one, 8, 4, 4, 16, 35, 32, 0, 0, 0, 9.0, 6.0, one, 8, one, 1 << 30, None) == -2
    assert lib.itr_scan_pair_scores(one, one, one, one, one, one, one, 8, 4, 4, 16, 36, 32, 0, 7, 0, 9.0, 6.0, one, 8, one, 1 << 30, None) == -1
    assert lib.itr_scan_pair_scores(one, one, one, one, one, one, one, 8, 4, 4, 16, 36, 32, 0, 0, 0, 9.0, 6.0, one, 8, one, 16, None) == -1


def np_reranked_ranks(coarse, fine, k, direction, im_div):
    """The definition: the k best of the coarse line in fine order, then all other candidates in coarse order; the rank of a query
    is the best position of a ground truth in that ranking.  Order of a line: larger score first, the higher index on ties."""
    M_c, M_f = (coarse, fine) if direction == 'i2t' else (coarse.T, fine.T)
    n = M_c.shape[1]
    ranks, lists = np.zeros(M_c.shape[0]), []
    for q in range(M_c.shape[0]):
        order_c = np.lexsort((-np.arange(n), -M_c[q]))
        short, rest = order_c[:k], order_c[k:]
        short = short[np.lexsort((-short, -M_f[q][short]))]
        ranking = np.concatenate([short, rest])
        gt = np.arange(im_div * q, im_div * (q + 1)) if direction == 'i2t' else np.asarray([q // im_div])
        ranks[q] = np.nonzero(np.isin(ranking, gt))[0].min()
        lists.append(short)
    return ranks, np.stack(lists)


def np_ranks(M, direction, im_div):
    M = M if direction == 'i2t' else M.T
    out = np.zeros(M.shape[0])
    for q in range(M.shape[0]):
        order = np.lexsort((-np.arange(M.shape[1]), -M[q]))
        gt = np.arange(im_div * q, im_div * (q + 1)) if direction == 'i2t' else np.asarray([q // im_div])
        out[q] = np.nonzero(np.isin(order, gt))[0].min()
    return out


@pytest.mark.parametrize("k", [10, 13, 35])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_reranked_ranking_definition_on_the_host(seed, k):
    from itr_amd.metricmodule import evaluation
    rng = np.random.RandomState(seed)
    Ni, im_div = 12, 5
    coarse = rng.randint(-4, 5, size=(Ni, Ni * im_div)).astype(np.float64)      # integer valued: many exact ties
    fine = rng.randint(-3, 4, size=(Ni, Ni * im_div)).astype(np.float64)
    for direction in ('i2t', 't2i'):
        if direction == 't2i' and k > Ni:
            continue
        want, lists = np_reranked_ranks(coarse, fine, k, direction, im_div)
        got = evaluation.rerank_rank_vector(lists, np_ranks(coarse, direction, im_div), direction, im_div)
        assert np.array_equal(got, want), (direction, k)
    with pytest.raises(ValueError):
        evaluation.rerank_rank_vector(np.zeros((2, 10), np.int64), np.zeros(2), 'bogus')
