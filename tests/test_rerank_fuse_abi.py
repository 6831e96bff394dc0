"""CPU: ensemble reranking exists in every layer (library, header, binding, ops, evaluation), itr_rerank_fuse_lists refuses bad
arguments before it touches the device, and the numpy oracle the GPU tests compare against (tests/helpers/ensemble_oracle.py) equals
a plain Python sort on a hand-written list with every hard case."""
import functools
import math
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ensemble_oracle                                                               # noqa: E402
from itr_amd import _lib                                                             # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "itr_rerank_fuse_lists"


def test_symbol_exported_declared_and_bound():
    lib = _lib.load()
    assert hasattr(lib, NAME), "libitr_hip.so does not export %s" % NAME
    assert NAME in _lib.SIGNATURES
    raw = open(os.path.join(ROOT, "include", "itr_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % NAME, src)
    assert m, "include/itr_hip.h does not declare %s" % NAME
    assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[NAME][1]) == 10
    assert re.search(r"#define\s+ITR_RERANK_MAX_MEMBERS\s+4\b", raw)
    # the entry is additive: the ABI version did not move
    assert int(re.search(r"#define\s+ITR_ABI_VERSION\s+(\d+)", raw).group(1)) == 35
    assert _lib.ABI_VERSION == 35 and lib.itr_abi_version() == 35


def test_refusals_without_a_gpu():
    """no kernel is launched: the calls are refused (or, for no lists, accepted) on their arguments, with null pointers"""
    lib = _lib.load()
    call = lambda M, n, K: lib.itr_rerank_fuse_lists(None, None, M, n, K, None, None, None, None, None)   # noqa: E731
    assert call(2, 4, 0) == -1
    assert call(2, 4, 129) == -2
    assert call(0, 4, 10) == -1
    assert call(5, 4, 10) == -2
    assert call(2, 0, 10) == 0
    assert call(2, -1, 10) == -1
    assert call(2, 4, 10) == -1 and b"null" in lib.itr_last_error()
    # an output on top of an input (host addresses are enough: refused before any use)
    buf = np.zeros(4 * 10 * 2 * 2, dtype=np.float64)
    a = buf.ctypes.data
    idx, val, io, fo, po = a, a + 160, a + 480, a + 640, a + 960
    assert lib.itr_rerank_fuse_lists(idx, val, 2, 4, 10, idx, fo, None, po, None) == -1 and b"alias" in lib.itr_last_error()
    assert lib.itr_rerank_fuse_lists(idx, val, 2, 4, 10, io, fo, val + 160, po, None) == -1 and b"alias" in lib.itr_last_error()
    assert lib.itr_rerank_fuse_lists(idx, val, 2, 4, 10, io, val, None, po, None) == -1 and b"alias" in lib.itr_last_error()


def test_python_entry_points_exist():
    from itr_amd import ops
    from itr_amd.metricmodule import evaluation
    for mod, name in ((ops, "rerank_fused_lists"), (evaluation, "rerank_ensemble"), (evaluation, "evalrank_rerank_ensemble")):
        fn = getattr(mod, name)
        assert callable(fn) and fn.__doc__ and len(fn.__doc__) > 100, name


def test_rerank_ensemble_refuses_on_the_host():
    import pytest
    from itr_amd.metricmodule import evaluation
    with pytest.raises(ValueError):
        evaluation.rerank_ensemble(np.zeros((2, 10), np.float32), [lambda cand, by: None], 9)
    with pytest.raises(ValueError):
        evaluation.rerank_ensemble(np.zeros((2, 10), np.float32), [], 10)
    with pytest.raises(ValueError):
        evaluation.rerank_ensemble(np.zeros((2, 10), np.float32), [lambda cand, by: None] * 5, 10)
    assert evaluation._is_factory(lambda: None) and not evaluation._is_factory(lambda cand, by: None)


def python_sort(idx, vals):
    """the order stated with Python floats and a comparison function, one list"""
    M, K = len(vals), len(idx)
    fused = []
    for i in range(K):
        acc = float(vals[0][i])
        for m in range(1, M):
            acc = acc + float(vals[m][i])
        fused.append(acc / float(M))

    def before(a, b):                 # < 0: entry a stands before entry b
        ca, cb = (math.inf if math.isnan(fused[x]) else fused[x] for x in (a, b))
        if ca != cb:                  # -0.0 == +0.0 as Python floats
            return -1 if ca > cb else 1
        if idx[a] != idx[b]:
            return -1 if idx[a] > idx[b] else 1
        return a - b
    perm = sorted(range(K), key=functools.cmp_to_key(before))
    return perm, fused


def test_oracle_equals_a_plain_python_sort():
    f32 = np.float32
    nan, inf = float('nan'), float('inf')
    #           tie by index      duplicate candidate   -0.0 beside +0.0    NaN     fused NaN   plain
    idx = [3, 9, 5,               7, 7,                 2, 4, 1,            6,      8,          0, 11]
    v0 = [0.5, 0.5, 0.25,         1.0, 1.0,             -0.0, 0.0, -0.0,    nan,    inf,        -inf, 0.75]
    v1 = [0.25, 0.25, 0.5,        0.5, 0.5,             -0.0, 0.0, 0.0,     0.0,    -inf,       1.0, -0.25]
    vals = np.asarray([v0, v1], dtype=f32)
    perm, fused = python_sort(idx, vals)
    # by hand: the two NaN entries (as +inf) first, the higher index (8) before 6; the duplicate 7s (0.75) in coarse order; the
    # 0.375 tie 9, 5, 3 by index; 11 (0.25); the three zeros by index 4, 2, 1 whatever their signs; -inf last
    assert [idx[p] for p in perm] == [8, 6, 7, 7, 9, 5, 3, 11, 4, 2, 1, 0]
    assert perm[2:4] == [3, 4]
    io, fo, vo, po = ensemble_oracle.fuse(np.asarray([idx], dtype=np.int32), vals[:, None, :])
    assert po[0].tolist() == perm and io[0].tolist() == [idx[p] for p in perm]
    want = np.asarray([fused[p] for p in perm], dtype=np.float64)
    assert np.isnan(fo[0][:2]).all() and np.isnan(want[:2]).all()
    assert np.array_equal(fo[0][2:].view(np.uint64), want[2:].view(np.uint64))          # signed zeros keep their sign
    assert np.array_equal(vo[:, 0, :].view(np.uint32), vals[:, perm].view(np.uint32))
    assert fo.dtype == np.float64 and vo.dtype == np.float32 and vo.shape == (2, 1, 12)
    # three members, the sum in member order: (a + b) + c, then / 3.0
    v3 = np.asarray([[0.1], [0.2], [0.3]], dtype=f32)
    _, f3, _, _ = ensemble_oracle.fuse(np.zeros((1, 1), np.int32), v3[:, None, :])
    assert f3[0, 0] == ((float(f32(0.1)) + float(f32(0.2))) + float(f32(0.3))) / 3.0
