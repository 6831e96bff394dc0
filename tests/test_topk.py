"""CPU: the top-K retrieval lists' C ABI (argument checks before any launch), the 2-rank gloo exchange of
evalpipe.finalize_topk (HIP kernels replaced by their numpy oracle, tests/helpers/topk_oracle.py) and the
command-line switch.  No compute kernel is launched here."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from itr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARG, UNSUPPORTED = -1, -2
TOPK_MAX = 128
# host addresses standing in for device pointers: every call below fails its checks before anything is launched
_buf = (C.c_double * 64)()
P = C.cast(_buf, C.c_void_p)
NUL = C.c_void_p(0)


def _topk(S=P, ld=40, row0=0, n=8, nc=40, k=5, ri=P, rv=P, ck=P, cv=P, ws=NUL, wsb=0):
    return _lib.load().itr_topk(S, ld, row0, n, nc, k, ri, rv, ck, cv, ws, wsb, NUL)


def _merge(pk=P, pv=P, parts=2, nc=40, k_in=5, k=5, ci=P, cv=P):
    return _lib.load().itr_topk_merge(pk, pv, parts, nc, k_in, k, ci, cv, NUL)


def _f64(S=P, ld=40, n=8, nc=40, k=5, ri=P, rv=P, ci=P, cv=P):
    return _lib.load().itr_topk_f64(S, ld, n, nc, k, ri, rv, ci, cv, NUL)


def test_topk_entry_points_check_arguments_before_launching():
    # null pointers: S, one output of a pair, no direction at all
    assert _topk(S=NUL) == BADARG
    assert _topk(rv=NUL) == BADARG and _topk(cv=NUL) == BADARG
    assert _topk(ri=NUL, rv=NUL, ck=NUL, cv=NUL) == BADARG
    assert _merge(pk=NUL) == BADARG and _merge(ci=NUL) == BADARG
    assert _f64(S=NUL) == BADARG and _f64(ci=NUL) == BADARG
    assert _f64(ri=NUL, rv=NUL, ci=NUL, cv=NUL) == BADARG
    # K = 0 / ITR_TOPK_MAX + 1
    assert _topk(k=0) == BADARG and _merge(k=0) == BADARG and _f64(k=0) == BADARG
    assert _topk(k=TOPK_MAX + 1, nc=400, ld=400) == UNSUPPORTED
    assert _merge(k=TOPK_MAX + 1, k_in=TOPK_MAX, parts=4) == UNSUPPORTED
    assert _f64(k=TOPK_MAX + 1, n=400, nc=400, ld=400) == UNSUPPORTED
    assert _merge(parts=33) == UNSUPPORTED
    # K longer than the line it selects from
    assert _topk(k=41, nc=40) == BADARG                              # a row of 40 columns
    assert _merge(k=11, k_in=5, parts=2) == BADARG                   # two lists of 5
    assert _f64(k=41, nc=40) == BADARG                               # a row
    assert _f64(k=9, n=8, ri=NUL, rv=NUL) == BADARG                  # a column of 8 rows
    # a workspace the call needs but does not get (5 000 rows: the column pass works in row chunks)
    need = _lib.load().itr_topk_workspace_bytes(5000, 40, 10)
    assert need > 0
    assert _topk(n=5000, k=10, ri=NUL, rv=NUL) == BADARG
    assert "workspace" in _lib.load().itr_last_error().decode()
    # empty matrices: success, nothing launched or written
    assert _topk(n=0) == 0 and _topk(nc=0, ld=0) == 0 and _merge(nc=0) == 0 and _f64(n=0) == 0
    assert _lib.load().itr_topk_workspace_bytes(100, 40, 10) == 0   # one row chunk: no workspace


def test_topk_ops_reject_cpu_tensors():
    from itr_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.topk_lists(torch.zeros(4, 8), 2)


def _oracle():
    sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
    import topk_oracle as T
    return T


def test_oracle_order_rules():
    T = _oracle()
    x = np.array([[1.0, np.nan, -0.0, 0.0, np.inf, 1.0, -np.inf]], np.float32)
    idx, val = T.topk_rows(x, 7)
    # NaN ranks as +inf (the tie with the +inf at index 4 goes to the higher index), -0.0 ties with +0.0
    assert idx[0].tolist() == [4, 1, 5, 0, 3, 2, 6]
    assert np.isnan(val[0, 1]) and np.signbit(val[0, 5]) and not np.signbit(val[0, 4])


def _worker(rank, world, port, ni, tmp):
    sys.path.insert(0, os.path.join(ROOT, "image-text-retrieval_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from itr_amd import evalpipe
    import topk_oracle as T
    rng = np.random.RandomState(ni)
    sims = rng.randn(ni, 5 * ni).astype(np.float32)
    sims[:, ::3] = np.round(sims[:, ::3])               # many exact ties, in rows and in columns
    sims[ni // 2] = 1.0                                 # a whole row of one value
    comm = evalpipe.Comm()
    assert comm.world == world and comm.on
    i0, i1 = evalpipe.block_range(ni, world, rank, 4)
    ok = True
    for k in sorted({1, 3, min(ni, 7)}):
        got = evalpipe.finalize_topk(comm, torch.from_numpy(sims[i0:i1].copy()), i0, ni, k, topk_fn=T.topk_lists,
                                     merge_fn=T.topk_merge_cols)
        want = T.topk_all(sims, k)
        for g, key in zip(got, ('i2t_topk', 'i2t_topk_scores', 't2i_topk', 't2i_topk_scores')):
            w = want[key]
            ok = ok and g.shape == w.shape and bool((np.asarray(g) == w).all())
    open(os.path.join(tmp, "ok_%d" % rank), "w").write("1" if ok else "0")
    dist.destroy_process_group()


@pytest.mark.parametrize("ni", [8, 22])
def test_sharded_topk_equals_single_process(tmp_path, ni):
    world = 2
    port = 27500 + (os.getpid() % 2000) + ni
    mp.spawn(_worker, args=(world, port, ni, str(tmp_path)), nprocs=world, join=True)
    for r in range(world):
        assert open(os.path.join(str(tmp_path), "ok_%d" % r)).read() == "1"


def test_finalize_topk_single_process_uses_the_part_as_is():
    T = _oracle()
    from itr_amd import evalpipe
    sims = np.random.RandomState(1).randn(6, 30).astype(np.float32)
    got = evalpipe.finalize_topk(evalpipe.Comm(), torch.from_numpy(sims), 0, 6, 4, topk_fn=T.topk_lists, merge_fn=T.topk_merge_cols)
    want = T.topk_all(sims, 4)
    assert (got[0] == want['i2t_topk']).all() and (got[2] == want['t2i_topk']).all()
    assert (got[3] == want['t2i_topk_scores']).all()


def test_test_py_lists_topk():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "image-text-retrieval_amd", "test.py"), "--help"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--topk" in r.stdout
