"""CPU: the hubness correction exists in every layer (library, header, binding, ops, evaluation, command line) and its entry points
refuse bad arguments before they touch the device.  No kernel is launched here."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import pytest
import torch

from itr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEST_PY = os.path.join(ROOT, "image-text-retrieval_amd", "test.py")
BADARG, UNSUPPORTED = -1, -2
NAMES = {"itr_hub_lse_workspace_bytes": 2, "itr_hub_lse_fold": 11, "itr_hub_lse_finish": 5, "itr_hub_list_mean": 7, "itr_hub_adjust": 10}
# host addresses standing in for device pointers: every call below is decided on its arguments
_buf = (C.c_double * 4096)()
BASE = C.addressof(_buf)
P = C.c_void_p(BASE)
NUL = C.c_void_p(0)


def _at(byte_offset):
    return C.c_void_p(BASE + byte_offset)


def _fold(S=P, f64=0, ld=40, n=8, nc=40, beta=20.0, row=P, col=P, ws=P, wsb=1 << 20):
    return _lib.load().itr_hub_lse_fold(S, f64, ld, n, nc, beta, row, col, ws, wsb, NUL)


def _finish(state=P, nc=40, beta=20.0, out=P):
    return _lib.load().itr_hub_lse_finish(state, nc, beta, out, NUL)


def _mean(val=P, f64=0, n=8, ld=16, k=5, out=P):
    return _lib.load().itr_hub_list_mean(val, f64, n, ld, k, out, NUL)


def _adjust(S=P, f64=1, ld=4, n=2, nc=4, a=NUL, b=NUL, out=None, ldo=4):
    return _lib.load().itr_hub_adjust(S, f64, ld, n, nc, a, b, _at(1024) if out is None else out, ldo, NUL)


def test_symbols_exported_declared_and_bound():
    lib = _lib.load()
    raw = open(os.path.join(ROOT, "include", "itr_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name, nargs in NAMES.items():
        assert hasattr(lib, name), "libitr_hip.so does not export %s" % name
        assert name in _lib.SIGNATURES
        m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, src)
        assert m, "include/itr_hip.h does not declare %s" % name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]) == nargs
    comment = [c for c in re.findall(r"/\*.*?\*/", raw, flags=re.S) if "itr_hub_lse_fold" in c]
    assert comment and any(re.search(r"additive", c) and "ITR_ABI_VERSION stays 35" in c for c in comment)
    assert int(re.search(r"#define\s+ITR_ABI_VERSION\s+(\d+)", raw).group(1)) == 35
    assert _lib.ABI_VERSION == 35 and lib.itr_abi_version() == 35
    assert os.path.exists(os.path.join(ROOT, "image-text-retrieval_amd", "csrc", "hubness.hip"))


def test_entries_check_arguments_before_launching():
    lib = _lib.load()
    # beta must be finite and positive
    for beta in (0.0, -1.0, float('nan'), float('inf')):
        assert _fold(beta=beta) == BADARG and b"beta" in lib.itr_last_error()
        assert _finish(beta=beta) == BADARG
    # k < 1, k above ITR_TOPK_MAX
    assert _mean(k=0) == BADARG and _mean(k=-2) == BADARG
    assert _mean(k=129, ld=200) == UNSUPPORTED and b"ITR_TOPK_MAX" in lib.itr_last_error()
    assert _mean(k=8, ld=7) == BADARG
    # ldS < Nc, negative sizes
    assert _fold(ld=39) == BADARG and _adjust(ld=3) == BADARG and _adjust(ldo=3) == BADARG
    assert _fold(n=-1) == BADARG and _fold(nc=-1, ld=0) == BADARG
    assert _finish(nc=-1) == BADARG and _mean(n=-1) == BADARG and _adjust(n=-1) == BADARG
    # null pointers
    assert _fold(S=NUL) == BADARG and b"null" in lib.itr_last_error()
    assert _fold(ws=NUL) == BADARG and _fold(wsb=8) == BADARG
    assert _finish(state=NUL) == BADARG and _finish(out=NUL) == BADARG
    assert _mean(val=NUL) == BADARG and _mean(out=NUL) == BADARG
    assert _adjust(S=NUL) == BADARG and _adjust(out=NUL) == BADARG
    # empty shapes: success, nothing launched or written (null pointers are fine then)
    assert _fold(n=0, S=NUL, row=NUL, col=NUL, ws=NUL, wsb=0) == 0 and _fold(nc=0, ld=0) == 0
    assert _finish(nc=0, state=NUL, out=NUL) == 0 and _mean(n=0, val=NUL, out=NUL) == 0
    assert _adjust(n=0, S=NUL, out=NUL) == 0 and _adjust(nc=0, ld=0, ldo=0) == 0
    # the workspace grows with the block, not with rows x Nc, and covers the partial sums of both directions
    small, big = lib.itr_hub_lse_workspace_bytes(640, 25000), lib.itr_hub_lse_workspace_bytes(5000, 25000)
    assert 0 < small <= big < 5000 * 25000 * 4 // 4
    assert lib.itr_hub_lse_workspace_bytes(0, 10) == 0


def test_adjust_refuses_partial_overlap():
    lib = _lib.load()
    # S: 2 x 4 doubles at BASE (64 bytes)
    assert _adjust(out=_at(8)) == BADARG and b"alias" in lib.itr_last_error()          # shifted by one element
    assert _adjust(out=_at(56)) == BADARG and b"alias" in lib.itr_last_error()         # the last element only
    assert _adjust(out=P, ld=4, ldo=5) == BADARG and b"alias" in lib.itr_last_error()  # same base, another stride
    assert _adjust(a=_at(1024 + 8)) == BADARG and b"alias" in lib.itr_last_error()     # a inside out
    assert _adjust(b=_at(1024 + 32)) == BADARG and b"alias" in lib.itr_last_error()
    # (in place, out == S with ldo == ldS, and disjoint buffers pass these checks: they reach the launch, which needs a GPU)


def test_ops_reject_cpu_tensors():
    from itr_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.hub_lse_fold(torch.zeros(4, 8), 20.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.hub_lse_cols(torch.zeros(8, 2, dtype=torch.float64), 20.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.hub_list_mean(torch.zeros(4, 8), 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.hub_adjust(torch.zeros(4, 8, dtype=torch.float64))


def test_python_entry_points_exist():
    from itr_amd import ops
    from itr_amd.metricmodule import evaluation
    for mod, name in ((ops, "hub_lse_fold"), (ops, "hub_lse_cols"), (ops, "hub_list_mean"), (ops, "hub_adjust"),
                      (evaluation, "hubness_vectors"), (evaluation, "hubness_bank_vectors"), (evaluation, "hubness_adjust")):
        fn = getattr(mod, name)
        assert callable(fn) and fn.__doc__ and len(fn.__doc__) > 100, name
    p = inspect.signature(ops.hub_lse_fold).parameters
    assert list(p) == ["S_block", "beta", "state", "rows", "cols"] and p["rows"].default is True and p["cols"].default is True
    assert list(inspect.signature(ops.hub_adjust).parameters) == ["S", "a", "b", "out"]
    for name in ("evalrank_single", "evalrank_ensemble"):
        p = inspect.signature(getattr(evaluation, name)).parameters
        assert p["hubness"].default is None and p["hub_k"].default == 10 and p["hub_beta"].default == 20.0, name
        assert p["querybank"].default == 'self', name
    assert "hubness" not in inspect.signature(evaluation.evalrank_fast).parameters


def test_evaluation_refuses_bad_hubness_arguments_on_the_host():
    from itr_amd.metricmodule import evaluation
    # decided before the checkpoint is opened: the path does not exist
    for kw, msg in ((dict(hubness='qbnorm'), "hubness must be one of"), (dict(hubness='csls', hub_k=0), "hub_k"),
                    (dict(hubness='invsoftmax', hub_beta=0.0), "hub_beta"), (dict(hubness='invsoftmax', hub_beta=float('inf')), "hub_beta"),
                    (dict(hub_k=3), "need hubness"), (dict(querybank='dev'), "need hubness"), (dict(hub_beta=5.0), "need hubness")):
        with pytest.raises(ValueError, match=msg):
            evaluation.evalrank_single('/nonexistent/model.pth.tar', **kw)
        with pytest.raises(ValueError, match=msg):
            evaluation.evalrank_ensemble('/nonexistent/a.pth.tar', '/nonexistent/b.pth.tar', **kw)


def _run(*args):
    return subprocess.run([sys.executable, TEST_PY] + list(args), capture_output=True, text=True, timeout=120)


def test_test_py_lists_and_refuses_the_flags():
    r = _run("--help")
    assert r.returncode == 0
    for flag in ("--hubness", "--hub-k", "--hub-beta", "--querybank"):
        assert flag in r.stdout, flag
    for args, msg in ((("m", "--hubness", "csls", "--fast"), "--hubness does not combine with --fast"),
                      (("m", "m", "--hubness", "invsoftmax", "--rerank", "4"), "--hubness does not combine with --rerank"),
                      (("m", "--hub-k", "3"), "need --hubness"), (("m", "--hub-beta", "5"), "need --hubness"),
                      (("m", "--querybank", "dev"), "need --hubness"), (("m", "--hubness", "qbnorm"), "invalid choice")):
        r = _run(*args)
        assert r.returncode == 2 and msg in r.stderr, (args, r.stderr[-500:])
