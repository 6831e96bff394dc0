"""CPU: the running top-K column lists exist in every layer (library, header, binding, ops, evalpipe, evaluation, command line) and
itr_topk_fold_cols refuses bad arguments before it touches the device.  No kernel is launched here."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest
import torch

from itr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARG, UNSUPPORTED = -1, -2
TOPK_MAX = 128
NAMES = {"itr_topk_fold_workspace_bytes": 3, "itr_topk_fold_cols": 11}
# host addresses standing in for device pointers: every call below is decided on its arguments
_buf = (C.c_double * 64)()
P = C.cast(_buf, C.c_void_p)
NUL = C.c_void_p(0)


def _fold(S=P, ld=40, row0=0, n=8, nc=40, k=5, ck=P, cv=P, ws=NUL, wsb=0):
    return _lib.load().itr_topk_fold_cols(S, ld, row0, n, nc, k, ck, cv, ws, wsb, NUL)


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
    # the header comment of the two entries says that they are additive, and the ABI version did not move
    comment = [c for c in re.findall(r"/\*.*?\*/", raw, flags=re.S) if "itr_topk_fold_cols" in c]
    assert comment and any(re.search(r"additive", c) and "ITR_ABI_VERSION stays 35" in c for c in comment)
    assert int(re.search(r"#define\s+ITR_ABI_VERSION\s+(\d+)", raw).group(1)) == 35
    assert _lib.ABI_VERSION == 35 and lib.itr_abi_version() == 35


def test_fold_checks_arguments_before_launching():
    lib = _lib.load()
    # K outside 1 .. ITR_TOPK_MAX
    assert _fold(k=TOPK_MAX + 1) == UNSUPPORTED
    assert _fold(k=0) == UNSUPPORTED and _fold(k=-3) == UNSUPPORTED
    # null pointers
    assert _fold(S=NUL) == BADARG
    assert _fold(ck=NUL) == BADARG and _fold(cv=NUL) == BADARG and _fold(ck=NUL, cv=NUL) == BADARG
    assert b"null" in lib.itr_last_error()
    # ldS < Nc, negative sizes
    assert _fold(ld=39) == BADARG
    assert _fold(n=-1) == BADARG and _fold(nc=-1, ld=0) == BADARG and _fold(row0=-1) == BADARG
    # rows beyond the 32-bit index of the key
    assert _fold(row0=0x7fffffff - 4, n=8) == BADARG and b"overflow" in lib.itr_last_error()
    assert _fold(row0=1 << 40) == BADARG
    # nothing to fold: success, nothing launched or written
    assert _fold(n=0) == 0 and _fold(nc=0, ld=0) == 0
    # the size query: no workspace grows with rows x Nc (0 bytes is allowed, and a null workspace with it)
    small, big = lib.itr_topk_fold_workspace_bytes(640, 25000, 100), lib.itr_topk_fold_workspace_bytes(640 * 64, 25000, 100)
    assert big == small


def test_ops_reject_cpu_tensors():
    from itr_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.topk_fold_cols(torch.zeros(4, 8), 2)


def test_python_entry_points_exist():
    from itr_amd import evalpipe, ops
    from itr_amd.metricmodule import evaluation
    import inspect
    for mod, name in ((ops, "topk_fold_cols"), (evalpipe, "score_topk_streamed"), (evaluation, "rerank_streamed"),
                      (evaluation, "rerank_ensemble_streamed")):
        fn = getattr(mod, name)
        assert callable(fn) and fn.__doc__ and len(fn.__doc__) > 100, name
    for name in ("evalrank_rerank", "evalrank_rerank_ensemble"):
        p = inspect.signature(getattr(evaluation, name)).parameters
        assert "stream_coarse" in p and p["stream_coarse"].default is False, name


def test_score_topk_streamed_refuses_a_live_comm():
    from itr_amd import evalpipe

    class Live:
        on, virtual = True, False
    with pytest.raises(NotImplementedError, match="one process"):
        evalpipe.score_topk_streamed(torch.zeros(4, 8), torch.zeros(20, 8), None, 10, comm=Live())


def test_test_py_lists_stream_coarse():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "image-text-retrieval_amd", "test.py"), "--help"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--stream-coarse" in r.stdout
