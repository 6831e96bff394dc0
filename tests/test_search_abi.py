"""CPU: the query-time search exists in every layer (library, header, binding, ops, itr_amd.search, command line) and
itr_search_topk refuses bad arguments before it touches the device.  No kernel is launched here."""
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
BADARG, UNSUPPORTED = -1, -2
TOPK_MAX, MAX_QUERIES, MAX_SLABS = 128, 64, 1024
NAMES = {"itr_search_topk_workspace_bytes": 4, "itr_search_topk": 16}
# host addresses standing in for device pointers: every call below is decided on its arguments
_buf = (C.c_double * 64)()
P = C.cast(_buf, C.c_void_p)
NUL = C.c_void_p(0)


def _search(q=P, ldq=40, nq=3, g=P, ldg=40, row0=0, n=100, d=40, k=5, slabs=0, key=P, val=P, idx=P, ws=P, wsb=1 << 40):
    return _lib.load().itr_search_topk(q, ldq, nq, g, ldg, row0, n, d, k, slabs, key, val, idx, ws, wsb, NUL)


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
    comment = [c for c in re.findall(r"/\*.*?\*/", raw, flags=re.S) if "itr_search_topk" in c]
    assert comment and any(re.search(r"additive", c) and c.rstrip(" */").endswith("ITR_ABI_VERSION stays 35.") for c in comment)
    assert any("Objectives.py:18-21" in c and "evaluation.py:169" in c and ":209" in c for c in comment)
    assert int(re.search(r"#define\s+ITR_SEARCH_MAX_QUERIES\s+(\d+)", raw).group(1)) == MAX_QUERIES
    assert int(re.search(r"#define\s+ITR_SEARCH_MAX_SLABS\s+(\d+)", raw).group(1)) == MAX_SLABS
    assert int(re.search(r"#define\s+ITR_ABI_VERSION\s+(\d+)", raw).group(1)) == 35
    assert _lib.ABI_VERSION == 35 and lib.itr_abi_version() == 35


def test_search_checks_arguments_before_launching():
    lib = _lib.load()
    # null pointers (idx alone may be null; a null workspace is refused: every call with a gallery needs one)
    assert _search(q=NUL) == BADARG and b"null" in lib.itr_last_error()
    assert _search(g=NUL) == BADARG and _search(key=NUL) == BADARG and _search(val=NUL) == BADARG
    assert _search(ws=NUL) == BADARG and _search(wsb=8) == BADARG
    # leading dimensions below D, negative sizes, D < 1
    assert _search(ldq=39) == BADARG and _search(ldg=39) == BADARG
    assert _search(nq=-1) == BADARG and _search(n=-1) == BADARG and _search(row0=-1) == BADARG
    assert _search(d=0, ldq=0, ldg=0) == BADARG and _search(d=-4) == BADARG
    # rows beyond the 32-bit index of the key
    assert _search(row0=0x7fffffff - 50, n=100) == BADARG and b"overflow" in lib.itr_last_error()
    assert _search(row0=1 << 40) == BADARG
    # n_slabs outside 0 .. the documented maximum
    assert _search(slabs=-1) == BADARG and _search(slabs=MAX_SLABS + 1) == BADARG
    # K or n_queries outside their ranges
    assert _search(k=0) == UNSUPPORTED and _search(k=-2) == UNSUPPORTED and _search(k=TOPK_MAX + 1) == UNSUPPORTED
    assert _search(nq=MAX_QUERIES + 1) == UNSUPPORTED and str(MAX_QUERIES).encode() in lib.itr_last_error()
    # no queries: success, nothing launched (not even the pointers are looked at)
    assert _search(nq=0) == 0 and _search(nq=0, q=NUL, key=NUL, val=NUL, ws=NUL, wsb=0) == 0
    # the size query: parts of the slabs, never rows x queries; 0 for arguments the entry refuses
    size = lib.itr_search_topk_workspace_bytes
    assert size(64, 566435, 100, 0) <= MAX_SLABS * 64 * 100 * 12 * 2 + 4096
    assert size(1, 1000, 10, 1) > 0 and size(1, 1000, 10, MAX_SLABS) >= MAX_SLABS * 10 * 12
    assert size(MAX_QUERIES + 1, 10, 10, 0) == 0 and size(1, 10, TOPK_MAX + 1, 0) == 0 and size(1, 10, 10, MAX_SLABS + 1) == 0


def test_ops_reject_cpu_tensors_and_too_many_queries():
    from itr_amd import ops
    assert ops.SEARCH_MAX_QUERIES == MAX_QUERIES and ops.SEARCH_MAX_SLABS == MAX_SLABS
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.search_topk(torch.zeros(2, 8), torch.zeros(10, 8), 3)
    assert ops.search_topk.__doc__ and len(ops.search_topk.__doc__) > 100


def test_gallery_index_and_its_methods_exist_with_docstrings():
    from itr_amd import search
    G = search.GalleryIndex
    assert G.__doc__ and len(G.__doc__) > 100
    for name in ("build", "from_embeddings", "save", "load", "encode_text", "encode_images", "search_embedded", "search_text",
                 "search_images"):
        fn = getattr(G, name)
        assert callable(fn) and fn.__doc__ and len(fn.__doc__) > 60, name
    assert "batch" in G.encode_text.__doc__ and "batch_invariant" in G.encode_text.__doc__
    p = inspect.signature(G.build).parameters
    assert list(p)[:5] == ["coarse_path", "fine_path", "data_path", "split", "sides"] and p["split"].default == "test"
    p = inspect.signature(G.search_embedded).parameters
    assert list(p)[1:] == ["q", "direction", "k", "rerank"] and p["rerank"].default is None
    assert list(inspect.signature(G.from_embeddings).parameters)[:4] == ["coarse", "fine", "fine_model", "im_div"]


@pytest.mark.parametrize("cfg,why", [({"name": "SCAN"}, "pooled"), ({"name": "SGRAF"}, "pooled"), ({"name": "CAMERA"}, "views"),
                                     ({"name": "SAEM", "measure": "cosine"}, "NaN"), ({"name": "VSE++", "measure": "order"}, "order")])
def test_unsupported_coarse_families_say_why(cfg, why):
    from itr_amd import search
    with pytest.raises(NotImplementedError, match=why):
        search._check_coarse(cfg)
    search._check_coarse({"name": "VSE++", "measure": "cosine"})
    search._check_coarse({"name": "VSRN", "measure": "cosine"})
    with pytest.raises(NotImplementedError, match="SCAN or SGRAF"):
        search._check_fine({"name": "VSE++"})


def test_search_py_lists_its_flags():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "image-text-retrieval_amd", "search.py"), "--help"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0
    for flag in ("--split", "--data-path", "--index", "--query", "--queries", "--query-images", "-k", "--rerank", "--out"):
        assert flag in r.stdout, flag
