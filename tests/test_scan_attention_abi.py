"""CPU: the SCAN pair-attention entry point exists in every layer (library, header, binding, ops, evaluation), the ABI version
is 35, every declared symbol is exported, and the entry refuses bad arguments on the host before anything touches a device."""
import ctypes as C
import os
import re

from itr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "itr_scan_pair_attention"


def header_source():
    src = open(os.path.join(ROOT, "include", "itr_hip.h")).read()
    return src, re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_symbol_exported_declared_and_bound():
    lib = _lib.load()
    raw, src = header_source()
    assert hasattr(lib, NAME), "libitr_hip.so does not export %s" % NAME
    m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % NAME, src)
    assert m, "include/itr_hip.h does not declare %s" % NAME
    declared = [a for a in m.group(1).split(",") if a.strip()]
    assert NAME in _lib.SIGNATURES
    assert len(declared) == len(_lib.SIGNATURES[NAME][1])
    assert _lib.SIGNATURES[NAME][0] is C.c_int
    # the reference lines it replaces are cited with the declaration
    at = raw.index("int %s(" % NAME)
    assert "Objectives.py:421-476" in raw[raw.rindex("/*", 0, at):at]


def test_abi_version_is_35_and_counts_agree():
    lib = _lib.load()
    raw, src = header_source()
    assert _lib.ABI_VERSION == 35 and lib.itr_abi_version() == 35
    assert int(re.search(r"#define\s+ITR_ABI_VERSION\s+(\d+)", raw).group(1)) == 35
    declared = sorted(set(re.findall(r"\b(itr_[a-z0-9_]+)\s*\(", src)))
    exported = [s for s in declared if hasattr(lib, s)]
    assert len(exported) == len(declared) == len(_lib.SIGNATURES)


def test_python_entry_points_exist():
    from itr_amd import ops
    from itr_amd.metricmodule import evaluation
    for mod, name in ((ops, "scan_pair_attention"), (ops, "scan_candidate_attention"), (ops, "ScanPairAttention"), (evaluation, "explain")):
        assert callable(getattr(mod, name))
    import inspect
    assert "explain" in inspect.signature(evaluation.evalrank_rerank).parameters
    assert hasattr(ops.ScanPairAttention, "matrix")


def call(lib, P=8, R=36, D=32, mode=0, norm=0, agg=0, ws_bytes=1 << 30, attn_len=8 * 96 * 36, row_len=8 * 96, pair_img=16, attn=16):
    one = 16                                                    # any non-null, 16-byte aligned value: refused before any use
    return lib.itr_scan_pair_attention(one, one, one, one, pair_img, one, P, 4, 4, 16, R, D, mode, norm, agg, 9.0, 6.0, attn, one, attn_len,
                                       one, one, row_len, one, one, ws_bytes, None)


def test_host_argument_checks():
    """no kernel is launched: every call is refused on its arguments"""
    lib = _lib.load()
    assert call(lib, R=35) == -2
    assert call(lib, D=24) == -2
    assert call(lib, P=(1 << 31) // (96 * 36) + 1) == -2             # P * 96 * 36 >= 2^31
    assert b"split" in lib.itr_last_error()
    assert call(lib, norm=7) == -1
    assert call(lib, agg=4) == -1
    assert call(lib, mode=2) == -1
    assert call(lib, ws_bytes=16) == -1
    assert b"workspace" in lib.itr_last_error()
    assert call(lib, P=-1) == -1
    assert call(lib, attn_len=-1) == -1
    assert call(lib, pair_img=None) == -1
    assert call(lib, attn=None) == -1
    assert b"null" in lib.itr_last_error()
