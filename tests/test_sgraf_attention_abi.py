"""CPU: the SGRAF pair-attention entry point exists in every layer (library, header, binding, ops, evaluation, command line), the
ABI version is still 35 (the addition changes no existing signature), every declared symbol is exported and bound, and the entry
refuses bad arguments on the host before anything touches a device."""
import ctypes as C
import inspect
import os
import re

from itr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "itr_sgraf_pair_attention"


def header_source():
    src = open(os.path.join(ROOT, "include", "itr_hip.h")).read()
    return src, re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_symbols_exported_declared_and_bound():
    lib = _lib.load()
    raw, src = header_source()
    for name, ret in ((NAME, C.c_int), (NAME + "_workspace_bytes", C.c_size_t)):
        assert hasattr(lib, name), "libitr_hip.so does not export %s" % name
        m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, src)
        assert m, "include/itr_hip.h does not declare %s" % name
        declared = [a for a in m.group(1).split(",") if a.strip()]
        assert name in _lib.SIGNATURES
        assert len(declared) == len(_lib.SIGNATURES[name][1])
        assert _lib.SIGNATURES[name][0] is ret
    # the reference lines it restates are cited with the declaration
    at = raw.index("int %s(" % NAME)
    comment = raw[raw.rindex("/*", 0, at):at]
    for cite in ("Fusionmodule.py:406-451", ":581-587", ":615-619", ":632-664"):
        assert cite in comment, cite
    assert "ITR_ABI_VERSION stays 35" in comment


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
    for mod, name in ((ops, "sgraf_pair_attention"), (ops, "sgraf_candidate_attention"), (ops, "SgrafPairAttention"),
                      (evaluation, "explain_sgraf")):
        assert callable(getattr(mod, name))
    params = inspect.signature(evaluation.evalrank_rerank).parameters
    assert "explain_sgraf" in params and params["explain_sgraf"].default is None
    for acc in ("matrix", "nodes", "edges"):
        assert hasattr(ops.SgrafPairAttention, acc)
    assert list(inspect.signature(ops.sgraf_pair_attention).parameters) == [
        "images", "words", "plan", "weights", "pairs", "module_name", "sgr_step", "state", "max_workspace_bytes"]
    cli = open(os.path.join(ROOT, "image-text-retrieval_amd", "test.py")).read()
    assert "--explain-sgraf" in cli


def call(lib, n_pairs=8, n_items=2, p0=0, R=36, D=32, S=64, module=0, steps=3, ws_bytes=1 << 40, state_bytes=1 << 40, attn_len=1 << 20,
         node_len=1 << 20, edge_len=1 << 20, out_len=8, img=16, pair_img=16, attn=16, node_w=16, edge=16, w=16):
    one = 16                                                    # any non-null, 16-byte aligned value: refused before any use
    return lib.itr_sgraf_pair_attention(img, one, one, pair_img, one, one, one, one, one, one, p0, n_pairs, 0, n_items, 4, 4, 16, R, D, S, module,
                                        steps, w, one, state_bytes, attn, one, attn_len, node_w, one, node_len, edge, one, edge_len, one, out_len,
                                        one, ws_bytes, None)


def test_host_argument_checks():
    """no kernel is launched: every call is refused on its arguments"""
    lib = _lib.load()
    assert call(lib, R=35) == -2
    assert call(lib, D=24) == -2
    assert call(lib, S=512) == -2
    assert b"sim_dim" in lib.itr_last_error()
    assert call(lib, S=40) == -2
    assert call(lib, module=1, steps=9) == -2
    assert call(lib, module=2) == -1
    assert call(lib, p0=(1 << 31) // 64) == -2                        # pair-count overflow: a column index is 64 x the item index in int32
    assert b"split" in lib.itr_last_error()
    assert call(lib, ws_bytes=16) == -1
    assert b"workspace" in lib.itr_last_error()
    assert call(lib, state_bytes=16) == -1
    assert b"state" in lib.itr_last_error()
    for kw in (dict(n_pairs=-1), dict(n_items=-1), dict(p0=-1), dict(out_len=-1), dict(attn_len=-1), dict(node_len=-1), dict(edge_len=-1),
               dict(n_pairs=2, n_items=3), dict(n_pairs=2, n_items=0)):
        assert call(lib, **kw) == -1, kw
    for kw in (dict(img=None), dict(pair_img=None), dict(attn=None), dict(node_w=None), dict(module=1, edge=None), dict(w=None)):
        assert call(lib, **kw) == -1, kw
        assert b"null" in lib.itr_last_error()
    # the buffer of the other module may be null
    sz = lib.itr_sgraf_pair_attention_workspace_bytes
    assert sz(8, 2, 32, 64, 0, 3) > 0 and sz(16, 4, 32, 64, 0, 3) > sz(8, 2, 32, 64, 0, 3)
    assert sz(-1, 2, 32, 64, 0, 3) == 0
    assert sz(8, 2, 32, 64, 1, 3) <= lib.itr_sgraf_pair_scores_workspace_bytes(8, 2, 32, 64, 1, 3)
