"""CPU: the SGRAF candidate-list entry points exist in every layer (library, header, binding, ops, evaluation), their workspace sizes
grow with the pair and item counts, bad arguments are refused with an error code and a message before anything touches a GPU, and the
item-indexed local-node kernel passes the inline-asm load audit its dense twin passes."""
import os
import re
import shutil
import sys

import pytest

from itr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["itr_sgraf_pairs_state_bytes", "itr_sgraf_pairs_prepare", "itr_sgraf_pairs_prepare_scratch_bytes", "itr_sgraf_pairs_plan_workspace_bytes", "itr_sgraf_pairs_plan",
       "itr_sgraf_pair_scores_workspace_bytes", "itr_sgraf_pair_scores"]


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
    assert _lib.ABI_VERSION > 33          # the parent's library returned 33
    src = open(os.path.join(ROOT, "include", "itr_hip.h")).read()
    assert int(re.search(r"#define\s+ITR_ABI_VERSION\s+(\d+)", src).group(1)) == _lib.ABI_VERSION


def test_python_entry_points_exist():
    from itr_amd import ops
    from itr_amd.metricmodule import evaluation
    for mod, name in ((ops, "sgraf_candidate_scores"), (ops, "sgraf_pairs_prepare"), (ops, "SgrafPairsState"), (evaluation, "_sgraf_score_fn")):
        assert callable(getattr(mod, name))


def test_workspace_sizes_are_monotone():
    lib = _lib.load()
    for mod in (0, 1):
        for S in (64, 256):
            last = 0
            for pairs, items in ((1, 1), (8, 1), (8, 2), (1000, 200), (1000, 300), (100000, 300), (3000000, 700000)):
                b = lib.itr_sgraf_pair_scores_workspace_bytes(pairs, items, 1024, S, mod, 3)
                assert b > last, (mod, S, pairs, items)
                last = b
            # an item holds 64 word rows of D floats at least
            assert lib.itr_sgraf_pair_scores_workspace_bytes(8, 2, 1024, S, mod, 3) >= 2 * 64 * 1024 * 4
    assert lib.itr_sgraf_pairs_state_bytes(5000, 25000, 325000, 1024, 256, 1, 3) > lib.itr_sgraf_pairs_state_bytes(5000, 25000, 325000, 1024, 256, 0, 3)
    assert lib.itr_sgraf_pairs_state_bytes(5000, 25000, 325000, 1024, 256, 0, 3) >= (5000 + 25000) * 1024 * 4 + 5000 * 36 * 36 * 4
    assert lib.itr_sgraf_pairs_plan_workspace_bytes(5000) >= 5001 * 4


def test_host_argument_checks():
    """no kernel is launched: the calls are refused on their arguments"""
    lib = _lib.load()
    one = 16                                                    # any non-null, 16-byte aligned value: refused before any use
    big = 1 << 40

    def score(R=36, D=32, S=256, module=0, steps=3, n_pairs=8, n_items=2, ws=big, state=big):
        return lib.itr_sgraf_pair_scores(one, one, one, one, one, one, one, one, one, one, 0, n_pairs, 0, n_items, 4, 4, 16, R, D, S, module, steps,
                                         one, one, state, one, 8, one, ws, None)

    assert score(module=2) == -1 and b"module_name" in lib.itr_last_error()
    assert score(R=35) == -2 and b"36 regions" in lib.itr_last_error()
    assert score(D=40) == -2
    assert score(S=2048) == -2
    assert score(module=1, steps=9) == -2 and b"sgr_step" in lib.itr_last_error()
    assert score(n_items=9) == -1 and b"items" in lib.itr_last_error()
    assert score(ws=16) == -1 and b"workspace too small" in lib.itr_last_error()
    assert score(state=16) == -1 and b"state buffer too small" in lib.itr_last_error()
    assert lib.itr_sgraf_pair_scores(None, one, one, one, one, one, one, one, one, one, 0, 8, 0, 2, 4, 4, 16, 36, 32, 256, 0, 3, one, one, big, one, 8,
                                     one, big, None) == -1
    assert lib.itr_sgraf_pairs_prepare(one, one, one, one, 4, 4, 16, 36, 32, 256, 0, 3, one, one, 16, one, big, None) == -1
    assert lib.itr_sgraf_pairs_prepare(one, one, one, one, 4, 4, 16, 36, 32, 256, 0, 3, one, one, big, one, 16, None) == -1 and b"scratch" in lib.itr_last_error()
    assert lib.itr_sgraf_pairs_prepare(one, one, one, one, 4, 4, 16, 35, 32, 256, 0, 3, one, one, big, one, big, None) == -2
    assert lib.itr_sgraf_pairs_prepare(one, one, one, one, 70000, 4, 16, 36, 32, 256, 0, 3, one, one, big, one, big, None) == -1
    # the state holds what scoring reads; the global nodes' intermediates are a scratch buffer of their own
    assert lib.itr_sgraf_pairs_state_bytes(5000, 25000, 325000, 1024, 256, 0, 3) < 200 * 2 ** 20
    assert lib.itr_sgraf_pairs_prepare_scratch_bytes(5000, 25000, 325000, 1024, 256, 0) > 325000 * 1024 * 4
    assert lib.itr_sgraf_pairs_plan(one, one, one, one, -1, 4, 4, 16, one, one, one, one, one, one, one, big, None) == -1
    assert lib.itr_sgraf_pairs_plan(one, one, one, one, 8, 4, 4, 16, one, one, one, one, one, one, one, 4, None) == -1
    assert lib.itr_sgraf_pairs_plan(one, one, one, one, 1 << 30, 4, 4, 16, one, one, one, one, one, one, one, big, None) == -2


def test_python_refusals_without_a_gpu():
    import torch
    from itr_amd import ops
    with pytest.raises(ValueError, match="Invalid input of config.module_name"):
        ops.sgraf_candidate_scores(torch.zeros(2, 36, 32), torch.zeros(4, 32), None, {}, torch.zeros(2, 1, dtype=torch.int32), 'image', module_name='AVE')
    with pytest.raises(ValueError, match="by must be"):
        ops.sgraf_candidate_scores(torch.zeros(2, 36, 32), torch.zeros(4, 32), None, {}, torch.zeros(2, 1, dtype=torch.int32), 'rows')
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sgraf_candidate_scores(torch.zeros(2, 36, 32), torch.zeros(4, 32), None, {}, torch.zeros(2, 1, dtype=torch.int32), 'image')


@pytest.mark.skipif(shutil.which("/opt/rocm/bin/hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")
def test_item_kernel_passes_the_asm_load_audit():
    """sgraf_loc_items_kernel runs the generated D loop of sgraf_loc_kernel (hand-counted asm loads): same audit, same rules"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import audit_asm_loads as A
    assert "sgraf_loc_items_kernel" in A.AUDITED_KERNELS["sgraf_loc.hip"]
    res = A.audit_file(os.path.join(ROOT, "image-text-retrieval_amd", "csrc", "sgraf_loc.hip"), no_scratch_in_loops=True, require_listed=True)
    hits = [name for name in res if "sgraf_loc_items_kernel" in name]
    assert hits
    for name in hits:
        assert res[name] == [], "%s:\n  %s" % (name, "\n  ".join(res[name][:20]))
