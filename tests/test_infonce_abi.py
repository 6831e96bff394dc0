"""CPU: the InfoNCE loss exists in every layer -- library, header, binding, ops, criterion, config -- the ABI version is still 35, every
declared symbol is exported and bound, and both entries refuse bad arguments on the host before anything touches a device."""
import ctypes as C
import inspect
import os
import re

import pytest

from itr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"itr_infonce_fwd": 10, "itr_infonce_bwd": 11, "itr_infonce_workspace_bytes": 1}
INF, NAN = float("inf"), float("nan")


def header_source():
    src = open(os.path.join(ROOT, "include", "itr_hip.h")).read()
    return src, re.sub(r"/\*.*?\*/", "", src, flags=re.S)


@pytest.mark.parametrize("name", sorted(NAMES))
def test_symbol_exported_declared_and_bound(name):
    lib = _lib.load()
    _, src = header_source()
    assert hasattr(lib, name), "libitr_hip.so does not export %s" % name
    m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, src)
    assert m, "include/itr_hip.h does not declare %s" % name
    declared = [a for a in m.group(1).split(",") if a.strip()]
    assert name in _lib.SIGNATURES
    assert len(declared) == len(_lib.SIGNATURES[name][1]) == NAMES[name]
    assert _lib.SIGNATURES[name][0] is (C.c_size_t if name.endswith("_bytes") else C.c_int)
    if not name.endswith("_bytes"):
        assert "group" in declared[1] and "int32_t" in declared[1] and "scale" in declared[4] and "float" in declared[4]


def test_header_comment():
    raw, _ = header_source()
    at = raw.index("size_t itr_infonce_workspace_bytes(")
    comment = raw[raw.rindex("/*", 0, at):at]
    assert "next to ContrastiveLoss.forward (Objectives.py:93-115) and replaces no reference line" in comment
    assert "Purely additive: no existing signature changes, ITR_ABI_VERSION stays 35" in comment
    for piece in ("group[i] == group[j]", "row_lse[i] = log sum_{j in A(i)} exp(z[i,j])", "col_lse[j] = log sum_{i in A(j)} exp(z[i,j])",
                  "/ (2 B)", "- 2 [i == j]", "dS[i,j] = 0 exactly at masked entries", "no float atomics", "NULL"):
        assert piece in comment, piece


def test_abi_version_is_35_and_counts_agree():
    lib = _lib.load()
    raw, src = header_source()
    assert _lib.ABI_VERSION == 35 and lib.itr_abi_version() == 35
    assert int(re.search(r"#define\s+ITR_ABI_VERSION\s+(\d+)", raw).group(1)) == 35
    declared = sorted(set(re.findall(r"\b(itr_[a-z0-9_]+)\s*\(", src)))
    exported = [s for s in declared if hasattr(lib, s)]
    assert len(exported) == len(declared) == len(_lib.SIGNATURES)
    assert set(NAMES) <= set(declared)


def test_workspace_bytes_on_the_host():
    lib = _lib.load()
    assert lib.itr_infonce_workspace_bytes(0) == 0 and lib.itr_infonce_workspace_bytes(-4) == 0
    sizes = [lib.itr_infonce_workspace_bytes(B) for B in (1, 64, 65, 128, 1024, 1025, 100000)]
    assert all(s > 0 and s % 8 == 0 for s in sizes) and sizes == sorted(sizes)
    # one (max, sum) pair per column and row slice; the slices stop growing, so the scratch stays linear in B
    assert sizes[0] == 8 and sizes[-1] <= 8 * 16 * 100000


def fwd(lib, S=16, group=16, B=8, ldS=8, scale=20.0, loss=16, row_lse=16, col_lse=16, ws=16):
    """16 = any non-null value: every call below is refused before any use"""
    return lib.itr_infonce_fwd(S, group, B, ldS, scale, loss, row_lse, col_lse, ws, None)


def bwd(lib, S=16, group=16, B=8, ldS=8, scale=20.0, row_lse=16, col_lse=16, grad=16, dS=16, lddS=8):
    return lib.itr_infonce_bwd(S, group, B, ldS, scale, row_lse, col_lse, grad, dS, lddS, None)


def test_host_argument_checks():
    """no kernel is launched: every call is refused on its arguments (group = NULL is no error: it means no mask, so each call
    below is made with and without a group vector)"""
    lib = _lib.load()
    for group in (16, None):
        for kw in (dict(S=None), dict(loss=None), dict(row_lse=None), dict(col_lse=None), dict(ws=None)):
            assert fwd(lib, group=group, **kw) == -1, kw
            assert b"itr_infonce_fwd: null pointer" in lib.itr_last_error(), kw
        for kw in (dict(B=0), dict(B=-3), dict(ldS=7)):
            assert fwd(lib, group=group, **kw) == -1, kw
            assert b"itr_infonce_fwd: bad shape" in lib.itr_last_error(), kw
        for kw in (dict(scale=0.0), dict(scale=-20.0), dict(scale=INF), dict(scale=-INF), dict(scale=NAN)):
            assert fwd(lib, group=group, **kw) == -1, kw
            assert b"itr_infonce_fwd: scale" in lib.itr_last_error(), kw
        for kw in (dict(S=None), dict(row_lse=None), dict(col_lse=None), dict(grad=None), dict(dS=None)):
            assert bwd(lib, group=group, **kw) == -1, kw
            assert b"itr_infonce_bwd: null pointer" in lib.itr_last_error(), kw
        for kw in (dict(B=0), dict(B=-3), dict(ldS=7), dict(lddS=7)):
            assert bwd(lib, group=group, **kw) == -1, kw
            assert b"itr_infonce_bwd: bad shape" in lib.itr_last_error(), kw
        for kw in (dict(scale=0.0), dict(scale=-20.0), dict(scale=INF), dict(scale=NAN)):
            assert bwd(lib, group=group, **kw) == -1, kw
            assert b"itr_infonce_bwd: scale" in lib.itr_last_error(), kw


def test_config_keys():
    from itr_amd import config
    assert config.DEFAULTS['loss'] == 'hinge' and config.DEFAULTS['temperature'] == 0.05
    assert 'loss' not in config.load_hyperparams and 'temperature' not in config.load_hyperparams      # training switches
    cfg = config.build_config(['with', 'SCAN'])
    assert cfg['loss'] == 'hinge' and cfg['temperature'] == 0.05
    cfg = config.build_config(['with', 'SCAN', 'loss=infonce', 'temperature=0.07'])
    assert cfg['loss'] == 'infonce' and cfg['temperature'] == 0.07


def test_python_entry_points():
    from itr_amd import ops
    from itr_amd.modalmodule import Models, Objectives
    assert list(inspect.signature(ops.infonce_loss).parameters) == ["scores", "temperature", "groups"]
    assert inspect.signature(ops.infonce_loss).parameters['temperature'].default == 0.05
    assert inspect.signature(ops.infonce_loss).parameters['groups'].default is None
    assert callable(ops.infonce_fwd) and callable(ops.infonce_bwd)
    assert list(inspect.signature(Objectives.InfoNCELoss.__init__).parameters) == ["self", "config", "temperature", "measure"]
    assert list(inspect.signature(Objectives.InfoNCELoss.forward).parameters) == list(inspect.signature(Objectives.ContrastiveLoss.forward).parameters)
    # the two criteria share one similarity dispatch: neither defines its own
    shared = [c for c in Objectives.InfoNCELoss.__mro__ if '_sim_on_tape' in vars(c)]
    assert shared == [c for c in Objectives.ContrastiveLoss.__mro__ if '_sim_on_tape' in vars(c)] and len(shared) == 1
    assert shared[0] not in (Objectives.InfoNCELoss, Objectives.ContrastiveLoss)
    assert callable(Models.base_module._hinge) and callable(Models.base_module._hinge_groups)


def test_unknown_loss_and_bad_temperature_are_refused_on_the_host():
    from itr_amd import ops
    from itr_amd.modalmodule import Models, Objectives
    for kind in ('softmax', 'Hinge', '', None):
        with pytest.raises(ValueError, match="unknown loss"):
            Models.base_module({'loss': kind})
    assert Models.base_module({})._hinge is not None and Models.base_module({'loss': 'infonce'}).config['loss'] == 'infonce'
    assert Objectives.retrieval_loss_kind({}) == 'hinge'              # a configuration from an old checkpoint
    for t in (0.0, -0.05, INF, NAN, 1e-60):
        with pytest.raises(ValueError, match="temperature"):
            ops._infonce_scale(t)
