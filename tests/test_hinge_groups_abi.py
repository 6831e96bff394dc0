"""CPU: the masked hinge (same-image captions are no negatives) exists in every layer -- library, header, binding, ops, losses, config --
the ABI version is still 35, every declared symbol is exported and bound, and both entries refuse bad arguments on the host before
anything touches a device."""
import ctypes as C
import inspect
import os
import re

import pytest

from itr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"itr_hinge_groups_fwd": 11, "itr_hinge_groups_bwd": 12}


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
    assert _lib.SIGNATURES[name][0] is C.c_int
    # the existing pair's arguments plus the group vector, in second place
    base = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name.replace("groups", "maxviol"), src).group(1).split(",")
    assert len(declared) == len(base) + 1 and "group" in declared[1] and "int32_t" in declared[1]
    assert len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES[name.replace("groups", "maxviol")][1]) + 1


def test_header_comment():
    raw, _ = header_source()
    at = raw.index("int itr_hinge_groups_fwd(")
    comment = raw[raw.rindex("/*", 0, at):at]
    for cite in ("Objectives.py:93-115", ":492-517"):
        assert cite in comment, cite
    assert "Purely additive: no existing signature changes, ITR_ABI_VERSION stays 35" in comment
    assert "group[i] == group[j]" in comment and "lower index" in comment and "UNMASKED" in comment


def test_abi_version_is_35_and_counts_agree():
    lib = _lib.load()
    raw, src = header_source()
    assert _lib.ABI_VERSION == 35 and lib.itr_abi_version() == 35
    assert int(re.search(r"#define\s+ITR_ABI_VERSION\s+(\d+)", raw).group(1)) == 35
    declared = sorted(set(re.findall(r"\b(itr_[a-z0-9_]+)\s*\(", src)))
    exported = [s for s in declared if hasattr(lib, s)]
    assert len(exported) == len(declared) == len(_lib.SIGNATURES)


def fwd(lib, S=16, group=16, B=8, ldS=8, mv=1, loss=16, row_arg=16, col_arg=16, ws=16):
    """16 = any non-null value: every call below is refused before any use"""
    return lib.itr_hinge_groups_fwd(S, group, B, ldS, 0.2, mv, loss, row_arg, col_arg, ws, None)


def bwd(lib, S=16, group=16, B=8, ldS=8, mv=1, row_arg=16, col_arg=16, grad=16, dS=16, lddS=8):
    return lib.itr_hinge_groups_bwd(S, group, B, ldS, 0.2, mv, row_arg, col_arg, grad, dS, lddS, None)


def test_host_argument_checks():
    """no kernel is launched: every call is refused on its arguments"""
    lib = _lib.load()
    for kw in (dict(S=None), dict(group=None), dict(loss=None), dict(ws=None)):
        assert fwd(lib, **kw) == -1, kw
        assert b"itr_hinge_groups_fwd" in lib.itr_last_error() and b"null" in lib.itr_last_error(), kw
    for kw in (dict(B=0), dict(B=-3), dict(ldS=7)):
        assert fwd(lib, **kw) == -1, kw
        assert b"itr_hinge_groups_fwd: bad shape" in lib.itr_last_error(), kw
    for kw in (dict(row_arg=None), dict(col_arg=None)):
        assert fwd(lib, **kw) == -1, kw
        assert b"required with max_violation" in lib.itr_last_error(), kw
    for kw in (dict(S=None), dict(group=None), dict(grad=None), dict(dS=None)):
        assert bwd(lib, **kw) == -1, kw
        assert b"itr_hinge_groups_bwd" in lib.itr_last_error() and b"null" in lib.itr_last_error(), kw
    for kw in (dict(B=0), dict(ldS=7), dict(lddS=7)):
        assert bwd(lib, **kw) == -1, kw
        assert b"itr_hinge_groups_bwd: bad shape" in lib.itr_last_error(), kw
    for kw in (dict(row_arg=None), dict(col_arg=None)):
        assert bwd(lib, **kw) == -1, kw
        assert b"required with max_violation" in lib.itr_last_error(), kw


def test_python_entry_points_and_config_key():
    from itr_amd import config, ops
    from itr_amd.modalmodule import Models, Objectives
    assert config.DEFAULTS['mask_same_image'] is False
    assert 'mask_same_image' not in config.load_hyperparams            # a training switch, not a property of the weights
    assert config.build_config(['with', 'SCAN'])['mask_same_image'] is False
    assert config.build_config(['with', 'SCAN', 'mask_same_image=True'])['mask_same_image'] is True
    for fn in (ops.hinge_loss, ops.hinge_fwd, ops.hinge_bwd):
        assert inspect.signature(fn).parameters['groups'].default is None, fn
    assert list(inspect.signature(ops.hinge_loss).parameters) == ["scores", "margin", "max_violation", "groups"]
    assert list(inspect.signature(Objectives.ContrastiveLoss.forward).parameters) == ["self", "im", "s", "s_l", "groups"]
    assert list(inspect.signature(Objectives.TripletLoss.forward).parameters) == ["self", "scores", "groups"]
    assert inspect.signature(Objectives.ContrastiveLoss.forward).parameters['groups'].default is None
    assert callable(Models.base_module._hinge_groups)


class _Comm(object):
    def __init__(self, world=1, rank=0):
        self.world, self.rank, self.on = world, rank, world > 1


def test_groups_helper_of_the_models_on_the_host():
    """base_module._hinge_groups needs no device: None with the switch off (or absent: a config from an old checkpoint), ids //
    train_im_div in batch order in one process and in _dp_shard's rank-major strided order under data parallelism."""
    import numpy as np
    from itr_amd.modalmodule import Models
    m = Models.base_module({'mask_same_image': False})
    assert m._hinge_groups(list(range(7)), _Comm()) is None
    assert Models.base_module({})._hinge_groups(list(range(7)), _Comm()) is None
    m = Models.base_module({'mask_same_image': True})
    with pytest.raises(ValueError, match="train_im_div"):
        m._hinge_groups(list(range(7)), _Comm())
    m.train_im_div = 5
    ids = [12, 3, 40, 11, 4, 27, 13]
    assert m._hinge_groups(ids, _Comm()).tolist() == [2, 0, 8, 2, 0, 5, 2]
    for world in (2, 3):
        order = [i for q in range(world) for i in range(q, len(ids), world)]
        for rank in range(world):
            got = m._hinge_groups(np.asarray(ids), _Comm(world, rank))
            assert got.tolist() == [ids[i] // 5 for i in order], (world, rank)
