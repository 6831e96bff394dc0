"""CPU: the cross-batch-memory entries exist in every layer -- library, header, binding, ops, membank, config -- the ABI version is
still 35, and every entry refuses bad arguments on the host before anything touches a device."""
import ctypes as C
import inspect
import os
import re

import pytest

from itr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"itr_xbm_workspace_bytes": 2, "itr_xbm_hinge_fwd": 18, "itr_xbm_hinge_bwd": 23, "itr_xbm_infonce_fwd": 17,
         "itr_xbm_infonce_bwd": 22, "itr_xbm_ring_write": 7}
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
    assert len(declared) == len(_lib.SIGNATURES[name][1]) == NAMES[name]
    assert _lib.SIGNATURES[name][0] is (C.c_size_t if name.endswith("_bytes") else C.c_int)


def test_abi_version_is_35_and_counts_agree():
    lib = _lib.load()
    raw, src = header_source()
    assert _lib.ABI_VERSION == 35 and lib.itr_abi_version() == 35
    assert int(re.search(r"#define\s+ITR_ABI_VERSION\s+(\d+)", raw).group(1)) == 35
    declared = sorted(set(re.findall(r"\b(itr_[a-z0-9_]+)\s*\(", src)))
    assert len([s for s in declared if hasattr(lib, s)]) == len(declared) == len(_lib.SIGNATURES)
    assert set(NAMES) <= set(declared)
    at = raw.index("size_t itr_xbm_workspace_bytes(")
    comment = raw[raw.rindex("/*", 0, at):at]
    for piece in ("Purely additive: no existing signature changes, ITR_ABI_VERSION stays 35", "group[i] == bank_group[k]",
                  "bank_group[k] == group[j]", "mask_batch && group[i] == group[j]", "no float atomics", "B (B + 2 n) >= 2^31",
                  "in slice order", "the earlier candidate"):
        assert piece in comment, piece


def test_workspace_bytes_on_the_host():
    lib = _lib.load()
    assert lib.itr_xbm_workspace_bytes(0, 5) == 0 and lib.itr_xbm_workspace_bytes(4, -1) == 0
    small, train, big = (lib.itr_xbm_workspace_bytes(B, n) for B, n in ((1, 0), (128, 4096), (128, 16384)))
    assert small == 12                                    # one slice: one pair and one row cost
    assert train == big == (2 * 128 + 1) * 128 * 4        # 128 slices x 2 column groups = 256 workgroups: the slice count is capped
    assert lib.itr_xbm_workspace_bytes(1024, 8192) == (2 * 32 + 1) * 1024 * 4          # 16 column groups: ceil(512 / 16) slices


def hinge_fwd(lib, S=16, ldS=8, R=16, ldR=12, C=16, ldC=8, group=16, bank=16, B=8, n=12, loss=16, ra=16, ca=16, ws=16):
    """16 = any non-null value: every call below is refused before any use"""
    return lib.itr_xbm_hinge_fwd(S, ldS, R, ldR, C, ldC, group, bank, B, n, 1, 0.2, 1, loss, ra, ca, ws, None)


def hinge_bwd(lib, S=16, ldS=8, R=16, ldR=12, C=16, ldC=8, group=16, bank=16, B=8, n=12, ra=16, ca=16, grad=16, dS=16, lddS=8, dR=16,
              lddR=12, dC=16, lddC=8):
    return lib.itr_xbm_hinge_bwd(S, ldS, R, ldR, C, ldC, group, bank, B, n, 1, 0.2, 1, ra, ca, grad, dS, lddS, dR, lddR, dC, lddC, None)


def nce_fwd(lib, S=16, ldS=8, R=16, ldR=12, C=16, ldC=8, group=16, bank=16, B=8, n=12, scale=20.0, loss=16, rl=16, cl=16, ws=16):
    return lib.itr_xbm_infonce_fwd(S, ldS, R, ldR, C, ldC, group, bank, B, n, 1, scale, loss, rl, cl, ws, None)


def nce_bwd(lib, S=16, ldS=8, R=16, ldR=12, C=16, ldC=8, group=16, bank=16, B=8, n=12, scale=20.0, rl=16, cl=16, grad=16, dS=16,
            lddS=8, dR=16, lddR=12, dC=16, lddC=8):
    return lib.itr_xbm_infonce_bwd(S, ldS, R, ldR, C, ldC, group, bank, B, n, 1, scale, rl, cl, grad, dS, lddS, dR, lddR, dC, lddC, None)


SHARED_NULLS = [dict(S=None), dict(R=None), dict(C=None), dict(group=None), dict(bank=None)]
SHARED_SHAPES = [dict(B=0), dict(B=-3), dict(n=-1), dict(ldS=7), dict(ldR=11), dict(ldC=7)]
TOO_LARGE = [dict(B=1 << 16, n=1 << 15, ldS=1 << 16, ldR=1 << 15, ldC=1 << 16), dict(B=2, n=1 << 29, ldR=1 << 29)]


@pytest.mark.parametrize("call,name,nulls,shapes", [
    (hinge_fwd, b"itr_xbm_hinge_fwd", [dict(loss=None), dict(ra=None), dict(ca=None), dict(ws=None)], []),
    (hinge_bwd, b"itr_xbm_hinge_bwd", [dict(ra=None), dict(ca=None), dict(grad=None), dict(dS=None), dict(dR=None), dict(dC=None)],
     [dict(lddS=7), dict(lddR=11), dict(lddC=7)]),
    (nce_fwd, b"itr_xbm_infonce_fwd", [dict(loss=None), dict(rl=None), dict(cl=None), dict(ws=None)], []),
    (nce_bwd, b"itr_xbm_infonce_bwd", [dict(rl=None), dict(cl=None), dict(grad=None), dict(dS=None), dict(dR=None), dict(dC=None)],
     [dict(lddS=7), dict(lddR=11), dict(lddC=7)]),
], ids=["hinge_fwd", "hinge_bwd", "infonce_fwd", "infonce_bwd"])
def test_host_argument_checks(call, name, nulls, shapes):
    """no kernel is launched: every call is refused on its arguments"""
    lib = _lib.load()
    for kw in SHARED_NULLS + nulls:
        assert call(lib, **kw) == -1, kw
        assert name + b": null pointer" in lib.itr_last_error(), kw
    for kw in SHARED_SHAPES + shapes:
        assert call(lib, **kw) == -1, kw
        assert name + b": bad shape" in lib.itr_last_error(), kw
    for kw in TOO_LARGE:
        if "lddS" in inspect.signature(call).parameters:
            kw = dict(kw, lddS=kw.get("ldS", 8), lddR=kw["ldR"], lddC=kw.get("ldC", 8))
        assert call(lib, **kw) == -1, kw
        assert name + b": too large" in lib.itr_last_error(), kw
    if b"infonce" in name:
        for scale in (0.0, -20.0, INF, NAN):
            assert call(lib, scale=scale) == -1, scale
            assert name + b": scale" in lib.itr_last_error(), scale


def test_ring_write_checks():
    lib = _lib.load()
    ring = lambda src=16, table=16, M=10, width=4, head=0, count=4: lib.itr_xbm_ring_write(src, table, M, width, head, count, None)
    for kw in (dict(M=0), dict(width=0), dict(head=-1), dict(head=10), dict(count=-1), dict(count=11)):
        assert ring(**kw) == -1, kw
        assert b"itr_xbm_ring_write: bad shape" in lib.itr_last_error(), kw
    for kw in (dict(src=None), dict(table=None)):
        assert ring(**kw) == -1, kw
        assert b"itr_xbm_ring_write: null pointer" in lib.itr_last_error(), kw
    assert ring(count=0, src=None) == 0          # nothing to write


def test_config_keys_and_refusals():
    from itr_amd import config
    from itr_amd.modalmodule import Models
    assert config.DEFAULTS['memory_bank'] == 0 and config.DEFAULTS['memory_start'] == 0
    assert 'memory_bank' not in config.load_hyperparams and 'memory_start' not in config.load_hyperparams      # training switches
    cfg = config.build_config(['with', 'VSE_PP', 'memory_bank=4096', 'memory_start=100'])
    assert cfg['memory_bank'] == 4096 and cfg['memory_start'] == 100
    assert Models.base_module({}).memory is None                       # a configuration from an old checkpoint: no memory
    for bad in (dict(memory_bank=-1), dict(memory_start=-2), dict(memory_bank=1.5), dict(memory_bank=True)):
        with pytest.raises(ValueError, match="non-negative integer"):
            Models.base_module(bad)
    with pytest.raises(ValueError, match="has no cross-batch memory"):
        Models.base_module(dict(memory_bank=64))                       # the families that have one say so: xbm_supported
    assert [c.__name__ for c in (Models.VSE_PP, Models.VSRN, Models.SAEM, Models.SCAN, Models.SGRAF, Models.CAMERA) if c.xbm_supported] \
        == ['VSE_PP', 'VSRN', 'SAEM']

    class Pooled(Models.base_module):
        xbm_supported = True
    with pytest.raises(ValueError, match="smaller than batch_size"):
        Pooled(dict(memory_bank=64, batch_size=128))
    assert Pooled(dict(memory_bank=128, batch_size=128)).memory is None


def test_python_entry_points():
    from itr_amd import membank, ops
    from itr_amd.modalmodule import Models
    assert list(inspect.signature(ops.xbm_hinge_loss).parameters) == ["S", "R", "C", "groups", "bank_groups", "margin", "max_violation", "mask_batch"]
    assert list(inspect.signature(ops.xbm_infonce_loss).parameters) == ["S", "R", "C", "groups", "bank_groups", "temperature", "mask_batch"]
    assert inspect.signature(ops.xbm_hinge_loss).parameters['mask_batch'].default is False
    assert list(inspect.signature(membank.MemoryBank.__init__).parameters) == ["self", "capacity", "device"]
    assert all(callable(getattr(membank.MemoryBank, m)) for m in ("push", "view", "reset"))
    assert list(inspect.signature(Models.base_module._hinge_memory).parameters)[:6] == ["self", "img", "cap", "scores", "ids", "pair_fn"]
    with pytest.raises(ValueError, match="capacity"):
        membank.MemoryBank(0, "cpu")
