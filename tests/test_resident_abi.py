"""CPU: the device-side collate entry point exists in every layer (library, header, binding, ops, data module, config), the ABI
version is still 35 (the addition changes no existing signature), every declared symbol is exported and bound, and the entry
refuses bad arguments on the host before anything touches a device."""
import ctypes as C
import inspect
import os
import re

from itr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "itr_collate_batch"


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
    assert len(declared) == len(_lib.SIGNATURES[NAME][1]) == 29
    assert _lib.SIGNATURES[NAME][0] is C.c_int
    # the reference lines it replaces are cited with the declaration
    at = raw.index("int %s(" % NAME)
    comment = raw[raw.rindex("/*", 0, at):at]
    for cite in ("data_loader.py:134-178", "data_loader.py:104-131"):
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


def test_python_entry_points_and_config_key():
    from itr_amd import config, ops
    from itr_amd.datamodule import resident
    assert config.DEFAULTS['resident_data'] is False
    assert config.build_config(['with', 'SCAN'])['resident_data'] is False
    assert config.build_config(['with', 'SCAN', 'resident_data=True'])['resident_data'] is True
    assert callable(ops.collate_batch)
    params = inspect.signature(ops.collate_batch).parameters
    assert list(params)[:2] == ["feat", "img_idx"] and params["check"].default is False
    assert list(inspect.signature(resident.ResidentTrainSet.__init__).parameters) == ["self", "dataset", "device", "max_bytes"]
    assert list(inspect.signature(resident.ResidentLoader.__init__).parameters) == ["self", "resident_set", "batch_size", "shuffle", "seed"]


def call(lib, img_idx=16, cap_idx=16, B=8, feat=16, n_img=4, row_elems=288, images_out=16, boxes=None, box_elems=0, boxes_out=None,
         img_wh=None, wh_out=None, packed=None, n_packed=0, off=None, n_cap=4, Lmax=0, ids_out=None, tab0=None, tab1=None, tab2=None,
         ftab=None, W=0, out0=None, out1=None, out2=None, fout=None, bad=16):
    """16 = any non-null, 16-byte aligned value: every call below is refused (or ends) before any use"""
    return lib.itr_collate_batch(img_idx, cap_idx, B, feat, n_img, row_elems, images_out, boxes, box_elems, boxes_out, img_wh, wh_out, packed,
                                 n_packed, off, n_cap, Lmax, ids_out, tab0, tab1, tab2, ftab, W, out0, out1, out2, fout, bad, None)


def test_host_argument_checks():
    """no kernel is launched: every call is refused on its arguments, or has nothing to do"""
    lib = _lib.load()
    ragged = dict(packed=16, n_packed=100, off=16, Lmax=9, ids_out=16)
    # null pointers
    for kw in (dict(img_idx=None), dict(feat=None), dict(images_out=None), dict(bad=None),
               dict(boxes=16, box_elems=144), dict(boxes_out=16), dict(img_wh=16), dict(wh_out=16),
               dict(packed=16), dict(off=16), dict(ids_out=16), dict(ragged, packed=None), dict(ragged, off=None), dict(ragged, ids_out=None),
               dict(ragged, cap_idx=None), dict(tab0=16, W=32), dict(out0=16, W=32), dict(tab1=16, W=32), dict(out2=16, W=32),
               dict(ftab=16, W=32), dict(fout=16, W=32), dict(tab0=16, out0=16, W=32, cap_idx=None)):
        assert call(lib, **kw) == -1, kw
        assert b"null" in lib.itr_last_error(), kw
    # negative sizes
    for kw in (dict(B=-1), dict(n_img=0), dict(n_img=-3), dict(row_elems=-1), dict(boxes=16, boxes_out=16, box_elems=-1),
               dict(ragged, Lmax=-1), dict(ragged, n_packed=-1), dict(ragged, n_cap=0), dict(tab0=16, out0=16, W=-1),
               dict(tab0=16, out0=16, W=32, n_cap=-1)):
        assert call(lib, **kw) == -1, kw
        assert b"bad shape" in lib.itr_last_error(), kw
    # more work than one grid holds: refused with a message, not truncated
    assert call(lib, B=1 << 30) == -2
    assert b"workgroups" in lib.itr_last_error()
    assert call(lib, B=1, **dict(ragged, Lmax=1 << 36)) == -2
    assert call(lib, B=1, **dict(ragged, Lmax=1 << 50)) == -2
    assert call(lib, B=1, row_elems=1 << 45) == -2
    assert call(lib, B=1 << 14, tab0=16, out0=16, W=1 << 24) == -2
    # an empty batch is a success and launches nothing (the pointers above are not real)
    assert call(lib, B=0) == 0
    assert call(lib, B=0, **ragged) == 0
    # the caption index vector is not needed without a caption table
    assert call(lib, B=0, cap_idx=None) == 0
