"""CPU: the score-distillation loss exists in every layer -- library, header, binding, ops, model -- the ABI version is still 35, every
declared symbol is exported and bound, and both entries refuse bad arguments on the host before anything touches a device."""
import ctypes as C
import inspect
import os
import re

import pytest

from itr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"itr_distill_fwd": 14, "itr_distill_bwd": 15, "itr_distill_workspace_bytes": 1}
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
        assert "const float *S" in declared[0] and "const float *T" in declared[1] and "int B" in declared[2]
        assert "int64_t ldS" in declared[3] and "int64_t ldT" in declared[4]
        assert "float scale_s" in declared[5] and "float scale_t" in declared[6] and "itr_stream_t" in declared[-1]
        assert _lib.SIGNATURES[name][1][5] is C.c_float and _lib.SIGNATURES[name][1][6] is C.c_float


def test_header_comment():
    raw, _ = header_source()
    at = raw.index("size_t itr_distill_workspace_bytes(")
    comment = raw[raw.rindex("/*", 0, at):at]
    assert "next to ContrastiveLoss.forward (Objectives.py:93-115) and replaces no reference line" in comment
    assert "Purely additive: no existing signature changes, ITR_ABI_VERSION stays 35" in comment
    for piece in ("p_row[i,:] = softmax_j z_t[i,:]", "q_row[i,:] = softmax_j z_s[i,:]", "p_col[:,j] = softmax_i z_t[:,j]",
                  "q_col[:,j] = softmax_i z_s[:,j]", "KL_row[i] = sum_j p_row[i,j] (z_t[i,j] - z_s[i,j]) - lse_t_row[i] + lse_s_row[i]",
                  "KL_col[j] = sum_i p_col[i,j] (z_t[i,j] - z_s[i,j]) - lse_t_col[j] + lse_s_col[j]",
                  "loss = ( sum_i KL_row[i] + sum_j KL_col[j] ) / (2 B)",
                  "dS[i,j] = g scale_s / (2 B) ( (q_row - p_row)[i,j] + (q_col - p_col)[i,j] )", "no group mask", "soft positives",
                  "scale_s = float32(1 / distill_temperature)", "scale_t = float32(1 / distill_teacher_temperature)", "bit-zero",
                  "B = 1 gives loss 0 and dS 0", "no float atomics", "ldS, ldT and lddS may exceed B"):
        assert piece in comment, piece


def test_kernel_file():
    src = open(os.path.join(ROOT, "image-text-retrieval_amd", "csrc", "distill.hip")).read()
    assert "#pragma clang fp contract(off)" in src                     # z = scale * X is one rounded product, like infonce.hip
    assert "atomic" not in src.split("#include", 1)[1]
    head = src.split("#include", 1)[0]
    assert "NO group mask" in head and "soft positives" in head
    for other in ("infonce.hip", "hinge.hip", "xbm_loss.hip"):          # its own file: it shares no code with the other losses
        assert '#include "%s"' % other not in src


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
    assert lib.itr_distill_workspace_bytes(0) == 0 and lib.itr_distill_workspace_bytes(-4) == 0
    sizes = [lib.itr_distill_workspace_bytes(B) for B in (1, 64, 65, 128, 1024, 1025, 100000)]
    assert all(s > 0 and s % 4 == 0 for s in sizes) and sizes == sorted(sizes)
    # five floats per column and row slice, and one KL term per row; the slices stop growing, so the scratch stays linear in B
    assert sizes[0] == 4 * (5 + 1) and sizes[-1] <= 4 * (5 * 16 + 1) * 100000
    big = [lib.itr_distill_workspace_bytes(B) for B in (2048, 4096, 8192)]
    assert big[1] == 2 * big[0] and big[2] == 2 * big[1]


def fwd(lib, S=16, T=16, B=8, ldS=8, ldT=8, scale_s=20.0, scale_t=20.0, loss=16, rls=16, cls=16, rlt=16, clt=16, ws=16):
    """16 = any non-null value: every call below is refused before any use"""
    return lib.itr_distill_fwd(S, T, B, ldS, ldT, scale_s, scale_t, loss, rls, cls, rlt, clt, ws, None)


def bwd(lib, S=16, T=16, B=8, ldS=8, ldT=8, scale_s=20.0, scale_t=20.0, rls=16, cls=16, rlt=16, clt=16, grad=16, dS=16, lddS=8):
    return lib.itr_distill_bwd(S, T, B, ldS, ldT, scale_s, scale_t, rls, cls, rlt, clt, grad, dS, lddS, None)


def test_host_argument_checks():
    """no kernel is launched: every call is refused on its arguments"""
    lib = _lib.load()
    for name in ("S", "T", "loss", "rls", "cls", "rlt", "clt", "ws"):
        assert fwd(lib, **{name: None}) == -1, name
        assert b"itr_distill_fwd: null pointer" in lib.itr_last_error(), name
    for kw in (dict(B=0), dict(B=-3), dict(ldS=7), dict(ldT=7)):
        assert fwd(lib, **kw) == -1, kw
        assert b"itr_distill_fwd: bad shape" in lib.itr_last_error(), kw
    for which in ("scale_s", "scale_t"):
        for bad in (0.0, -20.0, INF, -INF, NAN):
            assert fwd(lib, **{which: bad}) == -1, (which, bad)
            assert b"itr_distill_fwd: scale" in lib.itr_last_error(), (which, bad)
    for name in ("S", "T", "rls", "cls", "rlt", "clt", "grad", "dS"):
        assert bwd(lib, **{name: None}) == -1, name
        assert b"itr_distill_bwd: null pointer" in lib.itr_last_error(), name
    for kw in (dict(B=0), dict(B=-3), dict(ldS=7), dict(ldT=7), dict(lddS=7)):
        assert bwd(lib, **kw) == -1, kw
        assert b"itr_distill_bwd: bad shape" in lib.itr_last_error(), kw
    for which in ("scale_s", "scale_t"):
        for bad in (0.0, -20.0, INF, -INF, NAN):
            assert bwd(lib, **{which: bad}) == -1, (which, bad)
            assert b"itr_distill_bwd: scale" in lib.itr_last_error(), (which, bad)


def test_python_entry_points():
    from itr_amd import ops
    from itr_amd.modalmodule import Models
    sig = inspect.signature(ops.distill_loss)
    assert list(sig.parameters) == ["scores", "teacher_scores", "temperature", "teacher_temperature"]
    assert sig.parameters['temperature'].default == 0.05 and sig.parameters['teacher_temperature'].default == 0.05
    assert callable(ops.distill_fwd) and callable(ops.distill_bwd)
    assert callable(Models.base_module.attach_distill_teacher) and callable(Models.base_module._distill)
