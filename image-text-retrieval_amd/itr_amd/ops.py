"""Thin torch-tensor front end of the C ABI (include/itr_hip.h).

torch is plumbing here: it owns device memory and the current HIP stream; every op below hands
raw device pointers + sizes to libitr_hip.so.  CPU tensors are rejected -- there is no fallback.
"""
import ctypes as C
import weakref

import numpy as np
import torch

from . import _lib
from .settings import SETTINGS

SCAN_NT = 64
SCAN_R = 36            # regions per image the fused SCAN / SGRAF kernels are built for (csrc/scan_common.h SC_R)
_NORMS = {'clipped_l2norm': 0, 'l2norm': 1, 'softmax': 2, 'no_norm': 3, 'clipped': 4, 'l1norm': 5,
          'clipped_l1norm': 6}
_AGGS = {'LogSumExp': 0, 'Max': 1, 'Sum': 2, 'Mean': 3}
_ACTS = {None: 0, 'none': 0, 'relu': 1, 'tanh': 2, 'sigmoid': 3, 'gelu': 4, 'leaky_relu': 5, 'nan_to_zero': 6}


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(t, dtype=torch.float32, name="tensor"):
    if not torch.is_tensor(t):
        raise TypeError("%s must be a torch tensor" % name)
    if not t.is_cuda:
        raise RuntimeError("%s is on %s: the itr_amd ops only run on the GPU (no CPU fallback)" % (name, t.device))
    if t.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    return t.contiguous()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def h2d(arr, device, dtype=None):
    """Small host array -> device tensor through PINNED staging with a non-blocking copy.  A copy from pageable memory
    (torch.as_tensor(list, device=...), .to(device) of a numpy view) is synchronous: the host stops until the stream
    has drained, which put the whole training step in lock-step with the GPU (1.8 ms per call measured)."""
    t = torch.as_tensor(np.ascontiguousarray(arr)) if not torch.is_tensor(arr) else arr
    if dtype is not None and t.dtype != dtype:
        t = t.to(dtype)
    if torch.device(device).type != 'cuda':
        return t.to(device)
    return t.pin_memory().to(device, non_blocking=True)


def _host_i32(a):
    arr = np.ascontiguousarray(np.asarray([int(x) for x in a] if not isinstance(a, np.ndarray) else a, dtype=np.int32))
    return arr


# ------------------------------------------------------------------------------------------
def l2norm(x, dim=-1, eps=1e-8):
    """utils.l2norm (eps after the sqrt).  Any `dim`: the tensor is viewed with `dim` last."""
    return _norm(x, dim, eps, 0)


def l1norm(x, dim=-1, eps=1e-8):
    return _norm(x, dim, eps, 1)


def normalize(x, dim=-1, eps=1e-12):
    """F.normalize(p=2) semantics: x / max(||x||, eps)."""
    return _norm(x, dim, eps, 2)


def _norm(x, dim, eps, kind, take_abs=False):
    lib = _lib.load()
    x = _dev(x, name="x")
    dim = dim % x.dim()
    moved = dim != x.dim() - 1
    xs = x.movedim(dim, -1).contiguous() if moved else x
    y = torch.empty_like(xs)
    rows = xs.numel() // xs.shape[-1] if xs.numel() else 0
    _lib.check(lib.itr_l2norm_rows(_p(xs), _p(y), rows, xs.shape[-1], eps, kind, int(take_abs), _stream()))
    return y.movedim(-1, dim).contiguous() if moved else y


def mean_mid(x):
    """torch.mean(x, 1) for x (B, R, F)."""
    lib = _lib.load()
    x = _dev(x, name="x")
    B, R, F_ = x.shape
    y = torch.empty(B, F_, device=x.device, dtype=torch.float32)
    for b0 in range(0, B, 65535):
        b1 = min(B, b0 + 65535)
        _lib.check(lib.itr_mean_mid(_p(x[b0:b1]), _p(y[b0:b1]), b1 - b0, R, F_, _stream()))
    return y


# STUDY switches (STUDY_SPLIT_PRECISION.md): True routes the plain tower / score GEMMs (linear, linear_strided, cosine_scores) through the
# split-bf16 kernel (terms = 3, ~1e-6 of fp32) / its fp16-plane variant.  Set by the study tools and their tests in their own
# process, never from the environment: the product GEMM is exact fp32.
BF16X3 = False
FP16X3 = False


def _weight_planes(w):
    """hi / lo planes of a weight tensor.  Not cached: call sites hand over detached views and temporaries whose address
    and version counter do not identify their contents (a cached plane of a recycled temporary gave wrong CAMERA scores);
    splitting costs one read + one write of the weight, ~1 % of the GEMM it feeds."""
    return split_bf16(w)


GEMM_ALGOS = {None: 0, "auto": 0, "tile": 1, "stream_plain": 2, "stream_xcd": 3, "skinny": 4}


def linear(x, weight, bias=None, act=None, algo=None):
    """act(x @ weight^T + bias) on the fp32 MFMA GEMM.  x (..., K), weight (N, K).  algo: None = the library's own choice;
    "tile" / "stream_plain" / "stream_xcd" force a kernel (itr_gemm_nt_algo: cross-checks, bit-identical results)."""
    lib = _lib.load()
    x = _dev(x, name="x")
    weight = _dev(weight, name="weight")
    K = x.shape[-1]
    if weight.shape[1] != K:
        raise ValueError("linear: x (..., %d) vs weight %s" % (K, tuple(weight.shape)))
    M = x.numel() // K if K else 0
    N = weight.shape[0]
    b = _dev(bias, name="bias") if bias is not None else None
    out = torch.empty(x.shape[:-1] + (N,), device=x.device, dtype=torch.float32)
    if FP16X3 and M and N and K % 32 == 0:
        gemm_nt_f16x3(split_f16(x.reshape(M, K)), split_f16(weight), b, act, out=out.view(M, N))
        return out
    if BF16X3 and M and N and K % 32 == 0:
        gemm_nt_bf16(split_bf16(x.reshape(M, K)), _weight_planes(weight), b, 3, act, out=out.view(M, N))
        return out
    if algo is not None:
        _lib.check(lib.itr_gemm_nt_algo(_p(x), K, _p(weight), K, _p(b), _p(out), N, M, N, K, _ACTS[act], GEMM_ALGOS[algo], _stream()))
        return out
    _lib.check(lib.itr_gemm_nt(_p(x), K, _p(weight), K, _p(b), _p(out), N, M, N, K, _ACTS[act], _stream()))
    return out


def linear_strided(base, lda, M, K, weight, bias=None, act=None, out=None):
    """act(A @ weight^T + bias) where row m of A starts at base.data_ptr() + m*lda floats and is K long (rows may
    overlap: SAEM's Conv2d(1, C, (k, 768)) over a token sequence is this GEMM with lda = 768, K = k*768)."""
    lib = _lib.load()
    base = _dev(base, name="base")
    weight = _dev(weight, name="weight")
    if weight.shape[1] != K:
        raise ValueError("linear_strided: K=%d vs weight %s" % (K, tuple(weight.shape)))
    if (M - 1) * lda + K > base.numel():
        raise ValueError("linear_strided: the last row reads past the end of the buffer")
    N = weight.shape[0]
    b = _dev(bias, name="bias") if bias is not None else None
    if out is None:
        out = torch.empty(M, N, device=base.device, dtype=torch.float32)
    if FP16X3 and M and N and K % 32 == 0 and lda % 32 == 0:
        return gemm_nt_f16x3(split_f16(base), split_f16(weight), b, act, M=M, K=K, lda=lda, out=out)
    if BF16X3 and M and N and K % 32 == 0 and lda % 32 == 0:
        return gemm_nt_bf16(split_bf16(base), _weight_planes(weight), b, 3, act, M=M, K=K, lda=lda, out=out)
    _lib.check(lib.itr_gemm_nt(_p(base), lda, _p(weight), K, _p(b), _p(out), out.stride(0), M, N, K, _ACTS[act], _stream()))
    return out


def proj_l2norm(images, weight, bias, no_imgnorm=False, use_abs=False):
    """EncoderImagePrecomp.forward (ImgEncoder.py:133-147)."""
    lib = _lib.load()
    images = _dev(images, name="images")
    weight = _dev(weight, name="fc.weight")
    bias = _dev(bias, name="fc.bias")
    F_, D = images.shape[-1], weight.shape[0]
    if weight.shape[1] != F_:
        raise ValueError("proj_l2norm: feature dim %d vs fc.weight %s" % (F_, tuple(weight.shape)))
    rows = images.numel() // F_
    out = torch.empty(images.shape[:-1] + (D,), device=images.device, dtype=torch.float32)
    _lib.check(lib.itr_proj_l2norm(_p(images), _p(weight), _p(bias), _p(out), rows, F_, D, int(no_imgnorm),
                                   int(use_abs), _stream()))
    return out


def _score_out(out, Ni, Nc, dev, name):
    """The (Ni, Nc) result buffer of a score op: a fresh tensor, or the caller's -- possibly a column block of a wider score
    matrix (row stride > Nc; the sharded evaluation scores caption ranges into their columns, evalpipe.py)."""
    if out is None:
        return torch.empty(Ni, Nc, device=dev, dtype=torch.float32)
    if not (out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (Ni, Nc) and (Nc <= 1 or out.stride(1) == 1)):
        raise ValueError("%s: out must be a (%d, %d) fp32 CUDA view with contiguous rows" % (name, Ni, Nc))
    return out


def cosine_scores(im, s, out=None):
    """cosine_sim (Objectives.py:18-21): im @ s^T."""
    lib = _lib.load()
    im = _dev(im, name="im")
    s = _dev(s, name="s")
    if im.dim() != 2 or s.dim() != 2 or im.shape[1] != s.shape[1]:
        raise ValueError("cosine_scores: expected (Ni, D) and (Nc, D), got %s and %s" % (tuple(im.shape), tuple(s.shape)))
    if FP16X3 and im.shape[0] and s.shape[0] and im.shape[1] % 32 == 0:
        return gemm_nt_f16x3(split_f16(im), split_f16(s), None, out=out)
    if BF16X3 and im.shape[0] and s.shape[0] and im.shape[1] % 32 == 0:
        return gemm_nt_bf16(split_bf16(im), split_bf16(s), None, 3, out=out)
    S = _score_out(out, im.shape[0], s.shape[0], im.device, "cosine_scores")
    _lib.check(lib.itr_cosine_scores(_p(im), _p(s), _p(S), im.shape[0], s.shape[0], im.shape[1], S.stride(0) if S.shape[0] > 1 else max(S.shape[1], S.stride(0)), _stream()))
    return S


def pdist_cos(x1, x2, out=None):
    """Objectives.pdist_cos (:310-323): rows / ||row|| (no eps), mm, NaN -> 0."""
    lib = _lib.load()
    a = _norm(x1, -1, 0.0, 3)
    b = _norm(x2, -1, 0.0, 3)
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[1]:
        raise ValueError("pdist_cos: expected (Ni, D) and (Nc, D), got %s and %s" % (tuple(a.shape), tuple(b.shape)))
    if FP16X3 or BF16X3:      # study routing: the split-precision GEMMs have no NaN epilogue
        return torch.nan_to_num_(cosine_scores(a, b, out=out), nan=0.0, posinf=float('inf'), neginf=float('-inf'))
    # `res[res != res] = 0` (:321) rides in the GEMM's epilogue (activation code 6): no second pass over the matrix
    S = _score_out(out, a.shape[0], b.shape[0], a.device, "pdist_cos")
    ldS = S.stride(0) if S.shape[0] > 1 else max(S.shape[1], S.stride(0))
    _lib.check(lib.itr_gemm_nt(_p(a), a.shape[1], _p(b), a.shape[1], _p(None), _p(S), ldS, a.shape[0], b.shape[0], a.shape[1], _ACTS['nan_to_zero'],
                               _stream()))
    return S


def split_bf16(x):
    """fp32 [..., K] -> split-bf16 operand [rows, 2 K] (int16 storage): per row and 32-wide chunk 32 hi values then 32 lo values,
    x = hi + lo + O(2^-17 |x|).  K must be a multiple of 32."""
    lib = _lib.load()
    x = _dev(x, name="x")
    K = x.shape[-1]
    rows = x.numel() // K if K else 0
    out = torch.empty(rows, 2 * K, device=x.device, dtype=torch.int16)
    _lib.check(lib.itr_split_bf16(_p(x), _p(out), rows, K, _stream()))
    return out


def gemm_nt_bf16(a_il, b_il, bias=None, terms=3, act=None, M=None, K=None, lda=None, out=None):
    """STUDY / opt-in (STUDY_SPLIT_PRECISION.md): A B^T on the bf16 matrix core from split operands (split_bf16), fp32 accumulation.
    terms = 3: hi.hi + hi.lo + lo.hi; terms = 1: hi.hi.  The product GEMM (linear / cosine_scores) is exact fp32.
    M, K, lda (fp32 elements) describe strided / overlapping rows of a flat operand (linear_strided)."""
    lib = _lib.load()
    if b_il.dim() != 2 or (M is None and (a_il.dim() != 2 or a_il.shape[1] != b_il.shape[1])) or (K is not None and 2 * K != b_il.shape[1]):
        raise ValueError("gemm_nt_bf16: A %s vs B %s" % (tuple(a_il.shape), tuple(b_il.shape)))
    if M is None:
        M, K, lda = a_il.shape[0], a_il.shape[1] // 2, a_il.shape[1] // 2
    N = b_il.shape[0]
    b = _dev(bias, name="bias") if bias is not None else None
    if out is None:
        out = torch.empty(M, N, device=a_il.device, dtype=torch.float32)
    _lib.check(lib.itr_gemm_nt_bf16(_p(a_il), 2 * lda, _p(b_il), b_il.shape[1], _p(b), _p(out), out.stride(0), M, N, K,
                                    _ACTS[act], int(terms), _stream()))
    return out


def split_f16(x):
    """fp32 [..., K] -> (fp16x3 operand [rows, 2 K] int16, scale_state [2] float32 on the device): per row and 32-wide chunk 32 hi then
    32 scaled-lo fp16 values of x * s, s = the power of two that puts the tensor's absmax in [2^14, 2^15)."""
    lib = _lib.load()
    x = _dev(x, name="x")
    K = x.shape[-1]
    rows = x.numel() // K if K else 0
    out = torch.empty(rows, 2 * K, device=x.device, dtype=torch.int16)
    state = torch.empty(2, device=x.device, dtype=torch.float32)
    _lib.check(lib.itr_split_f16(_p(x), _p(out), _p(state), rows, K, _stream()))
    return out, state


def gemm_nt_f16x3(a, b, bias=None, act=None, M=None, K=None, lda=None, out=None):
    """STUDY / opt-in (STUDY_SPLIT_PRECISION.md): A B^T from split_f16 operands on the fp16 matrix core, fp32 accumulation, error at the fp32
    rounding level.  M, K, lda (fp32 elements) describe strided / overlapping rows of a flat operand (linear_strided)."""
    lib = _lib.load()
    (a_il, sa), (b_il, sb) = a, b
    if b_il.dim() != 2 or (M is None and (a_il.dim() != 2 or a_il.shape[1] != b_il.shape[1])) or (K is not None and 2 * K != b_il.shape[1]):
        raise ValueError("gemm_nt_f16x3: A %s vs B %s" % (tuple(a_il.shape), tuple(b_il.shape)))
    if M is None:
        M, K, lda = a_il.shape[0], a_il.shape[1] // 2, a_il.shape[1] // 2
    N = b_il.shape[0]
    bb = _dev(bias, name="bias") if bias is not None else None
    if out is None:
        out = torch.empty(M, N, device=a_il.device, dtype=torch.float32)
    _lib.check(lib.itr_gemm_nt_f16x3(_p(a_il), 2 * lda, _p(sa), _p(b_il), b_il.shape[1], _p(sb), _p(bb), _p(out), out.stride(0), M, N, K,
                                     _ACTS[act], _stream()))
    return out


def order_scores(im, s, out=None):
    """order_sim (Objectives.py:24-30): -sqrt(sum_d max(0, s - im)^2) for every (image, sentence) pair."""
    lib = _lib.load()
    im, s = _dev(im, name="im"), _dev(s, name="s")
    if im.dim() != 2 or s.dim() != 2 or im.shape[1] != s.shape[1]:
        raise ValueError("order_scores: im %s vs s %s" % (tuple(im.shape), tuple(s.shape)))
    res = torch.empty(im.shape[0], s.shape[0], device=im.device, dtype=torch.float32)
    _lib.check(lib.itr_order_scores(_p(im), _p(s), _p(res), im.shape[0], s.shape[0], im.shape[1], _stream()))
    if out is not None:          # (the order kernel writes dense rows: a column block of a wider matrix is filled by a copy)
        _score_out(out, im.shape[0], s.shape[0], im.device, "order_scores").copy_(res)
        return out
    return res


def pdist(x1, x2):
    """SAEM's euclidean `pdist` (Objectives.py:297-307): sqrt(|x1|^2 - 2 x1.x2 + |x2|^2 + 1e-4)."""
    lib = _lib.load()
    x1, x2 = _dev(x1, name="x1"), _dev(x2, name="x2")
    S = cosine_scores(x1, x2)
    n1 = torch.empty(x1.shape[0], device=x1.device, dtype=torch.float32)
    n2 = torch.empty(x2.shape[0], device=x1.device, dtype=torch.float32)
    _lib.check(lib.itr_row_sqnorm(_p(x1), _p(n1), x1.shape[0], x1.shape[1], _stream()))
    _lib.check(lib.itr_row_sqnorm(_p(x2), _p(n2), x2.shape[0], x2.shape[1], _stream()))
    _lib.check(lib.itr_pdist_finish(_p(S), _p(n1), _p(n2), S.shape[0], S.shape[1], _stream()))
    return S


def mvm_scores(imgs, caps, out=None):
    """MultiViewMatching.forward (Fusionmodule.py:674-692)."""
    lib = _lib.load()
    imgs = _dev(imgs, name="imgs")
    caps = _dev(caps, name="caps")
    if imgs.dim() != 3 or caps.dim() != 2 or imgs.shape[2] != caps.shape[1]:
        raise ValueError("mvm_scores: expected (Ni, k, D) and (Nc, D)")
    Ni, k, D = imgs.shape
    S = _score_out(out, Ni, caps.shape[0], imgs.device, "mvm_scores")
    _lib.check(lib.itr_mvm_scores(_p(imgs), _p(caps), _p(S), Ni, caps.shape[0], k, D, S.stride(0) if Ni > 1 else max(S.shape[1], S.stride(0)), _stream()))
    return S


# ------------------------------------------------------------------------------------------
def _hinge_groups(groups, B, device):
    """`groups` of the masked hinge -> int32 device tensor [B].  Host input (list, numpy, CPU tensor) is checked on the host and
    uploaded through pinned staging (one small copy); an integer device tensor is used where it lies (an int64 one is range-checked
    there, which reads one flag back)."""
    if torch.is_tensor(groups) and groups.is_cuda:
        if groups.dtype.is_floating_point or groups.dtype == torch.bool or groups.dtype.is_complex:
            raise TypeError("hinge loss: groups must be integers, got %s" % groups.dtype)
        if groups.dim() != 1 or groups.shape[0] != B:
            raise ValueError("hinge loss: groups must have length %d, got shape %s" % (B, tuple(groups.shape)))
        if groups.dtype != torch.int32:
            if groups.dtype.itemsize > 2 and bool(((groups < -2 ** 31) | (groups > 2 ** 31 - 1)).any()):
                raise ValueError("hinge loss: a group value does not fit int32")
            groups = groups.to(torch.int32)
        return groups.contiguous()
    arr = np.asarray(groups.numpy() if torch.is_tensor(groups) else groups)
    if arr.dtype.kind not in 'iu':
        raise TypeError("hinge loss: groups must be integers, got %s" % arr.dtype)
    if arr.ndim != 1 or arr.shape[0] != B:
        raise ValueError("hinge loss: groups must have length %d, got shape %s" % (B, arr.shape))
    if arr.size and (int(arr.min()) < -2 ** 31 or int(arr.max()) > 2 ** 31 - 1):
        raise ValueError("hinge loss: a group value does not fit int32")
    return h2d(arr.astype(np.int32), device)


def hinge_fwd(scores, margin, max_violation, groups=None):
    """-> (loss[1], row_arg, col_arg).  `groups` (length B, integers): entries (i, j), i != j, of one group are no negatives
    (itr_hinge_groups_fwd); None is the reference's loss, which masks the diagonal only."""
    lib = _lib.load()
    scores = _dev(scores, name="scores")
    if scores.dim() != 2 or scores.shape[0] != scores.shape[1]:
        raise ValueError("hinge loss needs a square score matrix, got %s" % (tuple(scores.shape),))
    B = scores.shape[0]
    if groups is not None:
        groups = _hinge_groups(groups, B, scores.device)
    loss = torch.empty(1, device=scores.device, dtype=torch.float32)
    row_arg = torch.empty(B, device=scores.device, dtype=torch.int32)
    col_arg = torch.empty(B, device=scores.device, dtype=torch.int32)
    ws = torch.empty(2 * B, device=scores.device, dtype=torch.float32)
    if groups is None:
        _lib.check(lib.itr_hinge_maxviol_fwd(_p(scores), B, B, float(margin), int(bool(max_violation)), _p(loss),
                                             _p(row_arg), _p(col_arg), _p(ws), _stream()))
    else:
        _lib.check(lib.itr_hinge_groups_fwd(_p(scores), _p(groups), B, B, float(margin), int(bool(max_violation)), _p(loss),
                                            _p(row_arg), _p(col_arg), _p(ws), _stream()))
    return loss, row_arg, col_arg


def hinge_bwd(scores, margin, max_violation, row_arg, col_arg, grad_loss, groups=None):
    lib = _lib.load()
    scores = _dev(scores, name="scores")
    B = scores.shape[0]
    g = _dev(grad_loss.reshape(1), name="grad_loss")
    dS = torch.empty_like(scores)
    if groups is None:
        _lib.check(lib.itr_hinge_maxviol_bwd(_p(scores), B, B, float(margin), int(bool(max_violation)), _p(row_arg),
                                             _p(col_arg), _p(g), _p(dS), B, _stream()))
    else:
        groups = _hinge_groups(groups, B, scores.device)
        _lib.check(lib.itr_hinge_groups_bwd(_p(scores), _p(groups), B, B, float(margin), int(bool(max_violation)), _p(row_arg),
                                            _p(col_arg), _p(g), _p(dS), B, _stream()))
    return dS


class _HingeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scores, margin, max_violation):
        scores = scores.contiguous()
        loss, ra, ca = hinge_fwd(scores, margin, max_violation)
        ctx.save_for_backward(scores, ra, ca)
        ctx.margin, ctx.mv = margin, max_violation
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad):
        scores, ra, ca = ctx.saved_tensors
        return hinge_bwd(scores, ctx.margin, ctx.mv, ra, ca, grad.contiguous()), None, None


class _HingeGroupsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scores, margin, max_violation, groups):
        scores = scores.contiguous()
        loss, ra, ca = hinge_fwd(scores, margin, max_violation, groups)
        ctx.save_for_backward(scores, ra, ca, groups)
        ctx.margin, ctx.mv = margin, max_violation
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad):
        scores, ra, ca, groups = ctx.saved_tensors
        return hinge_bwd(scores, ctx.margin, ctx.mv, ra, ca, grad.contiguous(), groups), None, None, None


def hinge_loss(scores, margin=0.2, max_violation=False, groups=None):
    """Differentiable (w.r.t. scores) bidirectional hinge loss, HIP forward and backward.  `groups` (length-B integer tensor, numpy
    array or list; no gradient): pairs of one group -- captions of the same image -- are not mined as negatives of each other."""
    if groups is None:
        return _HingeFn.apply(scores, margin, max_violation)
    if scores.dim() != 2 or scores.shape[0] != scores.shape[1]:
        raise ValueError("hinge loss needs a square score matrix, got %s" % (tuple(scores.shape),))
    return _HingeGroupsFn.apply(scores, margin, max_violation, _hinge_groups(groups, scores.shape[0], scores.device))


def _infonce_scale(temperature):
    """float32(1 / temperature), the factor the kernels multiply the scores by."""
    t = float(temperature)
    if not np.isfinite(t) or t <= 0.0:
        raise ValueError("InfoNCE loss: temperature must be finite and positive, got %r" % (temperature,))
    with np.errstate(over='ignore', under='ignore'):
        scale = float(np.float32(1.0 / t))
    if not np.isfinite(scale) or scale <= 0.0:
        raise ValueError("InfoNCE loss: 1 / temperature does not fit float32 for temperature %r" % (temperature,))
    return scale


def _infonce_scores(scores):
    scores = _dev(scores, name="scores")
    if scores.dim() != 2 or scores.shape[0] != scores.shape[1]:
        raise ValueError("InfoNCE loss needs a square score matrix, got %s" % (tuple(scores.shape),))
    return scores


def infonce_fwd(scores, temperature=0.05, groups=None):
    """-> (loss[1], row_lse[B], col_lse[B]) of the softmax contrastive loss on z = scores / temperature (itr_infonce_fwd): the mean over
    the B rows and the B columns of log-sum-exp minus the diagonal.  `groups` (length B, integers): entries (i, j), i != j, of one group
    are left out of both sums, the rule of hinge_fwd; None masks nothing."""
    lib = _lib.load()
    scores = _infonce_scores(scores)
    scale = _infonce_scale(temperature)
    B = scores.shape[0]
    if groups is not None:
        groups = _hinge_groups(groups, B, scores.device)
    loss = torch.empty(1, device=scores.device, dtype=torch.float32)
    row_lse = torch.empty(B, device=scores.device, dtype=torch.float32)
    col_lse = torch.empty(B, device=scores.device, dtype=torch.float32)
    ws = torch.empty(max(1, int(lib.itr_infonce_workspace_bytes(B))), device=scores.device, dtype=torch.uint8)
    _lib.check(lib.itr_infonce_fwd(_p(scores), _p(groups), B, B, scale, _p(loss), _p(row_lse), _p(col_lse), _p(ws), _stream()))
    return loss, row_lse, col_lse


def infonce_bwd(scores, temperature, row_lse, col_lse, grad_loss, groups=None):
    """dS of infonce_fwd from its saved log-sum-exps (itr_infonce_bwd); exactly 0 at masked entries."""
    lib = _lib.load()
    scores = _infonce_scores(scores)
    scale = _infonce_scale(temperature)
    B = scores.shape[0]
    if groups is not None:
        groups = _hinge_groups(groups, B, scores.device)
    g = _dev(grad_loss.reshape(1), name="grad_loss")
    row_lse, col_lse = _dev(row_lse, name="row_lse"), _dev(col_lse, name="col_lse")
    if row_lse.shape != (B,) or col_lse.shape != (B,):
        raise ValueError("InfoNCE loss: row_lse and col_lse must have length %d" % B)
    dS = torch.empty_like(scores)
    _lib.check(lib.itr_infonce_bwd(_p(scores), _p(groups), B, B, scale, _p(row_lse), _p(col_lse), _p(g), _p(dS), B, _stream()))
    return dS


class _InfoNCEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scores, temperature, groups):
        scores = scores.contiguous()
        loss, row_lse, col_lse = infonce_fwd(scores, temperature, groups)
        if groups is None:
            ctx.save_for_backward(scores, row_lse, col_lse)
        else:
            ctx.save_for_backward(scores, row_lse, col_lse, groups)
        ctx.temperature = temperature
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad):
        scores, row_lse, col_lse = ctx.saved_tensors[:3]
        groups = ctx.saved_tensors[3] if len(ctx.saved_tensors) > 3 else None
        return infonce_bwd(scores, ctx.temperature, row_lse, col_lse, grad.contiguous(), groups), None, None


def infonce_loss(scores, temperature=0.05, groups=None):
    """Differentiable (w.r.t. scores) InfoNCE loss, HIP forward and backward: image-to-text and text-to-image softmax cross-entropy on
    scores / temperature with the diagonal as the positive, averaged.  `groups` as in hinge_loss: pairs of one group -- captions of
    the same image -- are not each other's negatives."""
    scores = _infonce_scores(scores)
    _infonce_scale(temperature)
    if groups is not None:
        groups = _hinge_groups(groups, scores.shape[0], scores.device)
    return _InfoNCEFn.apply(scores, temperature, groups)


# ---- score distillation: a student's B x B matrix towards a teacher's ranking distribution over the batch (csrc/distill.hip)
def _distill_scale(temperature, which):
    """float32(1 / temperature) of the student's or the teacher's scores, checked like _infonce_scale."""
    t = float(temperature)
    if not np.isfinite(t) or t <= 0.0:
        raise ValueError("distillation loss: %s must be finite and positive, got %r" % (which, temperature))
    with np.errstate(over='ignore', under='ignore'):
        scale = float(np.float32(1.0 / t))
    if not np.isfinite(scale) or scale <= 0.0:
        raise ValueError("distillation loss: 1 / %s does not fit float32 for %s %r" % (which, which, temperature))
    return scale


def _distill_operands(scores, teacher_scores):
    """Checked (scores, teacher_scores): equal square shapes (refused before the device is asked for), fp32, contiguous, one device."""
    if torch.is_tensor(scores) and (scores.dim() != 2 or scores.shape[0] != scores.shape[1]):
        raise ValueError("distillation loss needs a square score matrix, got %s" % (tuple(scores.shape),))
    if torch.is_tensor(scores) and torch.is_tensor(teacher_scores) and teacher_scores.shape != scores.shape:
        raise ValueError("distillation loss: teacher scores %s do not match the student's %s" % (tuple(teacher_scores.shape), tuple(scores.shape)))
    scores, teacher_scores = _dev(scores, name="scores"), _dev(teacher_scores, name="teacher_scores")
    if teacher_scores.device != scores.device:
        raise ValueError("distillation loss: teacher scores on %s, student scores on %s" % (teacher_scores.device, scores.device))
    return scores, teacher_scores


def distill_fwd(scores, teacher_scores, temperature=0.05, teacher_temperature=0.05):
    """-> (loss[1], row_lse_s[B], col_lse_s[B], row_lse_t[B], col_lse_t[B]) of itr_distill_fwd: the mean over the B rows and the B columns
    of KL(softmax(teacher_scores / teacher_temperature) || softmax(scores / temperature)), and the log-sum-exps its backward reads."""
    lib = _lib.load()
    scores, teacher_scores = _distill_operands(scores, teacher_scores)
    scale_s = _distill_scale(temperature, "temperature")
    scale_t = _distill_scale(teacher_temperature, "teacher_temperature")
    B = scores.shape[0]
    loss = torch.empty(1, device=scores.device, dtype=torch.float32)
    lse = [torch.empty(B, device=scores.device, dtype=torch.float32) for _ in range(4)]
    ws = torch.empty(max(1, int(lib.itr_distill_workspace_bytes(B))), device=scores.device, dtype=torch.uint8)
    _lib.check(lib.itr_distill_fwd(_p(scores), _p(teacher_scores), B, B, B, scale_s, scale_t, _p(loss), _p(lse[0]), _p(lse[1]), _p(lse[2]),
                                   _p(lse[3]), _p(ws), _stream()))
    return (loss,) + tuple(lse)


def distill_bwd(scores, teacher_scores, temperature, teacher_temperature, row_lse_s, col_lse_s, row_lse_t, col_lse_t, grad_loss):
    """dS of distill_fwd from its four saved log-sum-exp vectors (itr_distill_bwd)."""
    lib = _lib.load()
    scores, teacher_scores = _distill_operands(scores, teacher_scores)
    scale_s = _distill_scale(temperature, "temperature")
    scale_t = _distill_scale(teacher_temperature, "teacher_temperature")
    B = scores.shape[0]
    g = _dev(grad_loss.reshape(1), name="grad_loss")
    lse = [_dev(v, name=n) for v, n in ((row_lse_s, "row_lse_s"), (col_lse_s, "col_lse_s"), (row_lse_t, "row_lse_t"), (col_lse_t, "col_lse_t"))]
    if any(v.shape != (B,) for v in lse):
        raise ValueError("distillation loss: the four log-sum-exp vectors must have length %d" % B)
    dS = torch.empty_like(scores)
    _lib.check(lib.itr_distill_bwd(_p(scores), _p(teacher_scores), B, B, B, scale_s, scale_t, _p(lse[0]), _p(lse[1]), _p(lse[2]), _p(lse[3]),
                                   _p(g), _p(dS), B, _stream()))
    return dS


class _DistillFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scores, teacher_scores, temperature, teacher_temperature):
        scores, teacher_scores = scores.contiguous(), teacher_scores.contiguous()
        out = distill_fwd(scores, teacher_scores, temperature, teacher_temperature)
        ctx.save_for_backward(scores, teacher_scores, *out[1:])
        ctx.temperature, ctx.teacher_temperature = temperature, teacher_temperature
        return out[0].reshape(())

    @staticmethod
    def backward(ctx, grad):
        scores, teacher_scores, rls, cls, rlt, clt = ctx.saved_tensors
        dS = distill_bwd(scores, teacher_scores, ctx.temperature, ctx.teacher_temperature, rls, cls, rlt, clt, grad.contiguous())
        return dS, None, None, None


def distill_loss(scores, teacher_scores, temperature=0.05, teacher_temperature=0.05):
    """Differentiable (w.r.t. scores) score-distillation loss, HIP forward and backward: the KL divergence from the teacher's softmax over
    teacher_scores / teacher_temperature to the student's over scores / temperature, along every row (image-to-text) and every column
    (text-to-image) of the batch, averaged.  There is no group mask: the teacher's scores say which other captions are positives.
    `teacher_scores` is a target, not a variable: one that requires grad is refused."""
    if torch.is_tensor(teacher_scores) and teacher_scores.requires_grad:
        raise ValueError("distillation loss: teacher_scores must not require grad (score the teacher under torch.no_grad(), or detach)")
    _distill_scale(temperature, "temperature")
    _distill_scale(teacher_temperature, "teacher_temperature")
    scores, teacher_scores = _distill_operands(scores, teacher_scores)
    return _DistillFn.apply(scores, teacher_scores, temperature, teacher_temperature)


# ---- cross-batch memory: both losses on batch u memory (csrc/xbm_loss.hip)
def _xbm_operands(who, S, R, C, groups, bank_groups):
    """Checked (S [B, B], R [B, n], C [n, B], groups int32 [B], bank_groups int32 [n]) on S's device."""
    S, R, C = _dev(S, name="S"), _dev(R, name="R"), _dev(C, name="C")
    if S.dim() != 2 or S.shape[0] != S.shape[1]:
        raise ValueError("%s needs a square score matrix, got %s" % (who, tuple(S.shape)))
    B = S.shape[0]
    if B < 1:
        raise ValueError("%s needs at least one pair, got S %s" % (who, tuple(S.shape)))
    if R.dim() != 2 or C.dim() != 2 or R.shape[0] != B or C.shape[1] != B or C.shape[0] != R.shape[1]:
        raise ValueError("%s needs R [%d, n] and C [n, %d], got R %s and C %s" % (who, B, B, tuple(R.shape), tuple(C.shape)))
    if R.device != S.device or C.device != S.device:
        raise ValueError("%s: S, R and C must lie on one device, got %s, %s, %s" % (who, S.device, R.device, C.device))
    n = R.shape[1]
    if B * (B + 2 * n) >= 2 ** 31:
        raise ValueError("%s: B (B + 2 n) must stay below 2^31, got B=%d n=%d" % (who, B, n))
    if groups is None or bank_groups is None:
        raise ValueError("%s needs the image of every pair (groups) and of every memory slot (bank_groups)" % who)
    return S, R, C, _hinge_groups(groups, B, S.device), _hinge_groups(bank_groups, n, S.device)


def xbm_hinge_fwd(S, R, C, groups, bank_groups, margin, max_violation, mask_batch=False):
    """-> (loss[1], row_arg[B], col_arg[B]) of the hinge on batch u memory (itr_xbm_hinge_fwd).  Max form: candidate indices in
    [0, B + n), < B in-batch, else memory slot arg - B.  Sum form: the violator counts of every row / column."""
    lib = _lib.load()
    S, R, C, groups, bank_groups = _xbm_operands("XBM hinge loss", S, R, C, groups, bank_groups)
    B, n = R.shape
    loss = torch.empty(1, device=S.device, dtype=torch.float32)
    row_arg = torch.empty(B, device=S.device, dtype=torch.int32)
    col_arg = torch.empty(B, device=S.device, dtype=torch.int32)
    ws = torch.empty(max(1, int(lib.itr_xbm_workspace_bytes(B, n))), device=S.device, dtype=torch.uint8)
    _lib.check(lib.itr_xbm_hinge_fwd(_p(S), B, _p(R), n, _p(C), B, _p(groups), _p(bank_groups), B, n, int(bool(mask_batch)),
                                     float(margin), int(bool(max_violation)), _p(loss), _p(row_arg), _p(col_arg), _p(ws), _stream()))
    return loss, row_arg, col_arg


def xbm_hinge_bwd(S, R, C, groups, bank_groups, margin, max_violation, row_arg, col_arg, grad_loss, mask_batch=False):
    """-> (dS, dR, dC) of xbm_hinge_fwd from its saved arg vectors (itr_xbm_hinge_bwd); bit-zero at dropped entries."""
    lib = _lib.load()
    S, R, C, groups, bank_groups = _xbm_operands("XBM hinge loss", S, R, C, groups, bank_groups)
    B, n = R.shape
    row_arg, col_arg = _dev(row_arg, torch.int32, "row_arg"), _dev(col_arg, torch.int32, "col_arg")
    if row_arg.shape != (B,) or col_arg.shape != (B,):
        raise ValueError("XBM hinge loss: row_arg and col_arg must have length %d" % B)
    g = _dev(grad_loss.reshape(1), name="grad_loss")
    dS, dR, dC = torch.empty_like(S), torch.empty_like(R), torch.empty_like(C)
    _lib.check(lib.itr_xbm_hinge_bwd(_p(S), B, _p(R), n, _p(C), B, _p(groups), _p(bank_groups), B, n, int(bool(mask_batch)),
                                     float(margin), int(bool(max_violation)), _p(row_arg), _p(col_arg), _p(g), _p(dS), B, _p(dR), n,
                                     _p(dC), B, _stream()))
    return dS, dR, dC


def xbm_infonce_fwd(S, R, C, groups, bank_groups, temperature=0.05, mask_batch=False):
    """-> (loss[1], row_lse[B], col_lse[B]) of the InfoNCE loss on batch u memory (itr_xbm_infonce_fwd)."""
    lib = _lib.load()
    S, R, C, groups, bank_groups = _xbm_operands("XBM InfoNCE loss", S, R, C, groups, bank_groups)
    scale = _infonce_scale(temperature)
    B, n = R.shape
    loss = torch.empty(1, device=S.device, dtype=torch.float32)
    row_lse = torch.empty(B, device=S.device, dtype=torch.float32)
    col_lse = torch.empty(B, device=S.device, dtype=torch.float32)
    ws = torch.empty(max(1, int(lib.itr_xbm_workspace_bytes(B, n))), device=S.device, dtype=torch.uint8)
    _lib.check(lib.itr_xbm_infonce_fwd(_p(S), B, _p(R), n, _p(C), B, _p(groups), _p(bank_groups), B, n, int(bool(mask_batch)), scale,
                                       _p(loss), _p(row_lse), _p(col_lse), _p(ws), _stream()))
    return loss, row_lse, col_lse


def xbm_infonce_bwd(S, R, C, groups, bank_groups, temperature, row_lse, col_lse, grad_loss, mask_batch=False):
    """-> (dS, dR, dC) of xbm_infonce_fwd from its saved log-sum-exps (itr_xbm_infonce_bwd); bit-zero at dropped entries."""
    lib = _lib.load()
    S, R, C, groups, bank_groups = _xbm_operands("XBM InfoNCE loss", S, R, C, groups, bank_groups)
    scale = _infonce_scale(temperature)
    B, n = R.shape
    row_lse, col_lse = _dev(row_lse, name="row_lse"), _dev(col_lse, name="col_lse")
    if row_lse.shape != (B,) or col_lse.shape != (B,):
        raise ValueError("XBM InfoNCE loss: row_lse and col_lse must have length %d" % B)
    g = _dev(grad_loss.reshape(1), name="grad_loss")
    dS, dR, dC = torch.empty_like(S), torch.empty_like(R), torch.empty_like(C)
    _lib.check(lib.itr_xbm_infonce_bwd(_p(S), B, _p(R), n, _p(C), B, _p(groups), _p(bank_groups), B, n, int(bool(mask_batch)), scale,
                                       _p(row_lse), _p(col_lse), _p(g), _p(dS), B, _p(dR), n, _p(dC), B, _stream()))
    return dS, dR, dC


class _XbmHingeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, S, R, C, groups, bank_groups, margin, max_violation, mask_batch):
        S, R, C = S.contiguous(), R.contiguous(), C.contiguous()
        loss, ra, ca = xbm_hinge_fwd(S, R, C, groups, bank_groups, margin, max_violation, mask_batch)
        ctx.save_for_backward(S, R, C, groups, bank_groups, ra, ca)
        ctx.margin, ctx.mv, ctx.mask_batch = margin, max_violation, mask_batch
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad):
        S, R, C, groups, bank_groups, ra, ca = ctx.saved_tensors
        dS, dR, dC = xbm_hinge_bwd(S, R, C, groups, bank_groups, ctx.margin, ctx.mv, ra, ca, grad.contiguous(), ctx.mask_batch)
        return (dS, dR, dC) + (None,) * 5


class _XbmInfoNCEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, S, R, C, groups, bank_groups, temperature, mask_batch):
        S, R, C = S.contiguous(), R.contiguous(), C.contiguous()
        loss, row_lse, col_lse = xbm_infonce_fwd(S, R, C, groups, bank_groups, temperature, mask_batch)
        ctx.save_for_backward(S, R, C, groups, bank_groups, row_lse, col_lse)
        ctx.temperature, ctx.mask_batch = temperature, mask_batch
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad):
        S, R, C, groups, bank_groups, row_lse, col_lse = ctx.saved_tensors
        dS, dR, dC = xbm_infonce_bwd(S, R, C, groups, bank_groups, ctx.temperature, row_lse, col_lse, grad.contiguous(), ctx.mask_batch)
        return (dS, dR, dC) + (None,) * 4


def xbm_hinge_loss(S, R, C, groups, bank_groups, margin, max_violation, mask_batch=False):
    """Differentiable (w.r.t. S, R and C) bidirectional hinge on batch u memory, HIP forward and backward.  S [B, B] is the step's
    matrix, R [B, n] scores the images against the memory's captions, C [n, B] the memory's images against the captions.  `groups`
    [B] / `bank_groups` [n] (as in hinge_loss) name the image of every pair / memory slot: a memory entry of the query's own image
    is never a negative; inside the batch the same rule holds with mask_batch=True.  With an empty memory (n = 0) this is hinge_loss
    on S, bit for bit."""
    S, R, C, groups, bank_groups = _xbm_operands("XBM hinge loss", S, R, C, groups, bank_groups)
    if R.shape[1] == 0:
        return hinge_loss(S, margin, max_violation, groups=groups if mask_batch else None)
    return _XbmHingeFn.apply(S, R, C, groups, bank_groups, margin, bool(max_violation), bool(mask_batch))


def xbm_infonce_loss(S, R, C, groups, bank_groups, temperature, mask_batch=False):
    """Differentiable (w.r.t. S, R and C) InfoNCE loss on batch u memory: every row's and every column's softmax also ranges over the
    memory's kept entries.  Operands and the two group vectors as in xbm_hinge_loss; n = 0 is infonce_loss on S, bit for bit."""
    S, R, C, groups, bank_groups = _xbm_operands("XBM InfoNCE loss", S, R, C, groups, bank_groups)
    _infonce_scale(temperature)
    if R.shape[1] == 0:
        return infonce_loss(S, temperature, groups=groups if mask_batch else None)
    return _XbmInfoNCEFn.apply(S, R, C, groups, bank_groups, temperature, bool(mask_batch))


def xbm_ring_write(src, table, head):
    """table[(head + r) % M] = src[r] for every row of `src` (itr_xbm_ring_write): one launch, across the wrap.  Both are contiguous
    device tensors of one 32-bit dtype with equal row shapes."""
    lib = _lib.load()
    if not (torch.is_tensor(src) and torch.is_tensor(table) and src.is_cuda and table.is_cuda):
        raise RuntimeError("xbm_ring_write: the itr_amd ops only run on the GPU (no CPU fallback)")
    if src.dtype != table.dtype or src.dtype.itemsize != 4:
        raise TypeError("xbm_ring_write: src and table must share one 32-bit dtype, got %s and %s" % (src.dtype, table.dtype))
    if src.dim() < 1 or src.shape[1:] != table.shape[1:] or src.shape[0] > table.shape[0] or not table.is_contiguous():
        raise ValueError("xbm_ring_write: src %s does not fit rows of table %s" % (tuple(src.shape), tuple(table.shape)))
    src = src.contiguous()
    M = table.shape[0]
    width = int(np.prod(table.shape[1:])) if table.dim() > 1 else 1
    _lib.check(lib.itr_xbm_ring_write(_p(src), _p(table), M, width, int(head), src.shape[0], _stream()))


# ------------------------------------------------------------------------------------------
class ScanPlan:
    """Column-tile plan of a caption set for the SCAN kernel (host-side, cheap, reusable).

    The fused kernel packs whole captions into 64-column tiles, so a caption of more than 64 words does not fit
    (Flickr30k has a few, up to 82 tokens).  Such captions are planned separately: the kernel scores the others and
    scan_xattn_scores fills their columns with the one-workgroup-per-pair forward of the training path
    (csrc/scan_train*.hip, up to 96 words).  `Nc` is always the full caption count."""

    def __init__(self, cap_off, cap_len, n_rows, device, max_kernel_len=None):
        lib = _lib.load()
        self.len_host = _host_i32(cap_len)
        self.off_host = np.asarray(cap_off, dtype=np.int64)
        self.Nc = len(self.len_host)
        self.n_rows = int(n_rows)
        self.device = device
        long_mask = self.len_host > (SCAN_NT if max_kernel_len is None else max_kernel_len)      # (SGRAF: 63 words + the global node)
        self.long_idx = np.nonzero(long_mask)[0] if long_mask.any() else None
        if self.long_idx is None:
            k_len, k_off = self.len_host, self.off_host
        else:
            self.short_idx = np.nonzero(~long_mask)[0]
            k_len, k_off = np.ascontiguousarray(self.len_host[self.short_idx]), self.off_host[self.short_idx]
        self.Nc_kernel = len(k_len)
        tb = np.zeros(self.Nc_kernel + 1, dtype=np.int32)
        order = np.zeros(max(self.Nc_kernel, 1), dtype=np.int32)
        nt = C.c_int64(0)
        _lib.check(lib.itr_scan_plan_tiles(k_len.ctypes.data_as(C.c_void_p), self.Nc_kernel, SCAN_NT,
                                           tb.ctypes.data_as(C.c_void_p), order.ctypes.data_as(C.c_void_p),
                                           C.byref(nt)))
        self.n_tiles = int(nt.value)
        self.tile_begin = h2d(tb[:self.n_tiles + 1].copy(), device)
        self.cap_order = h2d(order, device)
        self.cap_len = h2d(k_len.copy(), device)
        self.cap_off = h2d(np.asarray(k_off, dtype=np.int64), device)
        self._k_len = k_len
        self._node_groups = None

    def node_groups(self):
        """SGRAF-SGR's fused graph steps (csrc/sgr_fused.hip): groups of whole captions binned by NODE count (words + the global
        node), at most 64 node rows and 16 captions per group (itr_sgr_plan_node_groups, exact fill).
        -> (group_begin int32[n + 1], group_order int32[Nc_kernel], n) on the device, or None when a caption has more than 63
        words (its graph does not fit one workgroup)."""
        if self._node_groups is None:
            lib = _lib.load()
            if self.Nc_kernel == 0 or int(self._k_len.max()) + 1 > SCAN_NT:
                self._node_groups = False
            else:
                lens = np.ascontiguousarray(self._k_len.astype(np.int32))
                tb = np.zeros(self.Nc_kernel + 1, dtype=np.int32)
                order = np.zeros(self.Nc_kernel, dtype=np.int32)
                nt = C.c_int64(0)
                # SETTINGS.sgr_group_rows = 32 (cross-check): captions of <= 31 words in groups of <= 32 node rows, two workgroups per CU
                small = 32 if SETTINGS.sgr_group_rows == 32 else SCAN_NT
                _lib.check(lib.itr_sgr_plan_node_groups(lens.ctypes.data_as(C.c_void_p), self.Nc_kernel, small, tb.ctypes.data_as(C.c_void_p),
                                                        order.ctypes.data_as(C.c_void_p), C.byref(nt)))
                n = int(nt.value)
                # the bounds the device checks again (a group that breaks them is refused there and its columns come back NaN)
                cnt = np.diff(tb[:n + 1])
                rows = np.add.reduceat(lens[order] + 1, tb[:n]) if n else np.zeros(0, np.int64)
                assert n == 0 or (cnt.min() >= 1 and cnt.max() <= 16 and rows.max() <= SCAN_NT and int(cnt.sum()) == self.Nc_kernel)
                self._node_groups = (h2d(tb[:n + 1].copy(), self.device), h2d(order, self.device), n)
        return self._node_groups or None


def scan_prepare(images, words, plan, cross_attn='t2i'):
    """Per (image block, caption set) precompute for the SCAN kernel: tile-packed words, Gram matrices,
    norms.  Returns the prepared workspace (a uint8 tensor); None when the images do not have the fused kernel's 36 regions
    (scan_xattn_scores takes the pair kernels then, which prepare per block)."""
    lib = _lib.load()
    images = _dev(images, name="images")
    words = _dev(words, name="words")
    Ni, R, D = images.shape
    if R != SCAN_R:
        return None
    wsb = lib.itr_scan_workspace_bytes(Ni, R, words.shape[0], plan.Nc_kernel, plan.n_tiles, D)
    ws = torch.empty(wsb, device=images.device, dtype=torch.uint8)
    if Ni == 0 or plan.Nc_kernel == 0:
        return ws                      # nothing to prepare: the score matrix is empty
    _lib.check(lib.itr_scan_prepare(_p(images), _p(words), _p(plan.cap_off), _p(plan.cap_len), _p(plan.tile_begin),
                                    _p(plan.cap_order), plan.n_tiles, Ni, plan.Nc_kernel, words.shape[0], R, D,
                                    0 if cross_attn == 't2i' else 1, _p(ws), wsb, _stream()))
    return ws


def scan_xattn_scores(images, words, plan, cross_attn='t2i', raw_feature_norm='clipped_l2norm',
                      agg_func='LogSumExp', lambda_lse=6.0, lambda_softmax=9.0, out=None, workspace=None, precision='fp32'):
    """xattn_score_t2i / _i2t (Objectives.py:329-417).  images (Ni, R, D); words (n_rows, D) with the
    caption layout described by `plan` (ScanPlan).  -> (Ni, Nc).  R = 36 (every reference configuration): the fused kernel;
    any other R <= 100: the one-workgroup-per-pair kernels of the training path (_scan_scores_pairwise), same results.
    precision='bf16x3' / 'fp16x3' (opt-in study variants, STUDY_SPLIT_PRECISION.md): the region x word dot products run on the 16-bit
    matrix core from split operands (hi.hi + hi.lo + lo.hi, fp32 accumulation; bf16 planes: ~3e-6, fp16 planes: ~1e-7 of the
    fp32 result, fp16 needs |x| <= 65504); everything else is unchanged."""
    lib = _lib.load()
    if cross_attn not in ('t2i', 'i2t'):
        raise ValueError("unknown first norm type:", raw_feature_norm)  # the reference's message (Objectives.py:71)
    if raw_feature_norm not in _NORMS:
        raise ValueError("unknown first norm type:", raw_feature_norm)
    if agg_func not in _AGGS:
        raise ValueError("unknown aggfunc: {}".format(agg_func))
    images = _dev(images, name="images")
    words = _dev(words, name="words")
    Ni, R, D = images.shape
    n_rows = words.shape[0]
    if out is None:
        out = torch.empty(Ni, plan.Nc, device=images.device, dtype=torch.float32)
    if Ni == 0 or plan.Nc == 0:
        return out
    if R != SCAN_R:
        # the fused kernel is built for the 36 regions of every reference configuration (4 images = 144 rows = 9 MFMA row tiles);
        # any other region count takes the one-workgroup-per-pair kernels of the training path (1..100 regions)
        if precision != 'fp32':
            raise NotImplementedError("scan_xattn_scores: precision=%r with %d regions per image (the fused kernel: %d)" % (precision, R, SCAN_R))
        return _scan_scores_pairwise(images, words, plan, np.arange(plan.Nc), cross_attn, raw_feature_norm, agg_func, lambda_lse,
                                     lambda_softmax, out)
    if plan.long_idx is not None:
        if precision != 'fp32':
            raise NotImplementedError("scan_xattn_scores: precision=%r with captions of more than %d words" % (precision, SCAN_NT))
        return _scan_scores_with_long_captions(images, words, plan, cross_attn, raw_feature_norm, agg_func, lambda_lse, lambda_softmax,
                                               out, workspace)
    ws = workspace if workspace is not None else scan_prepare(images, words, plan, cross_attn)
    if precision in ('bf16x3', 'fp16x3'):
        bsz = lib.itr_scan_bf16_workspace_bytes(Ni, R, plan.n_tiles, D)
        bws = torch.empty(bsz, device=images.device, dtype=torch.uint8)
        _lib.check(lib.itr_scan_xattn_scores_bf16x3(
            _p(images), plan.n_tiles, Ni, plan.Nc, n_rows, R, D, 0 if cross_attn == 't2i' else 1,
            _NORMS[raw_feature_norm], _AGGS[agg_func], float(lambda_softmax), float(lambda_lse), _p(out), out.stride(0),
            _p(ws), ws.numel(), _p(bws), bsz, 1 if precision == 'fp16x3' else 0, _stream()))
        return out
    if precision != 'fp32':
        raise ValueError("scan_xattn_scores: precision must be 'fp32', 'bf16x3' or 'fp16x3'")
    _lib.check(lib.itr_scan_xattn_scores(
        _p(images), plan.n_tiles, Ni, plan.Nc, n_rows, R, D, 0 if cross_attn == 't2i' else 1,
        _NORMS[raw_feature_norm], _AGGS[agg_func], float(lambda_softmax), float(lambda_lse), _p(out), out.stride(0),
        _p(ws), ws.numel(), _stream()))
    return out


def scan_clock_probe(images, words, plan, cross_attn='t2i', raw_feature_norm='clipped_l2norm', agg_func='LogSumExp', lambda_lse=6.0,
                     lambda_softmax=9.0, workspace=None):
    """Shader clock [MHz] the chip sustains UNDER the SCAN kernel: one extra INSTRUMENTED launch (itr_debug_scan_clock_probe; the
    stamps cost the kernel a few percent, so it is never the timed launch).  Every workgroup adds its s_memtime (shader cycles) and
    s_memrealtime (100 MHz) deltas into eight counters at the head of a scratch buffer; clock = 100 * cycles / ticks."""
    lib = _lib.load()
    images = _dev(images, name="images")
    words = _dev(words, name="words")
    Ni, R, D = images.shape
    if R != SCAN_R or plan.long_idx is not None or Ni == 0 or plan.Nc == 0:
        return None
    ws = workspace if workspace is not None else scan_prepare(images, words, plan, cross_attn)
    ld = plan.Nc + 64 + (plan.Nc & 1)                      # an even row width: the int64 view of the head exists whatever Nc is
    scratch = torch.zeros(Ni, ld, device=images.device, dtype=torch.float32)
    _lib.check(lib.itr_debug_scan_clock_probe(
        _p(images), plan.n_tiles, Ni, plan.Nc, words.shape[0], R, D, 0 if cross_attn == 't2i' else 1, _NORMS[raw_feature_norm],
        _AGGS[agg_func], float(lambda_softmax), float(lambda_lse), _p(scratch), ld, _p(ws), ws.numel(), _stream()))
    torch.cuda.synchronize()
    c = scratch.view(torch.int64).flatten()[:8].cpu().numpy().astype(np.float64)
    return 100.0 * float(c[:7].sum()) / float(c[7]) if c[7] > 0 else None


def _scan_scores_with_long_captions(images, words, plan, cross_attn, norm, agg, lambda_lse, lambda_softmax, out, workspace):
    """Captions of 65..96 words (ScanPlan docstring): fused kernel for the rest, pair kernels for these."""
    from . import autograd
    lib = _lib.load()
    Ni, R, D = images.shape
    dev = images.device
    if plan.Nc_kernel:
        ws = workspace if workspace is not None else scan_prepare(images, words, plan, cross_attn)
        part = torch.empty(Ni, plan.Nc_kernel, device=dev, dtype=torch.float32)
        _lib.check(lib.itr_scan_xattn_scores(
            _p(images), plan.n_tiles, Ni, plan.Nc_kernel, words.shape[0], R, D, 0 if cross_attn == 't2i' else 1, _NORMS[norm],
            _AGGS[agg], float(lambda_softmax), float(lambda_lse), _p(part), part.stride(0), _p(ws), ws.numel(), _stream()))
        out[:, torch.from_numpy(plan.short_idx).to(dev)] = part
    return _scan_scores_pairwise(images, words, plan, plan.long_idx, cross_attn, norm, agg, lambda_lse, lambda_softmax, out)


SCAN_PAIR_MAXW, SCAN_PAIR_RMAX = 96, 100          # csrc/scan_train.hip: ST_MAXW, ST_RMAX


def _scan_scores_pairwise(images, words, plan, cap_idx, cross_attn, norm, agg, lambda_lse, lambda_softmax, out, budget_bytes=1 << 30):
    """out[:, cap_idx] through the forward of the training path (csrc/scan_train*.hip: one GEMM for the raw dot products of a block
    of pairs, one workgroup per (image, caption) pair for the rest) -- the captions the fused kernel does not take (65..96 words) and
    every caption when the images do not have the 36 regions it is built for.  The pairs are cut into blocks whose dot-product
    matrix [images x R, words] stays under `budget_bytes`."""
    from . import autograd
    Ni, R, D = images.shape
    dev = images.device
    cap_idx = np.asarray(cap_idx, dtype=np.int64)
    lens_all = plan.len_host[cap_idx]
    if R > SCAN_PAIR_RMAX or (len(lens_all) and int(lens_all.max()) > SCAN_PAIR_MAXW):
        raise NotImplementedError("scan_xattn_scores: %d regions per image / captions of %d words (supported: <= %d regions; "
                                  "captions of <= %d words)" % (R, int(lens_all.max()) if len(lens_all) else 0, SCAN_PAIR_RMAX, SCAN_PAIR_MAXW))
    fn = autograd.scan_t2i_scores if cross_attn == 't2i' else autograd.scan_i2t_scores
    bi = int(min(Ni, 1024, 65535 // R))                               # grid.y and the i2t kernels' 65535-row limits
    tok_budget = max(int(budget_bytes // (4 * bi * R)), SCAN_PAIR_MAXW)
    csum = np.concatenate([[0], np.cumsum(lens_all)])
    with torch.no_grad():
        c0 = 0
        while c0 < len(cap_idx):
            c1 = int(np.searchsorted(csum, csum[c0] + tok_budget, side='right')) - 1
            c1 = min(max(c1, c0 + 1), len(cap_idx))
            ids, lens = cap_idx[c0:c1], lens_all[c0:c1]
            rows = np.concatenate([np.arange(plan.off_host[c], plan.off_host[c] + plan.len_host[c]) for c in ids])
            w_blk = words[h2d(rows, dev)].contiguous()
            off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
            cols = h2d(ids, dev)
            for i0 in range(0, Ni, bi):
                out[i0:i0 + bi, cols] = fn(images[i0:i0 + bi], w_blk, off, lens, norm, agg, lambda_lse, lambda_softmax)
            c0 = c1
    return out


def scan_xattn_padded(images, captions, cap_lens, **kw):
    """Reference call shape: captions (Nc, L, D) padded + cap_lens (Objectives.py:329)."""
    Nc, L, D = captions.shape
    lens = [int(x) for x in cap_lens][:Nc]
    plan = ScanPlan(np.arange(Nc, dtype=np.int64) * L, lens, Nc * L, captions.device)
    return scan_xattn_scores(images, _dev(captions, name="captions").reshape(Nc * L, D), plan, **kw)


# ------------------------------------------------------------------------------------------ transformer blocks
def bert_embed_ln(ids, type_ids, word_emb, pos_emb, type_emb, gamma, beta, eps=1e-12):
    lib = _lib.load()
    ids = _dev(ids, torch.int64, "input_ids")
    ty = _dev(type_ids, torch.int64, "token_type_ids") if type_ids is not None else None
    B, L = ids.shape
    H = word_emb.shape[1]
    out = torch.empty(B, L, H, device=ids.device, dtype=torch.float32)
    _lib.check(lib.itr_bert_embed_ln(_p(ids), _p(ty), _p(_dev(word_emb)), _p(_dev(pos_emb)), _p(_dev(type_emb)),
                                     _p(_dev(gamma)), _p(_dev(beta)), _p(out), B, L, H, word_emb.shape[0],
                                     pos_emb.shape[0], type_emb.shape[0], eps, _stream()))
    return out


def add_layernorm(x, residual, gamma, beta, eps=1e-12):
    """BERTLayerNorm(x + residual) (bert.py:113-126): epsilon inside the sqrt."""
    lib = _lib.load()
    x = _dev(x, name="x")
    r = _dev(residual, name="residual") if residual is not None else None
    H = x.shape[-1]
    out = torch.empty_like(x)
    _lib.check(lib.itr_add_layernorm(_p(x), _p(r), _p(_dev(gamma)), _p(_dev(beta)), _p(out), x.numel() // H, H, eps,
                                     _stream()))
    return out


def mha_small(q, k, v, mask, B, L, heads, dk, scale, out=None):
    """q, k, v: 2-D views [B*L, *] (last dim contiguous, head h at columns h*dk .. h*dk+dk-1; they may be column
    slices of one fused QKV buffer).  mask: (B, L) float 0/1 or None.  -> (B*L, heads*dk).  `out`: a (B*L, heads*dk) view with a
    contiguous last dim (a column block of a wider buffer; rows that are not 16-byte aligned take the LDS-staged kernel)."""
    lib = _lib.load()
    for t in (q, k, v):
        if not (t.is_cuda and t.dtype == torch.float32 and t.stride(-1) == 1):
            raise ValueError("mha_small: q/k/v must be fp32 CUDA tensors with a contiguous last dim")
    m = _dev(mask.to(torch.float32), name="mask") if mask is not None else None
    if out is None:
        out = torch.empty(B * L, heads * dk, device=q.device, dtype=torch.float32)
    elif not (out.is_cuda and out.dtype == torch.float32 and out.stride(-1) == 1 and tuple(out.shape) == (B * L, heads * dk)):
        raise ValueError("mha_small: out must be a fp32 CUDA (B*L, heads*dk) view with a contiguous last dim")
    _lib.check(lib.itr_mha_small(_p(q), _p(k), _p(v), q.stride(0), k.stride(0), v.stride(0), _p(m), _p(out),
                                 out.stride(0), B, L, heads, dk, float(scale), _stream()))
    return out


def relu_maxpool(x, valid, out=None):
    """x (B, L, C) -> max over t < valid of relu(x) -> (B, C)."""
    lib = _lib.load()
    x = _dev(x, name="x")
    B, L, Cc = x.shape
    if out is None:
        out = torch.empty(B, Cc, device=x.device, dtype=torch.float32)
    for b0 in range(0, B, 65535):
        b1 = min(B, b0 + 65535)
        _lib.check(lib.itr_relu_maxpool(_p(x[b0:b1]), _p(out[b0:b1]), out.stride(0), b1 - b0, L, Cc, int(valid), _stream()))
    return out


# ------------------------------------------------------------------------------------------ CAMERA helpers
def mul_rows(a, b2d):
    """a (..., C) * b where b is a 2-D (R, C) view with contiguous last dim (may be a column slice)."""
    lib = _lib.load()
    a = _dev(a, name="a")
    Cc = a.shape[-1]
    R = a.numel() // Cc
    if not (b2d.is_cuda and b2d.dim() == 2 and b2d.stride(1) == 1 and b2d.shape[0] == R and b2d.shape[1] == Cc):
        raise ValueError("mul_rows: b must be a (R, C) CUDA view with a contiguous last dim")
    out = torch.empty_like(a)
    _lib.check(lib.itr_mul_rows(_p(a), _p(b2d), b2d.stride(0), _p(out), R, Cc, _stream()))
    return out


def agsa_gate(q2, k2, fc_q, fc_k, fc_g):
    """GatedQueryAttLayer's gate (camera_.py:36-44) on q2, k2 [rows, dk] (rows = positions x heads; dk = 16 or 32), fc_* = (weight,
    bias) of the three Linear layers -> (q2 * M[:, :dk], k2 * M[:, dk:]) with M = sigmoid(fc_g(fc_q(q2) * fc_k(k2))).  One kernel
    (csrc/agsa_gate.hip) instead of three skinny GEMMs and three elementwise products."""
    lib = _lib.load()
    q2, k2 = _dev(q2, name="q"), _dev(k2, name="k")
    rows, dk = q2.shape
    w = [_dev(t.detach(), name="gate weight") for pair in (fc_q, fc_k, fc_g) for t in pair]
    if w[0].shape != (dk, dk) or w[2].shape != (dk, dk) or w[4].shape != (2 * dk, dk) or k2.shape != q2.shape:
        raise ValueError("agsa_gate: q / k [rows, dk], fc_q / fc_k Linear(dk, dk), fc_g Linear(dk, 2 dk)")
    qo, ko = torch.empty_like(q2), torch.empty_like(k2)
    _lib.check(lib.itr_agsa_gate(_p(q2), _p(k2), rows, dk, _p(w[0]), _p(w[1]), _p(w[2]), _p(w[3]), _p(w[4]), _p(w[5]), _p(qo), _p(ko), _stream()))
    return qo, ko


def affine_cols(x, scale=None, shift=None, residual=None, act=None):
    """act(x*scale[c] + shift[c]) + residual (eval-mode BatchNorm1d folded to scale / shift)."""
    lib = _lib.load()
    x = _dev(x, name="x")
    Cc = x.shape[-1]
    out = torch.empty_like(x)
    sc = _dev(scale) if scale is not None else None
    sh = _dev(shift) if shift is not None else None
    rs = _dev(residual) if residual is not None else None
    _lib.check(lib.itr_affine_cols(_p(x), _p(sc), _p(sh), _p(rs), _p(out), x.numel() // Cc, Cc, _ACTS[act], _stream()))
    return out


def gemm_acc(x2d, lda, M, K, weight, bias, out, act=None):
    """out = act(out + A @ weight^T + bias), A rows at x2d.data_ptr() + m*lda."""
    lib = _lib.load()
    weight = _dev(weight, name="weight")
    b = _dev(bias) if bias is not None else None
    _lib.check(lib.itr_gemm_nt_acc(_p(x2d), lda, _p(weight), weight.shape[1], _p(b), _p(out), out.stride(0), M,
                                   weight.shape[0], K, _ACTS[act], _stream()))
    return out


def gemm_residual(x2d, weight, bias, residual, act=None):
    """act(residual + x2d @ weight^T + bias) -> new tensor (a residual connection without copying the residual into the output
    first; same arithmetic as gemm_acc on a clone)."""
    lib = _lib.load()
    x2d, weight, residual = _dev(x2d, name="x"), _dev(weight, name="weight"), _dev(residual, name="residual")
    M, K = x2d.shape
    N = weight.shape[0]
    if weight.shape[1] != K or tuple(residual.shape) != (M, N):
        raise ValueError("gemm_residual: x (%d, %d), weight %s, residual %s" % (M, K, tuple(weight.shape), tuple(residual.shape)))
    b = _dev(bias) if bias is not None else None
    out = torch.empty(M, N, device=x2d.device, dtype=torch.float32)
    _lib.check(lib.itr_gemm_nt_residual(_p(x2d), K, _p(weight), K, _p(b), _p(residual), N, _p(out), N, M, N, K, _ACTS[act], _stream()))
    return out


def gcn_relation(tpg, n_img, n_regions, channels):
    """Rs_GCN between its convolutions (vsrn_.py:50-67): tpg [n_img*N, 3C] rows = theta | phi | g ->
    y [n_img*N, C] = (theta phi^T / N) g per image."""
    lib = _lib.load()
    tpg = _dev(tpg, name="tpg")
    if tpg.dim() != 2 or tpg.shape[0] != n_img * n_regions or tpg.shape[1] != 3 * channels:
        raise ValueError("gcn_relation: tpg %s for %d images x %d regions x 3*%d" % (tuple(tpg.shape), n_img, n_regions, channels))
    y = torch.empty(n_img * n_regions, channels, device=tpg.device, dtype=torch.float32)
    _lib.check(lib.itr_gcn_relation(_p(tpg), tpg.shape[1], _p(y), channels, n_img, n_regions, channels, _stream()))
    return y


def camera_posenc(boxes, imgs_wh):
    lib = _lib.load()
    boxes = _dev(boxes.to(torch.float32), name="boxes")
    wh = _dev(imgs_wh.to(torch.float32), name="imgs_wh")
    B, R = boxes.shape[:2]
    out = torch.empty(B, R, 6, device=boxes.device, dtype=torch.float32)
    _lib.check(lib.itr_camera_posenc(_p(boxes), _p(wh), _p(out), B, R, _stream()))
    return out


def camera_summarize(smry_mat, X):
    """softmax over regions of smry (B, R, k); (L^T X) -> F.normalize -> (B, k, D)."""
    lib = _lib.load()
    smry_mat = _dev(smry_mat, name="smry_mat")
    X = _dev(X, name="X")
    B, R, k = smry_mat.shape
    D = X.shape[2]
    out = torch.empty(B, k, D, device=X.device, dtype=torch.float32)
    _lib.check(lib.itr_camera_summarize(_p(smry_mat), _p(X), _p(out), B, R, k, D, _stream()))
    return out


# ------------------------------------------------------------------------------------------
_SGRAF_MAP = {
    "v_loc_w": "v_global_w.embedding_local.0.weight", "v_loc_b": "v_global_w.embedding_local.0.bias",
    "v_loc_bn_w": "v_global_w.embedding_local.1.weight", "v_loc_bn_b": "v_global_w.embedding_local.1.bias",
    "v_loc_bn_mean": "v_global_w.embedding_local.1.running_mean", "v_loc_bn_var": "v_global_w.embedding_local.1.running_var",
    "v_glo_w": "v_global_w.embedding_global.0.weight", "v_glo_b": "v_global_w.embedding_global.0.bias",
    "v_glo_bn_w": "v_global_w.embedding_global.1.weight", "v_glo_bn_b": "v_global_w.embedding_global.1.bias",
    "v_glo_bn_mean": "v_global_w.embedding_global.1.running_mean", "v_glo_bn_var": "v_global_w.embedding_global.1.running_var",
    "v_com_w": "v_global_w.embedding_common.0.weight", "v_com_b": "v_global_w.embedding_common.0.bias",
    "t_loc_w": "t_global_w.embedding_local.0.weight", "t_loc_b": "t_global_w.embedding_local.0.bias",
    "t_glo_w": "t_global_w.embedding_global.0.weight", "t_glo_b": "t_global_w.embedding_global.0.bias",
    "t_com_w": "t_global_w.embedding_common.0.weight", "t_com_b": "t_global_w.embedding_common.0.bias",
    "loc_w": "sim_tranloc_w.weight", "loc_b": "sim_tranloc_w.bias", "glo_w": "sim_tranglo_w.weight",
    "glo_b": "sim_tranglo_w.bias", "eval_w": "sim_eval_w.weight", "eval_b": "sim_eval_w.bias",
}
_SAF_MAP = {"saf_w": "SAF_module.attn_sim_w.weight", "saf_b": "SAF_module.attn_sim_w.bias",
            "saf_bn_w": "SAF_module.bn.weight", "saf_bn_b": "SAF_module.bn.bias",
            "saf_bn_mean": "SAF_module.bn.running_mean", "saf_bn_var": "SAF_module.bn.running_var"}


SGRAF_MAX_WORDS = 63      # fused pair kernels: 63 words + the global node = one 64-row tile
SGRAF_COMPOSED_MAX_WORDS = 191   # the per-caption composition: 191 words + the global node = the 192 graph nodes itr_smry_fwd holds


SGRAF_FLAGS = {"unfused_steps": 1, "non_persistent": 2}       # include/itr_hip.h: ITR_SGRAF_UNFUSED_STEPS, ITR_SGRAF_NON_PERSISTENT
SGRAF_LAST_BLOCK = {}          # diagnostics: what the last sgraf_scores call ran with (image_block, workspace_bytes, budget)


def _sgraf_workspace(lib, dev, Ni, Nc, n_rows, n_tiles, D, S_dim, mod, flags, image_block, max_workspace_bytes):
    """Pick the pair stage's image block for the memory this process can have and allocate the workspace (a
    validation pass inside a training process -- optimizer state and activations resident -- or a co-tenant must shrink the
    block, not die).  Budget = `max_workspace_bytes` if given, else 90 % of (free device memory + what torch's caching allocator
    holds unused); the largest of 64 / 32 / 16 / 8 / 4 images whose workspace fits is taken (itr_sgraf_pick_image_block), and an
    allocation that still fails falls back to the next smaller block.  image_block / SETTINGS.sgraf_image_block pin the block instead.
    -> (workspace tensor, image_block)."""
    if image_block is None and SETTINGS.sgraf_image_block:
        image_block = int(SETTINGS.sgraf_image_block)          # explicit knob (several ranks sharing ONE GPU in the tests)
    if image_block is not None:
        wsb = lib.itr_sgraf_workspace_bytes(Ni, Nc, n_rows, n_tiles, D, S_dim, mod, int(image_block), flags)
        SGRAF_LAST_BLOCK.update(image_block=int(image_block), workspace_bytes=int(wsb), budget_bytes=None, pinned=True)
        return torch.empty(wsb, device=dev, dtype=torch.uint8), int(image_block)
    budget = _workspace_budget(dev, max_workspace_bytes)
    while True:
        wsb = C.c_size_t(0)
        ib = lib.itr_sgraf_pick_image_block(Ni, Nc, n_rows, n_tiles, D, S_dim, mod, flags, max(0, budget), C.byref(wsb))
        if ib < 0:
            raise torch.cuda.OutOfMemoryError("sgraf_scores: %s" % lib.itr_last_error().decode())
        try:
            ws = torch.empty(wsb.value, device=dev, dtype=torch.uint8)
        except torch.cuda.OutOfMemoryError:
            if max_workspace_bytes is not None and budget < wsb.value:
                raise
            torch.cuda.empty_cache()
            budget = wsb.value - 1                             # the next smaller block
            continue
        SGRAF_LAST_BLOCK.update(image_block=int(ib), workspace_bytes=int(wsb.value), budget_bytes=budget, pinned=False)
        return ws, int(ib)


def _sgraf_weight_names(module_name, sgr_step):
    """state_dict names of the tensors an EncoderSimilarity of this module reads"""
    names = list(_SGRAF_MAP.values())
    if module_name == 'SAF':
        names += list(_SAF_MAP.values())
    else:
        for k in range(sgr_step):
            names += ["SGR_module.sgr%d.%s.%s" % (k, m, t) for m in ("graph_query_w", "graph_key_w", "sim_graph_w") for t in ("weight", "bias")]
    return names


def _sgraf_weight_struct(weights, module_name, sgr_step):
    """-> (itr_sgraf_weights struct of device pointers, the tensors that keep them alive, sim_dim)"""
    keep = []
    st = _lib.SgrafWeights()

    def ptr(name):
        t = _dev(weights[name].detach(), name=name)
        keep.append(t)
        return t.data_ptr()

    for f, name in _SGRAF_MAP.items():
        setattr(st, f, ptr(name))
    S_dim = weights["sim_tranloc_w.weight"].shape[0]
    if module_name == 'SAF':
        for f, name in _SAF_MAP.items():
            setattr(st, f, ptr(name))
    else:
        if not 1 <= int(sgr_step) <= 8:      # (itr_sgraf_weights holds 8 steps: refused here as the library refuses it, not by an index error)
            raise NotImplementedError("itr_sgraf_scores: sgr_step must be in [1, 8]")
        for k in range(sgr_step):
            pre = "SGR_module.sgr%d." % k
            st.sgr_q_w[k] = ptr(pre + "graph_query_w.weight"); st.sgr_q_b[k] = ptr(pre + "graph_query_w.bias")
            st.sgr_k_w[k] = ptr(pre + "graph_key_w.weight"); st.sgr_k_b[k] = ptr(pre + "graph_key_w.bias")
            st.sgr_g_w[k] = ptr(pre + "sim_graph_w.weight"); st.sgr_g_b[k] = ptr(pre + "sim_graph_w.bias")
    return st, keep, S_dim


def sgraf_scores(images, words, plan, weights, module_name='SAF', sgr_step=3, out=None, image_block=None, max_workspace_bytes=None,
                 variant=()):
    """EncoderSimilarity.forward (Fusionmodule.py:406-451), eval mode.  images (Ni, 36, D); words (n_rows, D)
    with the caption layout of `plan` (ScanPlan on the WORD lengths); weights: the module's state_dict.
    image_block / max_workspace_bytes: see _sgraf_workspace (default: the largest block the free memory admits).
    variant: names from SGRAF_FLAGS -- the step-by-step / non-persistent forms the fused kernel is cross-checked against."""
    lib = _lib.load()
    if module_name not in ('SAF', 'SGR'):
        raise ValueError('Invalid input of config.module_name in configs.py')
    images = _dev(images, name="images")
    words = _dev(words, name="words")
    Ni, R, D = images.shape
    st, keep, S_dim = _sgraf_weight_struct(weights, module_name, sgr_step)
    mod = 0 if module_name == 'SAF' else 1
    flags = 0
    for v in ((variant,) if isinstance(variant, str) else variant):
        flags |= SGRAF_FLAGS[v]
    dev = images.device
    if out is None:
        out = torch.empty(Ni, plan.Nc, device=dev, dtype=torch.float32)
    if plan.Nc and int(plan.len_host.max()) > SGRAF_MAX_WORDS:
        plan = ScanPlan(plan.off_host, plan.len_host, plan.n_rows, plan.device, max_kernel_len=SGRAF_MAX_WORDS)

    def fused_call(Nc_k, max_len, dst):
        grp = plan.node_groups() if mod == 1 else None      # SGR: the graph steps of a group of captions run in one workgroup
        fl = flags | (SGRAF_FLAGS["unfused_steps"] if (mod == 1 and not grp) else 0)
        ws, ib = _sgraf_workspace(lib, dev, Ni, Nc_k, words.shape[0], plan.n_tiles, D, S_dim, mod, fl, image_block, max_workspace_bytes)
        _lib.check(lib.itr_sgraf_scores(_p(images), _p(words), _p(plan.cap_off), _p(plan.cap_len), _p(plan.tile_begin),
                                        _p(plan.cap_order), plan.n_tiles, Ni, Nc_k, words.shape[0], max_len, R, D, S_dim,
                                        mod, int(sgr_step), C.byref(st), _p(grp[0]) if grp else None, _p(grp[1]) if grp else None,
                                        grp[2] if grp else 0, ib, fl, _p(dst), dst.stride(0), _p(ws), ws.numel(), _stream()))

    if plan.long_idx is not None:
        # Captions of more than 63 words (Flickr30k has a few, up to 82 tokens) do not fit the 64-node tiles of the fused pair
        # kernels: the others are scored by the fused path, these by the per-caption composition of the training path run in
        # evaluation mode (Fusionmodule.encoder_similarity_train(training=False): same arithmetic, HIP kernels, up to 191 words).
        from .modalmodule import Fusionmodule
        if plan.Nc_kernel:
            part = torch.empty(Ni, plan.Nc_kernel, device=dev, dtype=torch.float32)
            fused_call(plan.Nc_kernel, int(plan.len_host[plan.short_idx].max()), part)
            out[:, torch.from_numpy(plan.short_idx).to(dev)] = part
        sim_enc = Fusionmodule.EncoderSimilarity(D, S_dim, module_name, sgr_step)
        own = sim_enc.state_dict()
        sim_enc.load_state_dict({k: (weights[k].detach() if k in weights else own[k]) for k in own if k in weights or k.endswith('num_batches_tracked')})
        sim_enc.to(dev).eval()
        lens = [int(plan.len_host[c]) for c in plan.long_idx]
        if max(lens) > SGRAF_COMPOSED_MAX_WORDS:
            raise NotImplementedError("sgraf_scores: captions of at most %d words are supported" % SGRAF_COMPOSED_MAX_WORDS)
        rows = np.concatenate([np.arange(plan.off_host[c], plan.off_host[c] + plan.len_host[c]) for c in plan.long_idx])
        w_long = words[torch.from_numpy(rows).to(dev)].contiguous()
        off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
        with torch.no_grad():
            out[:, torch.from_numpy(plan.long_idx).to(dev)] = Fusionmodule.encoder_similarity_train(sim_enc, images, w_long, off, lens, None,
                                                                                                   training=False)
        return out
    fused_call(plan.Nc, int(plan.len_host.max()) if plan.Nc else 1, out)
    return out


def sgraf_padded(images, captions, cap_lens, weights, module_name='SAF', sgr_step=3, **kw):
    """Reference call shape: captions (Nc, L, D) padded + cap_lens (Fusionmodule.py:406).  kw: sgraf_scores' image_block /
    max_workspace_bytes / variant."""
    Nc, L, D = captions.shape
    lens = [int(x) for x in cap_lens][:Nc]
    plan = ScanPlan(np.arange(Nc, dtype=np.int64) * L, lens, Nc * L, captions.device)
    return sgraf_scores(images, _dev(captions, name="captions").reshape(Nc * L, D), plan, weights, module_name, sgr_step, **kw)


_TOKENS_CHECKED = {}         # id(tensor) -> (weak reference, (version counter, vocabulary size)) of token tensors whose id range has been checked


def gru_encode(tokens_packed, tok_off, lengths, weights, bidirectional, no_txtnorm=False, use_abs=False,
               gather_last=False, out=None, batch_invariant=False, launch_form=None, chains=0):
    """EncoderText.forward on packed captions (TextEncoder.py:38-70).
    tokens_packed (n_tok,) int64 cuda; tok_off (B,) int64; lengths: host list sorted descending.
    weights: dict with the reference's state_dict names.  -> (n_tok, D) packed word embeddings, or
    (B, D) when gather_last.  `out`: the caller's contiguous (n_tok, D) / (B, D) result buffer -- e.g. the head of the
    send buffer of the sharded evaluation's all-gather (evalpipe.py).  batch_invariant: a caption's embedding does not
    depend, bit for bit, on which other captions share its batch (ITR_GRU_BATCH_INVARIANT, include/itr_hip.h).
    launch_form: None (default), "paired" or "input_after_fork" -- the bi-GRU launch orders kept as bit-identical cross-checks
    (ITR_GRU_PAIRED_DIRECTIONS / ITR_GRU_INPUT_AFTER_FORK flag bits); "per_token": the input projection as one GEMM row per TOKEN
    even where the call would project the vocabulary once (ITR_GRU_PER_TOKEN_INPUT; >= 2 tokens per vocabulary word) -- the
    cross-check of that form; "first_step_gemm": the recurrence GEMM of step 0 is launched although h = 0 makes it b_hh
    (ITR_GRU_FIRST_STEP_GEMM), the cross-check of skipping it.  chains: interleaved caption chains of the last-state recurrence (ITR_GRU_CHAINS; 0 = the library's choice)."""
    lib = _lib.load()
    form_bits = {None: 0, "paired": 4, "input_after_fork": 8, "per_token": 16, "paired+per_token": 20, "first_step_gemm": 256,
                 "per_token+first_step_gemm": 272}[launch_form]
    tokens_packed = _dev(tokens_packed, torch.int64, "tokens")
    len_host = _host_i32(lengths)
    B = len(len_host)
    n_tok = int(tokens_packed.numel())
    dev = tokens_packed.device
    tok_off = _dev(tok_off, torch.int64, "tok_off")
    len_dev = h2d(len_host.copy(), dev)
    emb = _dev(weights['embed.weight'], name="embed.weight")
    V, E = emb.shape
    if n_tok:
        # nn.Embedding raises on ids outside [0, V) (TextEncoder.py:41).  The check costs a device -> host round trip, so a token tensor
        # that has been checked is not checked again until it is written to (an evaluation loop encodes the same tokens every step)
        # (The cache trusts torch's version counter: writes through .data, raw pointers or DLPack do not bump it -- such a caller must
        # pass a fresh tensor.  Inference-mode tensors have no version counter: they are checked every time.)
        ver = None if tokens_packed.is_inference() else tokens_packed._version
        ent = _TOKENS_CHECKED.get(id(tokens_packed)) if ver is not None else None
        if not (ent is not None and ent[0]() is tokens_packed and ent[1] == (ver, int(V))):
            lo, hi = torch.aminmax(tokens_packed)
            if int(lo) < 0 or int(hi) >= V:
                raise IndexError("index out of range in self")
            if ver is not None:
                if len(_TOKENS_CHECKED) >= 16:
                    _TOKENS_CHECKED.clear()
                _TOKENS_CHECKED[id(tokens_packed)] = (weakref.ref(tokens_packed), (ver, int(V)))
    w_ih = _dev(weights['rnn.weight_ih_l0'])
    w_hh = _dev(weights['rnn.weight_hh_l0'])
    b_ih = _dev(weights['rnn.bias_ih_l0'])
    b_hh = _dev(weights['rnn.bias_hh_l0'])
    D = w_hh.shape[1]
    rev = [None] * 4
    if bidirectional:
        rev = [_dev(weights['rnn.weight_ih_l0_reverse']), _dev(weights['rnn.weight_hh_l0_reverse']),
               _dev(weights['rnn.bias_ih_l0_reverse']), _dev(weights['rnn.bias_hh_l0_reverse'])]
    wsb = lib.itr_gru_workspace_bytes(n_tok, B, E, D, int(bool(bidirectional)))
    ws = torch.empty(wsb, device=dev, dtype=torch.uint8)
    if out is not None and not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()
                                and tuple(out.shape) == ((B, D) if gather_last else (n_tok, D))):
        raise ValueError("gru_encode: out must be a contiguous fp32 CUDA tensor of shape %s" % (((B, D) if gather_last else (n_tok, D)),))
    res = out
    out = None if gather_last else (res if res is not None else torch.empty(n_tok, D, device=dev, dtype=torch.float32))
    out_last = (res if res is not None else torch.empty(B, D, device=dev, dtype=torch.float32)) if gather_last else None
    _lib.check(lib.itr_gru_fwd(_p(tokens_packed), _p(tok_off), _p(len_dev), len_host.ctypes.data_as(C.c_void_p), B,
                               n_tok, _p(emb), V, E, D, _p(w_ih), _p(w_hh), _p(b_ih), _p(b_hh), _p(rev[0]),
                               _p(rev[1]), _p(rev[2]), _p(rev[3]), int(no_txtnorm), int(use_abs), int(bool(gather_last)) | (2 if batch_invariant else 0) | form_bits | ((int(chains) & 7) << 5),
                               _p(out), _p(out_last), _p(ws), wsb, _stream()))
    return out_last if gather_last else out


# ------------------------------------------------------------------------------------------
def rank_counts(S, im_div=5, row0=0, s_gt=None, t2i_rank=None, t2i_best=None):
    """Sort-free ranks of a (local row block of a) similarity matrix, ONE pass over S for both directions.
    -> (i2t_rank int32[n_rows], i2t_top1 int32[n_rows], t2i_rank int32[Nc], t2i_best uint64-as-int64[Nc], s_gt)
    For a single GPU (row0 = 0, all rows local) t2i_rank is final and t2i_top1 = t2i_best & 0xffffffff.
    s_gt None: when the block holds every ground-truth row (the single-GPU call) the library reads the GT scores from S itself
    (no gather launch; the returned s_gt is then None); otherwise they are gathered here for the local rows (the sharded
    evaluation gathers, max-reduces over ranks and passes them in).  t2i_rank / t2i_best None: allocated here and zeroed INSIDE
    the call (ITR_RANK_INIT_COLUMNS); pass them to accumulate over several row blocks.
    A float64 matrix (the reference's cal_sims output, an ensemble average) is ranked in float64: `rank_counts_f64`."""
    lib = _lib.load()
    S = _dev(S, name="S")
    n_rows, Nc = S.shape
    dev = S.device
    if s_gt is None and not (row0 == 0 and n_rows * im_div >= Nc):
        s_gt = torch.full((Nc,), float('-inf'), device=dev, dtype=torch.float32)
        _lib.check(lib.itr_rank_gather_gt(_p(S), S.stride(0), row0, n_rows, Nc, im_div, _p(s_gt), _stream()))
    i2t_rank = torch.empty(n_rows, device=dev, dtype=torch.int32)
    i2t_top1 = torch.empty(n_rows, device=dev, dtype=torch.int32)
    if (t2i_rank is None) != (t2i_best is None):
        raise ValueError("rank_counts: pass both t2i_rank and t2i_best (accumulators of several row blocks) or neither")
    flags = 0
    if t2i_rank is None:
        t2i_rank = torch.empty(Nc, device=dev, dtype=torch.int32)
        t2i_best = torch.empty(Nc, device=dev, dtype=torch.int64)
        flags = 1                      # ITR_RANK_INIT_COLUMNS
    wsb = lib.itr_rank_workspace_bytes(n_rows, Nc)
    ws = torch.empty(wsb // 8 + 1, device=dev, dtype=torch.int64)
    _lib.check(lib.itr_rank_counts(_p(S), S.stride(0), row0, n_rows, Nc, im_div, _p(s_gt), _p(i2t_rank), _p(i2t_top1),
                                   _p(t2i_rank), _p(t2i_best), flags, _p(ws), wsb, _stream()))
    return i2t_rank, i2t_top1, t2i_rank, t2i_best, s_gt


def rank_counts_f64(S, im_div=5):
    """The same counts on a float64 similarity matrix (all rows local): index-exact against the reference's argsort of
    float64 rows / columns (evaluation.py:169, :209; ensemble averages: :380, :398).
    -> (i2t_rank, i2t_top1, t2i_rank, t2i_top1) int32."""
    lib = _lib.load()
    S = _dev(S, dtype=torch.float64, name="S")
    n_rows, Nc = S.shape
    dev = S.device
    s_gt = torch.full((Nc,), float('-inf'), device=dev, dtype=torch.float64)
    _lib.check(lib.itr_rank_gather_gt_f64(_p(S), S.stride(0), 0, n_rows, Nc, im_div, _p(s_gt), _stream()))
    i2t_rank = torch.empty(n_rows, device=dev, dtype=torch.int32)
    i2t_top1 = torch.empty(n_rows, device=dev, dtype=torch.int32)
    t2i_rank = torch.zeros(Nc, device=dev, dtype=torch.int32)
    t2i_key = torch.zeros(Nc, device=dev, dtype=torch.int64)
    t2i_top1 = torch.full((Nc,), -1, device=dev, dtype=torch.int32)
    _lib.check(lib.itr_rank_counts_f64(_p(S), S.stride(0), 0, n_rows, Nc, im_div, _p(s_gt), _p(i2t_rank), _p(i2t_top1),
                                       _p(t2i_rank), _p(t2i_key), _stream()))
    _lib.check(lib.itr_rank_t2i_top1_f64(_p(S), S.stride(0), 0, n_rows, Nc, _p(t2i_key), _p(t2i_top1), _stream()))
    return i2t_rank, i2t_top1, t2i_rank, t2i_top1


def gather_gt(S, im_div=5, row0=0, s_gt=None):
    lib = _lib.load()
    S = _dev(S, name="S")
    n_rows, Nc = S.shape
    if s_gt is None:
        s_gt = torch.full((Nc,), float('-inf'), device=S.device, dtype=torch.float32)
    _lib.check(lib.itr_rank_gather_gt(_p(S), S.stride(0), row0, n_rows, Nc, im_div, _p(s_gt), _stream()))
    return s_gt


def recall_from_ranks(ranks):
    """(r1, r5, r10, medr, meanr) from 0-based integer ranks (evaluation.py:181-185); host side."""
    lib = _lib.load()
    r = np.ascontiguousarray(np.asarray(ranks, dtype=np.int32))
    out = (C.c_double * 5)()
    _lib.check(lib.itr_recall_from_ranks(r.ctypes.data_as(C.c_void_p), len(r), out))
    return tuple(float(v) for v in out)


# ------------------------------------------------------------------------------------------ any ground-truth relation
def ground_truth_csr(pairs, n_images, n_captions):
    """Host side of `GroundTruth`: integer [nnz, 2] (image, caption) pairs -> (img_ptr [Ni + 1], img_cap [nnz], cap_ptr [Nc + 1],
    cap_img [nnz]) int32 numpy arrays, the relation by image (captions ascending) and by caption (images ascending).
    An index out of range or a pair given twice raises ValueError naming the pair: nothing unchecked reaches a kernel."""
    n_images, n_captions = int(n_images), int(n_captions)
    if n_images < 0 or n_captions < 0:
        raise ValueError("GroundTruth: negative gallery size (%d images, %d captions)" % (n_images, n_captions))
    p = pairs.detach().cpu().numpy() if torch.is_tensor(pairs) else np.asarray(pairs)
    if p.size == 0:
        p = np.zeros((0, 2), dtype=np.int64)
    if p.ndim != 2 or p.shape[1] != 2:
        raise ValueError("GroundTruth: pairs must have shape [nnz, 2] (image, caption), got %s" % (tuple(p.shape),))
    if not np.issubdtype(p.dtype, np.integer):
        raise TypeError("GroundTruth: pairs must be integers, got %s" % p.dtype)
    p = p.astype(np.int64, copy=False)
    nnz = p.shape[0]
    if nnz >= 2 ** 31 - 1 or n_images >= 2 ** 31 - 1 or n_captions >= 2 ** 31 - 1:
        raise NotImplementedError("GroundTruth: nnz, n_images and n_captions must be below 2^31")
    img, cap = p[:, 0], p[:, 1]
    bad = np.flatnonzero((img < 0) | (img >= n_images) | (cap < 0) | (cap >= n_captions))
    if bad.size:
        b = int(bad[0])
        raise ValueError("GroundTruth: pair %d = (image %d, caption %d) is out of range for %d images x %d captions"
                         % (b, int(img[b]), int(cap[b]), n_images, n_captions))
    by_img = np.lexsort((cap, img))
    key = img[by_img] * max(n_captions, 1) + cap[by_img]
    dup = np.flatnonzero(key[1:] == key[:-1])
    if dup.size:
        b = int(by_img[dup[0] + 1])
        raise ValueError("GroundTruth: pair %d = (image %d, caption %d) is given more than once" % (b, int(img[b]), int(cap[b])))
    by_cap = np.lexsort((img, cap))

    def ptr(idx, n):
        out = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(np.bincount(idx, minlength=n), out=out[1:])
        return out.astype(np.int32)
    return ptr(img, n_images), cap[by_img].astype(np.int32), ptr(cap, n_captions), img[by_cap].astype(np.int32)


class GroundTruth:
    """A ground-truth relation between n_images images and n_captions captions for `rank_positions`: any number of positives per
    query.  pairs: integer [nnz, 2] (image, caption), numpy or tensor, validated on the host (`ground_truth_csr`), then both CSR
    forms are uploaded once.  Attributes: img_ptr / img_cap / cap_ptr / cap_img (int32 device tensors), nnz, n_images, n_captions,
    device, and the host copies img_ptr_host / cap_ptr_host."""

    def __init__(self, pairs, n_images, n_captions, device):
        device = torch.device(device)
        if device.type != 'cuda':
            raise RuntimeError("GroundTruth on %s: the itr_amd ops only run on the GPU (no CPU fallback)" % device)
        ip, ic, cp, ci = ground_truth_csr(pairs, n_images, n_captions)
        self.n_images, self.n_captions, self.nnz, self.device = int(n_images), int(n_captions), int(ic.shape[0]), device
        self.img_ptr_host, self.cap_ptr_host = ip, cp
        self.img_ptr, self.img_cap, self.cap_ptr, self.cap_img = (
            h2d(a, device) if a.size else torch.zeros(0, device=device, dtype=torch.int32) for a in (ip, ic, cp, ci))

    @classmethod
    def from_layout(cls, n_images, n_captions, im_div, device):
        """The relation of the reference's layout: caption j belongs to image j // im_div (captions past the last image: to none)."""
        if int(im_div) < 1:
            raise ValueError("GroundTruth.from_layout: im_div must be >= 1, got %r" % (im_div,))
        cap = np.arange(int(n_captions), dtype=np.int64)
        img = cap // int(im_div)
        keep = img < int(n_images)
        return cls(np.stack([img[keep], cap[keep]], 1), n_images, n_captions, device)


class RankPositionsState:
    """Keys and accumulators of a row-block sweep (`rank_gather_keys`, then `rank_positions`): uint64-as-int64 [nnz] keys of both
    orders, int32 [nnz] positions."""

    def __init__(self, gt):
        z = lambda dt: torch.zeros(gt.nnz, device=gt.device, dtype=dt)       # noqa: E731
        self.gt = gt
        self.i2t_key, self.t2i_key, self.i2t_pos, self.t2i_pos = z(torch.int64), z(torch.int64), z(torch.int32), z(torch.int32)


def _rank_gt_block(who, S, gt, row0, state):
    if not isinstance(gt, GroundTruth):
        raise TypeError("%s: gt must be an ops.GroundTruth" % who)
    if not torch.is_tensor(S):
        raise TypeError("S must be a torch tensor")
    if S.dim() != 2:
        raise ValueError("%s: S must be 2-D, got shape %s" % (who, tuple(S.shape)))
    if S.dtype not in (torch.float32, torch.float64):
        raise TypeError("S must be torch.float32 or torch.float64, got %s" % S.dtype)
    S_ = _dev_view(S, S.dtype)
    if S_.device != gt.device:
        raise ValueError("%s: S is on %s, the relation on %s" % (who, S_.device, gt.device))
    row0 = int(row0)
    n, Nc = S_.shape
    if Nc != gt.n_captions or row0 < 0 or row0 + n > gt.n_images:
        raise ValueError("%s: S holds rows %d .. %d of %d columns, the relation is over %d images x %d captions"
                         % (who, row0, row0 + n - 1, Nc, gt.n_images, gt.n_captions))
    if state is not None and not (isinstance(state, RankPositionsState) and state.gt is gt):
        raise ValueError("%s: state must be the RankPositionsState of this relation's sweep" % who)
    if S_.dtype == torch.float64 and (state is not None or row0 != 0 or n != gt.n_images):
        raise ValueError("%s: a float64 matrix is ranked whole (row0 = 0, every row, no state)" % who)
    return S_, row0, n, Nc


def rank_gather_keys(S_block, gt, row0=0, state=None):
    """First sweep over the row blocks of a matrix: the order keys of the positives whose row lies in this block (fp32 [n, Nc]
    holding global rows row0 .. row0 + n - 1; any row stride and alignment) go into `state` (None: a new one) -> state.  A
    caption's positives may lie in other blocks' rows, so every block is gathered before the first is counted."""
    lib = _lib.load()
    S_, row0, n, Nc = _rank_gt_block("rank_gather_keys", S_block, gt, row0, state)
    if S_.dtype == torch.float64:
        raise ValueError("rank_gather_keys: a float64 matrix is ranked whole by rank_positions")
    if state is None:
        state = RankPositionsState(gt)
    if gt.nnz and n and Nc:
        _lib.check(lib.itr_rank_gt_gather(_p(S_), S_.stride(0), row0, n, Nc, gt.n_images, gt.nnz, _p(gt.img_ptr), _p(gt.img_cap), _p(gt.cap_ptr),
                                          _p(gt.cap_img), _p(state.i2t_key), _p(state.t2i_key), _stream()))
    return state


def rank_positions(S, gt, row0=0, state=None):
    """Where do the positives of `gt` rank?  -> (i2t_pos int32 [nnz] in image-CSR order, t2i_pos int32 [nnz] in caption-CSR order,
    state): the 0-based position of every positive in its query's ranked list, in the ranker's order (larger score first, the
    higher index on an exact tie, -0.0 == +0.0, NaN as +inf) -- counted, not sorted (csrc/rank_gt.hip).
    Whole matrix (row0 = 0, every row, state None): one call gathers and counts; both outputs are final.  float64 matrices are
    ranked in float64 and only whole.
    Row blocks (fp32): sweep `rank_gather_keys` over the blocks, then this function with the same state; after the last block both
    outputs (state.i2t_pos / state.t2i_pos, returned by every call) are final, whatever the partition and the order."""
    lib = _lib.load()
    S_, row0, n, Nc = _rank_gt_block("rank_positions", S, gt, row0, state)
    whole = state is None
    if whole and not (row0 == 0 and n == gt.n_images):
        raise ValueError("rank_positions: without a state S must be the whole matrix (%d rows from row 0), got %d rows from row %d; "
                         "row blocks are gathered first (rank_gather_keys)" % (gt.n_images, n, row0))
    if whole:
        state = RankPositionsState(gt)
    if not (gt.nnz and n and Nc):
        return state.i2t_pos, state.t2i_pos, state
    f64 = S_.dtype == torch.float64
    wsb = lib.itr_rank_gt_workspace_bytes(gt.nnz, 1 if f64 else 0)
    ws = torch.empty(wsb // 8 + 1, device=gt.device, dtype=torch.int64)
    if f64:
        _lib.check(lib.itr_rank_gt_positions_f64(_p(S_), S_.stride(0), n, Nc, gt.nnz, _p(gt.img_ptr), _p(gt.img_cap), _p(gt.cap_ptr),
                                                 _p(gt.cap_img), _p(state.i2t_pos), _p(state.t2i_pos), _p(ws), wsb, _stream()))
        return state.i2t_pos, state.t2i_pos, state
    if whole:
        _lib.check(lib.itr_rank_gt_gather(_p(S_), S_.stride(0), 0, n, Nc, gt.n_images, gt.nnz, _p(gt.img_ptr), _p(gt.img_cap), _p(gt.cap_ptr),
                                          _p(gt.cap_img), _p(state.i2t_key), _p(state.t2i_key), _stream()))
    _lib.check(lib.itr_rank_gt_count(_p(S_), S_.stride(0), row0, n, Nc, gt.n_images, gt.nnz, _p(gt.img_ptr), _p(gt.cap_ptr), _p(state.i2t_key),
                                     _p(state.t2i_key), _p(state.i2t_pos), _p(state.t2i_pos), 1 if whole else 0, _p(ws), wsb, _stream()))
    return state.i2t_pos, state.t2i_pos, state


# ------------------------------------------------------------------------------------------
TOPK_MAX = 128         # ITR_TOPK_MAX (include/itr_hip.h)
TOPK_MAX_PARTS = 32    # ITR_TOPK_MAX_PARTS


def topk_lists(S, k, row0=0, rows=True, cols=True):
    """The first k entries of every row's and every column's ranked list (inds = np.argsort(...)[::-1],
    evaluation.py:169, :209) in the ranker's order: larger score first, the higher index on exact ties, -0.0 == +0.0,
    NaN as +inf.  Scores are returned with their original bits.  S: a (row block of a) similarity matrix holding global
    rows row0 .. row0 + n - 1; any row stride and alignment.
    -> (row_idx int32 [n, k], row_val [n, k], col_part), None for a direction not asked for.
    fp32: col_part = (key int64 [Nc, k], val float32 [Nc, k]), this block's partial column lists (key = ordered score << 32 |
    global row; key 0 = empty entry); `topk_merge_cols` merges the parts of several blocks / ranks into the whole-matrix lists.
    float64 (whole matrices only, row0 = 0): col_part = (col_idx int32 [Nc, k], col_val float64 [Nc, k]), already final."""
    lib = _lib.load()
    if not torch.is_tensor(S):
        raise TypeError("S must be a torch tensor")
    f64 = S.dtype == torch.float64
    if S.dim() != 2:
        raise ValueError("topk_lists: S must be 2-D, got shape %s" % (tuple(S.shape),))
    S_ = _dev_view(S, torch.float64 if f64 else torch.float32)
    n, Nc = S_.shape
    dev = S_.device
    k = int(k)
    vdt = S_.dtype
    row_idx = torch.empty(n, k, device=dev, dtype=torch.int32) if rows else None
    row_val = torch.empty(n, k, device=dev, dtype=vdt) if rows else None
    if f64:
        if row0 != 0:
            raise ValueError("topk_lists: a float64 matrix is selected whole (row0 = 0)")
        col_idx = torch.empty(Nc, k, device=dev, dtype=torch.int32) if cols else None
        col_val = torch.empty(Nc, k, device=dev, dtype=vdt) if cols else None
        _lib.check(lib.itr_topk_f64(_p(S_), S_.stride(0), n, Nc, k, _p(row_idx), _p(row_val), _p(col_idx), _p(col_val), _stream()))
        return row_idx, row_val, ((col_idx, col_val) if cols else None)
    col_key = (torch.zeros if n == 0 else torch.empty)(Nc, k, device=dev, dtype=torch.int64) if cols else None
    col_val = (torch.zeros if n == 0 else torch.empty)(Nc, k, device=dev, dtype=vdt) if cols else None
    wsb = lib.itr_topk_workspace_bytes(n, Nc, k)
    ws = torch.empty(wsb // 8 + 1, device=dev, dtype=torch.int64) if wsb else None
    _lib.check(lib.itr_topk(_p(S_), S_.stride(0), int(row0), n, Nc, k, _p(row_idx), _p(row_val), _p(col_key), _p(col_val), _p(ws), wsb,
                            _stream()))
    return row_idx, row_val, ((col_key, col_val) if cols else None)


def _dev_view(t, dtype):
    """Like _dev, but keeps a row-strided view (the kernels take ldS): no copy of a column slice of a larger matrix."""
    if not t.is_cuda:
        raise RuntimeError("S is on %s: the itr_amd ops only run on the GPU (no CPU fallback)" % t.device)
    if t.dtype != dtype:
        raise TypeError("S must be %s, got %s" % (dtype, t.dtype))
    if t.stride(1) != 1 or t.stride(0) < max(t.shape[1], 1):
        t = t.contiguous()
    return t


def topk_merge_cols(parts, k):
    """Merge the column parts of `topk_lists` (row blocks of one matrix, or ranks) into the whole-matrix lists
    -> (col_idx int32 [Nc, k] global rows, col_val [Nc, k]).  Equal to the lists of the whole matrix for every partition of
    its rows.  A float64 part is already final: one part, cut to k."""
    parts = list(parts)
    if not parts:
        raise ValueError("topk_merge_cols: no parts")
    if parts[0][1].dtype == torch.float64:
        if len(parts) != 1 or parts[0][0].shape[1] < k:
            raise ValueError("topk_merge_cols: a float64 matrix is selected whole: one part with >= k entries per column")
        idx, val = parts[0]
        return idx[:, :k].contiguous(), val[:, :k].contiguous()
    lib = _lib.load()
    keys = torch.stack([_dev(p[0], torch.int64, "part key") for p in parts], 0).contiguous()
    vals = torch.stack([_dev(p[1], torch.float32, "part val") for p in parts], 0).contiguous()
    P, Nc, k_in = keys.shape
    col_idx = torch.empty(Nc, int(k), device=keys.device, dtype=torch.int32)
    col_val = torch.empty(Nc, int(k), device=keys.device, dtype=torch.float32)
    _lib.check(lib.itr_topk_merge(_p(keys), _p(vals), P, Nc, k_in, int(k), _p(col_idx), _p(col_val), _stream()))
    return col_idx, col_val


def topk_fold_cols(S_block, k, row0=0, state=None):
    """Fold ONE row block of a similarity matrix that is never stored into running column lists (csrc/topk_fold.hip).
    S_block: fp32 [n, Nc] holding global rows row0 .. row0 + n - 1; tensor rules of `topk_lists` (GPU only, a row-strided view is
    taken as it is).  state: (key int64 [Nc, k], val float32 [Nc, k]) in the layout of `topk_lists`' column part -- None starts
    from empty lists (zeros), a part of `topk_lists` (same k) is a valid state; a given state is updated IN PLACE and returned.
    After the call the lists hold the k largest keys of (the lists before) U (this block's columns): every partition of a matrix
    into row blocks, folded in any order, gives bit for bit the lists of the whole matrix.  The block's rows must not be in the
    lists already (not checked).  `topk_merge_cols([state], k)` is the finishing step -> (col_idx, col_val)."""
    lib = _lib.load()
    if not torch.is_tensor(S_block):
        raise TypeError("S_block must be a torch tensor")
    if S_block.dim() != 2:
        raise ValueError("topk_fold_cols: S_block must be 2-D, got shape %s" % (tuple(S_block.shape),))
    S_ = _dev_view(S_block, torch.float32)
    n, Nc = S_.shape
    dev = S_.device
    k = int(k)
    if k < 1 or k > TOPK_MAX:
        raise NotImplementedError("topk_fold_cols: k = %d outside 1 .. ITR_TOPK_MAX = %d" % (k, TOPK_MAX))
    if state is None:
        state = (torch.zeros(Nc, k, device=dev, dtype=torch.int64), torch.zeros(Nc, k, device=dev, dtype=torch.float32))
    else:
        if not (isinstance(state, (tuple, list)) and len(state) == 2 and all(torch.is_tensor(t) for t in state)):
            raise ValueError("topk_fold_cols: state must be (key int64 [Nc, k], val float32 [Nc, k])")
        key, val = state
        for t, dt, nm in ((key, torch.int64, "key"), (val, torch.float32, "val")):
            if tuple(t.shape) != (Nc, k) or t.dtype != dt or t.device != dev or not t.is_contiguous():
                raise ValueError("topk_fold_cols: state %s must be a contiguous %s tensor of shape (%d, %d) on %s, got %s %s on %s"
                                 % (nm, dt, Nc, k, dev, t.dtype, tuple(t.shape), t.device))
        state = (key, val)
    if n == 0 or Nc == 0:                  # nothing to fold (an empty tensor has no address to hand to the library)
        return state
    wsb = lib.itr_topk_fold_workspace_bytes(n, Nc, k)
    ws = torch.empty(wsb // 8 + 1, device=dev, dtype=torch.int64) if wsb else None
    _lib.check(lib.itr_topk_fold_cols(_p(S_), S_.stride(0), int(row0), n, Nc, k, _p(state[0]), _p(state[1]), _p(ws), wsb, _stream()))
    return state


SEARCH_MAX_QUERIES = 64    # ITR_SEARCH_MAX_QUERIES (include/itr_hip.h)
SEARCH_MAX_SLABS = 1024    # ITR_SEARCH_MAX_SLABS


def search_topk(queries, gallery, k, row0=0, n_slabs=0):
    """The k best gallery rows of a few queries, scored and selected in one pass over the gallery (csrc/search.hip): what
    `topk_lists(cosine_scores(queries, gallery), k, cols=False)` returns, bit for bit, without the score matrix.
    queries: fp32 [Q, D], Q <= SEARCH_MAX_QUERIES (more raises NotImplementedError: callers chunk); gallery: fp32 [N, D] holding
    global rows row0 .. row0 + N - 1.  Tensor rules of `topk_lists`: GPU only, a row-strided view is taken as it is.
    -> (idx int32 [Q, k] global rows, -1 where k > N; val float32 [Q, k]; (key int64 [Q, k], val)).  The last pair is a column part
    in the layout of `topk_lists`: `topk_merge_cols` merges the parts of gallery shards into the lists of the whole gallery.
    n_slabs pins the number of gallery slabs that select independently before the merge (0: the library's choice, else
    1 .. SEARCH_MAX_SLABS); every value gives the same bytes."""
    lib = _lib.load()
    for t, nm in ((queries, "queries"), (gallery, "gallery")):
        if not torch.is_tensor(t):
            raise TypeError("search_topk: %s must be a torch tensor" % nm)
        if t.dim() != 2:
            raise ValueError("search_topk: %s must be 2-D, got shape %s" % (nm, tuple(t.shape)))
    Q_, G_ = _dev_view(queries, torch.float32), _dev_view(gallery, torch.float32)
    if Q_.device != G_.device:
        raise ValueError("search_topk: queries are on %s, the gallery on %s" % (Q_.device, G_.device))
    nq, D = Q_.shape
    N = G_.shape[0]
    if G_.shape[1] != D:
        raise ValueError("search_topk: queries have %d columns, the gallery %d" % (D, G_.shape[1]))
    k, n_slabs = int(k), int(n_slabs)
    if nq > SEARCH_MAX_QUERIES:
        raise NotImplementedError("search_topk: %d queries > ITR_SEARCH_MAX_QUERIES = %d per call: chunk the queries"
                                  % (nq, SEARCH_MAX_QUERIES))
    if k < 1 or k > TOPK_MAX:
        raise NotImplementedError("search_topk: k = %d outside 1 .. ITR_TOPK_MAX = %d" % (k, TOPK_MAX))
    dev = Q_.device
    idx = torch.empty(nq, k, device=dev, dtype=torch.int32)
    key = torch.empty(nq, k, device=dev, dtype=torch.int64)
    val = torch.empty(nq, k, device=dev, dtype=torch.float32)
    if nq == 0:
        return idx, val, (key, val)
    if D == 0:
        raise ValueError("search_topk: D must be >= 1")
    wsb = lib.itr_search_topk_workspace_bytes(nq, N, k, n_slabs)
    ws = torch.empty(wsb // 8 + 1, device=dev, dtype=torch.int64)
    _lib.check(lib.itr_search_topk(_p(Q_), Q_.stride(0), nq, _p(G_), G_.stride(0) if N else D, int(row0), N, D, k, n_slabs, _p(key), _p(val),
                                   _p(idx), _p(ws), wsb, _stream()))
    return idx, val, (key, val)


# ------------------------------------------------------------------------------------------ hubness correction (csrc/hubness.hip)
def _hub_matrix(who, S):
    """A 2-D float32 / float64 GPU matrix as the hubness kernels take it (a row-strided view is kept) -> (view, f64 flag)."""
    if not torch.is_tensor(S):
        raise TypeError("%s: S must be a torch tensor" % who)
    if S.dim() != 2:
        raise ValueError("%s: S must be 2-D, got shape %s" % (who, tuple(S.shape)))
    if S.dtype not in (torch.float32, torch.float64):
        if not S.is_cuda:
            raise RuntimeError("S is on %s: the itr_amd ops only run on the GPU (no CPU fallback)" % S.device)
        raise ValueError("%s: S must be float32 or float64, got %s" % (who, S.dtype))
    return _dev_view(S, S.dtype), int(S.dtype == torch.float64)


def _hub_beta(who, beta):
    beta = float(beta)
    if not (beta > 0.0 and np.isfinite(beta)):
        raise ValueError("%s: beta = %r is not finite and positive" % (who, beta))
    return beta


def _hub_vector(who, name, t, n, dev):
    if t is None:
        return None
    if not torch.is_tensor(t):
        raise TypeError("%s: %s must be a torch tensor" % (who, name))
    if not t.is_cuda:
        raise RuntimeError("%s is on %s: the itr_amd ops only run on the GPU (no CPU fallback)" % (name, t.device))
    if t.dtype != torch.float64 or tuple(t.shape) != (n,) or t.device != dev:
        raise ValueError("%s: %s must be a float64 tensor of shape (%d,) on %s, got %s %s on %s"
                         % (who, name, n, dev, t.dtype, tuple(t.shape), t.device))
    return t.contiguous()


def hub_lse_fold(S_block, beta, state=None, rows=True, cols=True):
    """Fold ONE row block of a score matrix into the log-sum-exp statistics of the inverted softmax (csrc/hubness.hip), one pass
    over the block for both directions.  S_block: float32 or float64 [n, Nc]; tensor rules of `topk_lists` (GPU only, a row-strided
    view is taken as it is, any alignment).  beta: finite and positive.
    -> (row_lse, state).  row_lse float64 [n] = (1 / beta) log sum_j exp(beta S[r, j]), final because a block holds whole rows
    (None with rows=False).  state float64 [Nc, 2] = per column (running sum of exp(beta x - beta m), running maximum m) over
    every block folded so far; a sum of 0 means empty, so zeros are the starting state (None starts there); a given state is
    updated IN PLACE and returned (with cols=False it is returned untouched).  `hub_lse_cols(state, beta)` is the finishing step.
    -inf entries add nothing, only -inf gives -inf, a +inf gives +inf, a NaN gives NaN (|beta S| >= 3.7e8 counts as +-inf).  No
    atomics: the same call gives the same bits; another partition of the rows sums in another order and may differ in the last
    bits."""
    who = "hub_lse_fold"
    lib = _lib.load()
    S_, f64 = _hub_matrix(who, S_block)
    beta = _hub_beta(who, beta)
    n, Nc = S_.shape
    dev = S_.device
    if state is not None:
        if not torch.is_tensor(state) or tuple(state.shape) != (Nc, 2) or state.dtype != torch.float64 or state.device != dev \
                or not state.is_contiguous():
            raise ValueError("hub_lse_fold: state must be a contiguous float64 tensor of shape (%d, 2) on %s" % (Nc, dev))
    elif cols:
        state = torch.zeros(Nc, 2, device=dev, dtype=torch.float64)
    row_lse = torch.empty(n, device=dev, dtype=torch.float64) if rows else None
    if n == 0 or Nc == 0 or not (rows or cols):
        if rows and n:
            row_lse.fill_(float('-inf'))       # a row without entries: the empty sum
        return row_lse, state
    wsb = lib.itr_hub_lse_workspace_bytes(n, Nc)
    ws = torch.empty(wsb // 8 + 1, device=dev, dtype=torch.int64)
    _lib.check(lib.itr_hub_lse_fold(_p(S_), f64, S_.stride(0), n, Nc, beta, _p(row_lse), _p(state if cols else None), _p(ws), wsb, _stream()))
    return row_lse, state


def hub_lse_cols(state, beta):
    """The finishing step of `hub_lse_fold`: state float64 [Nc, 2] -> col_lse float64 [Nc] = m + log(sum) / beta, the log-sum-exp
    of every column over all blocks folded into the state (-inf for an empty column; NaN / +inf where the state holds one).  The
    state is left as it is: more blocks may be folded after the call."""
    lib = _lib.load()
    beta = _hub_beta("hub_lse_cols", beta)
    if not torch.is_tensor(state):
        raise TypeError("hub_lse_cols: state must be a torch tensor")
    if not state.is_cuda:
        raise RuntimeError("state is on %s: the itr_amd ops only run on the GPU (no CPU fallback)" % state.device)
    if state.dim() != 2 or state.shape[1] != 2 or state.dtype != torch.float64 or not state.is_contiguous():
        raise ValueError("hub_lse_cols: state must be a contiguous float64 tensor of shape (Nc, 2)")
    Nc = state.shape[0]
    col_lse = torch.empty(Nc, device=state.device, dtype=torch.float64)
    if Nc:
        _lib.check(lib.itr_hub_lse_finish(_p(state), Nc, beta, _p(col_lse), _stream()))
    return col_lse


def hub_list_mean(vals, k):
    """The CSLS statistic of best-first lists: vals float32 or float64 [n, K] in the layout of row_val / col_val of `topk_lists`
    and `topk_merge_cols` (GPU only; a row-strided view is taken as it is) -> float64 [n], 0.5 * mean of the first k entries of
    every list, the mean being the float64 sum added best first one at a time, divided by k.  1 <= k <= K; k above TOPK_MAX is
    NotImplementedError."""
    who = "hub_list_mean"
    lib = _lib.load()
    V, f64 = _hub_matrix(who, vals)
    k = int(k)
    if k < 1:
        raise ValueError("hub_list_mean: k = %d < 1" % k)
    if k > TOPK_MAX:
        raise NotImplementedError("hub_list_mean: k = %d above ITR_TOPK_MAX = %d" % (k, TOPK_MAX))
    n, K = V.shape
    if k > K:
        raise ValueError("hub_list_mean: k = %d above the lists' length %d" % (k, K))
    out = torch.empty(n, device=V.device, dtype=torch.float64)
    if n:
        _lib.check(lib.itr_hub_list_mean(_p(V), f64, n, V.stride(0), k, _p(out), _stream()))
    return out


def hub_adjust(S, a=None, b=None, out=None):
    """The hubness-corrected matrix S'[i, j] = dtype((double(S[i, j]) - a[i]) - b[j]): two float64 subtractions, each rounded on
    its own, then the cast to the dtype of S (float32 or float64) -- numpy reproduces it bit for bit.  S: [n, Nc], tensor rules of
    `topk_lists` (GPU only, a row-strided view is taken as it is).  a float64 [n] / b float64 [Nc]: None means zeros.  a is
    constant along a row and b along a column, so the i2t order is corrected by b alone and the t2i order by a alone: one matrix
    serves both directions.  out: None allocates; `out is S` (or the same view) works in place; a tensor of the same shape and
    dtype (any row stride) that does not overlap S is written; any other overlap is refused.  -> out."""
    who = "hub_adjust"
    lib = _lib.load()
    S_, f64 = _hub_matrix(who, S)
    n, Nc = S_.shape
    dev = S_.device
    a = _hub_vector(who, "a", a, n, dev)
    b = _hub_vector(who, "b", b, Nc, dev)
    if out is None:
        out = torch.empty(n, Nc, device=dev, dtype=S_.dtype)
    else:
        if not torch.is_tensor(out) or tuple(out.shape) != (n, Nc) or out.dtype != S_.dtype or out.device != dev:
            raise ValueError("hub_adjust: out must be a %s tensor of shape (%d, %d) on %s" % (S_.dtype, n, Nc, dev))
        if Nc and n and (out.stride(1) != 1 or out.stride(0) < Nc):
            raise ValueError("hub_adjust: out must have unit column stride and a row stride >= %d" % Nc)
        if out.data_ptr() == S.data_ptr() and S_.data_ptr() != S.data_ptr():
            raise ValueError("hub_adjust: in place needs S with unit column stride")
    if n and Nc:
        _lib.check(lib.itr_hub_adjust(_p(S_), f64, S_.stride(0), n, Nc, _p(a), _p(b), _p(out), out.stride(0), _stream()))
    return out


# ------------------------------------------------------------------------------------------ candidate lists (coarse-to-fine retrieval)
# The list and pair plumbing every candidate op below shares (SCAN / SGRAF scores, SCAN / SGRAF explanations).  `who` is the public
# function the messages name.
def _caption_tables(plan, dev, max_words):
    """Device copies of ALL captions' offsets (int64) and lengths (int32) (a ScanPlan keeps only those of the captions its column
    tiles hold) -> (off, lens).  Lengths above `max_words` become 0 = "not taken by the kernel"; max_words=None: the true lengths.
    Cached on the plan per device (offsets) and per (device, max_words) (lengths)."""
    cache = getattr(plan, "_caption_tables", None)
    if cache is None:
        cache = plan._caption_tables = {}
    if (dev, 'off') not in cache:
        cache[dev, 'off'] = h2d(np.asarray(plan.off_host, dtype=np.int64), dev)
    if (dev, max_words) not in cache:
        lens = plan.len_host if max_words is None else np.where(plan.len_host > max_words, 0, plan.len_host)
        cache[dev, max_words] = h2d(np.asarray(lens, dtype=np.int32), dev)
    return cache[dev, 'off'], cache[dev, max_words]


def _check_by(who, by):
    if by not in ('caption', 'image'):
        raise ValueError("%s: by must be 'caption' or 'image', got %r" % (who, by))


def _check_lists(who, cand, by, images, plan):
    """cand is an int32 device tensor [n_q, K] with one list per caption (by='caption') or per image -> (n_q, n_t, K): the number
    of queries (lists), of targets (what a list indexes) and the list length.  Copies nothing: a view is made contiguous by the
    caller, after the shape checks."""
    if not torch.is_tensor(cand) or not cand.is_cuda or cand.dtype != torch.int32:
        _dev(cand, torch.int32, name="cand")                      # (raises)
    if cand.dim() != 2:
        raise ValueError("%s: cand must be 2-D, got shape %s" % (who, tuple(cand.shape)))
    Ni, Nc = images.shape[0], plan.Nc
    n_q, n_t = (Nc, Ni) if by == 'caption' else (Ni, Nc)
    if cand.shape[0] != n_q:
        raise ValueError("%s: by=%r needs %d lists, got %d" % (who, by, n_q, cand.shape[0]))
    return n_q, n_t, cand.shape[1]


def _check_in_range(who, idx, bound):
    """One device reduction, so that nothing out of range reaches a kernel.  bound = n: the entries of the lists `idx` lie in
    [0, n); bound = (Ni, Nc): the columns of the [P, 2] pairs `idx` lie in [0, Ni) and [0, Nc)."""
    if isinstance(bound, tuple):
        Ni, Nc = bound
        lo, hi = torch.aminmax(idx, dim=0)
        (ilo, clo), (ihi, chi) = lo.tolist(), hi.tolist()
        if ilo < 0 or ihi >= Ni or clo < 0 or chi >= Nc:
            raise ValueError("%s: pair index out of range: images [%d, %d] of %d, captions [%d, %d] of %d" % (who, ilo, ihi, Ni, clo, chi, Nc))
    else:
        lo, hi = torch.aminmax(idx)
        lo, hi = int(lo), int(hi)
        if lo < 0 or hi >= bound:
            raise ValueError("%s: candidate index out of range [0, %d): min %d, max %d" % (who, bound, lo, hi))


def _lists_to_pairs(who, cand, by, n_q, m):
    """The first `m` columns of every list (all of them when m is None) as int32 [n_q m, 2] (image, caption) pairs: pair q * m + k
    is list q's entry k."""
    m = cand.shape[1] if m is None else int(m)
    if m < 0 or m > cand.shape[1]:
        raise ValueError("%s: m = %d outside [0, %d]" % (who, m, cand.shape[1]))
    flat = cand[:, :m].reshape(-1)
    qid = torch.arange(n_q, device=cand.device, dtype=torch.int32).repeat_interleave(m)
    return torch.stack((flat, qid) if by == 'caption' else (qid, flat), 1)


def _flat_pairs(cand, by, n_q, K):
    """Lists -> (caps, imgs, slot), int64 [n_q K] on the lists' device: the caption and the image of every entry, and its place in
    the flattened result."""
    flat = cand.reshape(-1).to(torch.int64)
    qid = torch.arange(n_q, device=cand.device, dtype=torch.int64).repeat_interleave(K)
    caps, imgs = (qid, flat) if by == 'caption' else (flat, qid)
    return caps, imgs, torch.arange(n_q * K, device=cand.device, dtype=torch.int64)


def _group_pairs(key, n_keys, cols, grouped):
    """Pairs -> CSR form by `key` (int64 [P], values in [0, n_keys)): -> (ptr int32 [n_keys + 1], key, *cols) with the pairs of key
    j at ptr[j] .. ptr[j + 1], in their incoming order (stable sort), and `cols` (tensors [P]) carried along.  grouped=True: the
    caller knows the keys already ascend (lists flattened by their own query), no sort is launched.  No pairs: only the zero
    pointer is made.  Works on host tensors too."""
    if key.numel() and not grouped:
        key, order = torch.sort(key, stable=True)
        cols = [c[order] for c in cols]
    ptr = torch.zeros(n_keys + 1, device=key.device, dtype=torch.int32)
    if key.numel():
        ptr[1:] = torch.cumsum(torch.bincount(key, minlength=n_keys), 0).to(torch.int32)
    return (ptr, key) + tuple(cols)


def _long_caption_pairs(images, words, plan, lm, caps, imgs, slot, out, make_col):
    """The listed pairs of captions too long for a pair kernel (mask `lm` over the pairs) are scored one caption at a time on that
    caption's listed images and scattered into `out`'s slots: make_col() -> col(images [n, R, D], words [l, D], l) -> the n scores.
    It is called only when there are such pairs.  -> (caps, imgs, slot) of the other pairs."""
    lcaps, limgs, lslot = caps[lm], imgs[lm], slot[lm]
    if lcaps.numel():
        col = make_col()
        flat = out.view(-1)
        with torch.no_grad():
            for c in torch.unique(lcaps).tolist():
                m = lcaps == c
                sel, inv = torch.unique(limgs[m], return_inverse=True)
                o, l = int(plan.off_host[c]), int(plan.len_host[c])
                flat[lslot[m]] = col(images[sel].contiguous(), words[o:o + l].contiguous(), l).reshape(-1)[inv]
    return caps[~lm], imgs[~lm], slot[~lm]


def _sgraf_item_plan(lib, img_ptr, pair_cap, off, klen, P, Ni, Nc, n_rows, dev):
    """itr_sgraf_pairs_plan on image-major pairs -> (pair_len, pair_col, pair_capok, item_begin, item_img) int32 on the device,
    n_items, and item_begin[:n_items + 1] on the host (int64): the chunk bounds need it, the plan's one read-back."""
    pair_len, pair_col, pair_capok = (torch.empty(P, device=dev, dtype=torch.int32) for _ in range(3))
    item_begin = torch.empty(P + 1, device=dev, dtype=torch.int32)
    item_img = torch.empty(P, device=dev, dtype=torch.int32)
    n_items_dev = torch.zeros(1, device=dev, dtype=torch.int32)
    pwb = lib.itr_sgraf_pairs_plan_workspace_bytes(Ni)
    pws = torch.empty(max(pwb, 1), device=dev, dtype=torch.uint8)
    _lib.check(lib.itr_sgraf_pairs_plan(_p(img_ptr), _p(pair_cap), _p(off), _p(klen), P, Ni, Nc, n_rows, _p(pair_len), _p(pair_col),
                                        _p(pair_capok), _p(item_begin), _p(item_img), _p(n_items_dev), _p(pws), pwb, _stream()))
    n_items = int(n_items_dev)
    return (pair_len, pair_col, pair_capok, item_begin, item_img), n_items, item_begin[:n_items + 1].cpu().numpy().astype(np.int64)


def _workspace_budget(dev, max_workspace_bytes):
    """The bytes a chunk's workspace may take: the caller's limit, or 90 % of the device's free + cached memory"""
    if max_workspace_bytes is not None:
        return int(max_workspace_bytes)
    free, _total = torch.cuda.mem_get_info(dev)
    cached = torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
    return int(0.9 * (free + cached))


def _chunks_within(who, need, n_items, budget):
    """[0, n_items) cut into the fewest chunks (it0, it1) of whole items with need(it0, it1) <= budget bytes, every chunk as long as
    fits; `need` is monotone in it1.  Host arithmetic only.  An item that does not fit alone: torch.cuda.OutOfMemoryError."""
    chunks, it0 = [], 0
    while it0 < n_items:
        if need(it0, it0 + 1) > budget:
            raise torch.cuda.OutOfMemoryError("%s: one item needs %d bytes of workspace, %d allowed" % (who, need(it0, it0 + 1), budget))
        lo, hi = it0 + 1, n_items                               # the largest it1 whose chunk fits
        while lo < hi:
            mid = (lo + hi + 1) // 2
            if need(it0, mid) <= budget:
                lo = mid
            else:
                hi = mid - 1
        chunks.append((it0, lo))
        it0 = lo
    return chunks


class _PairBlocks:
    """What ScanPairAttention and SgrafPairAttention share: the pair count and the bounds-checked host view of a block pointer"""

    def __len__(self):
        return self.score.shape[0]

    def _pair(self, p):
        p = int(p)
        if not 0 <= p < len(self):
            raise IndexError("pair %d of %d" % (p, len(self)))
        return p

    def _span(self, name, p):
        """(begin, end) of pair p in the flat tensor that the pointer `name` indexes; the pointer is read back once"""
        p = self._pair(p)
        if name not in self._host:
            self._host[name] = getattr(self, name).cpu().numpy()
        ptr = self._host[name]
        return int(ptr[p]), int(ptr[p + 1])


class ScanPairsWorkspace:
    """What `scan_pairs_prepare` computed and for what: the buffer, the cross-attention direction, and the identity of the
    operands (shapes, device pointers, the plan).  `scan_candidate_scores` refuses a workspace prepared for anything else -- its
    byte size alone would not tell a t2i workspace from an i2t one."""

    def __init__(self, buf, cross_attn, images, words, plan):
        self.buf, self.cross_attn, self.plan = buf, cross_attn, plan
        self.key = self._key(images, words)

    @staticmethod
    def _key(images, words):
        return (tuple(images.shape), tuple(words.shape), images.data_ptr(), words.data_ptr(), images._version, words._version)

    def check(self, cross_attn, images, words, plan):
        if self.cross_attn != cross_attn:
            raise ValueError("scan_candidate_scores: workspace was prepared for cross_attn=%r, called with %r" % (self.cross_attn, cross_attn))
        if self.plan is not plan or self.key != self._key(images, words):
            raise ValueError("scan_candidate_scores: workspace was prepared for other images, words or plan (or they were modified since)")


def scan_pairs_prepare(images, words, plan, cross_attn='t2i'):
    """Per image set / caption set precompute of `scan_candidate_scores` (region Gram matrices and word norms for t2i; region
    norms and caption Gram matrices for i2t): once per image and caption, never per pair.  -> ScanPairsWorkspace, valid for these
    images, words, plan and cross_attn only."""
    lib = _lib.load()
    if cross_attn not in ('t2i', 'i2t'):
        raise ValueError("unknown cross_attn: %r" % (cross_attn,))
    images = _dev(images, name="images")
    words = _dev(words, name="words")
    Ni, R, D = images.shape
    if R != SCAN_R:
        raise NotImplementedError("scan_pairs_prepare: %d regions per image (the pair kernel is built for %d)" % (R, SCAN_R))
    mode = 0 if cross_attn == 't2i' else 1
    off, klen = _caption_tables(plan, images.device, SCAN_NT)
    wsb = lib.itr_scan_pairs_workspace_bytes(Ni, R, words.shape[0], plan.Nc, mode)
    ws = torch.empty(max(wsb, 1), device=images.device, dtype=torch.uint8)
    _lib.check(lib.itr_scan_pairs_prepare(_p(images), _p(words), _p(off), _p(klen), Ni, plan.Nc, words.shape[0], R, D, mode, _p(ws), wsb,
                                          _stream()))
    return ScanPairsWorkspace(ws, cross_attn, images, words, plan)


def scan_candidate_scores(images, words, plan, cand, by, cross_attn='t2i', raw_feature_norm='clipped_l2norm', agg_func='LogSumExp',
                          lambda_lse=6.0, lambda_softmax=9.0, workspace=None):
    """SCAN scores (xattn_score_t2i / _i2t, Objectives.py:329-417) of candidate lists only -- the fine stage of coarse-to-fine
    retrieval.  With S the matrix `scan_xattn_scores` would return:
      by='caption': cand int32 [Nc, K] image indices   -> [Nc, K], out[c, k] = S[cand[c, k], c]
      by='image':   cand int32 [Ni, K] caption indices -> [Ni, K], out[i, k] = S[i, cand[i, k]]
    Only the listed pairs are computed (csrc/scan_pairs.hip), each to the same bits whatever else is listed.  Duplicates inside
    a list are allowed; any K >= 1; an empty dimension gives an empty result.  Captions of 65..96 words are scored by the pair
    path of the training kernels on their listed images (correct, not fast).  `workspace`: scan_pairs_prepare's, to reuse it."""
    lib = _lib.load()
    if cross_attn not in ('t2i', 'i2t'):
        raise ValueError("unknown first norm type:", raw_feature_norm)      # (the reference's message for a bad cross_attn: kept)
    if raw_feature_norm not in _NORMS:
        raise ValueError("unknown first norm type:", raw_feature_norm)
    if agg_func not in _AGGS:
        raise ValueError("unknown aggfunc: {}".format(agg_func))
    _check_by("scan_candidate_scores", by)
    images = _dev(images, name="images")
    words = _dev(words, name="words")
    n_q, n_t, K = _check_lists("scan_candidate_scores", cand, by, images, plan)
    cand = cand.contiguous()
    Ni, R, D = images.shape
    Nc = plan.Nc
    dev = images.device
    out = torch.empty(n_q, K, device=dev, dtype=torch.float32)
    if n_q == 0 or K == 0:                                        # (before `workspace` is looked at, unlike the ops below: kept)
        return out
    if R != SCAN_R:
        raise NotImplementedError("scan_candidate_scores: %d regions per image (the pair kernel is built for %d)" % (R, SCAN_R))
    if len(plan.len_host) and int(plan.len_host.max()) > SCAN_PAIR_MAXW:
        raise NotImplementedError("scan_candidate_scores: captions of %d words (supported: <= %d)" % (int(plan.len_host.max()), SCAN_PAIR_MAXW))
    _check_in_range("scan_candidate_scores", cand, n_t)
    if n_q * K >= 2 ** 31:
        raise NotImplementedError("scan_candidate_scores: %d pairs; split the lists" % (n_q * K))
    # ---- caption-major (CSR) form, on the device: no dense intermediate
    caps, imgs, slot = _flat_pairs(cand, by, n_q, K)
    if plan.long_idx is not None:
        is_long = torch.zeros(Nc, device=dev, dtype=torch.bool)
        is_long[h2d(plan.long_idx, dev)] = True
        caps, imgs, slot = _long_caption_pairs(images, words, plan, is_long[caps], caps, imgs, slot, out,
                                               lambda: _scan_long_caption_col(cross_attn, raw_feature_norm, agg_func, lambda_lse, lambda_softmax))
    P = caps.numel()
    if P == 0:
        return out
    cap_ptr, caps, imgs, slot = _group_pairs(caps, Nc, (imgs, slot), grouped=by == 'caption')
    pair_img, pair_out = imgs.to(torch.int32), slot.to(torch.int32)
    mode = 0 if cross_attn == 't2i' else 1
    off, klen = _caption_tables(plan, dev, SCAN_NT)
    if workspace is not None:
        if not isinstance(workspace, ScanPairsWorkspace):
            raise TypeError("scan_candidate_scores: workspace must come from scan_pairs_prepare")
        workspace.check(cross_attn, images, words, plan)
    ws = (workspace if workspace is not None else scan_pairs_prepare(images, words, plan, cross_attn)).buf
    _lib.check(lib.itr_scan_pair_scores(
        _p(images), _p(words), _p(off), _p(klen), _p(cap_ptr), _p(pair_img), _p(pair_out), P, Ni, Nc, words.shape[0], R, D, mode,
        _NORMS[raw_feature_norm], _AGGS[agg_func], float(lambda_softmax), float(lambda_lse), _p(out), out.numel(), _p(ws), ws.numel(),
        _stream()))
    return out


# ------------------------------------------------------------------------------------------ SCAN attention maps of listed pairs
class ScanPairAttention(_PairBlocks):
    """What `scan_pair_attention` returns for P pairs: `attn` float32 (flat; pair p holds its [W_p, 36] row-major block at
    attn_ptr[p]), `attn_ptr` int64 [P + 1], `row_sim` float32 (t2i: W_p cosines per pair at row_ptr[p]; i2t: 36 per pair at
    36 p), `row_ptr` int64 [P + 1], `score` float32 [P], `cap_len` int32 [P] (W_p), all on the device, and `pairs` int32 [P, 2]."""

    def __init__(self, pairs, attn, attn_ptr, row_sim, row_ptr, score, cap_len, cross_attn):
        self.pairs, self.attn, self.attn_ptr, self.row_sim, self.row_ptr = pairs, attn, attn_ptr, row_sim, row_ptr
        self.score, self.cap_len, self.cross_attn = score, cap_len, cross_attn
        self._host = {}

    def matrix(self, p):
        """the [W, R] attention matrix of pair p (a view): word-major, t2i rows / i2t columns sum to 1"""
        b, e = self._span('attn_ptr', p)
        return self.attn[b:e].view(-1, SCAN_R)

    def sims(self, p):
        """the cosine similarities pair p's score is aggregated from: one per word (t2i) or per region (i2t)"""
        if self.cross_attn == 'i2t':
            p = self._pair(p)
            return self.row_sim[p * SCAN_R:(p + 1) * SCAN_R]
        b, e = self._span('attn_ptr', p)
        return self.row_sim[b // SCAN_R:e // SCAN_R]


def scan_pair_attention(images, words, plan, pairs, cross_attn='t2i', raw_feature_norm='clipped_l2norm', agg_func='LogSumExp',
                        lambda_lse=6.0, lambda_softmax=9.0, workspace=None):
    """The attention matrices SCAN's scores are aggregated from (func_attention's second result, Objectives.py:421-476; its
    callers xattn_score_t2i / _i2t :350 / :398), the per-word / per-region cosines and the scores of LISTED pairs:
    pairs int32 [P, 2] of (image, caption), in any order, duplicates allowed -> ScanPairAttention (csrc/scan_attn.hip).  Every
    pair's outputs are the same bits whatever else is listed.  Captions of 1..96 words, 36 regions.  Argument checks and
    `workspace` (scan_pairs_prepare's) as scan_candidate_scores."""
    lib = _lib.load()
    if cross_attn not in ('t2i', 'i2t'):
        raise ValueError("unknown first norm type:", raw_feature_norm)      # (the reference's message for a bad cross_attn: kept)
    if raw_feature_norm not in _NORMS:
        raise ValueError("unknown first norm type:", raw_feature_norm)
    if agg_func not in _AGGS:
        raise ValueError("unknown aggfunc: {}".format(agg_func))
    images = _dev(images, name="images")
    words = _dev(words, name="words")
    pairs = _dev(pairs, torch.int32, name="pairs")
    if pairs.dim() != 2 or pairs.shape[1] != 2:
        raise ValueError("scan_pair_attention: pairs must be [P, 2] of (image, caption), got shape %s" % (tuple(pairs.shape),))
    Ni, R, D = images.shape
    Nc = plan.Nc
    dev = images.device
    P = pairs.shape[0]
    mode = 0 if cross_attn == 't2i' else 1
    if workspace is not None:
        if not isinstance(workspace, ScanPairsWorkspace):
            raise TypeError("scan_pair_attention: workspace must come from scan_pairs_prepare")
        workspace.check(cross_attn, images, words, plan)
    if P == 0:
        z64 = torch.zeros(1, device=dev, dtype=torch.int64)
        f = lambda: torch.empty(0, device=dev, dtype=torch.float32)
        return ScanPairAttention(pairs, f(), z64, f(), z64.clone(), f(), torch.empty(0, device=dev, dtype=torch.int32), cross_attn)
    if R != SCAN_R:
        raise NotImplementedError("scan_pair_attention: %d regions per image (the pair kernel is built for %d)" % (R, SCAN_R))
    if len(plan.len_host) and int(plan.len_host.max()) > SCAN_PAIR_MAXW:
        raise NotImplementedError("scan_pair_attention: captions of %d words (supported: <= %d)" % (int(plan.len_host.max()), SCAN_PAIR_MAXW))
    if P * SCAN_PAIR_MAXW * SCAN_R >= 2 ** 31:
        raise NotImplementedError("scan_pair_attention: %d pairs; split the list" % P)
    _check_in_range("scan_pair_attention", pairs, (Ni, Nc))
    off, lens = _caption_tables(plan, dev, None)
    pair_img, pair_cap = pairs[:, 0].contiguous(), pairs[:, 1].contiguous()
    cap_len = lens[pair_cap.long()]
    row_ptr = torch.zeros(P + 1, device=dev, dtype=torch.int64)
    row_ptr[1:] = torch.cumsum(cap_len, 0, dtype=torch.int64)
    attn_ptr = row_ptr * SCAN_R
    n_words = int(row_ptr[-1])
    attn = torch.empty(n_words * SCAN_R, device=dev, dtype=torch.float32)
    row_sim = torch.empty(n_words if mode == 0 else P * SCAN_R, device=dev, dtype=torch.float32)
    score = torch.empty(P, device=dev, dtype=torch.float32)
    ws = (workspace if workspace is not None else scan_pairs_prepare(images, words, plan, cross_attn)).buf
    _lib.check(lib.itr_scan_pair_attention(
        _p(images), _p(words), _p(off), _p(lens), _p(pair_img), _p(pair_cap), P, Ni, Nc, words.shape[0], R, D, mode,
        _NORMS[raw_feature_norm], _AGGS[agg_func], float(lambda_softmax), float(lambda_lse), _p(attn), _p(attn_ptr), attn.numel(),
        _p(row_sim), _p(row_ptr), row_sim.numel(), _p(score), _p(ws), ws.numel(), _stream()))
    return ScanPairAttention(pairs, attn, attn_ptr, row_sim, row_ptr, score, cap_len, cross_attn)


def scan_candidate_attention(images, words, plan, cand, by, m=None, **kw):
    """`scan_pair_attention` for candidate lists, `cand` and `by` as in scan_candidate_scores: explains the first `m` columns of
    every list (all of them when m is None) -> ScanPairAttention whose pair q * m + k is list q's entry k."""
    _check_by("scan_candidate_attention", by)
    n_q, _, _ = _check_lists("scan_candidate_attention", cand, by, images, plan)
    pairs = _lists_to_pairs("scan_candidate_attention", cand.contiguous(), by, n_q, m)
    return scan_pair_attention(images, words, plan, pairs, **kw)


# ------------------------------------------------------------------------------------------ SGRAF on candidate lists
class SgrafPairsState:
    """What `sgraf_pairs_prepare` computed and for what: the buffer (VisualSA / TextSA global vectors, the images' Gram matrices, SGR's
    folded and packed weights) and the identity of the operands, the weights and the module.  `sgraf_candidate_scores` refuses a state
    prepared for anything else.  The weights are identified by the CALLER's tensors (storage pointer and version counter of every
    state_dict entry the module reads), so a state is reusable with the same dict -- or another dict of the same tensors, such as a
    second `module.state_dict()` -- whatever copies the binding has to make of them."""

    def __init__(self, buf, images, words, plan, weights, module_name, sgr_step, struct, keep, S_dim):
        self.buf, self.plan, self.module_name, self.sgr_step = buf, plan, module_name, int(sgr_step)
        self.struct, self.keep, self.S_dim = struct, keep, S_dim
        self.key = self._key(images, words, weights, module_name, sgr_step)

    @staticmethod
    def _key(images, words, weights, module_name, sgr_step):
        return ((tuple(images.shape), tuple(words.shape), images.data_ptr(), words.data_ptr(), images._version, words._version),
                tuple((weights[n].data_ptr(), weights[n]._version, tuple(weights[n].shape)) for n in _sgraf_weight_names(module_name, int(sgr_step))))

    def check(self, images, words, plan, weights, module_name, sgr_step):
        if self.module_name != module_name or (module_name == 'SGR' and self.sgr_step != int(sgr_step)):
            raise ValueError("sgraf_candidate_scores: state was prepared for module %r (%d steps), called with %r (%d steps)"
                             % (self.module_name, self.sgr_step, module_name, int(sgr_step)))
        if self.plan is not plan or self.key != self._key(images, words, weights, module_name, sgr_step):
            raise ValueError("sgraf_candidate_scores: state was prepared for other images, words, plan or weights (or they were modified since)")


def sgraf_pairs_prepare(images, words, plan, weights, module_name='SAF', sgr_step=3):
    """Per image set / caption set / weights precompute of `sgraf_candidate_scores`: once per image and caption, never per pair or per
    chunk.  -> SgrafPairsState, valid for these images, words, plan, weights and module only."""
    lib = _lib.load()
    if module_name not in ('SAF', 'SGR'):
        raise ValueError('Invalid input of config.module_name in configs.py')
    images = _dev(images, name="images")
    words = _dev(words, name="words")
    Ni, R, D = images.shape
    if R != SCAN_R:
        raise NotImplementedError("sgraf_pairs_prepare: %d regions per image (VisualSA is built for %d)" % (R, SCAN_R))
    if plan.Nc and int(plan.len_host.max()) > SGRAF_COMPOSED_MAX_WORDS:
        raise NotImplementedError("sgraf_candidate_scores: captions of at most %d words are supported" % SGRAF_COMPOSED_MAX_WORDS)
    st, keep, S_dim = _sgraf_weight_struct(weights, module_name, sgr_step)
    mod = 0 if module_name == 'SAF' else 1
    off, klen = _caption_tables(plan, images.device, SGRAF_MAX_WORDS)
    nb = lib.itr_sgraf_pairs_state_bytes(Ni, plan.Nc, words.shape[0], D, S_dim, mod, int(sgr_step))
    buf = torch.empty(max(nb, 1), device=images.device, dtype=torch.uint8)
    sb = lib.itr_sgraf_pairs_prepare_scratch_bytes(Ni, plan.Nc, words.shape[0], D, S_dim, mod)
    scratch = torch.empty(max(sb, 1), device=images.device, dtype=torch.uint8)       # the global nodes' intermediates: freed on return
    _lib.check(lib.itr_sgraf_pairs_prepare(_p(images), _p(words), _p(off), _p(klen), Ni, plan.Nc, words.shape[0], R, D, S_dim, mod, int(sgr_step),
                                           C.byref(st), _p(buf), nb, _p(scratch), sb, _stream()))
    del scratch
    return SgrafPairsState(buf, images, words, plan, weights, module_name, sgr_step, st, keep, S_dim)


SGRAF_PAIRS_LAST = {}          # diagnostics: chunks, items and workspace of the last sgraf_candidate_scores call


def sgraf_candidate_scores(images, words, plan, weights, cand, by, module_name='SAF', sgr_step=3, max_workspace_bytes=None, state=None):
    """SGRAF scores (EncoderSimilarity.forward, Fusionmodule.py:406-451, eval mode) of candidate lists only -- the fine stage of
    coarse-to-fine retrieval.  With S the matrix `sgraf_scores` would return:
      by='caption': cand int32 [Nc, K] image indices   -> [Nc, K], out[c, k] = S[cand[c, k], c]
      by='image':   cand int32 [Ni, K] caption indices -> [Ni, K], out[i, k] = S[i, cand[i, k]]
    Only the listed pairs are computed (csrc/sgraf_pairs.hip), each to the same bits whatever else is listed, in any order, at any K,
    through either `by`, under any workspace budget.  Duplicates inside a list are allowed; any K >= 1; an empty dimension gives an
    empty result.  Captions of 64..191 words are scored by the per-caption composition of the training path on their listed images
    (correct, not fast).  The pairs are processed in chunks sized to `max_workspace_bytes` (default: 90 % of free + cached device
    memory).  `state`: sgraf_pairs_prepare's, to reuse the per-image / per-caption work across calls (both list directions).
    Pairs per call: the contract's refusal is at 2^31; the item plan indexes columns as 64 x item in int32, so lists of 2^31 / 64 =
    33 554 432 pairs or more are refused as well (NotImplementedError: split the lists)."""
    lib = _lib.load()
    if module_name not in ('SAF', 'SGR'):
        raise ValueError('Invalid input of config.module_name in configs.py')
    _check_by("sgraf_candidate_scores", by)
    images = _dev(images, name="images")
    words = _dev(words, name="words")
    n_q, n_t, K = _check_lists("sgraf_candidate_scores", cand, by, images, plan)
    Ni, R, D = images.shape
    Nc = plan.Nc
    dev = images.device
    if n_q * K >= 2 ** 31 // 64:
        raise NotImplementedError("sgraf_candidate_scores: %d pairs (at most %d per call); split the lists" % (n_q * K, 2 ** 31 // 64 - 1))
    cand = cand.contiguous()
    out = torch.empty(n_q, K, device=dev, dtype=torch.float32)
    if state is not None:
        if not isinstance(state, SgrafPairsState):
            raise TypeError("sgraf_candidate_scores: state must come from sgraf_pairs_prepare")
        state.check(images, words, plan, weights, module_name, sgr_step)
    if n_q == 0 or K == 0:
        return out
    if R != SCAN_R:
        raise NotImplementedError("sgraf_candidate_scores: %d regions per image (VisualSA is built for %d)" % (R, SCAN_R))
    if len(plan.len_host) and int(plan.len_host.max()) > SGRAF_COMPOSED_MAX_WORDS:
        raise NotImplementedError("sgraf_candidate_scores: captions of at most %d words are supported" % SGRAF_COMPOSED_MAX_WORDS)
    _check_in_range("sgraf_candidate_scores", cand, n_t)
    if state is None:
        state = sgraf_pairs_prepare(images, words, plan, weights, module_name, sgr_step)
    S_dim, st = state.S_dim, state.struct
    mod = 0 if module_name == 'SAF' else 1
    # ---- image-major (CSR) form, on the device: no dense intermediate
    caps, imgs, slot = _flat_pairs(cand, by, n_q, K)
    if len(plan.len_host) and int(plan.len_host.max()) > SGRAF_MAX_WORDS:
        is_long = h2d(plan.len_host > SGRAF_MAX_WORDS, dev)
        caps, imgs, slot = _long_caption_pairs(images, words, plan, is_long[caps], caps, imgs, slot, out,
                                               lambda: _sgraf_long_caption_col(images, weights, module_name, sgr_step, S_dim))
    P = caps.numel()
    if P == 0:
        return out
    img_ptr, imgs, caps, slot = _group_pairs(imgs, Ni, (caps, slot), grouped=by == 'image')
    pair_img, pair_cap, pair_out = imgs.to(torch.int32), caps.to(torch.int32), slot.to(torch.int32)
    off, klen = _caption_tables(plan, dev, SGRAF_MAX_WORDS)
    (pair_len, pair_col, pair_capok, item_begin, item_img), n_items, ib = _sgraf_item_plan(lib, img_ptr, pair_cap, off, klen, P, Ni, Nc,
                                                                                          words.shape[0], dev)
    # ---- chunks of whole items sized to the budget
    budget = _workspace_budget(dev, max_workspace_bytes)

    def need(it0, it1):
        return lib.itr_sgraf_pair_scores_workspace_bytes(int(ib[it1] - ib[it0]), it1 - it0, D, S_dim, mod, int(sgr_step))

    chunks = _chunks_within("sgraf_candidate_scores", need, n_items, budget)
    wsb = max(need(a, b) for a, b in chunks)
    ws = torch.empty(wsb, device=dev, dtype=torch.uint8)
    # (written only here: an early return above leaves the previous call's figures, unlike SGRAF_ATTN_LAST: kept)
    SGRAF_PAIRS_LAST.update(pairs=P, items=n_items, chunks=len(chunks), workspace_bytes=int(wsb), budget_bytes=budget)
    for a, b in chunks:
        _lib.check(lib.itr_sgraf_pair_scores(_p(images), _p(words), _p(off), _p(pair_img), _p(pair_capok), _p(pair_len), _p(pair_col), _p(pair_out),
                                             _p(item_begin), _p(item_img), int(ib[a]), int(ib[b] - ib[a]), a, b - a, Ni, Nc, words.shape[0], R, D,
                                             S_dim, mod, int(sgr_step), C.byref(st), _p(state.buf), state.buf.numel(), _p(out), out.numel(),
                                             _p(ws), wsb, _stream()))
    return out


# ------------------------------------------------------------------------------------------ SGRAF reasoning maps of listed pairs
SGRAF_ATTN_MAX_SIM_DIM = 256   # csrc/sgraf_attn.hip keeps an item's node rows on chip


class SgrafPairAttention(_PairBlocks):
    """What `sgraf_pair_attention` returns for P pairs, all on the device, in the caller's order.  Pair p has W_p words and
    n_p = W_p + 1 alignment nodes; NODE 0 IS THE GLOBAL NODE, node 1 + w is word w.
      attn / attn_ptr     float32 flat / int64 [P + 1]: the [W_p, 36] row-major SCAN_attention weights (rows sum to 1)
      node_w / node_ptr   SAF only: AttentionFiltration's n_p weights (sum to 1); None for SGR
      edge / edge_ptr     SGR only: GraphReasoning's [sgr_step, n_p, n_p] edges (rows sum to 1); None for SAF
      score float32 [P], cap_len int32 [P] (W_p), explained bool [P], pairs int32 [P, 2].
    A caption of more than 63 words has its score and explained[p] False: its blocks have length 0."""

    def __init__(self, pairs, attn, attn_ptr, node_w, node_ptr, edge, edge_ptr, score, cap_len, explained, module_name, sgr_step):
        self.pairs, self.attn, self.attn_ptr, self.node_w, self.node_ptr = pairs, attn, attn_ptr, node_w, node_ptr
        self.edge, self.edge_ptr, self.score, self.cap_len, self.explained = edge, edge_ptr, score, cap_len, explained
        self.module_name, self.sgr_step = module_name, int(sgr_step)
        self._host = {}

    def matrix(self, p):
        """the [W, 36] word x region attention of pair p (a view); [0, 36] for a pair that is not explained"""
        b, e = self._span('attn_ptr', p)
        return self.attn[b:e].view(-1, SCAN_R)

    def nodes(self, p):
        """SAF: the filtration weights of pair p's W + 1 nodes (a view), the global node first"""
        if self.node_w is None:
            raise ValueError("nodes: filtration weights exist for module SAF, this is %s" % self.module_name)
        b, e = self._span('node_ptr', p)
        return self.node_w[b:e]

    def edges(self, p):
        """SGR: the [sgr_step, W + 1, W + 1] graph edges of pair p (a view), row = querying node"""
        if self.edge is None:
            raise ValueError("edges: graph edges exist for module SGR, this is %s" % self.module_name)
        b, e = self._span('edge_ptr', p)
        n = int(round(((e - b) / max(self.sgr_step, 1)) ** 0.5))
        return self.edge[b:e].view(self.sgr_step, n, n)


SGRAF_ATTN_LAST = {}           # diagnostics: chunks, items and workspace of the last sgraf_pair_attention call


def sgraf_pair_attention(images, words, plan, weights, pairs, module_name='SAF', sgr_step=3, state=None, max_workspace_bytes=None):
    """Why SGRAF scored LISTED pairs as it did: pairs int32 [P, 2] of (image, caption) in any order, duplicates allowed ->
    SgrafPairAttention with SCAN_attention's word x region weights (Fusionmodule.py:632-664), SAF's filtration weights over the
    alignment nodes (:615-619) or SGR's graph edges at every step (:581-587), and the scores (:406-451) (csrc/sgraf_attn.hip).
    The pairs are regrouped image-major on the device as in sgraf_candidate_scores and the results come back in the caller's
    order; every pair's outputs are the same bits whatever else is listed, in any order, under any workspace budget.  36 regions,
    D % 32 == 0, sim_dim % 16 == 0 and <= 256 (NotImplementedError above), captions of 1..63 words.  A caption of 64..191 words is
    SCORED by the path sgraf_candidate_scores uses for it and not explained (empty blocks, explained[p] False); longer captions
    raise NotImplementedError.  `state` (sgraf_pairs_prepare's) and `max_workspace_bytes` as sgraf_candidate_scores."""
    lib = _lib.load()
    if module_name not in ('SAF', 'SGR'):
        raise ValueError('Invalid input of config.module_name in configs.py')
    images = _dev(images, name="images")
    words = _dev(words, name="words")
    pairs = _dev(pairs, torch.int32, name="pairs")
    if pairs.dim() != 2 or pairs.shape[1] != 2:
        raise ValueError("sgraf_pair_attention: pairs must be [P, 2] of (image, caption), got shape %s" % (tuple(pairs.shape),))
    Ni, R, D = images.shape
    Nc = plan.Nc
    dev = images.device
    P = pairs.shape[0]
    sgr = module_name == 'SGR'
    steps = int(sgr_step) if sgr else 0
    if state is not None:
        if not isinstance(state, SgrafPairsState):
            raise TypeError("sgraf_pair_attention: state must come from sgraf_pairs_prepare")
        state.check(images, words, plan, weights, module_name, sgr_step)
    S_dim = int(weights["sim_eval_w.weight"].shape[-1])
    if S_dim > SGRAF_ATTN_MAX_SIM_DIM or S_dim % 16:
        raise NotImplementedError("sgraf_pair_attention: sim_dim %d (supported: multiples of 16 up to %d)" % (S_dim, SGRAF_ATTN_MAX_SIM_DIM))
    f32 = lambda n: torch.empty(n, device=dev, dtype=torch.float32)
    if P == 0:
        z = lambda: torch.zeros(1, device=dev, dtype=torch.int64)
        return SgrafPairAttention(pairs, f32(0), z(), None if sgr else f32(0), None if sgr else z(), f32(0) if sgr else None, z() if sgr else None,
                                  f32(0), torch.empty(0, device=dev, dtype=torch.int32), torch.empty(0, device=dev, dtype=torch.bool),
                                  module_name, sgr_step)
    if R != SCAN_R:
        raise NotImplementedError("sgraf_pair_attention: %d regions per image (VisualSA is built for %d)" % (R, SCAN_R))
    if len(plan.len_host) and int(plan.len_host.max()) > SGRAF_COMPOSED_MAX_WORDS:
        raise NotImplementedError("sgraf_pair_attention: captions of at most %d words are supported" % SGRAF_COMPOSED_MAX_WORDS)
    if P >= 2 ** 31 // 64:
        raise NotImplementedError("sgraf_pair_attention: %d pairs (at most %d per call); split the list" % (P, 2 ** 31 // 64 - 1))
    _check_in_range("sgraf_pair_attention", pairs, (Ni, Nc))
    if state is None:
        state = sgraf_pairs_prepare(images, words, plan, weights, module_name, sgr_step)
    st = state.struct
    mod = 1 if sgr else 0
    # ---- the output layout, on the device
    imgs, caps = pairs[:, 0].to(torch.int64), pairs[:, 1].to(torch.int64)
    cap_len = _caption_tables(plan, dev, None)[1][caps]
    explained = cap_len <= SGRAF_MAX_WORDS
    w_eff = torch.where(explained, cap_len, torch.zeros_like(cap_len)).to(torch.int64)
    n_eff = torch.where(explained, w_eff + 1, torch.zeros_like(w_eff))

    def prefix(counts):
        ptr = torch.zeros(P + 1, device=dev, dtype=torch.int64)
        ptr[1:] = torch.cumsum(counts, 0)
        return ptr

    attn_ptr = prefix(w_eff * SCAN_R)
    aux_ptr = prefix(n_eff * n_eff * steps if sgr else n_eff)
    ends = torch.stack((attn_ptr[-1], aux_ptr[-1])).tolist()
    attn, aux, score = f32(ends[0]), f32(ends[1]), f32(P)
    result = SgrafPairAttention(pairs, attn, attn_ptr, None if sgr else aux, None if sgr else aux_ptr, aux if sgr else None,
                                aux_ptr if sgr else None, score, cap_len, explained, module_name, sgr_step)
    slot = torch.arange(P, device=dev, dtype=torch.int64)
    if len(plan.len_host) and int(plan.len_host.max()) > SGRAF_MAX_WORDS:
        caps, imgs, slot = _long_caption_pairs(images, words, plan, ~explained, caps, imgs, slot, score,
                                               lambda: _sgraf_long_caption_col(images, weights, module_name, sgr_step, S_dim))
    Ps = caps.numel()
    SGRAF_ATTN_LAST.update(pairs=Ps, items=0, chunks=0, workspace_bytes=0)      # (reset before the early return, unlike SGRAF_PAIRS_LAST: kept)
    if Ps == 0:
        return result
    # ---- image-major (CSR) form, on the device
    img_ptr, imgs, caps, slot = _group_pairs(imgs, Ni, (caps, slot), grouped=False)
    pair_img, pair_cap, pair_out = imgs.to(torch.int32), caps.to(torch.int32), slot.to(torch.int32)
    off, klen = _caption_tables(plan, dev, SGRAF_MAX_WORDS)
    (pair_len, pair_col, pair_capok, item_begin, item_img), n_items, ib = _sgraf_item_plan(lib, img_ptr, pair_cap, off, klen, Ps, Ni, Nc,
                                                                                          words.shape[0], dev)
    # ---- chunks of whole items sized to the budget
    budget = _workspace_budget(dev, max_workspace_bytes)

    def need(it0, it1):
        return lib.itr_sgraf_pair_attention_workspace_bytes(int(ib[it1] - ib[it0]), it1 - it0, D, S_dim, mod, int(sgr_step))

    chunks = _chunks_within("sgraf_pair_attention", need, n_items, budget)
    wsb = max(need(a, b) for a, b in chunks)
    ws = torch.empty(wsb, device=dev, dtype=torch.uint8)
    SGRAF_ATTN_LAST.update(items=n_items, chunks=len(chunks), workspace_bytes=int(wsb), budget_bytes=budget)
    node_args = (None, None, 0, _p(aux), _p(aux_ptr), aux.numel()) if sgr else (_p(aux), _p(aux_ptr), aux.numel(), None, None, 0)
    for a, b in chunks:
        _lib.check(lib.itr_sgraf_pair_attention(_p(images), _p(words), _p(off), _p(pair_img), _p(pair_capok), _p(pair_len), _p(pair_col),
                                                _p(pair_out), _p(item_begin), _p(item_img), int(ib[a]), int(ib[b] - ib[a]), a, b - a, Ni, Nc,
                                                words.shape[0], R, D, S_dim, mod, int(sgr_step), C.byref(st), _p(state.buf), state.buf.numel(),
                                                _p(attn), _p(attn_ptr), attn.numel(), *node_args, _p(score), P, _p(ws), wsb, _stream()))
    return result


def sgraf_candidate_attention(images, words, plan, weights, cand, by, m=None, **kw):
    """`sgraf_pair_attention` for candidate lists, `cand` and `by` as in sgraf_candidate_scores: explains the first `m` columns of
    every list (all of them when m is None) -> SgrafPairAttention whose pair q * m + k is list q's entry k."""
    _check_by("sgraf_candidate_attention", by)
    n_q, _, _ = _check_lists("sgraf_candidate_attention", cand, by, images, plan)
    pairs = _lists_to_pairs("sgraf_candidate_attention", cand.contiguous(), by, n_q, m)
    return sgraf_pair_attention(images, words, plan, weights, pairs, **kw)


def _sgraf_long_caption_col(images, weights, module_name, sgr_step, S_dim):
    """`_long_caption_pairs`' scorer for captions of 64..191 words: Fusionmodule.encoder_similarity_train(training=False) -- what
    sgraf_scores runs for such captions -- on one caption and its listed images."""
    from .modalmodule import Fusionmodule
    sim_enc = Fusionmodule.EncoderSimilarity(images.shape[2], S_dim, module_name, sgr_step)
    own = sim_enc.state_dict()
    sim_enc.load_state_dict({k: (weights[k].detach() if k in weights else own[k]) for k in own if k in weights or k.endswith('num_batches_tracked')})
    sim_enc.to(images.device).eval()
    return lambda im, w, l: Fusionmodule.encoder_similarity_train(sim_enc, im, w, np.zeros(1, np.int64), [l], None, training=False)


def _scan_long_caption_col(cross_attn, norm, agg, lambda_lse, lambda_softmax):
    """`_long_caption_pairs`' scorer for captions of 65..96 words: the one-workgroup-per-pair forward of the training path on one
    caption and its listed images."""
    from . import autograd
    fn = autograd.scan_t2i_scores if cross_attn == 't2i' else autograd.scan_i2t_scores
    return lambda im, w, l: fn(im, w, np.zeros(1, np.int64), np.asarray([l], np.int32), norm, agg, lambda_lse, lambda_softmax)


def rerank_lists(idx, val):
    """Re-order K-lists by new scores: idx int32 [n, K] candidates (in coarse order), val float32 [n, K] their new scores
    -> (idx_sorted, val_sorted, perm) in the ranker's order (larger score first, the higher index on exact ties, -0.0 == +0.0,
    NaN as +inf; equal entries keep their coarse order); perm[n, K] = old position of each entry.  1 <= K <= TOPK_MAX."""
    lib = _lib.load()
    idx = _dev(idx, torch.int32, name="idx")
    val = _dev(val, torch.float32, name="val")
    if idx.dim() != 2 or idx.shape != val.shape:
        raise ValueError("rerank_lists: idx and val must be 2-D of one shape, got %s and %s" % (tuple(idx.shape), tuple(val.shape)))
    n, K = idx.shape
    io, vo, po = torch.empty_like(idx), torch.empty_like(val), torch.empty_like(idx)
    if n == 0:
        return io, vo, po
    _lib.check(lib.itr_rerank_lists(_p(idx), _p(val), n, K, _p(io), _p(vo), _p(po), _stream()))
    return io, vo, po


def rerank_fused_lists(idx, vals):
    """Ensemble reranking: re-order K-lists by the mean of M models' scores.  idx int32 [n, K] candidates (in coarse order); vals a
    sequence of M float32 [n, K] tensors or one [M, n, K] tensor, the members' scores of those candidates.  The fused score is the
    float64 sum in member order divided by float64(M) (the reference's ensemble average on the listed pairs).
    -> (idx_sorted int32 [n, K], fused float64 [n, K], vals_sorted float32 [M, n, K], perm int32 [n, K]) in the float64 ranker's
    order (larger fused score first, the higher index on exact ties, -0.0 == +0.0, NaN as +inf; equal entries keep their coarse
    order); perm = old position of each entry, member scores keep their bits.  1 <= K <= TOPK_MAX, 1 <= M <= 4."""
    lib = _lib.load()
    idx = _dev(idx, torch.int32, name="idx")
    if torch.is_tensor(vals):
        val = _dev(vals, torch.float32, name="vals")
        if val.dim() != 3:
            raise ValueError("rerank_fused_lists: a vals tensor must be [M, n, K], got %s" % (tuple(val.shape),))
    else:
        members = [_dev(v, torch.float32, name="vals[%d]" % m) for m, v in enumerate(vals)]
        if not members:
            raise ValueError("rerank_fused_lists: no member scores")
        for m, v in enumerate(members):
            if v.shape != members[0].shape or v.dim() != 2:
                raise ValueError("rerank_fused_lists: every member's scores must be 2-D of one shape, got %s for member %d and %s for member 0"
                                 % (tuple(v.shape), m, tuple(members[0].shape)))
        val = torch.stack(members)
    if idx.dim() != 2 or idx.shape != val.shape[1:]:
        raise ValueError("rerank_fused_lists: idx must be [n, K] and vals [M, n, K], got %s and %s" % (tuple(idx.shape), tuple(val.shape)))
    M = val.shape[0]
    n, K = idx.shape
    io, po = torch.empty_like(idx), torch.empty_like(idx)
    fo = torch.empty((n, K), dtype=torch.float64, device=idx.device)
    vo = torch.empty_like(val)
    if n == 0:
        return io, fo, vo, po
    _lib.check(lib.itr_rerank_fuse_lists(_p(idx), _p(val), M, n, K, _p(io), _p(fo), _p(vo), _p(po), _stream()))
    return io, fo, vo, po


class CollatedBatch(object):
    """What collate_batch wrote: `images`, `boxes`, `img_wh`, `ids` (ragged form), `tables` (tuple, fixed-width form),
    `float_table`, each None when its source was not given, and the device int32 `bad_flag`."""
    __slots__ = ("images", "boxes", "img_wh", "ids", "tables", "float_table", "bad_flag")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))


def collate_batch(feat, img_idx, boxes=None, img_wh=None, cap_idx=None, packed=None, off=None, lmax=None, tables=(), float_table=None,
                  bad_flag=None, check=False):
    """One training batch gathered from device-resident tables in one launch (itr_collate_batch): the device form of
    PrecompDataset.__getitem__ + collate_fn for sample indices that are already in collate order.

    feat [n_img, ...] float32 and img_idx int64 [B] -> images [B, ...]; boxes [n_img, ...] / img_wh [n_img, 2] follow img_idx.
    Ragged caption ids: packed int64 [n], off int64 [n_cap + 1], cap_idx int64 [B], lmax -> ids int64 [B, lmax], zero padded.
    Fixed-width caption tables: up to three int64 `tables` [n_cap, W] and one float32 `float_table` [n_cap, W] follow cap_idx.
    An index outside its table reads row 0 and raises the device flag; the flag is read (a host synchronisation) only with
    check=True, which then raises IndexError.  bad_flag: a zeroed device int32 to reuse over calls (default: a fresh one)."""
    lib = _lib.load()
    feat = _dev(feat, name="feat")
    img_idx = _dev(img_idx, torch.int64, name="img_idx")
    if feat.dim() < 1 or img_idx.dim() != 1 or feat.shape[0] < 1:
        raise ValueError("collate_batch: feat must be [n_img >= 1, ...] and img_idx 1-D, got %s and %s" % (tuple(feat.shape), tuple(img_idx.shape)))
    dev, B, n_img = feat.device, img_idx.shape[0], feat.shape[0]
    tables = tuple(tables)
    if len(tables) > 3:
        raise ValueError("collate_batch: at most three int64 tables, got %d" % len(tables))
    ragged = packed is not None or off is not None
    fixed = tables + ((float_table,) if float_table is not None else ())
    n_cap = 0
    if ragged or fixed:
        if cap_idx is None:
            raise ValueError("collate_batch: caption tables need cap_idx")
        cap_idx = _dev(cap_idx, torch.int64, name="cap_idx")
        if cap_idx.shape != img_idx.shape:
            raise ValueError("collate_batch: cap_idx %s vs img_idx %s" % (tuple(cap_idx.shape), tuple(img_idx.shape)))

    def table(t, dtype, name, rows):
        t = _dev(t, dtype, name=name)
        if t.dim() < 1 or t.shape[0] != rows:
            raise ValueError("collate_batch: %s must have %d rows, got %s" % (name, rows, tuple(t.shape)))
        return t, torch.empty((B,) + tuple(t.shape[1:]), device=dev, dtype=dtype)

    images = torch.empty((B,) + tuple(feat.shape[1:]), device=dev, dtype=torch.float32)
    row_elems = feat[0].numel()
    boxes, boxes_out = table(boxes, torch.float32, "boxes", n_img) if boxes is not None else (None, None)
    if img_wh is not None:
        img_wh, wh_out = table(img_wh, torch.float32, "img_wh", n_img)
        if img_wh[0].numel() != 2:
            raise ValueError("collate_batch: img_wh must be [n_img, 2], got %s" % (tuple(img_wh.shape),))
    else:
        wh_out = None
    ids_out, n_packed = None, 0
    if ragged:
        if packed is None or off is None or lmax is None:
            raise ValueError("collate_batch: ragged ids need packed, off and lmax")
        packed, off = _dev(packed, torch.int64, name="packed"), _dev(off, torch.int64, name="off")
        if packed.dim() != 1 or off.dim() != 1 or off.shape[0] < 2 or int(lmax) < 0:
            raise ValueError("collate_batch: packed and off must be 1-D with off of n_cap + 1 >= 2 entries, lmax >= 0")
        n_cap, n_packed = off.shape[0] - 1, packed.shape[0]
        ids_out = torch.empty(B, int(lmax), device=dev, dtype=torch.int64)
    W, pairs = 0, []
    for k, t in enumerate(fixed):
        if not n_cap:
            n_cap = t.shape[0] if torch.is_tensor(t) and t.dim() == 2 else 0
        src, dst = table(t, torch.int64 if k < len(tables) else torch.float32, "tables[%d]" % k if k < len(tables) else "float_table", n_cap)
        if src.dim() != 2 or (pairs and src.shape[1] != W):
            raise ValueError("collate_batch: the fixed-width tables must be 2-D of one width, got %s" % (tuple(src.shape),))
        W = src.shape[1]
        pairs.append((src, dst))
    ipairs = pairs[:len(tables)] + [(None, None)] * (3 - len(tables))
    fpair = pairs[len(tables)] if float_table is not None else (None, None)
    if bad_flag is None:
        bad_flag = torch.zeros(1, device=dev, dtype=torch.int32)
    else:
        bad_flag = _dev(bad_flag, torch.int32, name="bad_flag")
    if B:      # (the tensors of an empty batch have no storage to point at)
        _lib.check(lib.itr_collate_batch(_p(img_idx), _p(cap_idx) if (ragged or fixed) else None, B, _p(feat), n_img, row_elems, _p(images),
                                         _p(boxes), boxes[0].numel() if boxes is not None else 0, _p(boxes_out), _p(img_wh), _p(wh_out),
                                         _p(packed) if ragged else None, n_packed, _p(off) if ragged else None, n_cap, int(lmax) if ragged else 0,
                                         _p(ids_out), _p(ipairs[0][0]), _p(ipairs[1][0]), _p(ipairs[2][0]), _p(fpair[0]), W, _p(ipairs[0][1]),
                                         _p(ipairs[1][1]), _p(ipairs[2][1]), _p(fpair[1]), _p(bad_flag), _stream()))
    if check and int(bad_flag.item()):
        raise IndexError("collate_batch: an index lies outside its table (img_idx vs %d image rows, cap_idx vs %d captions)" % (n_img, n_cap))
    return CollatedBatch(images=images, boxes=boxes_out, img_wh=wh_out, ids=ids_out, tables=tuple(d for _, d in pairs[:len(tables)]),
                         float_table=fpair[1], bad_flag=bad_flag)
