"""GPU: the score-distillation loss (csrc/distill.hip: itr_distill_fwd / _bwd; ops.distill_loss) against the float64 helper
(tests/helpers/distill_oracle.py) over the helper's case table.

Sizes: 1, 2, the wave (64) and workgroup (256) strides of the kernels and their neighbours, 300, and one global-batch size (1024: 16
column blocks x 16 row slices).  Student and teacher matrices are independent amp * rand draws at amplitudes 1 and 30 each (temperature
0.05: z within 25, or up to ~750, where exp without its maximum subtracted overflows fp32), each plus a quarter of its amplitude on the
last row and column, so that an index dropped at the end moves loss and dS by more than their tolerance (tests/test_distill_cpu.py
proves it for every case).  Upstream gradient 3.0.

Tolerances, the primary rule of tests/helpers/train_prim_cases.py with e32 the float32 helper's own error against float64:
dS and the four saved log-sum-exp vectors FACTOR * max(e32, U * max|want|); the loss FACTOR * max(e32, U * (max|z_s| + max|z_t|))."""
import os
import sys

import pytest
import torch

from itr_amd import _lib, autograd as ag, ops

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import distill_oracle as D  # noqa: E402

pytestmark = pytest.mark.gpu

TEMP = D.TEMPERATURE
IDS = ["B%d-s%g-t%g" % c for c in D.CASES]


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def run(S, T, dev, temperature=TEMP, teacher_temperature=TEMP, upstream=D.UPSTREAM):
    """-> dict(loss, dS, row_lse_s, col_lse_s, row_lse_t, col_lse_t): loss and dS through the tape, the vectors from the forward op"""
    s, t = S.to(dev).requires_grad_(True), T.to(dev)
    loss = ops.distill_loss(s, t, temperature, teacher_temperature)
    (loss * upstream).backward()
    out = dict(loss=loss.detach(), dS=s.grad)
    fwd = ops.distill_fwd(s.detach(), t, temperature, teacher_temperature)
    assert torch.equal(bits(fwd[0].reshape(())), bits(out["loss"]))
    out.update(zip(D.VECTORS, fwd[1:]))
    return out


def ratio(err, tol):
    """error / tolerance for the printed record (B = 1: want and tolerance of dS are exactly 0, and so must the error be)"""
    return err / tol if tol > 0 else (0.0 if err == 0 else float("inf"))


def compare(got, ref, label):
    failures = []
    for name in ("loss", "dS") + D.VECTORS:
        want, e32, tol = ref[name]
        g = got[name].cpu().double()
        err = float((g - want).abs().max())
        print("\n%s %s: got %.9g want %.9g (max|want| %.6g) err %.3g e32 %.3g tol %.3g ratio %.3f" % (
            label, name, float(g.reshape(-1)[0]), float(want.reshape(-1)[0]), float(want.abs().max()), err, e32, tol, ratio(err, tol)))
        if not (torch.isfinite(g).all() and err <= tol):
            failures.append((name, err, tol))
    assert not failures, failures


@pytest.mark.parametrize("B,amp_s,amp_t", D.CASES, ids=IDS)
def test_sweep_vs_float64(dev, B, amp_s, amp_t):
    ref = D.reference(B, amp_s, amp_t)
    got = run(ref["S"], ref["T"], dev)
    assert got["loss"].dtype == torch.float32 and got["loss"].dim() == 0 and got["dS"].shape == (B, B)
    assert all(got[v].shape == (B,) for v in D.VECTORS)
    compare(got, ref, "B=%d amp_s=%g amp_t=%g" % (B, amp_s, amp_t))


def raw(S, T, dev, ldS, ldT, lddS, upstream=D.UPSTREAM):
    """The C entries on matrices embedded in wider buffers (leading dimensions ldS, ldT, lddS >= B) -> run()'s dict + the dS buffer."""
    lib = _lib.load()
    B = S.shape[0]
    scale = D.scale_of(TEMP)
    bufS = torch.full((B, ldS), 1e30, device=dev)           # a read past column B would wreck every sum
    bufT = torch.full((B, ldT), -1e30, device=dev)
    bufS[:, :B], bufT[:, :B] = S.to(dev), T.to(dev)
    bufD = torch.full((B, lddS), 7.0, device=dev)
    loss = torch.empty(1, device=dev)
    vec = [torch.empty(B, device=dev) for _ in range(4)]
    ws = torch.empty(int(lib.itr_distill_workspace_bytes(B)), device=dev, dtype=torch.uint8)
    g = torch.full((1,), upstream, device=dev)
    p = ops._p
    _lib.check(lib.itr_distill_fwd(p(bufS), p(bufT), B, ldS, ldT, scale, scale, p(loss), p(vec[0]), p(vec[1]), p(vec[2]), p(vec[3]), p(ws),
                                   ops._stream()))
    _lib.check(lib.itr_distill_bwd(p(bufS), p(bufT), B, ldS, ldT, scale, scale, p(vec[0]), p(vec[1]), p(vec[2]), p(vec[3]), p(g), p(bufD),
                                   lddS, ops._stream()))
    torch.cuda.synchronize()
    out = dict(loss=loss.reshape(()), dS=bufD[:, :B].contiguous(), buffer=bufD)
    out.update(zip(D.VECTORS, vec))
    return out


@pytest.mark.parametrize("B,ldS,ldT,lddS", [(65, 80, 67, 66), (257, 258, 300, 320)])
@pytest.mark.parametrize("amp", D.AMPLITUDES)
def test_leading_dimensions_above_B(dev, B, ldS, ldT, lddS, amp):
    ref = D.reference(B, amp, amp)
    got = raw(ref["S"], ref["T"], dev, ldS, ldT, lddS)
    compare(got, ref, "B=%d ld %d/%d/%d amp=%g" % (B, ldS, ldT, lddS, amp))
    assert bool((got["buffer"][:, B:] == 7.0).all())                                     # nothing written past column B of dS
    dense = run(ref["S"], ref["T"], dev)
    for name in ("loss", "dS") + D.VECTORS:                                              # the same instructions on the same numbers
        assert torch.equal(bits(got[name]), bits(dense[name])), name


@pytest.mark.parametrize("B", [1, 64, 300])
@pytest.mark.parametrize("amp", D.AMPLITUDES)
def test_teacher_equal_to_student_is_bit_zero(dev, B, amp):
    S = D.reference(300, amp, amp)["S"][:B, :B].contiguous()
    got = run(S, S.clone(), dev)
    assert torch.equal(bits(got["loss"]), torch.zeros((), dtype=torch.int32))
    assert torch.equal(bits(got["dS"]), torch.zeros(B, B, dtype=torch.int32))
    assert torch.equal(bits(got["row_lse_s"]), bits(got["row_lse_t"])) and torch.equal(bits(got["col_lse_s"]), bits(got["col_lse_t"]))


def test_batch_of_one_is_zero(dev):
    for s, t in ((0.3, 0.3), (0.3, -0.9), (-40.0, 35.0), (35.0, 0.01), (1.5, 45.0)):
        got = run(torch.full((1, 1), s), torch.full((1, 1), t), dev)
        assert float(got["loss"]) == 0.0 and float(got["dS"].abs().max()) == 0.0 and got["dS"].shape == (1, 1)
    for amp_s in D.AMPLITUDES:
        for amp_t in D.AMPLITUDES:
            ref = D.reference(1, amp_s, amp_t)
            got = run(ref["S"], ref["T"], dev)
            assert float(got["loss"]) == 0.0 and float(got["dS"].abs().max()) == 0.0


@pytest.mark.parametrize("B,amp_s,amp_t", [(1, 1.0, 30.0), (65, 1.0, 1.0), (300, 30.0, 1.0), (1024, 1.0, 30.0), (1024, 30.0, 30.0)])
def test_same_bits_run_to_run(dev, B, amp_s, amp_t):
    ref = D.reference(B, amp_s, amp_t)
    a, b = run(ref["S"], ref["T"], dev), run(ref["S"], ref["T"], dev)
    for name in ("loss", "dS") + D.VECTORS:
        assert torch.equal(bits(a[name]), bits(b[name])), name


def test_temperatures(dev):
    """two different temperatures reach the kernels as two different scales"""
    ref = D.reference(65, 1.0, 1.0)
    for temperature, teacher_temperature in ((0.07, 0.05), (0.05, 0.1), (1.0, 0.02)):
        got = run(ref["S"], ref["T"], dev, temperature, teacher_temperature)
        want = D.tolerances(ref["S"], ref["T"], D.scale_of(temperature), D.scale_of(teacher_temperature))
        compare(got, want, "T=%g/%g" % (temperature, teacher_temperature))


def test_on_the_tape_through_cosine_scores(dev):
    """ops.distill_loss behind ag.cosine_scores(img, cap): the gradients of the two embedding matrices against float64 torch autograd
    of the helper's loss on the same leaves; tolerance by the primary rule, e32 the same chain in float32 on the CPU"""
    B, Dm = 65, 32
    g = torch.Generator().manual_seed(65)
    img0 = torch.nn.functional.normalize(torch.randn(B, Dm, generator=g), dim=1)
    cap0 = torch.nn.functional.normalize(torch.randn(B, Dm, generator=g), dim=1)
    T = D.reference(B, 1.0, 1.0)["T"]
    scale = D.scale_of(TEMP)
    want = {}
    for dtype in (torch.float64, torch.float32):
        im, cp = img0.clone().to(dtype).requires_grad_(True), cap0.clone().to(dtype).requires_grad_(True)      # (.to may return its argument)
        loss = D.distill_loss(im @ cp.t(), T, scale, scale, dtype)
        (loss * D.UPSTREAM).backward()
        want[dtype] = (loss.detach().double(), im.grad.double(), cp.grad.double())
    img, cap = img0.clone().to(dev).requires_grad_(True), cap0.clone().to(dev).requires_grad_(True)
    loss = ops.distill_loss(ag.cosine_scores(img, cap), T.to(dev), TEMP, TEMP)
    (loss * D.UPSTREAM).backward()
    assert img.grad.shape == (B, Dm) and cap.grad.shape == (B, Dm)
    S64 = img0.double() @ cap0.double().t()
    for name, got, k in (("loss", loss.detach(), 0), ("img.grad", img.grad, 1), ("cap.grad", cap.grad, 2)):
        w64 = want[torch.float64][k]
        e32 = float((want[torch.float32][k] - w64).abs().max())
        tol = D.loss_tolerance(e32, S64, T, scale, scale) if name == "loss" else D.FACTOR * max(e32, D.U * float(w64.abs().max()))
        err = float((got.cpu().double() - w64).abs().max())
        print("\ntape %s: err %.3g e32 %.3g tol %.3g ratio %.3f" % (name, err, e32, tol, ratio(err, tol)))
        assert err <= tol, (name, err, tol)


def test_refused_inputs(dev):
    S = torch.rand(6, 6, device=dev)
    with pytest.raises(ValueError, match="must not require grad"):
        ops.distill_loss(S, torch.rand(6, 6, device=dev, requires_grad=True))
    with pytest.raises(ValueError, match="must not require grad"):
        ops.distill_loss(S.clone().requires_grad_(True), ag.cosine_scores(S.clone().requires_grad_(True), S))
    ops.distill_loss(S, ag.cosine_scores(S.clone().requires_grad_(True), S).detach())                 # detached: a target like any other
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.distill_loss(S.cpu(), S.cpu())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.distill_loss(S, S.cpu())
    with pytest.raises(ValueError, match="square"):
        ops.distill_loss(S[:, :5], S[:, :5])
    with pytest.raises(ValueError, match="do not match"):
        ops.distill_loss(S, S[:5, :5])
    with pytest.raises(TypeError):
        ops.distill_loss(S, S.double())
    for bad in (0.0, -0.05, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="temperature"):
            ops.distill_loss(S, S.clone(), bad)
        with pytest.raises(ValueError, match="teacher_temperature"):
            ops.distill_fwd(S, S.clone(), 0.05, bad)
