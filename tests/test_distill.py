"""Distillation loss without a GPU: the fp64 restatement (tests/distill_ref.py) against torch's
fp64 autograd of F.cross_entropy + F.kl_div, the three C-ABI symbols, their argument checks
(DRNMI_EINVAL before any HIP call) and the Python criterion's argument errors."""
import ctypes
import itertools
import os
import re
import subprocess

import pytest
import torch
import torch.nn.functional as F

import distill_ref as R
from drnmi import _lib
from drnmi.build import build

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "drnmi.h")
SYMBOLS = ("drnmi_distill_workspace_bytes", "drnmi_distill_loss_f32", "drnmi_distill_loss_bwd_f32")


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_restatement_equals_fp64_autograd(shape):
    """loss, both terms and the gradient: 1e-7 relative to autograd of
    sw * F.cross_entropy(s, ignore_index) + dw * F.kl_div(log_softmax(s / T), softmax(t / T), "sum") / D."""
    s, t, tg = R.case_for(shape)
    n, hw = shape[0], shape[2] * shape[3]
    for T, red, (sw, dw) in itertools.product(R.TEMPERATURES, R.REDUCTIONS, R.WEIGHTS):
        sd = s.double().requires_grad_(True)
        ce = F.cross_entropy(sd, tg, ignore_index=255)
        d = n if red == "batchmean" else n * hw
        kd = F.kl_div(F.log_softmax(sd / T, 1), F.softmax(t.double() / T, 1), reduction="sum") / d
        loss = sw * ce + dw * kd
        loss.backward()
        got = R.distill_ref(s, t, tg, sw, dw, T, 255, red)
        for name, a, b in (("loss", got[0], loss), ("ce", got[1], ce), ("kd", got[2], kd)):
            assert abs(float(a) - float(b.detach())) <= 1e-7 * abs(float(b.detach())), (name, T, red, sw, dw)
        assert float(got[3]) == float((tg != 255).sum())
        err = float((got[4] - sd.grad).abs().max() / sd.grad.abs().max())
        assert err <= 1e-7, (T, red, sw, dw, err)


def test_restatement_edge_cases():
    s, t, tg = R.case_for((2, 2, 5, 7))
    # bit-equal teacher: kd and the kd gradient vanish exactly
    loss, ce, kd, _, g = R.distill_ref(s, s.clone(), tg, 0.5, 0.5, 2.0, 255)
    assert float(kd) == 0.0 and float(loss) == 0.5 * float(ce)
    assert torch.equal(g, R.distill_ref(s, t, tg, 0.5, 0.0, 2.0, 255)[4])
    # an out-of-range target: NaN loss, a finite gradient that ignores the pixel
    bad = tg.clone()
    bad[0, 1, 1] = 7
    loss, ce, kd, _, g = R.distill_ref(s, t, bad, 0.5, 0.5, 1.0, 255)
    assert torch.isnan(loss) and torch.isnan(ce) and torch.isfinite(kd) and bool(torch.isfinite(g).all())


def test_symbols_in_header_binding_and_library():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", build(verbose=False)], capture_output=True, text=True,
                         check=True).stdout
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES, name
        assert re.search(r" T %s\b" % name, out), name
    assert _lib.load().drnmi_distill_workspace_bytes() >= 4 * 8


def test_einval_without_a_device():
    """Every refusal of include/drnmi.h's list, returned before any HIP call (no device here)."""
    lib = _lib.load()
    buf = (ctypes.c_double * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    inf, nan = float("inf"), float("nan")
    good = dict(s=p, t=p, tg=p, n=1, c=19, hw=8, ign=255, sw=0.5, dw=0.5, T=1.0, bm=0)

    def fwd(out3=p, count=p, ws=p, **kw):
        a = {**good, **kw}
        return lib.drnmi_distill_loss_f32(a["s"], a["t"], a["tg"], a["n"], a["c"], a["hw"], a["ign"], a["sw"], a["dw"],
                                          a["T"], a["bm"], out3, count, ws, None)

    def bwd(dloss=p, count=p, g=p, **kw):
        a = {**good, **kw}
        return lib.drnmi_distill_loss_bwd_f32(a["s"], a["t"], a["tg"], a["n"], a["c"], a["hw"], a["ign"], a["sw"],
                                              a["dw"], a["T"], a["bm"], dloss, count, g, None)

    shared = [dict(s=None), dict(t=None), dict(tg=None), dict(n=0), dict(n=-1), dict(c=0), dict(hw=0), dict(hw=-4),
              dict(T=0.0), dict(T=-1.0), dict(T=inf), dict(T=nan), dict(sw=-0.5), dict(sw=inf), dict(sw=nan),
              dict(dw=-1e-3), dict(dw=inf), dict(dw=nan)]
    for kw in shared:
        assert fwd(**kw) == -1, ("fwd", kw)
        assert bwd(**kw) == -1, ("bwd", kw)
    for kw in (dict(out3=None), dict(count=None), dict(ws=None)):
        assert fwd(**kw) == -1, kw
    for kw in (dict(dloss=None), dict(count=None), dict(g=None)):
        assert bwd(**kw) == -1, kw


def test_criterion_argument_errors():
    from drnmi.train import DistillationLoss, teacher_logprobs
    for kw in (dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("inf")),
               dict(temperature=float("nan")), dict(student_wt=-0.1), dict(distill_wt=-1.0),
               dict(distill_wt=float("nan")), dict(kd_reduction="sum"), dict(kd_reduction="none")):
        with pytest.raises(ValueError):
            DistillationLoss(**kw)
    crit = DistillationLoss(ignore_index=255)
    assert (crit.student_wt, crit.distill_wt, crit.temperature, crit.kd_reduction) == (0.5, 0.5, 1.0, "mean")
    assert DistillationLoss().ignore_index == -100
    s, t, tg = R.case_for((2, 2, 5, 7))
    with pytest.raises(RuntimeError):                                   # CPU tensors: no fallback
        crit(s, t, tg)
    for args in ((s.double(), t, tg), (s, t.half(), tg), (s, t, tg.int()),          # dtypes
                 (s, t[:, :1], tg), (s, t[:1], tg), (s, t, tg[:, :4]), (s, t, tg[:1]),   # classes / shapes
                 (s, t.clone().requires_grad_(True), tg)):                         # a teacher in the graph
        with pytest.raises(ValueError):
            crit(*args)

    class Teacher(torch.nn.Module):
        def forward(self, x):
            return x + 1, None

    m = Teacher()
    with pytest.raises(RuntimeError):
        teacher_logprobs(m, s)                                           # train mode
    x = s.clone().requires_grad_(True)
    out = teacher_logprobs(m.eval(), x)
    assert torch.equal(out, s + 1) and not out.requires_grad
