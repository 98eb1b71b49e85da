"""Distillation loss on the GPU (drnmi.train.DistillationLoss on drnmi_distill_loss_f32 / _bwd_f32)
against the fp64 restatement of tests/distill_ref.py.

Tolerance: the project's cross-entropy one (test_gpu_train.py: loss 1e-5 relative, gradient
max|diff| / max|ref| <= 1e-5).  Torch's own fp32 CPU evaluation of the same formula on the 19- and
150-class shapes is within 8e-8 (loss) and 6e-7 (gradient) of fp64, so the bound leaves more than
10x for another summation order and hides nothing larger."""
import itertools

import pytest
import torch

import distill_ref as R
import train_case as TC

pytestmark = pytest.mark.gpu
DEV = "cuda"
RTOL = 1e-5


def _run(crit, s, t, tg):
    """(loss, ce, kd, grad) of one forward / backward of the criterion on the GPU."""
    sd = s.to(DEV).requires_grad_(True)
    loss = crit(sd, t.to(DEV), tg.to(DEV))
    loss.backward()
    return loss.detach(), crit.ce, crit.kd, sd.grad


def _close(a, b):
    a, b = float(a), float(b)
    return abs(a - b) <= RTOL * abs(b)


def _check_against_ref(crit, s, t, tg, tag):
    loss, ce, kd, g = _run(crit, s, t, tg)
    ref = R.distill_ref(s, t, tg, crit.student_wt, crit.distill_wt, crit.temperature, crit.ignore_index,
                        crit.kd_reduction)
    print(f"{tag}: loss {float(loss):.8g} / {float(ref[0]):.8g}  ce {float(ce):.8g} / {float(ref[1]):.8g}  "
          f"kd {float(kd):.8g} / {float(ref[2]):.8g}  grad err {TC.rel_err(g.cpu(), ref[4]):.2e}")
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda
    assert not ce.requires_grad and not kd.requires_grad and ce.is_cuda and kd.is_cuda
    assert _close(loss, ref[0]) and _close(ce, ref[1]) and _close(kd, ref[2]), tag
    assert bool(torch.isfinite(g).all()) and TC.rel_err(g.cpu(), ref[4]) <= RTOL, tag


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_matches_restatement(shape):
    from drnmi.train import DistillationLoss
    s, t, tg = R.case_for(shape)
    for T, red, (sw, dw) in itertools.product(R.TEMPERATURES, R.REDUCTIONS, R.WEIGHTS):
        crit = DistillationLoss(sw, dw, T, ignore_index=255, kd_reduction=red)
        _check_against_ref(crit, s, t, tg, f"{shape} T={T} {red} w=({sw},{dw})")


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ce_only_equals_cross_entropy(shape):
    from drnmi.train import CrossEntropyLoss, DistillationLoss
    s, t, tg = R.case_for(shape)
    sd = s.to(DEV).requires_grad_(True)
    ce = CrossEntropyLoss(ignore_index=255)(sd, tg.to(DEV))
    ce.backward()
    for T in R.TEMPERATURES:
        loss, ce_term, _, g = _run(DistillationLoss(1.0, 0.0, T, ignore_index=255), s, t, tg)
        assert torch.equal(loss, ce.detach()) and torch.equal(ce_term, ce.detach())
        assert torch.equal(g, sd.grad)


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_self_distillation_is_a_no_op(shape):
    from drnmi.train import CrossEntropyLoss, DistillationLoss
    s, _, tg = R.case_for(shape)
    sd = s.to(DEV).requires_grad_(True)
    ce = CrossEntropyLoss(ignore_index=255)(sd, tg.to(DEV))
    ce.backward()
    for T, red in itertools.product(R.TEMPERATURES, R.REDUCTIONS):
        loss, _, kd, g = _run(DistillationLoss(0.5, 0.5, T, ignore_index=255, kd_reduction=red), s, s.clone(), tg)
        assert float(kd) == 0.0
        assert torch.equal(loss, 0.5 * ce.detach())
        assert torch.equal(g, 0.5 * sd.grad)


def test_teacher_underflow_gives_zero_not_nan():
    """Teacher entries of -200 at T = 0.5: b = -400 below the row's lse, q = expf(.) = 0, and
    0 * (finite) contributes 0."""
    from drnmi.train import DistillationLoss
    for shape in R.SHAPES:
        s, t, tg = R.case_for(shape, seed=5)
        t = t.clone()
        t[:, 1::3] = -200.0
        crit = DistillationLoss(0.5, 0.5, 0.5, ignore_index=255)
        _check_against_ref(crit, s, t, tg, f"underflow {shape}")
        assert bool(torch.isfinite(crit.kd)) and float(crit.kd) > 0


def test_bad_target_gives_nan_loss():
    from drnmi.train import DistillationLoss
    for shape in R.SHAPES:
        s, t, tg = R.case_for(shape)
        for bad in (shape[1], -1):
            tb = tg.clone()
            tb[0, 2, 3] = bad
            crit = DistillationLoss(0.5, 0.5, 1.0, ignore_index=255)
            with torch.no_grad():
                loss = crit(s.to(DEV), t.to(DEV), tb.to(DEV))
            assert bool(torch.isnan(loss)) and bool(torch.isnan(crit.ce)) and bool(torch.isfinite(crit.kd))


def test_two_runs_are_bit_identical():
    from drnmi.train import DistillationLoss
    for shape in R.SHAPES:
        s, t, tg = R.case_for(shape)
        crit = DistillationLoss(0.5, 0.5, 2.0, ignore_index=255)
        a = _run(crit, s, t, tg)
        b = _run(crit, s, t, tg)
        for x, y in zip(a, b):
            assert torch.equal(x, y)


def test_end_to_end_student_and_frozen_teacher():
    """D-22 student (train mode, fp32x) distilled from a D-22 teacher (eval, bf16) on a 72 x 40 input
    (odd 9 x 5 maps): the gradient reaching the log-probs meets the restatement, every parameter
    gets a finite gradient, SGD steps, and the teacher is untouched."""
    from drnmi.drnseg import DRNSeg
    from drnmi.train import SGD, DistillationLoss, teacher_logprobs
    from drnmi.weights import synth_state_dict

    def model(seed):
        m = DRNSeg("drn_d_22", 19, pretrained=False)
        m.load_state_dict(synth_state_dict(m, seed))
        return m.to(DEV)

    student = model(21).train().set_precision("fp32x")
    teacher = model(22).eval().set_precision("bf16")
    before = {k: v.detach().clone() for k, v in teacher.state_dict().items()}
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, 3, 72, 40, generator=g).to(DEV)
    tg = torch.randint(0, 19, (1, 72, 40), generator=g)
    tg[torch.rand(1, 72, 40, generator=g) < 0.3] = 255
    tg = tg.to(DEV)

    crit = DistillationLoss(0.5, 0.5, 2.0, ignore_index=255)
    opt = SGD(student.optim_parameters(), 0.01, momentum=0.9, weight_decay=1e-4)
    tlp = teacher_logprobs(teacher, x)
    assert tlp.dtype == torch.float32 and not tlp.requires_grad and tlp.shape == (1, 19, 72, 40)
    lp = student(x)[0]
    seen = []
    lp.register_hook(lambda gr: seen.append(gr.detach().clone()))
    loss = crit(lp, tlp, tg)
    opt.zero_grad()
    loss.backward()
    loss = loss.detach()
    ref = R.distill_ref(lp, tlp, tg, 0.5, 0.5, 2.0, 255)
    print(f"end to end: loss {float(loss):.8g} / {float(ref[0]):.8g}, g_lp err {TC.rel_err(seen[0].cpu(), ref[4]):.2e}")
    assert _close(loss, ref[0]) and _close(crit.ce, ref[1]) and _close(crit.kd, ref[2])
    assert len(seen) == 1 and TC.rel_err(seen[0].cpu(), ref[4]) <= RTOL
    params = list(student.optim_parameters())
    assert params and all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in params)
    assert any(float(p.grad.abs().max()) > 0 for p in params)
    opt.step()
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(p).all()) for p in params)
    after = teacher.state_dict()
    assert before.keys() == after.keys() and all(torch.equal(before[k], after[k]) for k in before)
    assert all(p.grad is None for p in teacher.parameters())
    with pytest.raises(RuntimeError):
        teacher_logprobs(teacher.train(), x)
