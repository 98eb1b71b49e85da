"""Fine-tune path on the GPU (drnmi.train) vs the oracle / reference goldens.

Gates (fp32 throughout, the reference's arithmetic).  Parameters and stats: max-abs error
relative to the yardstick's max-abs.  Gradients: relative L2 error (train_case.rel_l2 — a ReLU
whose input sits within an ulp of zero may fall either way in any two fp32 implementations,
flipping that element's gradient path; measured on this case, the reference's own fp32 CPU run
and ours each show such isolated flips, ~1e-3 max-abs, at different layers):
  * vs the oracle run in fp64 (the exact value both fp32 implementations approximate):
    on a case with no ReLU at an ulp of zero, every gradient within 2e-5 max-abs (measured
    ~7e-6; the reference's fp32 CPU run on the GPU box is up to 3.5e-2 off on the same case);
    on the golden case, first-step gradients rel-L2 <= 2.5e-3 — there exactly one of 65536
    pre-ReLU values of layer.6.0.bn1 is -2.2e-7 in fp64 and +5.2e-7 in fp32 (scripts/
    train_diag3.py), which moves layer.6.0.bn1.bias's gradient by 1.8e-3 rel-L2 and
    everything upstream by ~3.5e-4; parameters after two SGD steps <= 1e-4;
  * vs the reference's own fp32 run (tests/golden/train.npz, lr 1e-3): loss rtol 1e-4,
    parameters and running stats <= 1e-4, second-step gradients rel-L2 <= 1e-2 (ReLU flips
    of the same kind: measured 3.4e-3 at layer.0.0.weight);
  * masked weights exactly zero.
Kernel-level checks compare each backward kernel with torch-CPU fp32 autograd of the same op."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import train_case as TC
from oracle import drn_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _run_hip_steps(m, pr, xs, ts, fused_mask=False, grads_per_step=None):
    from drnmi.train import SGD, CrossEntropyLoss
    m = m.to(DEV).train()
    if pr is not None:
        for k in list(pr.mask_dict):
            pr.mask_dict[k] = pr.mask_dict[k].to(DEV)
        pr.on_gpu = True
    crit = CrossEntropyLoss(ignore_index=255)
    opt = SGD(m.optim_parameters(), TC.LR, momentum=TC.MOMENTUM, weight_decay=TC.WD,
              pruner=pr if fused_mask else None, model=m if fused_mask else None)
    losses = []
    for x, t in zip(xs, ts):
        output = m(x.to(DEV))[0]
        loss = crit(output, t.to(DEV))
        opt.zero_grad()
        loss.backward()
        if grads_per_step is not None:
            grads_per_step.append({k: p.grad.detach().double().cpu() for k, p in m.named_parameters()
                                   if p.grad is not None})
        opt.step()
        if pr is not None and not fused_mask:
            pr.apply_masks(m)
        losses.append(float(loss.detach()))
    torch.cuda.synchronize()
    return m, losses


@pytest.mark.parametrize("fused_mask", [False, True])
def test_train_steps_match_reference(fused_mask):
    g = TC.load()
    m, pr = TC.model_and_masks(g)
    xs, ts = TC.inputs(g)
    masks = {k: v.float() for k, v in pr.mask_dict.items()}
    _, g64, _ = O.drnseg_train_steps(m.state_dict(), "drn_d_22", xs[:1], ts[:1], TC.LR, TC.MOMENTUM, TC.WD,
                                     masks=masks, dtype=torch.float64)
    _, _, f64 = O.drnseg_train_steps(m.state_dict(), "drn_d_22", xs, ts, TC.LR, TC.MOMENTUM, TC.WD,
                                     masks=masks, dtype=torch.float64)
    steps = []
    m, losses = _run_hip_steps(m, pr, xs, ts, fused_mask, grads_per_step=steps)
    np.testing.assert_allclose(losses, g[f"{TC.TAG}/losses"], rtol=1e-4)
    worst = worst_ref = 0.0
    for k, gr in steps[0].items():
        e = TC.rel_l2(gr.numpy(), g64[k].numpy())
        worst = max(worst, e)
        assert e <= 2.5e-3, (k, e)
    for k, gr in steps[1].items():
        e_ref = TC.rel_l2(TC.sample(gr).numpy(), g[f"{TC.TAG}/grad/{k}"])
        worst_ref = max(worst_ref, e_ref)
        assert e_ref <= 1e-2, (k, e_ref)
    for k, v in m.state_dict().items():
        key = f"{TC.TAG}/final/{k}"
        if key in g.files:
            e = TC.rel_err(TC.sample(v.detach().double().cpu()).numpy(), g[key])
            assert e <= 1e-4, (k, e)
            if v.is_floating_point():
                e64 = TC.rel_err(v.detach().double().cpu().numpy(), f64[k].numpy())
                assert e64 <= 1e-4, (k, e64)
    for k, mk in pr.mask_dict.items():
        w = m.state_dict()[k]
        assert torch.all(w[mk.to(w.device) == 0] == 0), k
    print(f"losses {losses}; step-1 grads vs fp64 {worst:.2e}; step-2 grads vs reference fp32 {worst_ref:.2e}")


# D-54 (Bottleneck, 2048-channel 1x1 convs) has many pre-activations near zero: the reference's
# own fp32 CPU gradients are 6e-3 (max-abs rel) away from fp64 on this case (scripts/archive/train_diag.py)
# D-24 / D-56 (two conv+BN+ReLU units in layer7 and layer8), seeds chosen on the CPU from the oracle alone:
#  * D-24, seed 5: the oracle's own fp32 CPU gradients are 4.0e-6 rel-L2 (worst parameter, layer.2.1.bias)
#    from its fp64 ones on this case (seeds 5 .. 8 tried: 4.0e-6, 1.3e-2, 4.4e-6, 1.1e-5), far inside the
#    2.5e-4 a case may spend of the 1e-3 gate;
#  * D-56, seed 7: tol = 4 x 4.75e-3 = 1.9e-2, 4.75e-3 being the rel-L2 of the oracle's fp32 CPU gradients
#    from its fp64 ones, worst over parameters (layer.6.2.conv1.weight): pre-activations within an ulp
#    of zero, as on D-54.  Seeds 5 .. 7 tried: 5.47e-3 (4 x that exceeds D-54's 2e-2), 1.2e-5, 4.75e-3.
#    Seed 6 is the one seed of the three on which torch's fp32 order happens to flip no ReLU; two in
#    three do, so another valid fp32 order (ours) may flip one there as well, and a tolerance of 4 x
#    rounding noise would gate on that luck, not on the kernels -- the first seed whose figure shows the
#    architecture's flips and stays within D-54's bound is taken.  (Every launch of a D-56 step is held
#    to fp64 without that slack in tests/train_audit.py d56_fp32x_1x64x64.)
@pytest.mark.parametrize("arch,seed,shape,tol", [("drn_d_38", 2, (1, 3, 64, 64), 1e-3),
                                                 ("drn_d_54", 3, (2, 3, 128, 128), 2e-2),
                                                 ("drn_d_22", 4, (1, 3, 72, 40), 1e-3),
                                                 ("drn_d_24", 5, (1, 3, 72, 40), 1e-3),
                                                 ("drn_d_56", 7, (1, 3, 64, 64), 1.9e-2)])
def test_train_step_matches_oracle(arch, seed, shape, tol):
    from drnmi.drnseg import DRNSeg
    from drnmi.weights import synth_state_dict
    torch.manual_seed(seed)
    m = DRNSeg(arch, 19, pretrained=False)
    m.load_state_dict(synth_state_dict(m, seed))
    x = torch.randn(*shape)
    t = torch.randint(0, 19, (shape[0], shape[2], shape[3]))
    t[torch.rand(t.shape) < 0.2] = 255
    losses, grads, final = O.drnseg_train_steps(m.state_dict(), arch, [x], [t], TC.LR, TC.MOMENTUM, TC.WD,
                                                dtype=torch.float64)
    m, hl = _run_hip_steps(m, None, [x], [t])
    assert abs(hl[0] - losses[0]) <= 1e-4 * abs(losses[0])
    worst = 0.0
    for k, p in m.named_parameters():
        if k.startswith("up."):
            continue
        e = TC.rel_l2(p.grad.detach().double().cpu().numpy(), grads[k].numpy())
        worst = max(worst, e)
        assert e <= tol, (k, e)
    print(f"{arch} {shape}: worst grad rel err vs fp64 {worst:.2e}")
    sd = m.state_dict()
    for k in ("layer.0.1.running_mean", "layer.0.1.running_var", "layer.0.1.num_batches_tracked"):
        np.testing.assert_allclose(sd[k].cpu().numpy(), final[k].numpy(), rtol=1e-4, atol=1e-6)


def test_train_grads_tight_vs_fp64():
    """No pre-activation within an ulp of zero on this case: every gradient is within 2e-5 of
    the fp64 value (max-abs relative) — the backward kernels themselves lose no precision."""
    from drnmi.drnseg import DRNSeg
    from drnmi.weights import synth_state_dict
    torch.manual_seed(0)
    m = DRNSeg("drn_d_22", 19, pretrained=False)
    m.load_state_dict(synth_state_dict(m, 11))
    x = torch.randn(2, 3, 64, 64)
    t = torch.randint(0, 19, (2, 64, 64))
    _, g64, _ = O.drnseg_train_steps(m.state_dict(), "drn_d_22", [x], [t], 0.0, 0.0, 0.0, dtype=torch.float64)
    steps = []
    m, _ = _run_hip_steps(m, None, [x], [t], grads_per_step=steps)
    worst = max(TC.rel_err(gr.numpy(), g64[k].numpy()) for k, gr in steps[0].items())
    print(f"worst gradient max-abs rel err vs fp64: {worst:.2e}")
    assert worst <= 2e-5


def test_train_is_deterministic():
    g = TC.load()
    outs = []
    for _ in range(2):
        m, pr = TC.model_and_masks(g)
        xs, ts = TC.inputs(g)
        m, losses = _run_hip_steps(m, pr, xs, ts)
        outs.append((losses, [p.detach().cpu().clone() for p in m.parameters()]))
    assert outs[0][0] == outs[1][0]
    assert all(torch.equal(a, b) for a, b in zip(outs[0][1], outs[1][1]))


@pytest.mark.parametrize("precision", ["fp32", "fp32x"])
def test_batched_weight_pack_matches_per_layer(precision, monkeypatch):
    """From the second step on the fine-tune re-packs every forward / dgrad weight (and the fp32x
    planes) in one launch (drnmi_pack_conv_weights_batched): losses and parameters after three
    steps are bit-identical to the per-layer packing."""
    import drnmi.train as T
    g = TC.load()
    outs = []
    for batched in (False, True):
        monkeypatch.setattr(T, "BATCHED_PACK", batched)
        m, pr = TC.model_and_masks(g)
        m.set_precision(precision)
        xs, ts = TC.inputs(g)
        m, losses = _run_hip_steps(m, pr, xs * 3, ts * 3)
        outs.append((losses, [p.detach().cpu().clone() for p in m.parameters()]))
        assert m._train_runner._packed_now == batched
    assert outs[0][0] == outs[1][0]
    assert all(torch.equal(a, b) for a, b in zip(outs[0][1], outs[1][1]))


def test_fused_bn_stats_match_separate_pass(monkeypatch):
    """fp32x: the BN batch statistics from the conv_x6 epilogue partials (FUSED_BN_STATS) vs the
    separate fp64 pass over y -- the same sums in another fixed order: three steps' losses and
    parameters agree to fp32 rounding."""
    import drnmi.train as T
    g = TC.load()
    outs = []
    for fused in (False, True):
        monkeypatch.setattr(T, "FUSED_BN_STATS", fused)
        m, pr = TC.model_and_masks(g)
        m.set_precision("fp32x")
        xs, ts = TC.inputs(g)
        m, losses = _run_hip_steps(m, pr, xs * 3, ts * 3)
        outs.append((losses, {k: v.detach().double().cpu() for k, v in m.state_dict().items()
                              if v.is_floating_point()}))
    np.testing.assert_allclose(outs[1][0], outs[0][0], rtol=1e-6)
    for k, v in outs[0][1].items():
        assert TC.rel_err(outs[1][1][k].numpy(), v.numpy()) <= 1e-5, k


@pytest.mark.parametrize("arch,shape", [("drn_d_54", (2, 3, 96, 64)), ("drn_d_22", (1, 3, 72, 40))])
def test_s2_class_dgrad_bit_identical(arch, shape, monkeypatch):
    """fp32x: the data gradient of every stride-2 conv as four parity-class convs of dy (y_sr
    strided stores, 2x2 / 1x1 class kernels) is bit-identical to the conv of the zero-inserted dy
    (3x3 classes with 1x1 .. 2x2 taps, and 1x1 downsamples whose odd classes no tap reaches).
    Split-K is off in both runs (it re-associates the sums)."""
    import drnmi.train as T
    from drnmi.drnseg import DRNSeg
    from drnmi.weights import synth_state_dict
    monkeypatch.setattr(T, "X6_SPLIT_K", False)
    torch.manual_seed(5)
    x = torch.randn(*shape)
    t = torch.randint(0, 19, (shape[0], shape[2], shape[3]))
    outs = []
    for cls in (False, True):
        monkeypatch.setattr(T, "S2_CLASS_DGRAD", cls)
        m = DRNSeg(arch, 19, pretrained=False)
        m.load_state_dict(synth_state_dict(m, 5))
        m.set_precision("fp32x")
        steps = []
        _run_hip_steps(m, None, [x, x], [t, t], grads_per_step=steps)
        outs.append(steps)
    for s0, s1 in zip(*outs):
        for k in s0:
            assert torch.equal(s0[k], s1[k]), k


def test_eval_after_train_uses_new_weights():
    """Training bumps parameter/buffer versions, so the eval plan repacks (drnseg._state_key)."""
    from drnmi.drnseg import DRNSeg
    from drnmi.weights import synth_state_dict
    m = DRNSeg("drn_d_22", 19, pretrained=False)
    m.load_state_dict(synth_state_dict(m, 6))
    x = torch.randn(1, 3, 64, 64)
    t = torch.randint(0, 19, (1, 64, 64))
    m, _ = _run_hip_steps(m, None, [x], [t])
    m.eval()
    lp, logits = m(x.to(DEV))
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    _, ref_logits, _ = O.drnseg_forward(sd, "drn_d_22", x)
    assert (logits.cpu() - ref_logits).abs().max().item() <= 1e-3


# ------------------------------------------------------------------ kernel-level checks
def _wgrad(dy_nhwc, x_nhwc, cin, cout, ks, stride, pad, dil, ho, wo, accumulate=None, x6=False):
    from drnmi import _lib
    lib = _lib.load()
    n, h, w, cs = x_nhwc.shape
    dw = accumulate.clone() if accumulate is not None else torch.empty(cout, cin, ks, ks, device=DEV)
    a = _lib.WgradArgs()
    a.dy, a.x, a.dw = dy_nhwc.data_ptr(), x_nhwc.data_ptr(), dw.data_ptr()
    a.n, a.h, a.w, a.cin, a.cin_stride = n, h, w, cin, cs
    a.ho, a.wo, a.cout, a.dy_stride = ho, wo, cout, dy_nhwc.shape[-1]
    a.ks, a.stride, a.pad, a.dil = ks, stride, pad, dil
    a.accumulate = 1 if accumulate is not None else 0
    nb = lib.drnmi_conv_wgrad_workspace_bytes(ctypes.byref(a))
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    a.ws, a.ws_bytes = ws.data_ptr(), nb
    fn = lib.drnmi_conv_wgrad_f32x3 if x6 else lib.drnmi_conv_wgrad_f32
    _lib.check(fn(ctypes.byref(a), ctypes.c_void_p(_lib.stream_ptr())), "wgrad")
    return dw


@pytest.mark.parametrize("cin,cs,cout,dys,ks,stride,pad,dil,h,w", [
    (3, 8, 16, 16, 7, 1, 3, 1, 40, 36),
    (16, 16, 32, 32, 3, 2, 1, 1, 33, 30),
    (64, 64, 64, 64, 3, 1, 2, 2, 20, 24),
    (128, 128, 256, 256, 1, 2, 0, 1, 18, 16),
    (512, 512, 19, 32, 1, 1, 0, 1, 12, 10),
    (256, 256, 512, 512, 3, 1, 4, 4, 16, 16),
    (96, 128, 200, 256, 3, 1, 1, 1, 13, 17),
    (256, 256, 256, 256, 3, 1, 2, 2, 48, 40),
    (3, 8, 16, 16, 7, 2, 3, 1, 30, 64),      # wo % 32 == 0: the direct small-cout fp32x kernel
    (16, 16, 16, 16, 3, 1, 1, 1, 9, 64),
    (16, 16, 32, 32, 3, 2, 1, 1, 21, 64),
    (32, 32, 19, 32, 1, 1, 0, 1, 5, 96),
])
@pytest.mark.parametrize("x6", [False, True])
def test_wgrad_kernel_matches_torch(cin, cs, cout, dys, ks, stride, pad, dil, h, w, x6):
    """fp32 wgrad and the fp32x split-bf16 one (drnmi_conv_wgrad_f32x3: the 64 x 64 tile, the
    128 x 128 tile where cout and K >= 128, the direct small-cout kernel where cout <= 32 and
    wo % 32 == 0; ragged cout / pixel counts included) vs torch autograd."""
    torch.manual_seed(cin + cout)
    n = 2
    x = torch.randn(n, cin, h, w)
    wt = torch.randn(cout, cin, ks, ks, requires_grad=True)
    y = F.conv2d(x, wt, stride=stride, padding=pad, dilation=dil)
    g = torch.randn_like(y)
    y.backward(g)
    ho, wo = y.shape[2], y.shape[3]
    xn = torch.zeros(n, h, w, cs)
    xn[..., :cin] = x.permute(0, 2, 3, 1)
    gn = torch.zeros(n, ho, wo, dys)
    gn[..., :cout] = g.permute(0, 2, 3, 1)
    dw = _wgrad(gn.to(DEV).contiguous(), xn.to(DEV).contiguous(), cin, cout, ks, stride, pad, dil, ho, wo, x6=x6)
    torch.cuda.synchronize()
    assert TC.rel_err(dw.cpu().numpy(), wt.grad.numpy()) <= 1e-4
    dw2 = _wgrad(gn.to(DEV).contiguous(), xn.to(DEV).contiguous(), cin, cout, ks, stride, pad, dil, ho, wo,
                 accumulate=dw, x6=x6)
    assert TC.rel_err(dw2.cpu().numpy(), 2 * wt.grad.numpy()) <= 1e-4


def test_bn_and_ce_kernels_match_torch():
    from drnmi import _lib
    from drnmi.train import CrossEntropyLoss
    lib = _lib.load()
    sp = ctypes.c_void_p(_lib.stream_ptr())
    torch.manual_seed(0)
    rows, C = 3000, 64
    y = torch.randn(rows, C) * 3 + 1
    gamma, beta = torch.rand(C) + 0.5, torch.randn(C)
    res = torch.randn(rows, C)
    # torch reference (NCHW-free: treat rows as batch of a 1x1 image per row)
    yt = y.clone().requires_grad_(True)
    gt, bt = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rm, rv = torch.zeros(C), torch.ones(C)
    z_ref = F.relu(F.batch_norm(yt, rm, rv, gt, bt, training=True, momentum=0.1, eps=1e-5) + res)
    dz = torch.randn(rows, C)
    z_ref.backward(dz)
    d = lambda t: t.to(DEV).contiguous()
    yd, gd, bd, rd, dzd = d(y), d(gamma), d(beta), d(res), d(dz)
    mean, invstd = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    rmd, rvd = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    nbt = torch.zeros((), dtype=torch.int64, device=DEV)
    ws = torch.empty(lib.drnmi_reduce_workspace_bytes(rows, C), dtype=torch.uint8, device=DEV)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    _lib.check(lib.drnmi_bn_stats_f32(vp(yd), rows, C, 1e-5, 0.1, vp(mean), vp(invstd), vp(rmd), vp(rvd), vp(nbt),
                                      vp(ws), sp), "stats")
    z = torch.empty_like(yd)
    _lib.check(lib.drnmi_bn_act_f32(vp(yd), vp(mean), vp(invstd), vp(gd), vp(bd), vp(rd), 1, rows, C, vp(z), sp), "act")
    dy = torch.empty_like(yd)
    dres = torch.empty_like(yd)
    dg, db = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    _lib.check(lib.drnmi_bn_act_bwd_f32(vp(dzd), vp(z), vp(yd), vp(mean), vp(invstd), vp(gd), 1, rows, C, vp(dy),
                                        vp(dres), 0, vp(dg), vp(db), 0, vp(ws), sp), "bwd")
    torch.cuda.synchronize()
    assert TC.rel_err(z.cpu(), z_ref.detach()) <= 1e-5
    assert TC.rel_err(rmd.cpu(), rm) <= 1e-5 and TC.rel_err(rvd.cpu(), rv) <= 1e-5 and int(nbt) == 1
    assert TC.rel_err(dy.cpu(), yt.grad) <= 1e-4
    assert TC.rel_err(dg.cpu(), gt.grad) <= 1e-4 and TC.rel_err(db.cpu(), bt.grad) <= 1e-5
    assert TC.rel_err(dres.cpu(), dz * (z_ref.detach() > 0)) == 0.0
    # residual-free BN + ReLU: the backward that recomputes the mask from y is bit-identical to the
    # one that reads z (many y sit exactly on the mean: ties at bn_value == 0 included)
    yq = yd.clone()
    yq[::7] = mean
    _lib.check(lib.drnmi_bn_stats_f32(vp(yq), rows, C, 1e-5, 0.1, vp(mean), vp(invstd), None, None, None, vp(ws), sp),
               "stats q")
    bz = bd.clone()
    bz[::3] = 0.0
    zq = torch.empty_like(yq)
    _lib.check(lib.drnmi_bn_act_f32(vp(yq), vp(mean), vp(invstd), vp(gd), vp(bz), None, 1, rows, C, vp(zq), sp), "act q")
    outs = []
    for from_y in (False, True):
        dyq, dgq, dbq = torch.empty_like(yq), torch.empty(C, device=DEV), torch.empty(C, device=DEV)
        if from_y:
            _lib.check(lib.drnmi_bn_relu_bwd_y_f32(vp(dzd), vp(yq), vp(mean), vp(invstd), vp(gd), vp(bz), rows, C,
                                                   vp(dyq), vp(dgq), vp(dbq), 0, vp(ws), sp), "bwd y")
        else:
            _lib.check(lib.drnmi_bn_act_bwd_f32(vp(dzd), vp(zq), vp(yq), vp(mean), vp(invstd), vp(gd), 1, rows, C,
                                                vp(dyq), None, 0, vp(dgq), vp(dbq), 0, vp(ws), sp), "bwd z")
        outs.append((dyq, dgq, dbq))
    torch.cuda.synchronize()
    assert int((zq == 0).sum()) > rows * C // 4
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    # cross entropy on log-probs with ignore_index
    lp = F.log_softmax(torch.randn(2, 19, 24, 40), 1).requires_grad_(True)
    t = torch.randint(0, 19, (2, 24, 40))
    t[torch.rand(t.shape) < 0.3] = 255
    loss_ref = F.cross_entropy(lp, t, ignore_index=255)
    loss_ref.backward()
    lpd = lp.detach().to(DEV).requires_grad_(True)
    loss = CrossEntropyLoss(ignore_index=255)(lpd, t.to(DEV))
    loss.backward()
    assert abs(loss.item() - loss_ref.item()) <= 1e-5 * abs(loss_ref.item())
    assert TC.rel_err(lpd.grad.cpu(), lp.grad) <= 1e-5


@pytest.mark.parametrize("h,w", [(6, 9), (11, 70)])
def test_head_backward_matches_autograd(h, w):
    """LogSoftmax + x8 transpose-conv backward (the LDS-tiled up8_bwd_kernel: 4 x 32 outputs per
    workgroup, so 11 x 70 has ragged tiles in both directions) against autograd, and the
    logits-only gradient (no log-prob term)."""
    from drnmi.drnseg import DRNSeg
    from drnmi import _lib
    lib = _lib.load()
    m = DRNSeg("drn_d_22", 19, pretrained=False)
    upw = m.up.weight.detach()
    torch.manual_seed(1)
    logits = torch.randn(2, 19, h, w, requires_grad=True)
    lp = F.log_softmax(F.conv_transpose2d(logits, upw, stride=8, padding=4, groups=19), 1)
    g = torch.randn_like(lp)
    gl = torch.randn_like(logits)
    (lp * g).sum().backward()
    ref = logits.grad + gl
    gd, lpd, gld, upd = [t.detach().to(DEV).contiguous() for t in (g, lp, gl, upw[0, 0])]
    du = torch.empty_like(lpd)
    out = torch.empty_like(gld)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    _lib.check(lib.drnmi_up8_lsm_bwd_f32(vp(gd), vp(lpd), vp(gld), vp(upd), 1.0, 2, 19, h, w, vp(du),
                                         vp(out), ctypes.c_void_p(_lib.stream_ptr())), "up8_lsm_bwd")
    out2 = torch.empty_like(gld)
    _lib.check(lib.drnmi_up8_lsm_bwd_f32(None, None, vp(gld), vp(upd), 0.5, 2, 19, h, w, None,
                                         vp(out2), ctypes.c_void_p(_lib.stream_ptr())), "up8_lsm_bwd logits-only")
    torch.cuda.synchronize()
    assert TC.rel_err(out.cpu(), ref) <= 1e-5
    assert torch.equal(out2.cpu(), 0.5 * gl)


@pytest.mark.parametrize("shape", [(2, 24, 40), (1, 23, 41)])
def test_ce_matches_torch_shapes(shape):
    """CE forward / backward (register-held classes; hw % 4 == 0 takes the four-pixel backward,
    23 x 41 the per-pixel one) against torch, ignore_index and all-ignored rows included."""
    from drnmi.train import CrossEntropyLoss
    n, h, w = shape
    g = torch.Generator().manual_seed(h * w)
    lp = F.log_softmax(torch.randn(n, 19, h, w, generator=g) * 3, 1).requires_grad_(True)
    t = torch.randint(0, 19, (n, h, w), generator=g)
    t[torch.rand(t.shape, generator=g) < 0.3] = 255
    t[0, 0] = 255
    loss_ref = F.cross_entropy(lp, t, ignore_index=255)
    loss_ref.backward()
    lpd = lp.detach().to(DEV).requires_grad_(True)
    loss = CrossEntropyLoss(ignore_index=255)(lpd, t.to(DEV))
    loss.backward()
    assert abs(loss.item() - loss_ref.item()) <= 1e-5 * abs(loss_ref.item())
    assert TC.rel_err(lpd.grad.cpu(), lp.grad) <= 1e-5


@pytest.mark.parametrize("nesterov,damp", [(False, 0.0), (True, 0.0), (False, 0.3)])
def test_sgd_matches_torch(nesterov, damp):
    from drnmi.train import SGD
    torch.manual_seed(2)
    ps = [torch.randn(33, 7), torch.randn(1000), torch.randn(5)]
    ref = [p.clone().requires_grad_(True) for p in ps]
    mine = [torch.nn.Parameter(p.clone().to(DEV)) for p in ps]
    kw = dict(lr=0.05, momentum=0.9, dampening=damp, weight_decay=1e-3, nesterov=nesterov)
    o_ref = torch.optim.SGD(ref, **kw)
    o = SGD(mine, **kw)
    for step in range(3):
        gs = [torch.randn_like(p) for p in ps]
        for r, q, gg in zip(ref, mine, gs):
            r.grad = gg.clone()
            q.grad = gg.to(DEV)
        o_ref.step()
        o.step()
    for r, q in zip(ref, mine):
        assert TC.rel_err(q.detach().cpu(), r.detach()) <= 1e-6


def test_sgd_matches_torch_100_tensors_masked():
    """100 small tensors, every third with a pruner mask: three 48-tensor launches, the last ragged (4
    tensors), masked and unmasked parameters mixed in each -- the batching a 109 / 111-conv net's step
    goes through (about 7 launches) -- against torch.optim.SGD followed by the mask multiply."""
    from drnmi import pruners as P
    from drnmi.train import SGD

    class Masks(P.Pruner):
        def parse_config_file(self, config_fp):
            return []

    torch.manual_seed(3)
    shapes = [(1 + i % 7, 3 + i % 5) if i % 2 else (5 + 11 * (i % 9),) for i in range(100)]
    ps = [torch.randn(*s) for s in shapes]
    masks = {i: (torch.rand(*shapes[i]) < 0.5).float() for i in range(0, 100, 3)}
    ref = [p.clone().requires_grad_(True) for p in ps]
    model = torch.nn.Module()
    model.ps = torch.nn.ParameterList([torch.nn.Parameter(p.clone().to(DEV)) for p in ps])
    mine = list(model.ps)
    pr = Masks(None, on_gpu=True)
    for i, mk in masks.items():
        pr.mask_dict[f"ps.{i}"] = mk.to(DEV)
    kw = dict(lr=0.05, momentum=0.9, dampening=0.0, weight_decay=1e-3, nesterov=False)
    o_ref = torch.optim.SGD(ref, **kw)
    o = SGD(mine, pruner=pr, model=model, **kw)
    assert len(o._mask_of) == 34
    for step in range(3):
        gs = [torch.randn_like(p) for p in ps]
        for r, q, gg in zip(ref, mine, gs):
            r.grad = gg.clone()
            q.grad = gg.to(DEV)
        o_ref.step()
        with torch.no_grad():
            for i, mk in masks.items():
                ref[i].mul_(mk)
        o.step()
    for i, (r, q) in enumerate(zip(ref, mine)):
        assert TC.rel_err(q.detach().cpu(), r.detach()) <= 1e-6, i
        if i in masks:
            assert bool((q.detach().cpu()[masks[i] == 0] == 0).all()), i
            assert TC.rel_err(o.state[q]["momentum_buffer"].cpu(), o_ref.state[r]["momentum_buffer"]) <= 1e-6, i
