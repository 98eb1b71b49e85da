"""fp8 precision (OCP e4m3 on v_mfma_f32_16x16x128_f8f6f4; include/drnmi.h DRNMI_F8) on the GPU,
against tests/fp8_ref.py: the quantiser byte for byte, the conv kernels bit for bit on integer
data (the MFMA lane-map proof) and within the accumulation bound on real data, every fp8 launch
of a network, labels against the reference's, the user-facing paths and the refusals."""
import ctypes

import numpy as np
import pytest
import torch

import fp8_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"

# Accumulation constant of the bound |acc - acc64| <= ACC_C * sum|a b| (fp8_ref.tolerance): 4 x the
# largest ratio measured on the CASES below with fp32 output, scale 1 and shift 0
# (test_accumulation_constant prints them; profiles/fp8/README.txt).  Measured on MI355X: 1.825e-05, on
# the 1x1 64 -> 128 case (K = 64, one MFMA per output); 1.17e-05 at K = 128, 1.6e-06 .. 5.8e-06 on the
# 3x3 cases (K = 576 .. 9216).  The short-K figures are above what a k-ordered fp32 chain explains
# (K * 2^-24 = 3.8e-06 at K = 64): the error is set by the instruction's own summation of its products,
# about 2^-16 of their sum|a b|, and averages out rather than grows over the MFMAs of a long K.  The
# strip-staged kernel gives the generic kernel's figures digit for digit (the same K order), and so
# does the K-64 step shape on the 1x1 cases (each K-128 as two half-zero MFMAs).
ACC_MEASURED = 1.825e-05
ACC_C = 4 * ACC_MEASURED

# (n, h, w, cin, cout, ks, stride, dil, residual)
GENERIC = [
    (1, 16, 24, 256, 256, 3, 1, 2, True),
    (2, 9, 13, 128, 128, 3, 1, 1, False),       # ragged pixel tile, the 128-wide tile
    (1, 16, 16, 64, 128, 3, 2, 1, False),       # cin 64: 64-B rows, the K-64 step; stride 2
    (1, 16, 16, 64, 128, 1, 2, 1, False),       # 1x1 stride-2 downsample
    (1, 10, 10, 512, 19, 1, 1, 1, False),       # seg head: cout 19 (fp32 outputs only)
    (1, 9, 17, 128, 256, 1, 1, 1, True),        # ragged 1x1 with a residual
]
# whole 256-pixel output rows, cin % 256 == 0, cout % 256 == 0: conv_f8_stag_kernel
STAG = [
    (1, 5, 256, 256, 256, 3, 1, 2, True),
    (1, 4, 512, 512, 512, 3, 1, 4, True),
    (2, 3, 256, 1024, 256, 3, 1, 1, False),
]
# (2, 3, 256, 128 -> 128, d1, residual) is not admitted by the strip check for fp8 (cin % 256 != 0);
# it runs on the generic kernel like every other 128 -> 128 launch:
GENERIC_ROWS = [(2, 3, 256, 128, 128, 3, 1, 1, True)]
CASES = GENERIC + GENERIC_ROWS + STAG


def _lib():
    from drnmi import _lib
    return _lib, _lib.load()


def _stream():
    from drnmi import _lib
    return ctypes.c_void_p(_lib.stream_ptr(torch.device(DEV)))


def _finite_bf16():
    bits = np.arange(1 << 16, dtype=np.uint16)
    x = torch.from_numpy(bits.view(np.int16).copy()).view(torch.bfloat16)
    return x[~torch.isnan(x.float())]               # every pattern but the NaNs (the infinities stay)


def _quantize_gpu(x, inv):
    L, lib = _lib()
    y = torch.full((x.numel() + 16,), 0xA5, dtype=torch.uint8, device=DEV)
    code = L.DRNMI_BF16 if x.dtype == torch.bfloat16 else L.DRNMI_F32
    L.check(lib.drnmi_quantize_f8(x.data_ptr(), code, x.numel(), inv, y.data_ptr(), _stream()), "quantize_f8")
    torch.cuda.synchronize()
    assert bool((y[x.numel():] == 0xA5).all()), "wrote past n"
    return y[:x.numel()].cpu()


@pytest.mark.parametrize("scale", [1.0, 0.37, 2.0 ** -5])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_quantize_f8_exact(dtype, scale):
    x = _finite_bf16()
    assert x.numel() % 16 != 0                      # 65282 values: the scalar tail runs
    if dtype == "f32":
        x = x.float()
    inv = float(np.float32(1.0 / scale))
    got = _quantize_gpu(x.to(DEV), inv)
    ref = R.quantize(x, inv)
    assert torch.equal(got, ref), f"{int((got != ref).sum())} bytes differ"
    # lengths 1 .. 33: every tail length, with and without a vector body
    for n in (1, 15, 16, 17, 33):
        assert torch.equal(_quantize_gpu(x[1000:1000 + n].contiguous().to(DEV), inv), ref[1000:1000 + n])


def _geom(case):
    n, h, w, cin, cout, ks, st, dil, has_res = case
    pad = dil * (ks // 2)
    ho = (h + 2 * pad - dil * (ks - 1) - 1) // st + 1
    wo = (w + 2 * pad - dil * (ks - 1) - 1) // st + 1
    return pad, ho, wo, (cout + 127) // 128 * 128


def _launch(case, t, out, tile=-1, ysp=None):
    """One DRNMI_F8 launch of `case` on the device tensors t (x, w, scale, shift, res) -> output on the host:
    "f32" NCHW planes, "f32rows" NHWC rows of ysp floats, "bf16" / "f8" dense NHWC."""
    L, lib = _lib()
    n, h, w, cin, cout, ks, st, dil, has_res = case
    pad, ho, wo, cout_pad = _geom(case)
    a = L.ConvArgs()
    a.x, a.wgt, a.scale, a.shift = (t[k].data_ptr() for k in ("x", "w", "scale", "shift"))
    a.res = t["res"].data_ptr() if has_res else None
    if out == "f32":
        y = torch.full((n, cout, ho, wo), float("nan"), device=DEV)
        a.y_sn, a.y_sp, a.y_sc, a.out_dtype = cout * ho * wo, 1, ho * wo, L.DRNMI_F32
    elif out == "f32rows":
        y = torch.full((n, ho, wo, ysp), 7.0, device=DEV)
        a.y_sn, a.y_sp, a.y_sc, a.out_dtype = ho * wo * ysp, ysp, 1, L.DRNMI_F32
    else:
        y = torch.zeros((n, ho, wo, cout), dtype=torch.uint8 if out == "f8" else torch.bfloat16, device=DEV)
        a.y_sn, a.y_sp, a.y_sc = ho * wo * cout, cout, 1
        a.out_dtype = L.DRNMI_F8 if out == "f8" else L.DRNMI_BF16
    a.y = y.data_ptr()
    a.n, a.h, a.w, a.cin, a.ho, a.wo, a.cout, a.cout_pad = n, h, w, cin, ho, wo, cout, cout_pad
    a.ks, a.stride, a.pad, a.dil, a.k, a.k_pad = ks, st, pad, dil, ks * ks * cin, ks * ks * cin
    a.relu, a.dtype, a.tile, a.algo = t["relu"], L.DRNMI_F8, tile, L.ALGO_IGEMM
    a.res_scale, a.out_scale = t["res_scale"], t["out_scale"]
    name = lib.drnmi_conv_kernel_name(ctypes.byref(a))
    assert name is not None, (case, out, tile)
    want = "conv_f8_stag_kernel" if case in STAG else "conv_f8_occ2_kernel<" if ks == 1 else "conv_f8_kernel<"
    assert name.decode().startswith(want), (name, case)
    L.check(lib.drnmi_conv2d_bn_act(ctypes.byref(a), _stream()), f"conv f8 {case} {out} tile {tile}")
    torch.cuda.synchronize()
    y = y.cpu()
    if out == "f32":
        return y.permute(0, 2, 3, 1).contiguous()
    if out == "f32rows":
        assert bool((y[..., (cout + 3) // 4 * 4:] == 7.0).all()), "wrote past the row's own padding"
        return y[..., :cout].contiguous()
    return y


def _outs(case):
    return ("f32", "f32rows") if case[4] == 19 else ("f32", "bf16", "f8")


def _tiles(case):
    return (-1, 19) if case in STAG else (-1,)


def _to_dev(t):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in t.items()}


_INT = {}


def _int_case(case):
    """Integer operands as e4m3 bytes (every integer up to 16 is an e4m3 value) and the exact result."""
    if case not in _INT:
        n, h, w, cin, cout, ks, st, dil, has_res = case
        pad, ho, wo, cout_pad = _geom(case)
        g = torch.Generator().manual_seed(CASES.index(case))
        k = ks * ks * cin
        x = torch.randint(0, 4, (n, h, w, cin), generator=g).float()
        wt = torch.zeros(cout_pad, k)
        wt[:cout] = torch.randint(-2, 3, (cout, k), generator=g).float()     # independent per (row, k): asymmetric
        t = {"x": R.e4m3(x), "w": R.e4m3(wt), "scale": torch.ones(cout_pad),
             "shift": torch.randint(-3, 4, (cout_pad,), generator=g).float(), "relu": CASES.index(case) % 2,
             "res": R.e4m3(torch.randint(-3, 4, (n, ho, wo, cout), generator=g).float()) if has_res else None,
             "res_scale": 1.0, "out_scale": 2.0 ** -7}
        assert torch.equal(R.dequant(t["x"]).float(), x) and torch.equal(R.dequant(t["w"]).float(), wt)
        ref = R.conv_f8(t["x"], t["w"], t["scale"], t["shift"], cout, ks, st, pad, dil, bool(t["relu"]), t["res"], 1.0,
                        t["out_scale"])
        assert float(ref["sumabs"].max()) < 2 ** 24 and float(ref["acc"].abs().max()) > 64   # exact in fp32, not trivial
        _INT[case] = (_to_dev(t), ref)
    return _INT[case]


@pytest.mark.parametrize("case", CASES)
def test_conv_f8_exact_on_integers(case):
    """A = integer weights drawn per (row, k), B = integer activations: every product and partial sum
    is an integer below 2^24, so any summation order gives the same fp32 bits and a wrong pairing of
    A and B K positions inside the K-128 MFMA (or a wrong row, tap, pad or tail) cannot."""
    t, ref = _int_case(case)
    v = ref["v"]
    for tile in _tiles(case):
        for out in _outs(case):
            got = _launch(case, t, out, tile, ysp=20)
            if out in ("f32", "f32rows"):
                assert torch.equal(got, v.float()), (out, tile, float((got - v.float()).abs().max()))
            elif out == "bf16":
                assert torch.equal(got.view(torch.int16), v.float().to(torch.bfloat16).view(torch.int16)), (out, tile)
            else:
                assert torch.equal(got, R.e4m3(ref["vq"])), (out, tile)
                assert 0 < float((got & 0x7F).float().mean()), "all-zero output"


_REAL = {}


def _real_case(case):
    """Gaussian data through the real quantisers: activations and residual by drnmi_quantize_f8, weights
    by the pack's arithmetic (fp8_ref.pack_weights)."""
    if case not in _REAL:
        n, h, w, cin, cout, ks, st, dil, has_res = case
        pad, ho, wo, cout_pad = _geom(case)
        g = torch.Generator().manual_seed(100 + CASES.index(case))
        k = ks * ks * cin
        sx, sr, sy = 3.0 / 448, 2.5 / 448, 3.0 / 448            # clips at 3 / 2.5 / 3 sigma: some saturation
        xb = torch.randn(n, h, w, cin, generator=g).to(torch.bfloat16)
        x8 = _quantize_gpu(xb.to(DEV).view(-1), float(np.float32(1 / sx))).view(n, h, w, cin)
        assert torch.equal(x8, R.quantize(xb, float(np.float32(1 / sx))))
        wt = torch.zeros(cout_pad, k)
        wt[:cout] = torch.randn(cout, k, generator=g) * (1.0 / k ** 0.5)
        w8, sw = R.pack_weights(wt)
        bn = torch.ones(cout_pad)
        bn[:cout] = torch.rand(cout, generator=g) + 0.5
        t = {"x": x8, "w": w8, "scale": (sw * sx * bn).float(), "shift": torch.randn(cout_pad, generator=g) * 0.5,
             "relu": 1, "res": None, "res_scale": sr, "out_scale": 1 / sy}
        if has_res:
            rb = torch.randn(n, ho, wo, cout, generator=g).to(torch.bfloat16)
            t["res"] = _quantize_gpu(rb.to(DEV).view(-1), float(np.float32(1 / sr))).view(n, ho, wo, cout)
        ref = R.conv_f8(t["x"], t["w"], t["scale"], t["shift"], cout, ks, st, pad, dil, True, t["res"], sr, 1 / sy)
        _REAL[case] = (_to_dev(t), ref)
    return _REAL[case]


def _check_real(got, ref, out, out_scale, where):
    tol = R.tolerance(ref, ACC_C, out, out_scale)
    if out == "f8":
        lo, hi = R.f8_interval(ref, tol)
        g = R.dequant(got)
        bad = (g < lo) | (g > hi)
        assert not bool(bad.any()), f"{where}: {int(bad.sum())} of {bad.numel()} fp8 outputs outside [e4m3(ref - tol), e4m3(ref + tol)]"
        return float((lo != hi).double().mean())
    err = (got.to(torch.float64) - ref["v"]).abs()
    bad = err > tol
    assert not bool(bad.any()), f"{where}: {int(bad.sum())} outputs off by up to {float((err / tol).max()):.2f} x the bound"
    return float((err / tol).max())


@pytest.mark.parametrize("case", CASES)
def test_conv_f8_real_values(case):
    t, ref = _real_case(case)
    assert float(ref["v"].abs().mean()) > 0.05 and float((ref["v"] == 0).double().mean()) < 0.9
    for tile in _tiles(case):
        for out in _outs(case):
            got = _launch(case, t, out, tile, ysp=20)
            r = _check_real(got, ref, out, t["out_scale"], f"{case} {out} tile {tile}")
            print(f"{case} {out} tile {tile}: {'open intervals' if out == 'f8' else 'max err / bound'} {r:.3f}")


def test_accumulation_constant():
    """Measures max |acc - acc64| / sum|a b| (fp32 output, scale 1, shift 0) over the cases: ACC_C is 4 x
    the measured maximum, and never below it here."""
    worst = 0.0
    for case in CASES:
        t, ref = _real_case(case)
        cout_pad = _geom(case)[3]
        u = dict(t, scale=torch.ones(cout_pad, device=DEV), shift=torch.zeros(cout_pad, device=DEV), relu=0)
        if case[8]:
            u["res"] = torch.zeros_like(t["res"])
        for tile in _tiles(case):
            got = _launch(case, u, "f32", tile).to(torch.float64)
            ratio = float(((got - ref["acc"]).abs() / ref["sumabs"].clamp_min(1e-30)).max())
            exact = float((got.float() == ref["acc"].float()).double().mean())
            k = case[5] ** 2 * case[3]
            print(f"{case} tile {tile}: max |acc - acc64| / sum|ab| = {ratio:.3e} (K * 2^-24 = {k * 2.0 ** -24:.3e}); "
                  f"equal to fp32(acc64): {exact:.4f}")
            worst = max(worst, ratio)
    print(f"max over the cases: {worst:.3e}; ACC_C = {ACC_C:.3e}")
    assert worst <= ACC_C


# ------------------------------------------------------------------------------------------ networks
def _norm():
    from drnmi.drnseg import INFO_MEAN, INFO_STD
    return INFO_MEAN, INFO_STD


@pytest.mark.parametrize("model,shape", [("drn_d_22", (2, 64, 128)), ("drn_d_54", (1, 32, 64)),
                                         ("drn_d_24", (2, 72, 136)), ("drn_d_107", (1, 32, 64))])
def test_fp8_network_every_launch(model, shape):
    """keep_all fp8 plan, synthetic weights, absmax scales of one calibration batch: every fp8 launch
    re-stated from the kernel's own input buffers, every quantised copy byte for byte, and the same
    launches 8-bit as in the int8 plan."""
    from drnmi import _lib as L
    from drnmi.drnseg import build
    from drnmi.weights import synth_frames
    n, h, w = shape
    m = build(model, 19, seed=0, device=DEV)
    frames = torch.from_numpy(synth_frames(7, n, h, w)).to(DEV)
    m.calibrate_int8(frames)
    i8_plan = m.set_precision("int8").plan(n, h, w, keep_all=True)
    want = {i for i, nd in enumerate(i8_plan.packed.graph.nodes) if nd.i8}
    plan = m.set_precision("fp8").plan(n, h, w, keep_all=True)
    pk = plan.packed
    lib = L.load()
    got8 = set()
    for l in plan.launches("u8"):
        nm = l.kernel_name(lib)
        if nm.startswith("conv_f8"):
            got8.update(l.nodes)
    assert got8 == {i for i, nd in enumerate(pk.graph.nodes) if nd.i8} == want and len(want) >= 10
    i8_names = {i8_plan.launches("u8")[k].kernel_name(lib) for k in range(len(i8_plan.launches("u8")))}
    assert any("i8" in s for s in i8_names)
    stream = L.stream_ptr(torch.device(DEV))
    plan.ingest_u8(frames, *_norm(), False, stream)
    plan.run_backbone(stream)
    torch.cuda.synchronize()
    assert pk.quant_after
    for vals in pk.quant_after.values():
        for v in vals:
            ref = R.quantize(plan.bufs[v].cpu(), float(np.float32(1.0 / pk.act_scale(v))))
            assert torch.equal(plan.bufs["q:" + v].cpu(), ref), v
    has_f8_res = False
    for i in sorted(want):
        nd = pk.graph.nodes[i]
        kw, out = R.node_case(plan, nd)
        has_f8_res |= kw["res"] is not None and nd.conv.kernel_size[0] == 1
        ref = R.conv_f8(**kw)
        oh, ow = plan.shapes[nd.dst]
        got = plan.bufs[nd.dst].cpu()
        got = got.permute(0, 2, 3, 1).contiguous() if out == "f32" else got.view(n, oh, ow, -1)
        _check_real(got, ref, out, nd.out_scale, f"{model} {nd.name}")
    assert has_f8_res == (model in ("drn_d_54", "drn_d_107"))      # Bottleneck 1x1s with an fp8 residual
    if model in ("drn_d_24", "drn_d_107"):         # the two-conv tail: every unit 8-bit, fp8 values in between
        names = {pk.graph.nodes[i].name for i in want}
        assert {"layer.7.0", "layer.7.3", "layer.8.0", "layer.8.3", "seg"} <= names
        by = {nd.name: nd for nd in pk.graph.nodes}
        assert all(pk.value_code(by[k].dst) == L.DRNMI_F8 for k in ("layer.7.0", "layer.7.3", "layer.8.0", "layer.8.3"))


_NET = {}


def _net(golden):
    if "m" not in _NET:
        from drnmi.drnseg import build
        case = "d22_2x128x256"
        m = build("drn_d_22", 19, seed=int(golden[case + "/meta"][0]), device=DEV)
        frames = torch.from_numpy(golden[case + "/frames"]).to(DEV)
        m.calibrate_int8(frames)
        _NET["m"], _NET["frames"] = m, frames
    return _NET["m"], _NET["frames"]


# just below the fp8 agreement with the reference fp32 labels measured on MI355X: 0.8819 of 65536 px
# (int8 in the same run: 0.9566, bf16: 0.9944).  fp8 does NOT reach the int8 agreement on this case:
# with one scale per tensor and these hash-initialised weights (no outliers for a linear grid to waste
# its range on) e4m3's 3 mantissa bits -- a relative step of 2^-3 on every weight and activation --
# cost more than int8's absolute step of clip / 127.  A finding (README.md), so the gate is
# the measured floor alone; the int8 figure of the same run is printed beside it.
FP8_AGREE = 0.875


def test_fp8_labels_vs_reference(golden_forward):
    """fp8 network vs the reference fp32 forward (the goldens test_int8_labels_vs_reference uses).
    Measured: fp8 0.8819, int8 0.9566, bf16 0.9944 -- fp8 is below int8 here, see FP8_AGREE."""
    m, frames = _net(golden_forward)
    ref = golden_forward["d22_2x128x256/labels"]
    agree = {}
    for prec in ("int8", "fp8", "bf16"):
        lab = m.set_precision(prec).segment(frames).long().cpu().numpy()
        agree[prec] = float((lab == ref).mean())
    print(f"label agreement with the reference fp32 forward: fp8 {agree['fp8']:.4f}, int8 {agree['int8']:.4f}, "
          f"bf16 {agree['bf16']:.4f}")
    assert agree["fp8"] >= FP8_AGREE


def test_fp8_paths_agree(golden_forward):
    """segment() / predict() / forward() in fp8 as in int8; size=, render=, a captured graph; and the
    other precisions' labels are untouched by switching through fp8."""
    from oracle import drn_oracle as O
    m, frames = _net(golden_forward)
    before = {p: m.set_precision(p).segment(frames).clone() for p in ("bf16", "int8")}
    m.set_precision("fp8")
    plan = m.plan(*frames.shape[:3])
    assert plan.labels_path() == "nhwc" and plan.seg_fused is None
    seg = m.segment(frames)
    x = O.preprocess_u8(frames.cpu().numpy()).to(DEV)
    pred = m.predict(x)
    lp, logits = m(x)
    assert torch.equal(pred, torch.max(lp, 1)[1])
    # the labels-only NHWC head on the fp8 seg conv's rows gives the labels of the logits planes
    from drnmi import engine
    engine.LABELS_NHWC = False
    try:
        assert m.plan(*frames.shape[:3]).labels_path() == "nchw"
        assert torch.equal(m.segment(frames), seg)
    finally:
        engine.LABELS_NHWC = True
    # segment() runs the fused uint8 front (f16 stem arithmetic on the frame bytes), predict() the three
    # bf16 convs on the host-normalised floats: two roundings of the same 32-channel layer2 output.  On
    # these hash-initialised weights an 8-bit net turns that into label changes -- int8 too (no test
    # gates it there).  Measured on MI355X: fp8 0.9109, int8 0.9529 of 65536 px; the floor sits just below
    # the fp8 figure (the FP8_AGREE convention) and int8's is printed beside it.
    same = {}
    for p in ("int8", "fp8"):
        m.set_precision(p)
        same[p] = float((m.segment(frames).long() == m.predict(x)).float().mean())
    print(f"segment() == predict(): fp8 {same['fp8']:.4f}, int8 {same['int8']:.4f}")
    assert same["fp8"] >= 0.90
    small = m.segment(frames, size=(96, 160))
    assert small.shape == (frames.shape[0], 96, 160) and small.dtype == torch.uint8
    lab2, img = m.segment(frames, render="overlay")
    assert torch.equal(lab2, seg) and img.shape == frames.shape and img.dtype == torch.uint8
    out = torch.empty_like(seg)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        m.segment(frames, labels=out)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            m.segment(frames, labels=out)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, seg)
    for p in ("bf16", "int8", "fp8", "bf16", "int8"):
        lab = m.set_precision(p).segment(frames)
        assert torch.equal(lab, seg if p == "fp8" else before[p]), p


def test_fp8_refusals(golden_forward):
    L, lib = _lib()
    case = STAG[0]
    t, _ = _int_case(case)
    n, h, w, cin, cout, ks, st, dil, has_res = case
    pad, ho, wo, cout_pad = _geom(case)
    a = L.ConvArgs()
    y = torch.full((n * ho * wo * cout,), 0x5A, dtype=torch.uint8, device=DEV)
    a.x, a.wgt, a.scale, a.shift, a.y = t["x"].data_ptr(), t["w"].data_ptr(), t["scale"].data_ptr(), t["shift"].data_ptr(), y.data_ptr()
    a.n, a.h, a.w, a.cin, a.ho, a.wo, a.cout, a.cout_pad = n, h, w, cin, ho, wo, cout, cout_pad
    a.ks, a.stride, a.pad, a.dil, a.k, a.k_pad = ks, st, pad, dil, ks * ks * cin, ks * ks * cin
    a.y_sn, a.y_sp, a.y_sc = ho * wo * cout, cout, 1
    a.dtype, a.out_dtype, a.algo, a.out_scale = L.DRNMI_F8, L.DRNMI_F8, L.ALGO_IGEMM, 1.0
    for tile in (L.TILE_W1, L.TILE_W1H):
        a.tile = tile
        assert lib.drnmi_conv2d_bn_act(ctypes.byref(a), _stream()) == -2
    a.tile = -1
    part = torch.zeros(2 * n * ho * wo * 20, dtype=torch.float32, device=DEV)
    assert lib.drnmi_conv_stag_seg(ctypes.byref(a), t["w"].data_ptr(), cout, 32, part.data_ptr(), _stream()) == -2
    a.out_dtype = L.DRNMI_I8
    assert lib.drnmi_conv2d_bn_act(ctypes.byref(a), _stream()) == -1
    torch.cuda.synchronize()
    assert bool((y == 0x5A).all()) and not bool(part.any()), "a refused launch wrote"
    m, frames = _net(golden_forward)
    m.set_precision("fp8").train()
    try:
        with pytest.raises(NotImplementedError):
            m(torch.zeros(1, 3, 32, 32, device=DEV))
    finally:
        m.eval()
