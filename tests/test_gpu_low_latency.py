"""The split-K bf16 conv (include/drnmi.h drnmi_conv_splitk, csrc/conv_sk.hip) and the low-latency mode
(DRNSeg.set_low_latency) on the GPU: bit for bit on integer data at every split class, within the bf16
conv bound of tests/test_gpu_kernels.py on real data, the same bytes on a second launch into the same
workspace, the refusals, and a network in the mode."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from drnmi import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (n, h, w, cin, cout, ks, stride, dil, residual)
CASES = [
    (1, 38, 38, 512, 512, 3, 1, 2, True),      # the real layer7 shape; ragged last pixel tile
    (2, 9, 13, 128, 128, 3, 1, 1, False),      # tiles crossing the image boundary
    (1, 19, 19, 256, 512, 3, 1, 4, True),      # taps wholly in the padding
    (1, 16, 16, 64, 128, 3, 2, 1, False),      # stride 2
    (1, 16, 16, 64, 128, 1, 2, 1, False),      # 1x1 downsample
    (1, 9, 17, 2048, 512, 1, 1, 1, True),      # D-54 bottleneck 1x1 with a long K
]
_DATA = {}


def _stream():
    return ctypes.c_void_p(L.stream_ptr(torch.device(DEV)))


def _data(case, kind):
    """Operands on the device and the float64 result (before the output's rounding), once per (case, kind)."""
    if (case, kind) not in _DATA:
        n, h, w, cin, cout, ks, st, dil, has_res = case
        pad = dil * (ks // 2)
        g = torch.Generator().manual_seed(CASES.index(case))
        if kind == "int":       # integers, weights drawn per (row, k): every partial sum is exact in fp32
            x = torch.randint(0, 4, (n, cin, h, w), generator=g).double()
            wt = torch.randint(-2, 3, (cout, cin, ks, ks), generator=g).double()
            sc, sh = torch.ones(cout).double(), torch.randint(-3, 4, (cout,), generator=g).double()
        else:
            x = torch.randn(n, cin, h, w, generator=g).bfloat16().double()
            wt = (torch.randn(cout, cin, ks, ks, generator=g) * (2.0 / (ks * ks * cout)) ** 0.5).bfloat16().double()
            sc, sh = torch.rand(cout, generator=g).double() + 0.5, torch.rand(cout, generator=g).double() - 0.5
        acc = F.conv2d(x, wt, stride=st, padding=pad, dilation=dil)
        res = None
        if has_res:
            res = (torch.randint(-3, 4, acc.shape, generator=g) if kind == "int" else torch.randn(acc.shape, generator=g)).bfloat16().double()
        relu = CASES.index(case) % 2 == 0
        ref = acc * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1) + (res if has_res else 0)
        ref = (F.relu(ref) if relu else ref).permute(0, 2, 3, 1).contiguous()
        if kind == "int":
            sumabs = F.conv2d(x.abs(), wt.abs(), stride=st, padding=pad, dilation=dil)
            assert float(sumabs.max()) < 2 ** 24 and float(acc.abs().max()) > 64      # exact in fp32, not trivial
        cout_pad = (cout + 127) // 128 * 128
        wp = torch.zeros(cout_pad, ks * ks * cin)
        wp[:cout] = wt.permute(0, 2, 3, 1).reshape(cout, -1).float()
        pads = [torch.zeros(cout_pad), torch.zeros(cout_pad)]
        pads[0][:cout], pads[1][:cout] = sc.float(), sh.float()
        _DATA[(case, kind)] = {
            "x": x.permute(0, 2, 3, 1).contiguous().to(DEV, torch.bfloat16), "w": wp.to(DEV, torch.bfloat16),
            "scale": pads[0].to(DEV), "shift": pads[1].to(DEV), "relu": relu, "ref": ref,
            "res": res.permute(0, 2, 3, 1).contiguous().to(DEV, torch.bfloat16) if has_res else None}
    return _DATA[(case, kind)]


def _args(case, t, y, ws=None):
    n, h, w, cin, cout, ks, st, dil, _ = case
    a = L.ConvArgs()
    pad = dil * (ks // 2)
    a.n, a.h, a.w, a.cin, a.cout, a.cout_pad = n, h, w, cin, cout, t["w"].shape[0]
    a.ho, a.wo = t["ref"].shape[1:3]
    a.ks, a.stride, a.pad, a.dil, a.k, a.k_pad = ks, st, pad, dil, ks * ks * cin, ks * ks * cin
    a.x, a.wgt, a.scale, a.shift, a.y = t["x"].data_ptr(), t["w"].data_ptr(), t["scale"].data_ptr(), t["shift"].data_ptr(), y.data_ptr()
    a.res = t["res"].data_ptr() if t["res"] is not None else None
    a.relu, a.dtype, a.tile, a.algo = int(t["relu"]), L.DRNMI_BF16, -1, L.ALGO_IGEMM
    a.out_dtype = L.DRNMI_BF16 if y.dtype == torch.bfloat16 else L.DRNMI_F32
    a.y_sn, a.y_sp, a.y_sc = a.ho * a.wo * cout, cout, 1
    if ws is not None:
        a.ws, a.ws_bytes = ws.data_ptr(), ws.numel()
    return a


def _splits(case):
    """{class: S}: 1, 2, a count that does not divide the K steps, the largest admitted, auto (0)."""
    steps = case[5] ** 2 * case[3] // 64
    top = min(16, steps)                                  # include/drnmi.h DRNMI_SPLITK_MAX
    odd = next((s for s in range(3, top + 1) if steps % s), None)
    return {k: s for k, s in (("one", 1), ("two", 2), ("odd", odd), ("max", top), ("auto", 0)) if s is not None and s <= top}


def _run(case, t, S, dtype, ws=None):
    lib = L.load()
    y = torch.full(t["ref"].shape, float("nan"), dtype=dtype, device=DEV)
    a = _args(case, t, y)
    need = lib.drnmi_conv_splitk_workspace_bytes(ctypes.byref(a), S)
    assert need >= 0
    if ws is None:
        ws = torch.zeros(max(need, 16), dtype=torch.uint8, device=DEV)     # tickets zeroed once, by the allocator
    a = _args(case, t, y, ws)
    assert lib.drnmi_conv_splitk_kernel_name(ctypes.byref(a), S) == b"conv_sk_kernel<%d>" % case[5]
    L.check(lib.drnmi_conv_splitk(ctypes.byref(a), S, _stream()), f"conv_splitk S={S}")
    torch.cuda.synchronize()
    return y, ws


SPLIT_CASES = [(c, k) for c in CASES for k in _splits(c)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case,cls", SPLIT_CASES, ids=[f"{CASES.index(c)}-{k}" for c, k in SPLIT_CASES])
def test_exact_on_integers(case, cls, dtype):
    """Every product and partial sum is an integer below 2^24, so any split and any order must give the
    float64 result bit for bit: a wrong K range, a dropped or doubled remainder step, a stale partial
    or a wrong tile / ticket pairing cannot."""
    t = _data(case, "int")
    y, _ = _run(case, t, _splits(case)[cls], dtype)
    assert torch.equal(y.cpu(), t["ref"].to(dtype))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=range(len(CASES)))
def test_real_values_within_the_bf16_conv_bound(case, dtype):
    """Against float64 on the bf16-rounded operands, the bound of test_gpu_kernels.py::test_conv_bn_act:
    |got - ref| <= 2^-8 |ref| + 1e-3 max|ref|, at every split class."""
    t = _data(case, "real")
    ref = t["ref"]
    bound = 2.0 ** -8 * ref.abs() + 1e-3 * float(ref.abs().max())
    for cls, S in _splits(case).items():
        y, _ = _run(case, t, S, dtype)
        worst = float(((y.cpu().double() - ref).abs() / bound).max())
        print(f"case {CASES.index(case)} {cls} (S={S}): worst error {worst:.3f} x the bound")
        assert worst <= 1.0, (cls, worst)


@pytest.mark.parametrize("cls", ["two", "odd", "max", "auto"])
def test_same_bytes_on_a_second_run(cls):
    """Two launches into one workspace, the tickets not zeroed in between: a fixed reduction order and a
    ticket that is set back give identical bytes (and a third launch of another shape finds its tickets zero)."""
    case = CASES[0]
    t = _data(case, "real")
    S = _splits(case)[cls]
    y0, ws = _run(case, t, S, torch.float32)
    y1, _ = _run(case, t, S, torch.float32, ws)
    assert torch.equal(y0.view(torch.int32), y1.view(torch.int32)) and not bool(torch.isnan(y0).any())
    t2 = _data(CASES[2], "int")
    y2, _ = _run(CASES[2], t2, 2, torch.float32, ws)
    assert torch.equal(y2.cpu(), t2["ref"].float())


def test_refusals():
    lib = L.load()
    case = CASES[1]
    t = _data(case, "int")
    y = torch.zeros(t["ref"].shape, dtype=torch.bfloat16, device=DEV)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)

    def status(**kw):
        a = _args(case, t, y, ws)
        for k, v in kw.items():
            setattr(a, k, v)
        st = lib.drnmi_conv_splitk_status(ctypes.byref(a), 2)
        assert (lib.drnmi_conv_splitk_kernel_name(ctypes.byref(a), 2) is None) == (st != 0)
        assert lib.drnmi_conv_splitk(ctypes.byref(a), 2, _stream()) == st
        return st
    assert status() == 0
    assert status(x2=t["x"].data_ptr(), cin2=128, h2=9, w2=13, stride2=1, k=9 * 128 + 128, k_pad=9 * 128 + 128) == -2
    assert status(unit_mask=ws.data_ptr()) == -2
    assert status(dtype=L.DRNMI_F32) == -2
    assert status(cin=32, k=9 * 32, k_pad=9 * 32) == -2
    assert status(ws_bytes=lib.drnmi_conv_splitk_workspace_bytes(ctypes.byref(_args(case, t, y)), 2) - 1) == -1
    assert status(ws=None) == -1
    torch.cuda.synchronize()


def _restate(plan, i):
    """Node i's launch from its own input buffers, in float64 (bf16 operands, the launch's epilogue)."""
    pk, a = plan.packed, plan.args[i]
    nd = pk.graph.nodes[i]
    x = plan.bufs[nd.x_val].view(a.n, a.h, a.w, a.cin).double().permute(0, 3, 1, 2)
    w = nd.wpk[:a.cout].double().view(a.cout, a.ks, a.ks, a.cin).permute(0, 3, 1, 2)
    v = F.conv2d(x, w, stride=a.stride, padding=a.pad, dilation=a.dil)
    if a.scale:
        v = v * nd.scale[:a.cout].double().view(1, -1, 1, 1)
    v = v + nd.shift[:a.cout].double().view(1, -1, 1, 1)
    if a.res:
        v = v + plan.bufs[nd.r_val].view(a.n, a.ho, a.wo, a.cout).double().permute(0, 3, 1, 2)
    return (F.relu(v) if a.relu else v).permute(0, 2, 3, 1)


@pytest.mark.parametrize("shape", ["d22_2x128x256", (1, 64, 64)], ids=["golden", "1x64x64"])
def test_network(shape, golden_forward):
    from drnmi.drnseg import INFO_MEAN, INFO_STD, build
    from drnmi.weights import synth_frames
    from oracle import drn_oracle as O
    lib = L.load()
    golden = isinstance(shape, str)
    m = build("drn_d_22", 19, seed=int(golden_forward[shape + "/meta"][0]) if golden else 0, device=DEV, precision="bf16")
    if golden:
        x = torch.from_numpy(golden_forward[shape + "/input"]).to(DEV)
        n, h, w = x.shape[0], x.shape[2], x.shape[3]
    else:
        n, h, w = shape
    frames = torch.from_numpy(synth_frames(3, n, h, w)).to(DEV)
    plain = m.segment(frames).clone()
    m.set_low_latency(True)
    # every conv_sk launch of a keep_all plan, restated from its own input buffers
    plan = m.plan(n, h, w, keep_all=True)
    stream = L.stream_ptr(torch.device(DEV))
    plan.ingest_u8(frames, INFO_MEAN, INFO_STD, False, stream)
    plan.run_backbone(stream)
    torch.cuda.synchronize()
    ls = plan.launches("u8")
    routed = [l for l in ls if l.kernel_name(lib).startswith("conv_sk_kernel")]
    assert routed and all(l.kind == "conv_sk" for l in routed)
    nodes = plan.packed.graph.nodes
    assert m.low_latency_layers(n, h, w) and \
        {nodes[i].name for i in m.plan(n, h, w).sk} == set(m.low_latency_layers(n, h, w))
    assert {nodes[l.row].name for l in routed} == {nodes[i].name for i in plan.sk}
    for l in routed:
        ref = _restate(plan, l.row)
        got = plan.bufs[nodes[l.row].dst].view(ref.shape).double()
        bound = 2.0 ** -8 * ref.abs() + 1e-3 * float(ref.abs().max())
        assert bool(((got - ref).abs() <= bound).all()), nodes[l.row].name
    # the user-facing paths: predict() is forward()'s argmax, segment() its own replayed graph, and the
    # golden labels are met as the bf16 test asks
    lab = m.segment(frames)
    xf = O.preprocess_u8(frames.cpu().numpy()).to(DEV)
    assert torch.equal(m.predict(xf), torch.max(m(xf)[0], 1)[1])
    if golden:
        pred = m.predict(x)
        agree = (pred.cpu().numpy() == golden_forward[shape + "/labels"]).mean()
        print(f"{shape} low latency: argmax agreement {agree:.4f}")
        assert agree >= 0.990                      # tests/test_gpu_forward.py::test_bf16_forward_agreement's gate
    out = torch.empty_like(lab)
    m.segment(frames, labels=out)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        m.segment(frames, labels=out)
    for _ in range(3):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, lab)
    m.set_low_latency(False)
    assert m.low_latency_layers(n, h, w) == [] and torch.equal(m.segment(frames), plain)
