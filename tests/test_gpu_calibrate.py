"""Histogram-based int8 calibration on the GPU: drnmi_abs_histogram against np.bincount, exact,
and DRNSeg.calibrate_int8's streamed / percentile / MSE modes end to end on the golden frames."""
import ctypes

import numpy as np
import pytest
import torch

from drnmi import calibrate as C

pytestmark = pytest.mark.gpu
DEV = "cuda"
BINS = 32768

# one lane; a grid with idle lanes in its last workgroup (every lane at most one load); a full grid
# (one 1024-lane workgroup per CU, 256 of them) whose lanes each run the four-loads-deep loop once
# and three of them the one-load tail loop after it
SIZES = {"one_lane": 8, "ragged": 8 * 12347, "two_loops": 8 * (4096 * 256 + 3)}
# +0, -0, the smallest subnormal, the largest finite bf16, +inf, -inf, a NaN (bf16 bit patterns)
PLANTED = [0x0000, 0x8000, 0x0001, 0x7f7f, 0x7f80, 0xff80, 0x7fc1]


def _lib():
    from drnmi import _lib
    return _lib, _lib.load()


def _stream():
    from drnmi import _lib
    return ctypes.c_void_p(_lib.stream_ptr(torch.device(DEV)))


def _make(content, n, dtype):
    g = torch.Generator(device=DEV).manual_seed(n % 1000 + len(content))
    if content == "planted":
        x = (torch.randn(n, device=DEV, generator=g) * 3.0).to(dtype)
        if dtype == torch.bfloat16:
            x.view(torch.int16)[:7] = torch.from_numpy(np.array(PLANTED, np.uint16).view(np.int16)).to(DEV)
        else:
            x.view(torch.int32)[:7] = torch.from_numpy((np.array(PLANTED, np.uint32) << 16).view(np.int32)).to(DEV)
    elif content == "relu":
        x = torch.relu(torch.randn(n, device=DEV, generator=g))
        x = (x * (torch.rand(n, device=DEV, generator=g) > 0.2)).to(dtype)
    else:
        x = torch.full((n,), 1.5, device=DEV, dtype=dtype)
    return x


def _reference(x):
    bits = x.float().cpu().numpy().view(np.int32)
    return np.bincount((bits & 0x7fffffff) >> 16, minlength=BINS)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("content", ["planted", "relu", "constant"])
@pytest.mark.parametrize("size", sorted(SIZES))
def test_abs_histogram_exact(size, content, dtype):
    from drnmi.ops import abs_histogram
    n = SIZES[size]
    x = _make(content, n, dtype)
    hist = abs_histogram(x)
    assert hist.dtype == torch.int64 and tuple(hist.shape) == (BINS,)
    ref = _reference(x)
    got = hist.cpu().numpy()
    np.testing.assert_array_equal(got, ref)
    assert int(got.sum()) == n
    if content == "planted":
        assert ref[0] >= 2 and ref[1] >= 1 and ref[0x7f7f] >= 1 and ref[0x7f80] == 2 and ref[0x7fc1] == 1
    elif content == "relu":
        assert n < 100 or 0.55 < ref[0] / n < 0.65
    else:
        assert ref[0x3fc0] == n


def test_abs_histogram_accumulates_and_carries():
    from drnmi.ops import abs_histogram
    x = _make("planted", SIZES["ragged"], torch.bfloat16)
    hist = abs_histogram(x)
    once = hist.clone()
    assert abs_histogram(x, hist) is hist
    assert torch.equal(hist, 2 * once)
    # a carry out of the low 32 bits of one counter
    y = torch.zeros(16, device=DEV, dtype=torch.bfloat16)
    y[3:13] = 1.5
    seeded = torch.zeros(BINS, dtype=torch.int64, device=DEV)
    seeded[0x3fc0] = 2 ** 32 - 5
    abs_histogram(y, seeded)
    want = np.zeros(BINS, np.int64)
    want[0x3fc0], want[0] = 2 ** 32 + 5, 6
    np.testing.assert_array_equal(seeded.cpu().numpy(), want)
    with pytest.raises(ValueError):
        abs_histogram(y, torch.zeros(BINS, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        abs_histogram(y.to(torch.float16))
    with pytest.raises(RuntimeError):
        abs_histogram(y[:12])                                          # n % 8


def test_histogram_absmax_is_todays_absmax():
    from drnmi.ops import abs_histogram
    L, lib = _lib()
    g = torch.Generator(device=DEV).manual_seed(11)
    x = (torch.randn(8 * 12347, device=DEV, generator=g) * 0.37).to(torch.bfloat16)
    amax = torch.empty(1, device=DEV)
    L.check(lib.drnmi_absmax(x.data_ptr(), L.DRNMI_BF16, x.numel(), amax.data_ptr(), _stream()), "absmax")
    hist = abs_histogram(x).cpu().numpy()
    assert C.scale_from_histogram(hist, "absmax") == float(amax.item()) / 127.0
    assert C.scale_from_histogram(hist, "percentile", 100.0) == float(amax.item()) / 127.0


# ------------------------------------------------------------------ end to end
def _norm():
    from drnmi.drnseg import INFO_MEAN, INFO_STD
    return INFO_MEAN, INFO_STD


def _run_keep_all(m, frames):
    from drnmi import _lib as L
    n, h, w = frames.shape[:3]
    plan = m.plan(n, h, w, keep_all=True)
    stream = L.stream_ptr(torch.device(DEV))
    plan.ingest_u8(frames, *_norm(), False, stream)
    plan.run_backbone(stream)
    torch.cuda.synchronize()
    return plan


@pytest.fixture(scope="module")
def net(golden_forward):
    """One D-22 on the golden frames (built as tests/test_gpu_int8.py builds its own), taken
    through every calibration mode once, in this order; the tests read what each step returned."""
    from drnmi.drnseg import build
    case = "d22_2x128x256"
    seed = int(golden_forward[case + "/meta"][0])
    m = build("drn_d_22", 19, seed=seed, device=DEV)
    frames = torch.from_numpy(golden_forward[case + "/frames"]).to(DEV)
    r = {"m": m, "frames": frames, "seed": seed, "label_shape": golden_forward[case + "/labels"].shape}
    r["absmax_tensor"] = m.calibrate_int8(frames)
    r["hists_after_tensor"] = m.int8_histograms()
    r["absmax_list"] = m.calibrate_int8([frames], method="absmax")
    r["absmax_split"] = m.calibrate_int8([frames[:1], frames[1:]], method="absmax")
    r["hists_split"] = m.int8_histograms()
    r["mse"] = m.calibrate_int8(frames, method="mse")
    r["hists"] = m.int8_histograms()
    r["state_mse"] = m.int8_state()
    r["percentile"] = m.calibrate_int8(iter([frames]), method="percentile")
    r["state_percentile"] = m.int8_state()
    return r


def test_absmax_modes_agree(net):
    a = net["absmax_tensor"]
    assert len(a) >= 20 and all(isinstance(s, float) and s > 0 for s in a.values())
    assert net["hists_after_tensor"] is None                 # the one-tensor absmax path keeps none
    assert net["absmax_list"] == a
    assert net["absmax_split"] == a                          # max over batches == max of the whole
    hs = net["hists_split"]
    assert set(hs) == set(a) and all(h.dtype == np.int64 and h.shape == (BINS,) for h in hs.values())
    for v, h in net["hists"].items():                        # two half batches count what one whole does
        np.testing.assert_array_equal(hs[v], h, err_msg=v)


def test_predicted_sse_is_the_measured_sse(net):
    L, lib = _lib()
    m, frames, s_mse, s_abs, hists = net["m"], net["frames"], net["mse"], net["absmax_tensor"], net["hists"]
    assert set(s_mse) == set(s_abs) == set(hists)
    prev = m.precision
    plan = _run_keep_all(m.set_precision("bf16"), frames)
    m.set_precision(prev)
    below = 0
    for v, s in s_mse.items():
        buf = plan.bufs[v]
        assert buf.dtype == torch.bfloat16 and int(hists[v].sum()) == buf.numel(), v
        q = torch.empty(buf.numel(), dtype=torch.int8, device=DEV)
        L.check(lib.drnmi_quantize_i8(buf.data_ptr(), L.DRNMI_BF16, q.data_ptr(), buf.numel(), 1.0 / s, _stream()),
                "quantize")
        measured = float(((buf.double() - q.double() * s) ** 2).sum().item())
        predicted = C.quant_sse(hists[v], s)
        predicted_absmax = C.quant_sse(hists[v], s_abs[v])
        print(f"{v}: scale mse/absmax {s / s_abs[v]:.4f}  sse predicted {predicted:.9e} measured {measured:.9e} "
              f"(absmax scale: {predicted_absmax:.9e})")
        assert predicted == pytest.approx(measured, rel=1e-9, abs=0.0), v
        assert predicted <= predicted_absmax, v
        assert s_abs[v] / 16.0 <= s <= s_abs[v], v
        below += s < s_abs[v]
    print(f"mse picked a clip below absmax for {below} of {len(s_mse)} activations")


def test_percentile_scales_reach_the_engine(net):
    from oracle import int8_oracle as Q
    m, frames, sp = net["m"], net["frames"], net["percentile"]
    assert net["state_percentile"] == {"version": 1, "method": "percentile", "percentile": 99.99, "scales": sp}
    assert all(sp[v] <= net["absmax_tensor"][v] for v in sp)
    m.load_int8_state(net["state_percentile"])               # (whatever test ran before this one)
    plan = _run_keep_all(m.set_precision("int8"), frames)
    pk = plan.packed
    assert pk.act_scales == sp
    assert pk.quant_after
    for vals in pk.quant_after.values():
        for v in vals:
            src = plan.bufs[v].float().cpu().numpy()
            ref = Q.quantize_i8(src, np.float32(1.0 / sp[v]))
            np.testing.assert_array_equal(plan.bufs["q:" + v].cpu().numpy(), ref)
    lab = m.segment(frames)
    assert lab.dtype == torch.uint8 and tuple(lab.shape) == tuple(net["label_shape"])
    assert int(lab.max()) < 19


def test_rescale_equals_fresh_calibration(net):
    m = net["m"]
    m.calibrate_int8([net["frames"]], method="percentile", percentile=99.9)
    assert m.int8_state()["percentile"] == 99.9
    assert m.rescale_int8("mse") == net["mse"]
    assert m.int8_state() == net["state_mse"]
    assert m.rescale_int8("absmax") == net["absmax_tensor"]


def test_saved_state_reproduces_the_labels(net):
    from drnmi.drnseg import build
    m, frames = net["m"], net["frames"]
    m.load_int8_state(net["state_mse"])
    lab = m.set_precision("int8").segment(frames)
    m2 = build("drn_d_22", 19, seed=net["seed"], device=DEV)
    with pytest.raises(RuntimeError):
        m2.set_precision("int8").segment(frames)             # no scales yet
    m2.load_int8_state(net["state_mse"])
    lab2 = m2.segment(frames)
    assert lab2.dtype == torch.uint8 and torch.equal(lab, lab2)
