"""Histogram-based int8 calibration, the parts that need no GPU: the drnmi_abs_histogram
argument rules, drnmi.calibrate's scales against a brute-force restatement, and the int8
state's JSON / checkpoint round trip."""
import ctypes
import json
import math
import os
import struct

import numpy as np
import pytest
import torch

from drnmi import _lib
from drnmi import calibrate as C

FINITE = 0x7f80


def _value(b):
    """The bf16 magnitude with bit pattern b, as a Python float."""
    return struct.unpack("<f", struct.pack("<I", b << 16))[0]


def _bin(v):
    bits = struct.unpack("<I", struct.pack("<f", v))[0]
    assert bits & 0xffff == 0, f"{v} is not a bf16 value"
    return (bits & 0x7fffffff) >> 16


def _hist(pairs):
    h = np.zeros(C.HIST_BINS, np.int64)
    for v, c in pairs:
        h[_bin(v)] += c
    return h


# ------------------------------------------------------------------ C-ABI without a GPU
def test_abs_histogram_argument_rules_without_gpu():
    lib = _lib.load()
    assert _lib.HIST_BINS == C.HIST_BINS == 32768
    x = (ctypes.c_uint16 * 16)()
    h = (ctypes.c_int64 * C.HIST_BINS)()
    px, ph = ctypes.addressof(x), ctypes.addressof(h)
    assert lib.drnmi_abs_histogram(None, _lib.DRNMI_BF16, 8, ph, None) == -1
    assert lib.drnmi_abs_histogram(px, _lib.DRNMI_BF16, 8, None, None) == -1
    assert lib.drnmi_abs_histogram(px, _lib.DRNMI_BF16, 12, ph, None) == -1       # n % 8
    assert lib.drnmi_abs_histogram(px, _lib.DRNMI_F32, -8, ph, None) == -1
    assert lib.drnmi_abs_histogram(px, _lib.DRNMI_I8, 8, ph, None) == -1          # bad dtype
    assert lib.drnmi_abs_histogram(px, 77, 0, ph, None) == -1                     # ... even with n == 0
    assert lib.drnmi_abs_histogram(px, _lib.DRNMI_BF16, 0, ph, None) == 0         # nothing launched
    assert lib.drnmi_abs_histogram(px, _lib.DRNMI_F32, 0, ph, None) == 0
    assert not any(h)


def test_bin_values():
    v = C.bin_values()
    assert v.shape == (32768,) and v.dtype == np.float64
    assert v[0] == 0.0 and v[0x3f80] == 1.0 and v[0x4000] == 2.0 and v[1] == 2.0 ** -133
    assert np.isfinite(v[:FINITE]).all() and np.isinf(v[FINITE]) and np.isnan(v[FINITE + 1:]).all()
    assert (np.diff(v[:FINITE]) > 0).all()
    assert v[FINITE - 1] == float(torch.finfo(torch.bfloat16).max)
    assert all(v[b] == _value(b) for b in (1, 0x7f, 0x80, 0x3f81, 0x7f7f))


# ------------------------------------------------------------------ brute-force restatement
def _q(v, inv32):
    """The engine's quantiser on one value: one fp32 multiply, round-half-even, clamp."""
    r = round(float(np.float32(v) * inv32))          # Python's round(): half to even
    return float(max(-127, min(127, r)))


def _brute_sse(hist, s):
    inv32 = np.float32(1.0 / s)
    cost = 0.0
    for b in range(FINITE):
        if hist[b]:
            e = _value(b) - s * _q(_value(b), inv32)
            cost += (e * e) * float(hist[b])
    return cost


def _brute_scale(hist, method, p=99.99):
    amax = 0.0
    for b in range(FINITE):
        if hist[b]:
            amax = _value(b)
    if method == "absmax":
        return amax / 127.0 if amax > 0 else 1.0
    if method == "percentile":
        total = sum(int(hist[b]) for b in range(FINITE))
        need, seen = math.ceil(p / 100.0 * total), 0
        for b in range(FINITE):
            seen += int(hist[b])
            if seen >= need:
                return _value(b) / 127.0 if _value(b) > 0 else 1.0
        raise AssertionError("unreachable")
    if amax == 0.0:
        return 1.0
    best = None
    for b in range(FINITE):
        if hist[b] and _value(b) >= amax / 16.0:
            cost = _brute_sse(hist, _value(b) / 127.0)
            if best is None or cost < best[0] or (cost == best[0] and _value(b) > best[1]):
                best = (cost, _value(b))
    return best[1] / 127.0


def _bulk_and_outlier():
    # a dense bulk below 1.0 (counts falling with magnitude, as a post-ReLU activation's) plus a
    # zero spike and one element far out at 96.0
    h = np.zeros(C.HIST_BINS, np.int64)
    h[0] = 50000
    for i, b in enumerate(range(_bin(0.0078125), _bin(1.0) + 1, 3)):
        h[b] = 4000 - 13 * i
    assert h.min() >= 0
    h[_bin(96.0)] = 1
    return h


HAND_BUILT = {
    "single_bin": _hist([(0.75, 9)]),
    "all_zero_values": _hist([(0.0, 1234)]),
    "empty": np.zeros(C.HIST_BINS, np.int64),
    "bulk_and_outlier": _bulk_and_outlier(),
    # every term is exact in fp64: at clip 127 (s = 1) the 63.5s round to 64 (0.25 each), at clip
    # 63.5 (s = 0.5) the one 127 clips to 63.5 (63.5^2 = 4032.25); 16129 * 0.25 == 4032.25, and
    # the 0.25s cost 1/16 each either way.  The tie goes to the larger clip.
    "tie": _hist([(0.25, 1000), (63.5, 16129), (127.0, 1)]),
}


@pytest.mark.parametrize("name", sorted(HAND_BUILT))
@pytest.mark.parametrize("method", C.METHODS)
def test_scale_matches_brute_force(name, method):
    h = HAND_BUILT[name]
    for p in ((99.99, 50.0, 100.0, 0.0, 99.0) if method == "percentile" else (99.99,)):
        got = C.scale_from_histogram(h, method, p)
        assert isinstance(got, float)
        assert got == _brute_scale(h, method, p), (name, method, p)


def test_hand_built_expectations():
    assert C.scale_from_histogram(HAND_BUILT["single_bin"], "mse") == 0.75 / 127.0
    assert C.scale_from_histogram(HAND_BUILT["single_bin"], "percentile") == 0.75 / 127.0
    for m in C.METHODS:
        assert C.scale_from_histogram(HAND_BUILT["all_zero_values"], m) == 1.0
        assert C.scale_from_histogram(HAND_BUILT["empty"], m) == 1.0
    t = HAND_BUILT["tie"]
    assert C.quant_sse(t, 1.0) == C.quant_sse(t, 0.5) == 1000 / 16 + 4032.25
    assert C.scale_from_histogram(t, "mse") == 1.0                    # the larger clip, 127 / 127
    t2 = t.copy()
    t2[_bin(63.5)] -= 1                                               # one 63.5 fewer: 127 wins outright
    assert C.scale_from_histogram(t2, "mse") == 1.0
    t2[_bin(63.5)] += 2                                               # one more: 63.5 wins
    assert C.scale_from_histogram(t2, "mse") == 0.5
    b = HAND_BUILT["bulk_and_outlier"]
    assert C.scale_from_histogram(b, "absmax") == 96.0 / 127.0
    bulk_top = _value(int(np.flatnonzero(b)[-2]))
    assert 0.9 < bulk_top < 1.0
    assert C.scale_from_histogram(b, "percentile", 99.99) == bulk_top / 127.0   # the outlier is 1 in ~7e5
    # the outlier's octaves hold nothing else, so "mse" can only keep it (candidates >= 96 / 16)
    assert C.scale_from_histogram(b, "mse") == 96.0 / 127.0
    for name, h in HAND_BUILT.items():
        for s in (0.011, 1.0, 96.0 / 127.0):
            want = _brute_sse(h, s)
            assert C.quant_sse(h, s) == pytest.approx(want, rel=1e-12, abs=0.0), name


# ------------------------------------------------------------------ derivable invariants
def _random_hist(seed):
    rng = np.random.default_rng(seed)
    h = np.zeros(C.HIST_BINS, np.int64)
    lo, hi = _bin(2.0 ** -20), _bin(float(2.0 ** rng.integers(-3, 8)))
    bins = rng.integers(lo, hi + 1, size=int(rng.integers(1, 400)))
    h[bins] = rng.integers(1, 100000, size=bins.size)
    h[0] = int(rng.integers(0, 10 ** 6))
    if seed % 3 == 0:                                  # a far outlier
        h[min(hi + int(rng.integers(100, 600)), FINITE - 1)] = 1
    return h


@pytest.mark.parametrize("seed", range(12))
def test_invariants_on_random_histograms(seed):
    h = _random_hist(seed)
    s_abs = C.scale_from_histogram(h, "absmax")
    s_mse = C.scale_from_histogram(h, "mse")
    assert C.quant_sse(h, s_mse) <= C.quant_sse(h, s_abs)           # absmax is a candidate
    assert s_abs / 16.0 <= s_mse <= s_abs
    assert C.scale_from_histogram(h, "percentile", 100.0) == s_abs
    # the percentile's clip value grows with p; while it still falls in the zero spike the scale
    # is the 1.0 of an all-zero tensor, from the first nonzero clip on the scale itself grows
    total, prev, left_zero = int(h.sum()), 0.0, False
    for p in (0.001, 1.0, 25.0, 50.0, 90.0, 99.0, 99.9, 99.99, 99.999, 100.0):
        s = C.scale_from_histogram(h, "percentile", p)
        if math.ceil(p / 100.0 * total) <= int(h[0]):
            assert s == 1.0 and not left_zero, p
            continue
        left_zero = True
        assert prev <= s <= s_abs, p
        prev = s
    assert left_zero
    # the histogram's integer type does not matter, and the argument is not modified
    keep = h.copy()
    assert C.scale_from_histogram(h.astype(np.uint64), "mse") == s_mse
    assert C.scale_from_histogram(torch.from_numpy(h), "mse") == s_mse
    np.testing.assert_array_equal(h, keep)


@pytest.mark.parametrize("bad_bin", [FINITE, FINITE + 1, 32767])
def test_nonfinite_bins(bad_bin):
    h = _random_hist(1)
    s_abs = C.scale_from_histogram(h, "absmax")
    h[bad_bin] = 1
    assert C.scale_from_histogram(h, "absmax") == s_abs              # finite bins only
    for m in ("percentile", "mse"):
        with pytest.raises(ValueError):
            C.scale_from_histogram(h, m)


def test_bad_arguments():
    h = _random_hist(2)
    with pytest.raises(ValueError):
        C.scale_from_histogram(h, "kl")
    with pytest.raises(ValueError):
        C.scale_from_histogram(h[:100], "absmax")
    with pytest.raises(ValueError):
        C.scale_from_histogram(h.astype(np.float64), "absmax")
    with pytest.raises(ValueError):
        C.scale_from_histogram(h, "percentile", 100.5)
    with pytest.raises(ValueError):
        C.quant_sse(h, 0.0)


# ------------------------------------------------------------------ int8 state and checkpoints
@pytest.fixture(scope="module")
def cpu_model():
    from drnmi.drnseg import DRNSeg
    return DRNSeg("drn_d_22", 19, pretrained=False)


def _scales(m, seed=0):
    rng = np.random.default_rng(seed)
    # awkward floats: nothing a short decimal would hold
    return {v: float(rng.uniform(1e-4, 3.0)) * (1.0 + 2.0 ** -52) for v in m._int8_values()}


def test_int8_state_round_trip(cpu_model):
    m = cpu_model
    values = m._int8_values()
    assert len(values) >= 20 and "input" not in values and "logits" not in values
    assert set(values) | {"input", "logits"} == set(m._graph.channels)
    sc = _scales(m)
    m._packed["int8"], m._plans[("int8", 1, 8, 8, False)], m._plans[("bf16", 1, 8, 8, False)] = "pk", "pl", "keep"
    m._pack_key = "stale"
    assert m.load_int8_state({"version": 1, "method": "mse", "percentile": None, "scales": sc}) is m
    assert "int8" not in m._packed and list(m._plans) == [("bf16", 1, 8, 8, False)] and m._pack_key is None
    m._plans.clear()
    st = m.int8_state()
    assert st == {"version": 1, "method": "mse", "percentile": None, "scales": sc}
    back = json.loads(json.dumps(st))
    assert back == st and all(back["scales"][v].hex() == sc[v].hex() for v in sc)
    assert m.int8_histograms() is None
    with pytest.raises(RuntimeError):
        m.rescale_int8("mse")


def test_load_int8_state_rejects(cpu_model):
    m = cpu_model
    sc = _scales(m, 1)
    m.load_int8_state({"version": 1, "method": "absmax", "percentile": None, "scales": sc})
    first = next(iter(sc))
    missing = {k: v for k, v in sc.items() if k != first}
    bad = [{"version": 1, "scales": missing},
           {"version": 1, "scales": {**sc, "no_such_value": 1.0}},
           {"version": 1, "scales": {**missing, "input": 1.0}},
           {"version": 2, "scales": sc},
           {"scales": sc},
           {"version": 1}]
    for s in (0.0, -0.5, float("inf"), float("nan"), None, "0.1", True):
        bad.append({"version": 1, "scales": {**sc, first: s}})
    for st in bad:
        with pytest.raises(ValueError):
            m.load_int8_state(st)
    assert m.int8_state()["scales"] == sc                            # a refused state changes nothing


def test_int8_state_needs_scales():
    from drnmi.drnseg import DRNSeg
    with pytest.raises(RuntimeError):
        DRNSeg("drn_d_22", 19, pretrained=False).int8_state()


def test_checkpoint_int8_round_trip(cpu_model, tmp_path):
    from drnmi.checkpoint import int8_path, resume, save_checkpoint
    from drnmi.drnseg import DRNSeg
    m = cpu_model
    sc = _scales(m, 2)
    m.load_int8_state({"version": 1, "method": "percentile", "percentile": 99.9, "scales": sc})
    state = {"epoch": 3, "state_dict": m.state_dict()}
    save_checkpoint(state, True, save_dir=str(tmp_path), int8_model=m)
    ck = os.path.join(str(tmp_path), "checkpoint.pth.tar")
    best = os.path.join(str(tmp_path), "checkpoint_best.pth.tar")
    assert int8_path(ck) == ck + ".int8.json"
    assert open(int8_path(ck)).read() == open(int8_path(best)).read()
    assert json.load(open(int8_path(ck))) == m.int8_state()
    for path in (ck, best):
        m2 = DRNSeg("drn_d_22", 19, pretrained=False)
        assert resume(path, m2, int8=True)["epoch"] == 3
        st = m2.int8_state()
        assert st == m.int8_state()
        assert all(st["scales"][v].hex() == sc[v].hex() for v in sc)   # every scale bit for bit
    # defaults: no file written, none read
    save_checkpoint(state, False, save_dir=str(tmp_path), filename="plain.pth.tar")
    plain = os.path.join(str(tmp_path), "plain.pth.tar")
    assert not os.path.exists(int8_path(plain))
    m3 = DRNSeg("drn_d_22", 19, pretrained=False)
    resume(plain, m3)
    assert m3._act_scales is None
    with pytest.raises(FileNotFoundError):
        resume(plain, m3, int8=True)


def test_pickle_keeps_the_scales(cpu_model):
    import pickle
    m = cpu_model
    sc = _scales(m, 3)
    m.load_int8_state({"version": 1, "method": "mse", "percentile": None, "scales": sc})
    m2 = pickle.loads(pickle.dumps(m))
    assert m2.int8_state() == m.int8_state()
