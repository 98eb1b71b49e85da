"""Quantisation-aware fine-tuning, the parts that need no GPU: the numpy restatement against the int8
oracle, the lifted int8 layout decision (engine.int8_layout) with its sets pinned by name, the
set_qat / qat_layers interface, and the new entry points' argument checks."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import qat_ref as R
from oracle.int8_oracle import quantize_i8, quantize_weight_rows

F32 = np.float32


def _edge_values(s, rng, n_random=4096):
    s = F32(s)
    k = np.arange(-130, 131, dtype=F32)
    parts = [np.array([0.0, -0.0], dtype=F32), (k + F32(0.5)) * s, k * s,
             np.array([127, -127, 127.5, -127.5, 128, -128, 1e6, -1e6], dtype=F32) * s,
             np.array([1e-45, -1e-45, 1e-40, -1e-40, 1.1754942e-38], dtype=F32),
             (rng.standard_normal(n_random) * 60).astype(F32) * s]
    return np.concatenate(parts).astype(F32)


@pytest.mark.parametrize("s", [0.25, 0.0371])
def test_fq_is_dequantised_quantize_i8(s):
    x = _edge_values(s, np.random.default_rng(0))
    s32, inv = R.scale_pair(s)
    assert inv == F32(1.0 / s)
    want = s32 * quantize_i8(x, inv).astype(F32)
    got = R.fq(x, s)
    assert got.dtype == F32 and np.array_equal(got.view(np.uint32), want.astype(F32).view(np.uint32))
    # on the grid: an integer level in [-127, 127] whose fp32 product with s is the value itself
    # (fl(q * s) / s is q only up to that product's rounding, so the level is taken by rint)
    lvl = np.rint(got.astype(np.float64) / np.float64(s32))
    assert np.abs(lvl).max() == 127 and np.array_equal((lvl.astype(F32) * s32).astype(F32), got)
    m = R.mask(x, s)
    assert not m.all() and m.any()
    # the mask is "the clamp did not bind": inside it fq is the unclamped level
    with np.errstate(over="ignore"):
        assert np.array_equal(np.rint(x * inv)[m] * s32, got[m])
    dq = np.random.default_rng(1).standard_normal(x.size).astype(F32)
    dx = np.random.default_rng(2).standard_normal(x.size).astype(F32)
    assert np.array_equal(R.fq_bwd(dq, x, s), np.where(m, dq, F32(0)))
    assert np.array_equal(R.fq_bwd(dq, x, s, dx), dx + np.where(m, dq, F32(0)))


def test_row_codes_are_the_int8_packs():
    rng = np.random.default_rng(3)
    w = rng.standard_normal((19, 27)).astype(F32)
    w[2] = 0
    w[5] = 0
    w[5, 7] = -0.3
    w[7, 3] = -9.0           # the absmax is a negative weight
    q, s = R.row_codes(w)
    q0, s0 = quantize_weight_rows(w)
    assert np.array_equal(q, q0) and np.array_equal(s, s0)
    wq, s1 = R.fq_rows(w)
    assert np.array_equal(s1, s0) and np.array_equal(wq, q0.astype(F32) * s0[:, None])
    assert np.all(wq[2] == 0) and s0[2] == 1 and q0[7, 3] == -127 and np.count_nonzero(wq[5]) == 1
    # quantising the shadow again gives the same codes: the int8 pack of a QAT weight is its grid
    assert np.array_equal(quantize_weight_rows(wq)[0], q0)


# The sets PackedNet._int8_layout produced before the decision was lifted out of it, by name.  E: the
# convs precision "int8" launches W8A8 (given as the complement, which is shorter); Q: what they read.
_LAYOUTS = {
    "drn_d_22": dict(
        n_nodes=26,
        not_e=["layer.0.0", "layer.1.0", "layer.2.0", "layer.3.0.conv1", "layer.3.0.downsample.0", "layer.3.0.conv2",
               "layer.3.1.conv1", "layer.3.1.conv2", "layer.4.0.conv1", "layer.4.0.downsample.0", "layer.4.0.conv2"],
        first_e="layer.4.1.conv1", q=[f"v{i}" for i in range(11, 26)]),
    "drn_d_38": dict(
        n_nodes=42,
        not_e=["layer.0.0", "layer.1.0", "layer.2.0", "layer.3.0.conv1", "layer.3.0.downsample.0", "layer.3.0.conv2",
               "layer.3.1.conv1", "layer.3.1.conv2", "layer.3.2.conv1", "layer.3.2.conv2", "layer.4.0.conv1",
               "layer.4.0.downsample.0", "layer.4.0.conv2"],
        first_e="layer.4.1.conv1", q=[f"v{i}" for i in range(13, 42)]),
    "drn_d_54": dict(
        n_nodes=58,
        not_e=["layer.0.0", "layer.1.0", "layer.2.0", "layer.3.0.conv1", "layer.3.0.conv2", "layer.3.0.downsample.0",
               "layer.3.1.conv1", "layer.3.1.conv2", "layer.3.2.conv1", "layer.3.2.conv2", "layer.4.0.conv1",
               "layer.4.0.conv2", "layer.4.1.conv1", "layer.4.2.conv1", "layer.4.3.conv1"],
        first_e="layer.3.0.conv3", q=[f"v{i}" for i in range(5, 58) if i not in (8, 11, 14)]),
}


@pytest.mark.parametrize("arch", sorted(_LAYOUTS))
def test_int8_layout_is_pinned(arch):
    from drnmi.drnseg import DRNSeg
    from drnmi.engine import channel_strides, int8_layout
    want = _LAYOUTS[arch]
    m = DRNSeg(arch, 19, pretrained=False)
    g = m._graph
    names = [nd.name for nd in g.nodes]
    assert len(names) == want["n_nodes"]
    elig, q8_values, need = int8_layout(g, channel_strides(g))
    e_names = [names[i] for i in sorted(elig)]
    assert [n for n in names if n not in e_names] == want["not_e"]
    assert e_names[0] == want["first_e"] and e_names[-1] == "seg"
    assert sorted(need, key=lambda v: int(v[1:])) == want["q"]
    assert "input" not in need and "logits" not in need
    # an int8 value is produced by E and read by E only; what E reads that is not int8 gets a copy
    readers = {}
    for i, nd in enumerate(g.nodes):
        for v in (nd.src, nd.res):
            if v:
                readers.setdefault(v, set()).add(i)
    producer = {nd.dst: i for i, nd in enumerate(g.nodes)}
    for v in q8_values:
        assert producer[v] in elig and readers[v] <= elig and v in need
    assert m.qat_layers() == (e_names, want["q"])


def _scales(m, s=0.05):
    return {"version": 1, "method": "absmax", "percentile": None, "scales": {v: s for v in m._int8_values()}}


def test_set_qat_interface():
    from drnmi.drnseg import DRNSeg
    m = DRNSeg("drn_d_22", 19, pretrained=False)
    assert m._qat is None
    with pytest.raises(ValueError):
        m.set_qat("int4")
    with pytest.raises(RuntimeError, match="no calibrated activation scale"):
        m.set_qat("int8")
    assert m._qat is None
    m.load_int8_state(_scales(m))
    assert m.set_qat("int8") is m and m._qat == "int8"
    assert sorted(m._qat_scales()) == sorted(m.qat_layers()[1])
    c = copy.deepcopy(m)                      # dropped from the copied state, like the train runner
    assert getattr(c, "_qat", None) is None and m._qat == "int8"
    assert m.set_qat(None) is m and m._qat is None
    mc = DRNSeg("drn_c_26", 19, pretrained=False)
    with pytest.raises(NotImplementedError):
        mc.set_qat("int8")
    with pytest.raises(ValueError):
        mc.set_qat("int4")
    assert mc.set_qat(None) is mc


def test_entry_points_reject_bad_arguments_without_gpu():
    """DRNMI_EINVAL before any HIP call: NULL / misaligned pointers, n % 8 != 0, a non-positive scale."""
    from drnmi import _lib
    lib = _lib.load()
    p, odd = 0x1000, 0x1004
    assert lib.drnmi_fake_quant_f32(None, 8, 0.5, 2.0, p, None) == -1
    assert lib.drnmi_fake_quant_f32(p, 8, 0.5, 2.0, None, None) == -1
    assert lib.drnmi_fake_quant_f32(odd, 8, 0.5, 2.0, p, None) == -1
    assert lib.drnmi_fake_quant_f32(p, 12, 0.5, 2.0, p, None) == -1
    assert lib.drnmi_fake_quant_f32(p, 8, 0.0, 2.0, p, None) == -1
    assert lib.drnmi_fake_quant_f32(p, 8, 0.5, 0.0, p, None) == -1
    assert lib.drnmi_fake_quant_f32(p, 8, float("nan"), 2.0, p, None) == -1
    assert lib.drnmi_fake_quant_f32(p, 0, 0.5, 2.0, p, None) == 0
    assert lib.drnmi_fake_quant_bwd_f32(None, p, 8, 2.0, p, 0, None) == -1
    assert lib.drnmi_fake_quant_bwd_f32(p, None, 8, 2.0, p, 0, None) == -1
    assert lib.drnmi_fake_quant_bwd_f32(p, p, 8, 2.0, None, 0, None) == -1
    assert lib.drnmi_fake_quant_bwd_f32(p, p, 8, 2.0, odd, 0, None) == -1
    assert lib.drnmi_fake_quant_bwd_f32(p, p, 12, 2.0, p, 0, None) == -1
    assert lib.drnmi_fake_quant_bwd_f32(p, p, 8, 0.0, p, 1, None) == -1
    assert lib.drnmi_fake_quant_bwd_f32(p, p, 8, 2.0, p, 2, None) == -1
    assert lib.drnmi_fake_quant_bwd_f32(p, p, 0, 2.0, p, 1, None) == 0
    assert lib.drnmi_fake_quant_rows_f32(None, 4, 27, p, p, None) == -1
    assert lib.drnmi_fake_quant_rows_f32(p, 4, 27, None, p, None) == -1
    assert lib.drnmi_fake_quant_rows_f32(p, 4, 27, p, None, None) == -1
    assert lib.drnmi_fake_quant_rows_f32(odd, 4, 27, p, p, None) == -1
    assert lib.drnmi_fake_quant_rows_f32(p, 4, 0, p, p, None) == -1
    assert lib.drnmi_fake_quant_rows_f32(p, -1, 27, p, p, None) == -1
    assert lib.drnmi_fake_quant_rows_f32(p, 0, 27, p, p, None) == 0
    assert lib.drnmi_fake_quant_rows_batched_f32(None, 1, 4, None) == -1
    assert lib.drnmi_fake_quant_rows_batched_f32(p, 0, 4, None) == -1
    assert lib.drnmi_fake_quant_rows_batched_f32(p, 1, 0, None) == -1
    tab = np.array([[0x1000, 0x2000, 0x3000, 16, 27, 0], [0x4000, 0x5000, 0x3040, 5, 4608, 16]], dtype=np.int64)
    tot = ctypes.c_int64(0)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.drnmi_fake_quant_rows_table_check(ptr(tab), 2, ctypes.byref(tot)) == 0 and tot.value == 21
    for r, c, v in ((1, 5, 15), (0, 4, 0), (1, 3, 0), (0, 1, 0), (1, 0, 0x4004), (0, 2, 0x3002)):
        bad = tab.copy()
        bad[r, c] = v
        assert lib.drnmi_fake_quant_rows_table_check(ptr(bad), 2, ctypes.byref(tot)) == -1, (r, c, v)
    assert lib.drnmi_fake_quant_rows_table_check(None, 2, ctypes.byref(tot)) == -1
    assert lib.drnmi_fake_quant_rows_table_check(ptr(tab), 0, ctypes.byref(tot)) == -1


def test_qat_off_is_the_default_and_needs_no_scales():
    from drnmi.drnseg import DRNSeg
    m = DRNSeg("drn_d_22", 19, pretrained=False)
    e, q = m.qat_layers()                      # a property of the architecture: no scales, no device
    assert "seg" in e and len(q) == 15 and m._act_scales is None
    assert getattr(m, "_qat", "x") is None
