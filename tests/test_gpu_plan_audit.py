"""Every launch of the shipped fused plans against a high-precision reference (tests/plan_audit.py).

The per-stage network tests run keep_all plans (no fused front, block64, folded downsamples,
seg-fused layer8 or buffer reuse) on frames too narrow for the strip kernels; the tests that reach
the strip kernels gate on label agreement or compare one GPU kernel with another.  Here the plan
DRNSeg.segment() ships runs on thin 2048- and 4096-wide frames, which take the headline's exact
routing (it depends on the spatial size only through wo % 256), and every launch is re-computed
on the CPU from the inputs the GPU gave it: float64 for the bf16 launches (gate: one output
rounding plus the measured accumulation-order term), oracle/int8_oracle.py bit for bit for the
int8 ones.  The CPU tests (no gpu mark) prove the audit itself: its reference against float64
F.conv2d, and that it notices a missing 8-channel chunk, a dropped K step, a shifted row and a
two-ulp error.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import plan_audit as A
from oracle import int8_oracle as Q

F64 = np.float64

# DESIGN.md §3.1, kernel column (bf16 headline path) and its int8 list (§3.1 / §3.6) on top of the
# bf16 launches an int8 net keeps (layer0-3 and layer4.0 with its folded downsample)
D22_BF16_KERNELS = {"front3", "conv_s2row<32>", "conv_s2row<64>", "conv_s1x2row", "block64", "conv_w1h",
                    "conv_w1h_x2", "conv_stag", "conv_stag_x2", "conv_w1", "conv_w1_seg", "up8_labels_tile"}
D22_INT8_KERNELS = {"front3", "conv_s2row<32>", "conv_s2row<64>", "conv_s1x2row", "block64", "conv_w1h_x2",
                    "conv_w1h_i8", "conv_i8_occ2", "conv_i8_stag", "conv_w1_i8_seg", "up8_labels_tile"}


# ----------------------------------------------------------------------------- GPU: the audit
@pytest.mark.gpu
@pytest.mark.parametrize("group", A.GROUPS)
@pytest.mark.parametrize("cfg", list(A.CONFIGS))
def test_plan_launches_match_reference(cfg, group):
    """Every launch of `group` in the shipped plan of `cfg`, from its own inputs.  All figures are
    printed before the verdict: a (accumulation-order term), worst excess over the gate (<= 0
    passes), share beyond the tight gate, excluded head pixels."""
    recs = A.launches(cfg, group)
    assert recs, f"no launch of {group} captured"
    failed = []
    for rec in recs:
        try:
            st = A.check_launch(rec)
        except AssertionError as e:
            st = f"FAILED: {str(e)[:600]}"
            failed.append(rec.name)
        print(f"{cfg} #{rec.index} {rec.name} [{rec.kernel}]: {st}")
    assert not failed, failed


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", list(A.CONFIGS))
def test_plan_launches_all_audited(cfg):
    """Every captured launch falls in exactly one audited group and has a reference; the D-22 and
    D-24 plans run the kernels DESIGN.md §3.1 lists, all of them and no other."""
    recs = A.capture(cfg)
    assert [r.index for r in recs] == sorted({r.index for r in recs})
    assert sum(len(A.launches(cfg, g)) for g in A.GROUPS) == len(recs)
    for r in recs:
        assert r.group in A.GROUPS and r.kind in ("front", "block64", "conv", "seg_conv", "head"), r.name
        assert (r.conv is not None) == (r.kind in ("conv", "seg_conv")), r.name
    assert {r.group for r in recs} == set(A.GROUPS)
    names = {A.short_name(r.kernel) for r in recs}
    print(f"{cfg}: {len(recs)} launches, kernels {sorted(names)}")
    # (D-24: D-22 with a second conv+BN+ReLU unit in layer7 and layer8, on the kernels D-22 runs)
    if cfg.startswith(("d22_bf16", "d24_bf16")):
        assert names == D22_BF16_KERNELS, names ^ D22_BF16_KERNELS
    elif cfg.startswith(("d22_int8", "d24_int8")):
        assert names == D22_INT8_KERNELS, names ^ D22_INT8_KERNELS
        assert any(r.quant for r in recs), "no bf16 -> int8 copy audited"
    else:
        assert {"front3", "conv_stag", "conv_w1", "conv_w1_seg", "up8_labels_tile"} <= names


# ----------------------------------------------------------------------------- CPU: the audit itself
def _bf16(a):
    return A.bf16_round(np.asarray(a, np.float32))


def _synthetic(seed, n, h, w, cin, cs, cout, dil, x2=False, res=True, fold=True):
    """A launch record packed by the numpy packer, with its logical operands."""
    g = np.random.default_rng(seed)
    x = np.zeros((n, h, w, cs), np.float32)
    x[..., :cin] = _bf16(np.maximum(g.normal(0, 1, (n, h, w, cin)), 0))
    wl = _bf16(g.normal(0, np.sqrt(2.0 / (9 * cin)), (cout, cin, 3, 3)))
    scale = g.uniform(0.5, 1.5, cout).astype(np.float32)
    shift = g.normal(0, 0.2, cout).astype(np.float32)
    d = {"x": x, "w": wl, "scale": scale, "shift": shift, "res": None, "x2": None, "w_ds": None}
    if res and not x2:
        d["res"] = _bf16(np.maximum(g.normal(0, 1, (n, h, w, cout)), 0))
    if x2:
        d["x2"] = _bf16(np.maximum(g.normal(0, 1, (n, 2 * h, 2 * w - 1, 32)), 0))
        d["w_ds"] = _bf16(g.normal(0, np.sqrt(2.0 / 32), (cout, 32)))
    wpk, k = A.pack_conv_weight(wl, cs, scale if fold else None, d["w_ds"])
    wpk = _bf16(wpk) if fold else wpk.astype(np.float32)
    rec = A.ConvRec(x=x, wpk=wpk, shift=np.pad(shift, (0, wpk.shape[0] - cout)), k=k, k_pad=wpk.shape[1], cout=cout,
                    ks=3, stride=1, pad=dil, dil=dil, relu=True,
                    scale=None if fold else np.pad(scale, (0, wpk.shape[0] - cout)), res=d["res"], x2=d["x2"], stride2=2)
    return rec, d


@pytest.mark.parametrize("case", ["dil4", "x2"])
def test_reference_matches_float64_conv2d(case):
    """conv_value64 (im2col in the packed K order) == float64 F.conv2d on the logical weights
    (+ the 1x1 stride-2 conv of x2) * scale + shift + residual; the fp32 value agrees to fp32."""
    rec, d = _synthetic(1, 2, 7, 11, 12, 16, 24, 4 if case == "dil4" else 1, x2=case == "x2", fold=False)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=F64))
    x = t(d["x"][..., :12]).permute(0, 3, 1, 2)
    v = F.conv2d(x, t(d["w"]), padding=rec.pad, dilation=rec.dil)
    if case == "x2":
        v = v + F.conv2d(t(d["x2"]).permute(0, 3, 1, 2), t(d["w_ds"]).view(24, 32, 1, 1), stride=2)
    v = v * t(d["scale"]).view(1, -1, 1, 1) + t(d["shift"]).view(1, -1, 1, 1)
    v = v.permute(0, 2, 3, 1)
    if d["res"] is not None:
        v = v + t(d["res"])
    got = A.conv_value64(rec)
    assert got.shape == tuple(v.shape) == (2, 7, 11, 24)
    np.testing.assert_allclose(got, v.numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(A.conv_value32(rec), v.numpy(), rtol=0, atol=2e-5)
    a = A.order_term(rec, got)
    assert 0 < a < 1e-4, a


@pytest.mark.parametrize("out,res,ks,stride", [("i8", True, 3, 1), ("bf16", False, 3, 2), ("f32", True, 1, 1)])
def test_int8_value_matches_oracle(out, res, ks, stride):
    """conv_i8_value (float64 matmul) == oracle/int8_oracle.py conv_i8 (int64 matmul), bit for bit."""
    g = np.random.default_rng(5)
    n, h, w, cin, cout = 2, 6, 9, 64, 40
    x = g.integers(-127, 128, (n, h, w, cin), dtype=np.int8)
    k = ks * ks * cin
    wpk = np.zeros((128, k), np.int8)
    wpk[:cout] = g.integers(-127, 128, (cout, k), dtype=np.int8)
    scale = (g.uniform(0.5, 1.5, 128) / (np.sqrt(k) * 5400.0)).astype(np.float32)
    shift = g.normal(0, 0.5, 128).astype(np.float32)
    pad = 2 if ks == 3 else 0
    ho, wo = (h + 2 * pad - 2 * (ks - 1) - 1) // stride + 1, (w + 2 * pad - 2 * (ks - 1) - 1) // stride + 1
    r = g.integers(-127, 128, (n, ho, wo, cout), dtype=np.int8) if res else None
    rec = A.ConvRec(x=x, wpk=wpk, shift=shift, k=k, k_pad=k, cout=cout, ks=ks, stride=stride, pad=pad, dil=2, relu=True,
                    scale=scale, res=r, i8=True, out=out, res_scale=0.011, out_scale=1.0 / 0.023)
    want = Q.conv_i8(x, wpk, scale, shift, cout, ks, stride, pad, 2, True, r, 0.011, out, 1.0 / 0.023)
    np.testing.assert_array_equal(A.conv_i8_value(rec), want)
    rec.got = want
    assert A.check_conv(rec)["exact"]
    rec.got = want.copy()
    rec.got.reshape(-1)[7] += 1
    with pytest.raises(AssertionError):
        A.check_conv(rec)


def _sensitivity_case():
    rec, _ = _synthetic(2, 1, 6, 10, 128, 128, 32, 2)
    v = A.conv_value64(rec)
    rec.got = _bf16(np.maximum(v, 0))
    return rec, v


def test_gate_passes_rounded_reference():
    """The bf16-rounded float64 value passes, with nothing to spare beyond half an ulp + a."""
    rec, _ = _sensitivity_case()
    st = A.check_conv(rec)
    print(st)
    assert st["worst_excess"] <= 0 and 0 < st["a"] < 1e-4


def test_gate_fails_missing_chunk_at_border_pixel():
    """One 8-channel chunk of one tap (the centre one) missing at the corner pixel."""
    rec, v = _sensitivity_case()
    cin = 128
    cols = slice(4 * cin + 8, 4 * cin + 16)
    v2 = v[0, 0, 0] - rec.wpk[:32, cols].astype(F64) @ rec.x[0, 0, 0, 8:16].astype(F64)
    assert np.abs(v2 - v[0, 0, 0]).max() > 0
    rec.got[0, 0, 0] = _bf16(np.maximum(v2, 0))
    with pytest.raises(AssertionError, match="worst at"):
        A.check_conv(rec)


def test_gate_fails_dropped_last_k_step():
    rec, v = _sensitivity_case()
    cols, _, _ = A._cols(rec)
    v2 = v - (cols[:, rec.k - 64:] @ rec.wpk[:32, rec.k - 64:rec.k].astype(F64).T).reshape(v.shape)
    rec.got = _bf16(np.maximum(v2, 0))
    with pytest.raises(AssertionError, match="worst at"):
        A.check_conv(rec)


def test_gate_fails_row_shifted_by_one_pixel():
    rec, _ = _sensitivity_case()
    rec.got[0, 3] = np.roll(rec.got[0, 3], 1, axis=0)
    with pytest.raises(AssertionError, match="worst at"):
        A.check_conv(rec)


def test_gate_fails_two_ulps():
    rec, v = _sensitivity_case()
    idx = np.unravel_index(int(np.argmax(rec.got)), rec.got.shape)
    ulp = 2.0 ** (np.floor(np.log2(rec.got[idx])) - 7)
    rec.got[idx] += np.float32(2 * ulp)
    assert _bf16(rec.got[idx]) == rec.got[idx]
    with pytest.raises(AssertionError, match=str(tuple(int(i) for i in idx)).replace("(", r"\(").replace(")", r"\)")):
        A.check_conv(rec)


def test_packing_check():
    """check_packing accepts the bf16 rounding of w*scale (with the downsample columns) and refuses
    an unscaled row or a non-zero padding column."""
    rec, d = _synthetic(3, 1, 4, 6, 64, 64, 24, 1, x2=True)
    rec.w, rec.bn_scale, rec.w_ds, rec.bn_scale_ds = d["w"], d["scale"], d["w_ds"], None
    A.check_packing(rec)
    bad = rec.wpk.copy()
    bad[5, :64 * 9] = _bf16(bad[5, :64 * 9] / d["scale"][5])
    rec.wpk = bad
    with pytest.raises(AssertionError):
        A.check_packing(rec)
    rec, d = _synthetic(3, 1, 4, 6, 16, 16, 24, 1)
    rec.w, rec.bn_scale = d["w"], d["scale"]
    A.check_packing(rec)
    rec.wpk[0, rec.k + 1] = 1.0
    with pytest.raises(AssertionError, match="padding"):
        A.check_packing(rec)


def _seg_part(rec, act):
    part = np.stack([act[:, b * 256:(b + 1) * 256].astype(F64) @ rec.wseg[:19, b * 256:(b + 1) * 256].astype(F64).T
                     for b in range(2)])
    return part.reshape(2, 1, 3, 8, 19).astype(np.float32)


def _seg_case():
    """A 128 -> 512 conv with a 19-class seg product; returns (record, float64 v, act [24, 512])."""
    rec, _ = _synthetic(4, 1, 3, 8, 128, 128, 512, 1, res=False)
    g = np.random.default_rng(9)
    rec.wseg = np.zeros((32, 512), np.float32)
    rec.wseg[:19] = _bf16(g.normal(0, np.sqrt(2.0 / 19), (19, 512)))
    v = A.conv_value64(rec)
    act = _bf16(np.maximum(v, 0)).reshape(-1, 512)
    rec.part = _seg_part(rec, act)
    return rec, v, act


def test_seg_gate_resolution():
    """The seg-fused gate at the resolution it claims: the fp32-rounded float64 partials pass, and
    so do one-ulp flips of three activations whose v lies within the conv's order term of a
    rounding tie; a two-ulp error of one activation that cannot flip fails, and so does an
    8-channel chunk of the centre tap missing at the corner pixel, carried through wseg."""
    rec, v, act = _seg_case()
    st = A.check_seg_conv(rec)
    print(st)
    assert st["worst_excess"] <= 0 and st["worst_excess_flips"] <= 0 and st["beyond_a"] == 0 and st["a"] < 1e-4
    a_conv = A.order_term(rec, v)
    lo, hi = (_bf16(np.maximum(v + s * a_conv, 0)).reshape(-1, 512) for s in (-1, 1))
    can = np.argwhere((hi - lo) * np.abs(rec.wseg[:19]).max(axis=0)[None, :] > 1e-4)
    assert len(can) >= 3, len(can)
    flipped = act.copy()
    for p, c in can[:3]:
        flipped[p, c] = lo[p, c] if act[p, c] == hi[p, c] else hi[p, c]
    rec.part = _seg_part(rec, flipped)
    st = A.check_seg_conv(rec)
    assert st["beyond_a"] > 0 and st["max_diff"] > 10 * st["a"]

    fixed = np.where(hi == lo, act * np.abs(rec.wseg[:19]).max(axis=0)[None, :], 0)
    p, c = np.unravel_index(int(np.argmax(fixed)), fixed.shape)
    off = act.copy()
    off[p, c] += np.float32(2 * 2.0 ** (np.floor(np.log2(act[p, c])) - 7))
    rec.part = _seg_part(rec, off)
    with pytest.raises(AssertionError, match="worst at"):
        A.check_seg_conv(rec)

    cols = slice(4 * 128 + 8, 4 * 128 + 16)
    v2 = v.reshape(-1, 512).copy()
    v2[0] -= rec.wpk[:512, cols].astype(F64) @ rec.x[0, 0, 0, 8:16].astype(F64)
    rec.part = _seg_part(rec, _bf16(np.maximum(v2, 0)))
    with pytest.raises(AssertionError, match="worst at"):
        A.check_seg_conv(rec)


def test_head_reference():
    """Labels from the float64 head equal torch's fp32 transposed conv + argmax wherever the margin
    is decided; a changed label fails."""
    from drnmi.weights import bilinear_up_kernel
    rec, _, _ = _seg_case()
    up = bilinear_up_kernel(16).astype(np.float32)
    bias = np.linspace(-0.1, 0.1, 19).astype(np.float32)
    logits = torch.from_numpy(rec.part[0] + rec.part[1] + bias).permute(0, 3, 1, 2)
    lab = F.conv_transpose2d(logits, torch.from_numpy(up).expand(19, 1, 16, 16), stride=8, padding=4, groups=19).argmax(1)
    d = {"part": rec.part, "bias": bias, "scale": None, "up": up, "got": lab.to(torch.uint8).numpy()}
    st = A.check_head(d)
    assert st["mismatch_decided"] == 0 and d["got"].shape == (1, 24, 64)
    d["got"] = d["got"].copy()
    d["got"][0, 11, 30] = (d["got"][0, 11, 30] + 1) % 19
    with pytest.raises(AssertionError):
        A.check_head(d)


def test_groups_and_names():
    assert [A.group_of(s) for s in ("layer.0.0", "layer.2.0", "layer.3.1.conv2", "layer.6.0.downsample.0",
                                    "layer.8.0", "seg", None)] == \
        ["front", "front", "layer3", "layer6", "layer8+seg", "layer8+seg", "head"]
    # the second conv+BN+ReLU unit of layer7 / layer8 (D-24 / 40 / 56 / 107)
    assert [A.group_of(s) for s in ("layer.7.0", "layer.7.3", "layer.8.3")] == ["layer7", "layer7", "layer8+seg"]
    assert A.short_name("conv_s2row_kernel<32, 7, 2>") == "conv_s2row<32>"
    assert A.short_name("conv_big_kernel<1, 128, 2, 2, 64, false, 4, false, true>") == "conv_big"
    assert A.short_name("conv_w1h_x2_kernel") == "conv_w1h_x2" and A.short_name("front3_kernel") == "front3"
