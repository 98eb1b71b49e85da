"""The DRN-D variants beyond D-22 / 38 / 54 without a GPU: drn_d_24 / 40 / 56 (two conv+BN+ReLU units
in layer7 and in layer8) and drn_d_105 / 107 (23 Bottlenecks in layer5).  The CPU oracle against
reference goldens of their own, the module tree's state_dict, the lowering's wiring and the host's
8-bit layout decision on the two-conv tail.

Goldens: tests/golden/drn_d_more.N.npz (tests/golden/make_drn_d_more_golden.py ran the reference's own
drn.drn_d_24 / 40 / 56 / 105 / 107 under the lmodels/drnseg.DRNSeg head; no case has a pixel whose
reference top-2 margin is <= 1e-4, and the oracle's fp64 logits lie within 2.5e-4 of every case's)."""
from __future__ import annotations

import glob
import json
import os

import numpy as np
import pytest
import torch

from drnmi import drn
from drnmi.drnseg import DRNSeg
from drnmi.engine import channel_strides, int8_layout
from drnmi.weights import synth_state_dict
from oracle import drn_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = {"d24_2x72x136": "drn_d_24", "d40_1x64x128": "drn_d_40", "d56_1x64x128": "drn_d_56",
         "d105_1x32x64": "drn_d_105", "d107_1x32x64": "drn_d_107"}
NEW_ARCHS = tuple(CASES.values())
D_ARCHS = tuple(drn._DRN_D)
TWO_CONV_TAIL = ("drn_d_24", "drn_d_40", "drn_d_56", "drn_d_107")
_GOLD = {}
_MODELS = {}


def golden():
    """All arrays of tests/golden/drn_d_more.N.npz as one dict (loaded once)."""
    if not _GOLD:
        paths = sorted(glob.glob(os.path.join(GOLDEN, "drn_d_more.*.npz")))
        assert paths, "tests/golden/drn_d_more.N.npz missing"
        for p in paths:
            z = np.load(p, allow_pickle=False)
            for k in z.files:
                assert k not in _GOLD
                _GOLD[k] = z[k]
    return _GOLD


def cpu_model(arch, seed=0):
    if (arch, seed) not in _MODELS:
        m = DRNSeg(arch, 19, pretrained=False)
        m.load_state_dict(synth_state_dict(m, seed))
        _MODELS[(arch, seed)] = m.eval()
    return _MODELS[(arch, seed)]


def test_fixture_conditions():
    """What the recipe promised: the five cases, no pixel at or below the 1e-4 margin (the GPU label
    gate excludes nothing), every part under the 1 MiB limit of a committed file."""
    g = golden()
    for case in CASES:
        assert int((g[case + "/top2_margin"] <= 1e-4).sum()) == 0, case
        n, h, w = (int(v) for v in g[case + "/meta"][1:])
        assert g[case + "/input"].shape == (n, 3, h, w) and g[case + "/logits"].shape == (n, 19, h // 8, w // 8)
        assert len(np.unique(g[case + "/labels"])) > 1
    for p in glob.glob(os.path.join(GOLDEN, "drn_d_more.*.npz")):
        assert os.path.getsize(p) < 1 << 20, p


@pytest.mark.parametrize("case", list(CASES))
def test_oracle_matches_reference(case):
    """tests/test_oracle_golden.py's gates on the new cases: the same ATen kernels on the same weights
    give max-abs 0 on logits and log-probs, identical labels on every pixel, and the per-stage sums
    (plus the stage crops, bit for bit)."""
    torch.set_num_threads(8)
    g = golden()
    arch, seed = CASES[case], int(g[case + "/meta"][0])
    sd = cpu_model(arch, seed).state_dict()
    x = torch.from_numpy(g[case + "/input"])
    np.testing.assert_array_equal(O.preprocess_u8(g[case + "/frames"]).numpy(), g[case + "/input"])
    lp, logits, stages = O.drnseg_forward(sd, arch, x)
    assert np.abs(logits.numpy() - g[case + "/logits"]).max() == 0
    assert np.abs(lp.numpy()[:, :, ::7, ::7] - g[case + "/logprobs_sub7"]).max() == 0
    assert np.array_equal(O.labels_of(lp).numpy().astype(np.uint8), g[case + "/labels"])
    ref_planes = g[case + "/logprob_plane_sum"]
    assert np.abs(lp.double().sum(dim=(2, 3)).numpy() - ref_planes).max() <= 1e-9 * np.abs(ref_planes).max()
    assert sorted(stages) == [f"layer{i}" for i in range(9)]
    for k, v in stages.items():
        ref = g[case + "/stage_sum/" + k]
        assert abs(v.double().sum().item() - ref[0]) <= 1e-4 * ref[1] + 1e-6, k
        assert np.array_equal(v[:, :, :4, :4].numpy(), g[f"{case}/stage_crop/{k}"]), k


def test_arch_tables_agree():
    """drnmi.drn's D table and the oracle's name the same eight variants with the same block counts."""
    assert set(D_ARCHS) == set(O.ARCHS) and len(D_ARCHS) == 8
    for name, (block, layers) in drn._DRN_D.items():
        assert O.ARCHS[name] == ("basic" if block is drn.BasicBlock else "bottleneck", layers), name
        assert name in drn.ARCHS and callable(getattr(drn, name))


@pytest.mark.parametrize("arch", D_ARCHS)
def test_state_dict_keys_and_shapes(arch):
    """Every name of the D table against the reference's own DRNSeg-wrapped model: keys/<arch> of the
    fixture that recorded it (D-22 / 38 / 54: no key list was recorded; their keys are pinned by
    loading the reference's state_dict order in test_oracle_golden / test_weights)."""
    m = DRNSeg(arch, 19, pretrained=False)
    got = sorted([k, list(v.shape)] for k, v in m.state_dict().items())
    if arch in NEW_ARCHS:
        assert got == json.loads(str(golden()["keys/" + arch]))
    else:
        # the three older variants are the newer ones minus the second layer7 / layer8 unit
        twin = {"drn_d_22": "drn_d_24", "drn_d_38": "drn_d_40", "drn_d_54": "drn_d_56"}[arch]
        want = [kv for kv in json.loads(str(golden()["keys/" + twin]))
                if not kv[0].startswith(("layer.7.3.", "layer.7.4.", "layer.8.3.", "layer.8.4."))]
        assert got == want


def _expected_nodes(sd, arch):
    """The conv launches in the oracle's execution order (oracle/drn_oracle.py backbone: conv-bn-relu
    units; blocks as conv1, [conv2,] the downsample where the block has one, then the block's last
    conv), as (name, src name or None = the input, residual name or None), from the block structure."""
    kind, layers = O.ARCHS[arch]
    out, cur = [], None

    def unit(name, src):
        out.append((name, src, None))
        return name

    cur = unit("layer.0.0", cur)
    for li, n in ((1, layers[0]), (2, layers[1])):
        for j in range(n):
            cur = unit(f"layer.{li}.{3 * j}", cur)
    convs = ("conv1", "conv2") if kind == "basic" else ("conv1", "conv2", "conv3")
    for li, n in ((3, layers[2]), (4, layers[3]), (5, layers[4]), (6, layers[5])):
        for b in range(n):
            p, x = f"layer.{li}.{b}", cur
            for cv in convs[:-1]:
                cur = unit(f"{p}.{cv}", cur)
            res = x
            if f"{p}.downsample.0.weight" in sd:
                res = unit(f"{p}.downsample.0", x)
            out.append((f"{p}.{convs[-1]}", cur, res))
            cur = f"{p}.{convs[-1]}"
    for li, n in ((7, layers[6]), (8, layers[7])):
        for j in range(n):
            cur = unit(f"layer.{li}.{3 * j}", cur)
    out.append(("seg", cur, None))
    return out


@pytest.mark.parametrize("arch", D_ARCHS)
def test_lowering_order_and_wiring(arch):
    m = cpu_model(arch)
    sd = m.state_dict()
    g = m._graph
    want = _expected_nodes(sd, arch)
    assert [nd.name for nd in g.nodes] == [w[0] for w in want]
    # one node per 4-D non-up. weight
    assert sorted(nd.name for nd in g.nodes) == sorted(k[:-len(".weight")] for k, v in sd.items()
                                                      if k.endswith(".weight") and v.dim() == 4 and not k.startswith("up."))
    by = {nd.name: nd for nd in g.nodes}
    dst_of = {nd.name: nd.dst for nd in g.nodes}
    assert len(set(dst_of.values())) == len(g.nodes)
    for name, src, res in want:
        nd = by[name]
        assert nd.src == ("input" if src is None else dst_of[src]), name
        assert nd.res == (None if res is None else dst_of[res]), name
        assert nd.conv is dict(m.named_modules())[name]
        assert nd.relu == (not name.endswith("downsample.0") and name != "seg"), name
        assert g.channels[nd.dst] == nd.conv.out_channels
    # every block but the first of a layer adds its own input; the first adds the downsample's output
    kind, layers = O.ARCHS[arch]
    last = "conv2" if kind == "basic" else "conv3"
    for li, n in ((3, layers[2]), (4, layers[3]), (5, layers[4]), (6, layers[5])):
        # _make_layer (lmodels/drn.py:181-186): a downsample where the stride or the width changes
        first = [by[f"layer.{li}.0.{cv}"].conv for cv in (("conv1", "conv2") if kind == "basic" else ("conv1", "conv2", "conv3"))]
        assert (f"layer.{li}.0.downsample.0" in by) == \
            (first[0].in_channels != first[-1].out_channels or any(c.stride[0] != 1 for c in first))
        for b in range(1, n):
            assert f"layer.{li}.{b}.downsample.0" not in by
            assert by[f"layer.{li}.{b}.{last}"].res == by[f"layer.{li}.{b - 1}.{last}"].dst
    assert list(g.stage_outputs) == [f"layer{i}" for i in range(9)]
    ends = {0: "layer.0.0", 1: f"layer.1.{3 * (layers[0] - 1)}", 2: f"layer.2.{3 * (layers[1] - 1)}",
            7: f"layer.7.{3 * (layers[6] - 1)}", 8: f"layer.8.{3 * (layers[7] - 1)}"}
    for li, n in ((3, layers[2]), (4, layers[3]), (5, layers[4]), (6, layers[5])):
        ends[li] = f"layer.{li}.{n - 1}.{last}"
    for i, name in ends.items():
        assert g.stage_outputs[f"layer{i}"] == by[name].dst, i
    assert by["seg"].src == g.stage_outputs["layer8"] and by["seg"].out_fp32_nchw


def test_node_counts():
    """28 / 44 / 60 / 109 / 111 conv launches (D-22 / 38 / 54: 26 / 42 / 58)."""
    want = {"drn_d_22": 26, "drn_d_24": 28, "drn_d_38": 42, "drn_d_40": 44, "drn_d_54": 58, "drn_d_56": 60,
            "drn_d_105": 109, "drn_d_107": 111}
    assert {a: len(cpu_model(a)._graph.nodes) for a in D_ARCHS} == want


@pytest.mark.parametrize("arch", D_ARCHS)
def test_int8_layout(arch):
    """The 8-bit layout of each variant: a value is 8-bit in HBM only when an eligible (W8A8) node
    produces it and nothing but eligible nodes read it; `need` is exactly what the eligible nodes read,
    and every needed value is either 8-bit already or produced by some node (so PackedNet can quantise
    a copy after it); the whole tail -- the second layer7 unit, both layer8 units and seg -- is W8A8
    with 8-bit values in between."""
    g = cpu_model(arch)._graph
    elig, q8, need = int8_layout(g, channel_strides(g))
    by = {nd.name: i for i, nd in enumerate(g.nodes)}
    producer = {nd.dst: i for i, nd in enumerate(g.nodes)}
    readers = {}
    for i, nd in enumerate(g.nodes):
        for v in (nd.src, nd.res):
            if v:
                readers.setdefault(v, set()).add(i)
    assert len(set(q8)) == len(q8)
    for v in q8:
        assert producer[v] in elig, v
        assert readers[v] and readers[v] <= elig, v
    # ... and no value that could be 8-bit is left out
    for i in elig:
        v = g.nodes[i].dst
        if v != "logits" and readers.get(v) and readers[v] <= elig:
            assert v in q8, v
    assert need == {v for i in elig for v in (g.nodes[i].src, g.nodes[i].res) if v}
    assert "input" not in need and "logits" not in q8
    for v in need:
        assert v in q8 or v in producer, v
    tail = [n for n in ("layer.7.0", "layer.7.3", "layer.8.0", "layer.8.3", "seg") if n in by]
    assert len(tail) == (5 if arch in TWO_CONV_TAIL else 3)
    for a, b in zip(tail, tail[1:]):
        assert by[a] in elig and by[b] in elig
        assert g.nodes[by[b]].src == g.nodes[by[a]].dst and g.nodes[by[a]].dst in q8, (a, b)
    # qat_layers() is the same decision by name
    names, vals = cpu_model(arch).qat_layers()
    assert names == [g.nodes[i].name for i in sorted(elig)] and set(vals) == need
    assert all(n in names for n in tail)


def test_int8_oracle_float64_sums_are_the_int64_ones():
    """oracle/int8_oracle.py conv_i8(acc_via_f64=True), which the whole-network int8 checks of the new
    variants use, is conv_i8 bit for bit: all-127 operands at the largest K of any DRN-D conv (3 x 3 x
    512: the largest sum the form has to hold exactly) and random ones with a residual."""
    from oracle import int8_oracle as Q
    rng = np.random.default_rng(3)
    k = 9 * 512
    for fill in (127, None):
        x = np.full((1, 5, 6, 512), 127, np.int8) if fill else rng.integers(-127, 128, (1, 5, 6, 512), dtype=np.int8)
        w = np.full((128, k), -127, np.int8) if fill else rng.integers(-127, 128, (128, k), dtype=np.int8)
        res = rng.integers(-127, 128, (1, 5, 6, 40), dtype=np.int8)
        scale = np.full(128, 1.0 / (np.sqrt(k) * 5400.0), np.float32)
        shift = rng.normal(0, 0.5, 128).astype(np.float32)
        for out in ("i8", "bf16", "f32"):
            a, b = (Q.conv_i8(x, w, scale, shift, 40, 3, 1, 2, 2, True, res, 0.011, out, 1.0 / 0.023, acc_via_f64=f)
                    for f in (False, True))
            np.testing.assert_array_equal(a, b)
