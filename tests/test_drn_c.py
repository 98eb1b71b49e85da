"""DRN-C (drn_c_26 / 42 / 58) without a GPU: the CPU restatement against the reference goldens, the
module tree's state_dict, the lowering's wiring, and the host side of the fused 16-channel block.

Goldens: tests/golden/drn_c.N.npz (tests/golden/make_drn_c_golden.py ran the reference's own
drn.drn_c_26 / drn_c_42 under the lmodels/drnseg.DRNSeg head)."""
from __future__ import annotations

import ctypes
import glob
import json
import os

import numpy as np
import pytest
import torch

import drn_c_ref as R
from drnmi import _lib
from drnmi.drnseg import DRNSeg
from drnmi.weights import synth_state_dict

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# (c58: the Bottleneck trunk and the residual=False BasicBlocks that carry an unused downsample)
CASES = {"c26_2x72x136": "drn_c_26", "c42_1x64x128": "drn_c_42", "c58_1x32x64": "drn_c_58"}
_GOLD = {}


def golden():
    """All arrays of tests/golden/drn_c.N.npz as one dict (loaded once)."""
    if not _GOLD:
        paths = sorted(glob.glob(os.path.join(GOLDEN, "drn_c.*.npz")))
        assert paths, "tests/golden/drn_c.N.npz missing"
        for p in paths:
            z = np.load(p, allow_pickle=False)
            for k in z.files:
                assert k not in _GOLD
                _GOLD[k] = z[k]
    return _GOLD


_MODELS = {}


def cpu_model(arch, seed):
    if (arch, seed) not in _MODELS:
        m = DRNSeg(arch, 19, pretrained=False)
        m.load_state_dict(synth_state_dict(m, seed))
        _MODELS[(arch, seed)] = m.eval()
    return _MODELS[(arch, seed)]


@pytest.mark.parametrize("case", list(CASES))
def test_restatement_equals_reference(case):
    g = golden()
    arch, seed = CASES[case], int(g[case + "/meta"][0])
    sd = cpu_model(arch, seed).state_dict()
    x = torch.from_numpy(g[case + "/input"])
    lp, logits, stages = R.drnseg_forward(sd, arch, x)
    assert np.abs(logits.numpy() - g[case + "/logits"]).max() == 0
    assert np.abs(lp.numpy()[:, :, ::7, ::7] - g[case + "/logprobs_sub7"]).max() == 0
    assert np.array_equal(torch.max(lp, 1)[1].numpy().astype(np.uint8), g[case + "/labels"])
    assert sorted(stages) == [f"layer{i}" for i in range(9)]
    for name, v in stages.items():
        assert np.array_equal(v[:, :, :4, :4].numpy(), g[f"{case}/stage_crop/{name}"]), name


def test_fixture_margins():
    """At most 0.01 % of a case's pixels may have a reference top-2 margin <= 1e-4 (the GPU label
    comparison leaves those out); the reference has none."""
    g = golden()
    for case in CASES:
        m = g[case + "/top2_margin"]
        assert (m <= 1e-4).sum() <= 1e-4 * m.size


@pytest.mark.parametrize("arch", ["drn_c_26", "drn_c_42", "drn_c_58"])
def test_state_dict_keys_and_shapes(arch):
    want = json.loads(str(golden()["keys/" + arch]))
    m = DRNSeg(arch, 19, pretrained=False)
    got = sorted([k, list(v.shape)] for k, v in m.state_dict().items())
    assert got == want
    assert "layer.0.weight" in m.state_dict() and "layer.1.running_var" in m.state_dict()
    assert not any(k.startswith("layer.2.") for k in m.state_dict())


def test_factories_and_arch_list():
    from drnmi import drn
    for name in ("drn_c_26", "drn_c_42", "drn_c_58"):
        assert name in drn.ARCHS and callable(getattr(drn, name))
    assert "drn_d_22" in drn.ARCHS
    with pytest.raises(KeyError):
        DRNSeg("drn_a_50", 19, pretrained=False)


@pytest.mark.parametrize("prefix", ["base.", "module.", "module.base."])
def test_prefixed_checkpoints_load(prefix):
    m = cpu_model("drn_c_26", 6)
    sd = m.state_dict()
    ck = {}
    for k, v in sd.items():
        k2 = k[len("layer."):] if k.startswith("layer.") and "base." in prefix else k
        p = prefix if k.startswith("layer.") else prefix.replace("base.", "")
        ck[p + k2] = v.clone()
    m2 = DRNSeg("drn_c_26", 19, pretrained=False)
    m2.load_state_dict(ck)
    for k, v in m2.state_dict().items():
        assert torch.equal(v, sd[k]), k


def test_lowering_wiring():
    m = cpu_model("drn_c_26", 6)
    g = m._graph
    by = {nd.name: nd for nd in g.nodes}
    keys = set(m.state_dict())
    for nd in g.nodes:                              # node names are state_dict prefixes
        assert nd.name + ".weight" in keys, nd.name
    assert g.nodes[0].name == "layer.0" and g.nodes[0].bn is m.layer[1]
    stem = by["layer.0"].dst
    assert g.stage_outputs["layer0"] == stem
    assert by["layer.3.0.conv1"].src == stem and by["layer.3.0.conv2"].res == stem
    assert by["layer.4.0.conv2"].res == by["layer.4.0.downsample.0"].dst
    assert by["layer.4.0.downsample.0"].src == by["layer.3.0.conv2"].dst
    assert by["layer.9.0.conv2"].res is None and by["layer.10.0.conv2"].res is None
    assert list(g.stage_outputs) == [f"layer{i}" for i in range(9)]
    assert g.stage_outputs["layer1"] == by["layer.3.0.conv2"].dst
    assert g.stage_outputs["layer8"] == by["layer.10.0.conv2"].dst == by["seg"].src
    # the D family keeps its names
    d = DRNSeg("drn_d_22", 19, pretrained=False)._graph
    assert list(d.stage_outputs) == [f"layer{i}" for i in range(9)] and d.nodes[0].name == "layer.0.0"
    assert d.stage_outputs["layer0"] == d.nodes[0].dst


def test_c58_lowering_leaves_unused_downsample_out():
    """layer7 of drn_c_58 is a BasicBlock(2048 -> 512, residual=False): _make_layer gives it a 1x1
    downsample that forward never runs (lmodels/drn.py:49-65).  Its weights are in the state_dict;
    the graph has no node for it, and the block's last conv has no residual."""
    m = cpu_model("drn_c_58", 9)
    assert "layer.9.0.downsample.0.weight" in m.state_dict()
    by = {nd.name: nd for nd in m._graph.nodes}
    assert "layer.9.0.downsample.0" not in by and by["layer.9.0.conv2"].res is None
    assert by["layer.9.0.conv1"].src == by["layer.8.2.conv3"].dst
    assert by["layer.5.0.conv3"].res == by["layer.5.0.downsample.0"].dst
    assert by["layer.5.1.conv3"].res == by["layer.5.0.conv3"].dst


def test_launch_work_of_a_fused_block16():
    """drnmi.roofline.launch_work on a plan with the fused block: the launch's row is the second
    conv's (where timing_hook reports it), carries both convs' FLOPs, and its activation bytes are x
    in + y out (64 B per pixel in bf16) instead of the two launches' 160 B; conv1's row is empty and
    the intermediate has no HBM buffer.  (A Plan on the CPU device: no launch is made.)"""
    from drnmi.engine import PackedNet, Plan
    from drnmi.roofline import launch_work, node_work
    m = cpu_model("drn_c_26", 6)
    n, h, w = 2, 72, 136
    plan = Plan(PackedNet(m._graph, "bf16", torch.device("cpu"), block_sparse=False), n, h, w)
    i = [nd.name for nd in plan.packed.graph.nodes].index("layer.3.0.conv1")
    assert list(plan.block16) == [i] and not plan.stem_fused and not plan.front_fused
    assert plan.args[i] is None and plan.packed.graph.nodes[i].dst not in plan.bufs
    rows, fused = node_work(plan), launch_work(plan)
    assert fused[i][1:] == (0.0, 0.0)
    assert fused[i + 1][1] == rows[i][1] + rows[i + 1][1] == 2 * 2.0 * n * h * w * 16 * 144
    px = n * h * w
    assert rows[i][2] + rows[i + 1][2] - fused[i + 1][2] == 3 * px * 32      # t written, t read, x read again
    weights = fused[i + 1][2] - 64 * px
    assert 0 <= weights <= 2 * (16 * 144 * 2 + 1024)                          # what is left: the two convs' weights
    keep = Plan(plan.packed, n, h, w, keep_all=True)
    assert not keep.block16 and launch_work(keep)[i][1] == rows[i][1]


def test_int8_refused_on_arch_c():
    m = cpu_model("drn_c_26", 6)
    with pytest.raises(NotImplementedError, match="int8"):
        m.set_precision("int8")
    assert m.precision == "fp32"
    assert m.set_precision("bf16").precision == "bf16"
    m.set_precision("fp32")


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    w1 = torch.randn(16, 16, 3, 3, generator=g) * (2 / 144) ** 0.5
    w2 = torch.randn(16, 16, 3, 3, generator=g) * (2 / 144) ** 0.5
    s1, s2 = torch.rand(16, generator=g) + 0.5, torch.rand(16, generator=g) + 0.5
    b1, b2 = torch.randn(16, generator=g) * 0.2, torch.randn(16, generator=g) * 0.2
    return w1, s1, b1, w2, s2, b2


def pack16(lib, p):
    arrs = [t.contiguous().float().numpy() for t in p]
    out = np.zeros(int(lib.drnmi_block16_pack_bytes()), dtype=np.uint8)
    rc = lib.drnmi_block16_pack(*[a.ctypes.data_as(ctypes.c_void_p) for a in arrs], out.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0
    return out


def test_block16_pack_and_supported_without_gpu():
    lib = _lib.load()
    nw = 2 * 5 * 64 * 16
    assert lib.drnmi_block16_pack_bytes() == nw + 2 * 16 * 4
    assert lib.drnmi_block16_supported(8, 1024, 2048) == 1
    assert lib.drnmi_block16_supported(0, 8, 8) == 0
    assert lib.drnmi_block16_supported(1, 0, 8) == 0 and lib.drnmi_block16_supported(1, 8, 0) == 0
    assert lib.drnmi_block16_supported(32, 1024, 2048) == 0      # 2^31 bytes: one past the resources' range
    assert lib.drnmi_block16_supported(1, 1, 1) == 1
    assert lib.drnmi_basic_block16(None, None, None, 1, 8, 8, None) == -1
    buf = (ctypes.c_char * 64)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.drnmi_basic_block16(ptr, ptr, None, 1, 8, 8, None) == -1
    assert lib.drnmi_basic_block16(ptr, ptr, ptr, 1, 8, 8, None) == -1      # y aliases x
    assert lib.drnmi_basic_block16(ptr, ptr, ctypes.c_void_p(ptr.value + 32), 0, 8, 8, None) == -1
    assert lib.drnmi_block16_pack(None, None, None, None, None, None, None) == -1
    p = _params(3)
    blob = pack16(lib, p)
    frag = blob[:nw].view(np.uint16).reshape(2, 5, 64, 8)
    # (conv 1, chunk 2, lane 53 (fr 5, fq 3), element 6): tap 2 * 2 + 1 = 5 (kh 1, kw 2), input channel
    # 8 * 1 + 6: w2[5][14][1][2] * s2[5] in bf16
    want = (p[3][5, 14, 1, 2] * p[4][5]).bfloat16().view(torch.int16).item() & 0xffff
    assert int(frag[1, 2, 53, 6]) == want
    # (conv 0, chunk 4, lane 9 (fr 9, fq 0), element 0): tap 8 (kh 2, kw 2), channel 0
    want = (p[0][9, 0, 2, 2] * p[1][9]).bfloat16().view(torch.int16).item() & 0xffff
    assert int(frag[0, 4, 9, 0]) == want
    assert not frag[:, 4, 32:, :].any()                          # the tenth tap: zero weights
    sh = blob[nw:].view(np.float32)
    np.testing.assert_array_equal(sh[:16], p[2].numpy())
    np.testing.assert_array_equal(sh[16:], p[5].numpy())
