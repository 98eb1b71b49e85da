"""The DRN-D variants no other GPU test builds -- drn_d_24 / 40 / 56 (two conv+BN+ReLU units in layer7
and in layer8) and drn_d_105 / 107 (23 Bottlenecks in layer5: 109 / 111 conv launches) -- end to end on
the HIP engine, against reference goldens of their own (tests/golden/drn_d_more.N.npz) and the oracles.

They are other launch lists than D-22 / 38 / 54's: in D-24 the seg classifier folds into layer.8.3 and
layer.8.0 is a plain 512 -> 512 dilation-1 launch (a shape D-22 only runs seg-fused); the 8-bit layout
has 8-bit values between four tail convs; D-105 / 107 reuse buffers over 100+ launches.

Gates: fp32 / fp32x logits and subsampled log-probs within 1e-3 max-abs of the reference and identical
labels on every pixel (no fixture pixel has a top-2 margin <= 1e-4); stage taps within 1e-4 x max(1,
|ref|max); the shipped (buffer-reusing) plan bit-equal to the keep_all plan in fp32; bf16 relative logit
error <= 0.03 and label agreement >= 0.98, then 1 - 2 x (1 - measured); int8 every launch bit for bit
against oracle/int8_oracle.py; 2:4 and graph capture as tests/test_gpu_sp24*.py and test_gpu_torch_ops.py."""
from __future__ import annotations

import json

import numpy as np
import pytest
import torch

from oracle import drn_oracle as O
from test_drn_d_variants import CASES, golden
from test_gpu_int8 import _int8_net, check_int8_every_launch
from test_gpu_plan_audit import D22_BF16_KERNELS

pytestmark = pytest.mark.gpu
DEV = "cuda"
TAIL = ("layer.7.0", "layer.7.3", "layer.8.0", "layer.8.3")
_MODELS = {}


def model(case):
    """One model per golden case (its arch, the case's weight seed), shared by the tests below; every
    test leaves it at precision fp32."""
    from drnmi.drnseg import build
    if case not in _MODELS:
        _MODELS[case] = build(CASES[case], 19, seed=int(golden()[case + "/meta"][0]), device=DEV)
    return _MODELS[case]


def _stream():
    from drnmi import _lib
    return _lib.stream_ptr(torch.device(DEV))


# ----------------------------------------------------------------------------- fp32 / fp32x parity
@pytest.mark.parametrize("precision", ["fp32", "fp32x"])
@pytest.mark.parametrize("case", list(CASES))
def test_fp32_forward_matches_reference(case, precision):
    g = golden()
    m = model(case).set_precision(precision)
    x = torch.from_numpy(g[case + "/input"]).to(DEV)
    lp, logits = m(x)
    m.set_precision("fp32")
    torch.cuda.synchronize()
    err = np.abs(logits.cpu().numpy() - g[case + "/logits"]).max()
    lperr = np.abs(lp.cpu().numpy()[:, :, ::7, ::7] - g[case + "/logprobs_sub7"]).max()
    labels = torch.max(lp, 1)[1].cpu().numpy()
    diff = int((labels != g[case + "/labels"]).sum())
    print(f"{case} {precision}: logit max-abs {err:.2e}, log-prob max-abs {lperr:.2e}, labels differ {diff} px of "
          f"{labels.size} ({int((g[case + '/top2_margin'] <= 1e-4).sum())} px with margin <= 1e-4)")
    assert err <= 1e-3 and lperr <= 1e-3
    assert diff == 0


@pytest.mark.parametrize("case", ["d24_2x72x136", "d56_1x64x128", "d107_1x32x64"])
def test_fp32_stages_match_oracle(case):
    """Per-stage taps (layer0 .. layer8) of a keep_all plan against the oracle's stages."""
    from drnmi import _lib
    g = golden()
    m = model(case).set_precision("fp32")
    x = torch.from_numpy(g[case + "/input"])
    plan = m.plan(x.shape[0], x.shape[2], x.shape[3], keep_all=True)
    plan.ingest_nchw(x.to(DEV), _lib.stream_ptr())
    plan.run_backbone(_lib.stream_ptr())
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    _, _, stages = O.drnseg_forward(sd, CASES[case], x)
    assert list(m._graph.stage_outputs) == [f"layer{i}" for i in range(9)]
    worst = 0.0
    for name, val in m._graph.stage_outputs.items():
        ref = stages[name]
        err = (plan.stage_nchw(val).cpu() - ref).abs().max().item()
        worst = max(worst, err / max(1.0, ref.abs().max().item()))
        assert err <= 1e-4 * max(1.0, ref.abs().max().item()), f"{name}: {err}"
    print(f"{case}: worst stage error / max(1, |ref|max) {worst:.2e}")


@pytest.mark.parametrize("precision", ["fp32", "fp32x"])
@pytest.mark.parametrize("case", ["d24_2x72x136", "d107_1x32x64"])
def test_reusing_plan_equals_keep_all_plan(case, precision):
    """m(x) on the shipped plan, whose buffers are reused as soon as their last reader has run, equals
    the keep_all plan (a buffer per value) bit for bit: on the NCHW path an fp32 / fp32x plan has no
    fused launch (the front, stem + layer1, block and downsample fusions are bf16 or uint8-frame
    forms), so both plans issue the same kernels on the same operands -- asserted below -- and only
    the buffer assignment differs.  A buffer handed on while a later launch still reads it shows here,
    at 28 and 111 nodes."""
    from drnmi import _lib
    g = golden()
    m = model(case).set_precision(precision)
    x = torch.from_numpy(g[case + "/input"]).to(DEV)
    n, _, h, w = x.shape
    lp, logits = m(x)
    plan, keep = m.plan(n, h, w), m.plan(n, h, w, keep_all=True)
    lib = _lib.load()
    sig = [[(l.kind, l.nodes, l.kernel_name(lib)) for l in p.launches("nchw")] for p in (plan, keep)]
    assert sig[0] == sig[1] and len(sig[0]) == len(m._graph.nodes)
    nbuf = [len({t.data_ptr() for v, t in p.bufs.items()}) for p in (plan, keep)]
    assert nbuf[0] < nbuf[1] and nbuf[1] >= len(m._graph.nodes)
    keep.ingest_nchw(x, _stream())
    keep.run_backbone(_stream())
    lp2 = torch.empty_like(lp)
    m._head(keep, _stream(), lp2, None)
    torch.cuda.synchronize()
    m.set_precision("fp32")
    print(f"{case} {precision}: {len(sig[0])} launches, {nbuf[0]} buffers reused vs {nbuf[1]} kept")
    assert torch.equal(logits, keep.bufs["logits"])
    assert torch.equal(lp, lp2)


# ----------------------------------------------------------------------------- bf16 shipped plan
def _launch_sig(plan):
    from drnmi import _lib
    import plan_audit as A
    lib = _lib.load()
    nodes = plan.packed.graph.nodes
    return [(l.kind, tuple(nodes[i].name for i in l.nodes), A.short_name(l.kernel_name(lib))) for l in plan.launches("u8", True)]


@pytest.mark.parametrize("arch,base", [("drn_d_24", "drn_d_22"), ("drn_d_56", "drn_d_54")])
def test_bf16_shipped_plan_structure(arch, base):
    """The plan segment() ships at 1 x 72 x 2048 (the strip kernels' routing): the launch list of the
    variant with one unit per tail layer plus exactly two launches, layer.7.3 and layer.8.0; the seg
    classifier folded into layer.8.3 (not into layer.8.0, which D-22 / D-54 fold it into); layer.8.0 a
    launch of its own whose output only layer.8.3 reads.  Then one run of it."""
    import plan_audit as A
    from drnmi.drnseg import build
    from drnmi.weights import synth_frames
    n, h, w = 1, 72, 2048
    m = build(arch, 19, seed=7, device=DEV, precision="bf16")
    plan = m.plan(n, h, w)
    sig = _launch_sig(plan)
    ref = _launch_sig(build(base, 19, seed=7, device=DEV, precision="bf16").plan(n, h, w))
    assert plan.fuse and plan.front_fused and plan.labels_path() == "seg2"
    names = {s[2] for s in sig} | {A.short_name("up8_labels_tile_kernel")}
    if arch == "drn_d_24":
        assert names == D22_BF16_KERNELS, names ^ D22_BF16_KERNELS
    assert {s[2] for s in sig} == {s[2] for s in ref}
    extra = [s for s in sig if s[1] in (("layer.7.3",), ("layer.8.0",))]
    assert len(extra) == 2 and len(sig) == len(ref) + 2
    rest = [s for s in sig if s not in extra]
    assert rest[:-1] == ref[:-1]
    assert ref[-1][:2] == ("conv_seg", ("layer.8.0", "seg")) and rest[-1] == ("conv_seg", ("layer.8.3", "seg"), ref[-1][2])
    nodes = plan.packed.graph.nodes
    by = {nd.name: i for i, nd in enumerate(nodes)}
    seg_launch = [l for l in plan.launches("u8", True) if l.kind == "conv_seg"]
    assert len(seg_launch) == 1 and seg_launch[0].nodes == (by["layer.8.3"], by["seg"])
    assert plan.seg_fused["conv"] == by["layer.8.3"]
    l80 = [l for l in plan.launches("u8", True) if by["layer.8.0"] in l.nodes]
    assert len(l80) == 1 and l80[0].kind == "conv" and l80[0].nodes == (by["layer.8.0"],)
    v = nodes[by["layer.8.0"]].dst
    assert l80[0].writes == (v,) and l80[0].reads == (nodes[by["layer.7.3"]].dst,)
    readers = [nd.name for nd in nodes if v in (nd.src, nd.res)]
    assert readers == ["layer.8.3"] and seg_launch[0].reads == (v,)
    # one run: the rows issued are the list's, then the head; labels agree with the NCHW bf16 path
    frames_np = synth_frames(7, n, h, w)
    frames = torch.from_numpy(frames_np).to(DEV)
    rows = []
    m.timing_hook = lambda i, nd, before: rows.append(i) if before else None
    try:
        lab = m.segment(frames)
    finally:
        m.timing_hook = None
    assert rows == [l.row for l in plan.launches("u8", True)] + [len(nodes)]
    pred = m.predict(O.preprocess_u8(frames_np).to(DEV))
    agree = (lab.long() == pred).float().mean().item()
    print(f"{arch} bf16 1x72x2048: {len(sig)} launches ({base}: {len(ref)}), segment vs predict agreement {agree:.4f}")
    assert len(lab.unique()) > 1 and agree >= 0.99


# 1 - 2 x (1 - measured agreement with the reference labels), rounded down to 3 decimals: a regression
# that doubles the mismatch rate fails (the rule of test_gpu_forward.test_bf16_forward_agreement)
BF16_AGREE = {
    "d24_2x72x136": 0.998,      # measured 0.9993 of 19584 px (logit relative error 7.3e-3)
    "d40_1x64x128": 0.982,      # measured 0.99133 (8121 of 8192 px; 1.27e-2)
    "d56_1x64x128": 0.980,      # measured 0.99048 (8114 of 8192 px; 9.7e-3)
    "d105_1x32x64": 0.974,      # measured 0.98730 (2022 of 2048 px; 9.3e-3): below the 0.98 floor, which then is the gate
    "d107_1x32x64": 0.983,      # measured 0.99170 (2031 of 2048 px; 1.12e-2)
}


@pytest.mark.parametrize("case", list(CASES))
def test_bf16_forward_agreement(case):
    """bf16 network against the reference golden (never another drnmi precision)."""
    g = golden()
    m = model(case).set_precision("bf16")
    x = torch.from_numpy(g[case + "/input"]).to(DEV)
    lp, logits = m(x)
    m.set_precision("fp32")
    ref_logits = g[case + "/logits"]
    rel = np.abs(logits.cpu().numpy() - ref_logits).max() / np.abs(ref_logits).max()
    agree = (torch.max(lp, 1)[1].cpu().numpy() == g[case + "/labels"]).mean()
    print(f"{case} bf16: logit rel err {rel:.3e}, argmax agreement {agree:.4f}")
    assert rel <= 0.03
    assert agree >= 0.98                     # the bf16 floor
    assert agree >= BF16_AGREE[case]


@pytest.mark.parametrize("case", ["d24_2x72x136", "d107_1x32x64"])
def test_bf16_segment_matches_bf16_forward_labels(case):
    """bf16 video path (uint8 frames, fused front) against bf16 predict() on the preprocessed input."""
    g = golden()
    m = model(case).set_precision("bf16")
    frames = torch.from_numpy(g[case + "/frames"]).to(DEV)
    x = torch.from_numpy(g[case + "/input"]).to(DEV)
    lab_seg = m.segment(frames).long()
    lab_fwd = m.predict(x)
    front = m.plan(*frames.shape[:3]).front_fused
    m.set_precision("fp32")
    agree = (lab_seg == lab_fwd).float().mean().item()
    agree_ref = (lab_seg.cpu() == torch.from_numpy(g[case + "/labels"]).long()).float().mean().item()
    print(f"{case} bf16 segment vs predict agreement {agree:.4f}, vs reference {agree_ref:.4f}")
    assert front
    assert agree >= 0.99


# ----------------------------------------------------------------------------- 8-bit
@pytest.mark.parametrize("case", ["d24_2x72x136", "d107_1x32x64"])
def test_int8_network_every_launch_exact(case):
    """test_gpu_int8.test_int8_network_every_launch_exact on the two-conv tail and at 111 nodes,
    calibrated on the case's frames: every boundary quantisation and every int8 conv from its own HBM
    inputs, bit for bit; the whole tail among them, with int8 values in between."""
    from drnmi import _lib as L
    m, frames = _int8_net(golden(), CASES[case], case)
    names, copies, sat = check_int8_every_launch(m, frames, acc_via_f64=True)
    pk = m.plan(*frames.shape[:3], keep_all=True).packed
    print(f"{case} int8: launches checked {len(names)} of {len(pk.graph.nodes)} nodes, boundary copies {len(copies)}, "
          f"max saturated fraction {sat:.4f}")
    assert set(TAIL) | {"seg"} <= set(names) and copies
    assert names == m.qat_layers()[0]                  # every W8A8 launch of the layout decision (17 / 96)
    by = {nd.name: nd for nd in pk.graph.nodes}
    for a, b in zip(TAIL, TAIL[1:] + ("seg",)):
        assert by[b].x_val == by[a].dst and pk.value_code(by[a].dst) == L.DRNMI_I8, (a, b)
    lab = m.segment(frames).cpu().numpy()          # the shipped (buffer-reusing) int8 plan runs too
    print(f"{case} int8: label agreement with the reference fp32 forward {float((lab == golden()[case + '/labels']).mean()):.4f}")
    assert len(np.unique(lab)) > 1


# ----------------------------------------------------------------------------- 2:4 on the two-conv tail
_SP = {}


def _masked_d24(tmp_path_factory):
    """D-24 (the d24 case's weights) with NMPruner 2:4 magnitude masks on every conv with cin >= 64, and
    int8 scales calibrated on the case's frames after the masks."""
    if "m" not in _SP:
        from drnmi import pruners as P
        from drnmi.drnseg import build
        g = golden()
        case = "d24_2x72x136"
        m = build("drn_d_24", 19, seed=int(g[case + "/meta"][0]), device=DEV)
        layers = [nd.name + ".weight" for nd in m._graph.nodes if nd.conv.in_channels >= 64]
        cfg = tmp_path_factory.mktemp("sp24_d24") / "nm.json"
        cfg.write_text(json.dumps({"pruner_type": "nm", "configs": [{"layer_set": layers, "n": 2, "m": 4}]}))
        pr = P.make_pruner(str(cfg))
        pr.generate_masks(m)
        pr.apply_masks(m)
        frames = torch.from_numpy(g[case + "/frames"]).to(DEV)
        m.calibrate_int8(frames)
        _SP.update(m=m, frames=frames)
    return _SP["m"], _SP["frames"]


def test_sparse24_bf16_two_conv_tail(tmp_path_factory):
    """bf16 set_sparse24 on a 2:4-masked D-24: all four tail convs run sparse (a sparse layer.8.3 keeps
    the seg conv a launch of its own), and the labels agree with the dense run of the same masked
    weights under test_gpu_sp24's gate (0.990)."""
    from drnmi import _lib
    m, frames = _masked_d24(tmp_path_factory)
    n, h, w = frames.shape[:3]
    try:
        ref = m.set_precision("fp32").segment(frames).cpu()
        dense = m.set_precision("bf16").segment(frames).cpu()
        m.set_sparse24(True)
        sparse = m.sparse24_layers()
        assert set(TAIL) <= set(sparse), sparse
        got = m.segment(frames).cpu()
        plan = m.plan(n, h, w)
        lib = _lib.load()
        nodes = plan.packed.graph.nodes
        sp = {nodes[l.row].name for l in plan.launches("u8", True) if "sp24" in l.kernel_name(lib)}
        assert sp == set(sparse) and plan.seg_fused is None       # a sparse layer.8.3: the seg conv is its own launch
        agree = (got == dense).float().mean().item()
        print(f"2:4 D-24 2x72x136 bf16: {len(sparse)} sparse launches; sparse vs dense bf16 {agree:.4f}, sparse vs fp32 "
              f"{(got == ref).float().mean().item():.4f}, dense bf16 vs fp32 {(dense == ref).float().mean().item():.4f}")
        assert len(got.unique()) > 1
        assert agree >= 0.990
    finally:
        m.set_sparse24(False).set_precision("fp32")


def test_sparse24_int8_two_conv_tail(tmp_path_factory):
    """int8 set_sparse24 on the same model: int32 sums are exact, so the labels equal the dense int8
    ones bit for bit; both layer7 convs run sparse and neither layer8 conv.

    What the code decides for layer.8.0: engine.SP24_I8_SHAPES lists launch shapes, and leaves out the
    512 -> 512 dilation-1 shape because in D-22 that launch is the seg-fused producer.  In D-24
    layer.8.0 has that shape without being the producer (layer.8.3 is), so it stays dense by shape,
    not for the reason given there: the seg-fused launch (layer.8.3's, at the strip shapes:
    tests/plan_audit.py d24_int8_1x72x2048) is kept either way, the labels are the same
    bits either way (asserted with SP24_I8_EVERY, which routes both layer8 convs and the seg conv
    sparse), and the only thing left on the table is that one launch's possible gain -- right for
    correctness, unmeasured for speed."""
    from drnmi import engine
    m, frames = _masked_d24(tmp_path_factory)
    n, h, w = frames.shape[:3]
    try:
        dense = m.set_precision("int8").segment(frames).cpu()
        m.set_sparse24(True)
        sparse = m.sparse24_layers()
        assert {"layer.7.0", "layer.7.3"} <= set(sparse) and not {"layer.8.0", "layer.8.3", "seg"} & set(sparse), sparse
        got = m.segment(frames).cpu()
        assert torch.equal(got, dense) and len(got.unique()) > 1
        engine.SP24_I8_EVERY = True
        try:
            m.set_sparse24(True)                      # (re-packs with the switch on)
            every = m.sparse24_layers()
            assert set(TAIL) | {"seg"} <= set(every), every
            assert torch.equal(m.segment(frames).cpu(), dense)
        finally:
            engine.SP24_I8_EVERY = False
    finally:
        m.set_sparse24(False).set_precision("fp32")


# ----------------------------------------------------------------------------- graph capture
def test_bf16_segment_graph_capture_d107():
    """torch.ops.drnmi.segment of D-107 (105 launches in the shipped bf16 plan) captured into a graph:
    replays on new frames equal the eager labels (default queue settings)."""
    from drnmi.drnseg import INFO_MEAN, INFO_STD
    from drnmi.weights import synth_frames
    case = "d107_1x32x64"
    m = model(case).set_precision("bf16")
    frames = torch.from_numpy(golden()[case + "/frames"]).to(DEV).clone()
    mean, std = [float(v) for v in INFO_MEAN], [float(v) for v in INFO_STD]

    def step():
        return torch.ops.drnmi.segment(frames, m._handle, mean, std, False)

    try:
        s = torch.cuda.Stream()                  # warm-up off the capture: packing, plan buffers, attributes
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                step()
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = step()
        for seed in (4, 11):
            frames.copy_(torch.from_numpy(synth_frames(seed, 1, 32, 64)).to(DEV))
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(captured, step())
        assert len(captured.unique()) > 1
    finally:
        m.set_precision("fp32")
