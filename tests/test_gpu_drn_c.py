"""DRN-C on the GPU: the fused 16-channel BasicBlock kernel (drnmi_basic_block16, csrc/block16.hip),
whole-network parity of drn_c_26 / drn_c_42 against the reference goldens (tests/golden/drn_c.N.npz)
and the CPU restatement (tests/drn_c_ref.py), the launch plans, one fine-tune step and a pruner mask.

Gates: fp32 / fp32x logits within 1e-3 max-abs of the reference and identical labels on every pixel
whose reference top-2 margin is > 1e-4 (the fixtures have no pixel at or below it); per-stage taps
within 1e-4 x max(1, |ref|max); bf16 logit relative error <= 0.03 and label agreement >= 0.98, then
tightened to just below the measured agreement; the block kernel within test_block64's two-level
bf16 tolerance of the torch restatement on the same bf16 input."""
from __future__ import annotations

import ctypes
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import drn_c_ref as R
import train_case as TC
from drnmi import _lib
from test_drn_c import CASES, _params, golden, pack16

pytestmark = pytest.mark.gpu
DEV = "cuda"
STRIP = 254          # csrc/block16.hip kOW: output columns per strip
XRING = 5            # its x ring depth
_MODELS = {}


def model(case):
    from drnmi.drnseg import build
    if case not in _MODELS:
        _MODELS[case] = build(CASES[case], 19, seed=int(golden()[case + "/meta"][0]), device=DEV)
    return _MODELS[case]


def reference16(x_nhwc_bf16: torch.Tensor, p) -> torch.Tensor:
    """test_block64.reference at 16 channels: fp32 torch on the bf16 input, BN scale folded into
    bf16 weights, the intermediate rounded to bf16."""
    w1, s1, b1, w2, s2, b2 = p
    x = x_nhwc_bf16.float().permute(0, 3, 1, 2)
    w1f = (w1 * s1.view(-1, 1, 1, 1)).bfloat16().float()
    w2f = (w2 * s2.view(-1, 1, 1, 1)).bfloat16().float()
    t = torch.relu(F.conv2d(x, w1f, padding=1) + b1.view(1, -1, 1, 1)).bfloat16().float()
    y = torch.relu(F.conv2d(t, w2f, padding=1) + b2.view(1, -1, 1, 1) + x)
    return y.permute(0, 2, 3, 1)


def within_block_tolerance(got, ref):
    d = (got - ref).abs()
    scale = ref.abs().max()
    loose = (d > 2.0 ** -8 * ref.abs() + 1e-3 * scale).float().mean()
    return bool((d <= 2.0 ** -6 * ref.abs() + 4e-3 * scale).all()) and float(loose) <= 5e-3, float(d.max()), float(loose)


# one pixel; smaller than a tile; one column past a strip; fewer rows than the x ring with three
# strips; 3 x 3 x 33 = 297 row items over 512 workgroups' ranges (every range boundary inside a frame,
# one row each); 3 x 3 x 201 = 1809 row items: the persistent walk, as the 1024 x 2048 plans run it
@pytest.mark.parametrize("n,h,w", [(1, 1, 1), (1, 5, 9), (2, 3, STRIP + 1), (1, XRING - 2, 2 * STRIP + 3),
                                   (3, 33, 2 * STRIP + 2), (3, 201, 2 * STRIP + 2)])
def test_block16_matches_reference(n, h, w):
    lib = _lib.load()
    if h == 201:
        # the host gives each of 2 x CUs workgroups per_wg = ceil(n * strips * h / (2 CUs)) consecutive
        # row items (csrc/block16.hip drnmi_basic_block16).  Here per_wg > 1 and does not divide h, so
        # ranges start and end inside a strip's rows, run on into the next strip and the next frame, and
        # a workgroup walks several rows and begins a second segment on used rings
        wgs = 2 * torch.cuda.get_device_properties(0).multi_processor_count
        total = n * ((w + STRIP - 1) // STRIP) * h
        per_wg = (total + wgs - 1) // wgs
        assert total > wgs and per_wg > 1 and h % per_wg != 0, (total, wgs, per_wg)
    p = _params(n + h + w)
    blob = torch.from_numpy(pack16(lib, p)).to(DEV)
    g = torch.Generator().manual_seed(w)
    x = torch.relu(torch.randn(n, h, w, 16, generator=g)).bfloat16()
    xd = x.to(DEV)
    y = torch.full_like(xd, float("nan"))
    _lib.check(lib.drnmi_basic_block16(xd.data_ptr(), blob.data_ptr(), y.data_ptr(), n, h, w,
                                       ctypes.c_void_p(_lib.stream_ptr())), "basic_block16")
    torch.cuda.synchronize()
    got = y.float().cpu()
    assert not torch.isnan(got).any()
    ok, dmax, loose = within_block_tolerance(got, reference16(x, p))
    print(f"block16 {n}x{h}x{w}: max |d| {dmax:.3e}, beyond the tight level {loose:.2e}")
    assert ok, (dmax, loose)


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
    margin = g[case + "/top2_margin"]
    sure = margin > 1e-4
    diff = int((labels != g[case + "/labels"])[sure].sum())
    print(f"{case} {precision}: logit max-abs {err:.2e}, log-prob max-abs {lperr:.2e}, labels differ {diff} px "
          f"({int((~sure).sum())} px with margin <= 1e-4)")
    assert (~sure).sum() <= 1e-4 * margin.size
    assert err <= 1e-3 and lperr <= 1e-3
    assert diff == 0


@pytest.mark.parametrize("case", list(CASES))
def test_fp32_stages_match_restatement(case):
    g = golden()
    m = model(case).set_precision("fp32")
    x = torch.from_numpy(g[case + "/input"])
    plan = m.plan(x.shape[0], x.shape[2], x.shape[3], keep_all=True)
    plan.ingest_nchw(x.to(DEV), _lib.stream_ptr())
    plan.run_backbone(_lib.stream_ptr())
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    _, _, stages = R.drnseg_forward(sd, CASES[case], x)
    assert list(m._graph.stage_outputs) == [f"layer{i}" for i in range(9)]
    for name, val in m._graph.stage_outputs.items():
        ref = stages[name]
        err = (plan.stage_nchw(val).cpu() - ref).abs().max().item()
        assert err <= 1e-4 * max(1.0, ref.abs().max().item()), f"{name}: {err}"


def test_fp32_torch_up_head():
    """DRNSeg(use_torch_up=True) on an arch-C trunk: the bilinear head against the restatement."""
    from drnmi.drnseg import DRNSeg
    from drnmi.weights import synth_state_dict
    g = golden()
    m = DRNSeg("drn_c_26", 19, pretrained=False, use_torch_up=True)
    m.load_state_dict(synth_state_dict(m, 6))
    m = m.to(DEV).eval()
    x = torch.from_numpy(g["c26_2x72x136/input"])
    lp, logits = m(x.to(DEV))
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    assert "up.weight" not in sd
    ref_lp, ref_logits, _ = R.drnseg_forward(sd, "drn_c_26", x)
    assert (logits.cpu() - ref_logits).abs().max().item() <= 1e-3
    assert (lp.cpu() - ref_lp).abs().max().item() <= 1e-3


# just below the measured agreement with the reference labels (MI355X: 1.0000 of 19584 px on c26,
# 0.9999 of 8192 px on c42; logit relative error 4.7e-3 / 9.0e-3)
BF16_AGREE = {"c26_2x72x136": 0.9995, "c42_1x64x128": 0.999}


@pytest.mark.parametrize("case", list(BF16_AGREE))
def test_bf16_forward_agreement(case):
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
    assert agree >= BF16_AGREE[case]         # just below the measured agreement


def _layer1_tap(m, x):
    """The layer1 stage of a fused (not keep_all) bf16 forward, copied out right after the launch
    that produces it (its buffer is reused later in the step)."""
    plan = m.plan(x.shape[0], x.shape[2], x.shape[3])
    val = m._graph.stage_outputs["layer1"]
    idx = [i for i, nd in enumerate(plan.packed.graph.nodes) if nd.dst == val][0]
    out, seen = {}, []

    def hook(i, nd, before):
        seen.append((i, before))
        if i == idx and not before:
            out["v"] = plan.stage_nchw(val)
    plan.ingest_nchw(x.to(DEV), _lib.stream_ptr())
    plan.run_backbone(_lib.stream_ptr(), hook)
    torch.cuda.synchronize()
    return plan, out["v"].cpu(), seen


def test_plans_and_fused_layer1(monkeypatch):
    from drnmi import engine
    from drnmi.drnseg import build
    g = golden()
    case = "c26_2x72x136"
    x = torch.from_numpy(g[case + "/input"])
    m = build("drn_c_26", 19, seed=6, device=DEV).set_precision("bf16")
    plan, fused, seen = _layer1_tap(m, x)
    names = [nd.name for nd in plan.packed.graph.nodes]
    i1 = names.index("layer.3.0.conv1")
    assert list(plan.block16) == [i1] and names[i1 + 1] == "layer.3.0.conv2"
    assert not plan.stem_fused and not plan.front_fused
    # one launch for the pair, reported under the second conv's index
    assert (i1, True) not in seen and (i1 + 1, True) in seen and (i1 + 1, False) in seen
    # a keep_all plan keeps the two launches
    assert not m.plan(2, 72, 136, keep_all=True).block16
    monkeypatch.setattr(engine, "FUSE_BLOCK16", False)
    m2 = build("drn_c_26", 19, seed=6, device=DEV).set_precision("bf16")
    plan2, unfused, seen2 = _layer1_tap(m2, x)
    assert not plan2.block16 and (i1, True) in seen2
    ok, dmax, loose = within_block_tolerance(fused, unfused)
    print(f"layer1 fused vs two launches: max |d| {dmax:.3e}, beyond the tight level {loose:.2e}")
    assert ok, (dmax, loose)
    assert fused.abs().max() > 0


def test_segment_paths():
    g = golden()
    case = "c26_2x72x136"
    m = model(case)
    frames = torch.from_numpy(g[case + "/frames"]).to(DEV)
    x = torch.from_numpy(g[case + "/input"]).to(DEV)
    ref = torch.from_numpy(g[case + "/labels"]).long()
    for precision in ("fp32", "fp32x"):
        m.set_precision(precision)
        lab_pred = m.predict(x).cpu()
        lab_seg = m.segment(frames).cpu()
        assert lab_seg.dtype == torch.uint8 and lab_seg.shape == (2, 72, 136)
        assert torch.equal(lab_pred, lab_seg.long()), precision
        assert torch.equal(lab_pred, ref), precision
    m.set_precision("bf16")
    lab_seg = m.segment(frames).long()
    lab_fwd = m.predict(x)
    agree = (lab_seg == lab_fwd).float().mean().item()
    agree_ref = (lab_seg.cpu() == ref).float().mean().item()
    print(f"bf16 segment vs predict agreement {agree:.4f}, vs reference {agree_ref:.4f}")
    m.set_precision("fp32")
    assert agree >= 0.99                                 # measured 0.9999 (and 0.9999 against the reference)


def test_bf16_segment_graph_capture():
    from drnmi.drnseg import INFO_MEAN, INFO_STD
    from drnmi.weights import synth_frames
    m = model("c26_2x72x136").set_precision("bf16")
    frames = torch.from_numpy(synth_frames(106, 2, 72, 136)).to(DEV)
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
        assert m.plan(2, 72, 136).block16
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = step()
        for seed in (4, 11):
            frames.copy_(torch.from_numpy(synth_frames(seed, 2, 72, 136)).to(DEV))
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(captured, step())
        assert len(captured.unique()) > 1
    finally:
        m.set_precision("fp32")


@pytest.mark.parametrize("precision", ["fp32", "fp32x"])
def test_train_step_matches_fp64(precision):
    """One fine-tune step of drn_c_26 at 1x3x64x64 against the fp64 restatement: loss within 1e-4
    relative, every gradient's rel-L2 <= 1e-3, parameters after the step rtol 1e-4 / atol 1e-6."""
    from drnmi.drnseg import DRNSeg
    from drnmi.train import SGD, CrossEntropyLoss
    from drnmi.weights import synth_state_dict
    seed = 8
    torch.manual_seed(seed)
    m = DRNSeg("drn_c_26", 19, pretrained=False)
    m.load_state_dict(synth_state_dict(m, seed))
    x = torch.randn(1, 3, 64, 64)
    t = torch.randint(0, 19, (1, 64, 64))
    t[torch.rand(t.shape) < 0.2] = 255
    losses, grads, final = R.drnseg_train_steps(m.state_dict(), "drn_c_26", [x], [t], TC.LR, TC.MOMENTUM, TC.WD,
                                                dtype=torch.float64)
    m = m.to(DEV).train().set_precision(precision)
    crit = CrossEntropyLoss(ignore_index=255)
    opt = SGD(m.optim_parameters(), TC.LR, momentum=TC.MOMENTUM, weight_decay=TC.WD)
    loss = crit(m(x.to(DEV))[0], t.to(DEV))
    opt.zero_grad()
    loss.backward()
    got = {k: p.grad.detach().double().cpu().numpy() for k, p in m.named_parameters() if not k.startswith("up.")}
    opt.step()
    torch.cuda.synchronize()
    print(f"drn_c_26 {precision}: loss {float(loss.detach()):.6f} vs fp64 {losses[0]:.6f}")
    assert abs(float(loss.detach()) - losses[0]) <= 1e-4 * abs(losses[0])
    assert set(got) == set(grads)
    worst = ("", 0.0)
    for k, gk in got.items():
        e = TC.rel_l2(gk, grads[k].numpy())
        worst = max(worst, (k, e), key=lambda kv: kv[1])
    print(f"drn_c_26 {precision}: worst grad rel-L2 vs fp64 {worst[1]:.2e} ({worst[0]})")
    for k, gk in got.items():
        assert TC.rel_l2(gk, grads[k].numpy()) <= 1e-3, k
    sd = m.state_dict()
    for k, p in m.named_parameters():
        if not k.startswith("up."):
            np.testing.assert_allclose(p.detach().cpu().numpy(), final[k].numpy(), rtol=1e-4, atol=1e-6, err_msg=k)
    for k in ("layer.1.running_mean", "layer.1.running_var", "layer.3.0.bn2.running_var"):
        np.testing.assert_allclose(sd[k].cpu().numpy(), final[k].numpy(), rtol=1e-4, atol=1e-6, err_msg=k)


def test_block16_repack_after_mask_apply(tmp_path):
    """A BlockPruner mask on layer.3.0.conv2.weight, applied in place, must reach the fused block's
    packed weights: the next bf16 forward matches the restatement on the masked weights."""
    from drnmi import pruners as P
    from drnmi.drnseg import build
    g = golden()
    case = "c26_2x72x136"
    x = torch.from_numpy(g[case + "/input"])
    m = build("drn_c_26", 19, seed=6, device=DEV).set_precision("bf16")
    plan, before, _ = _layer1_tap(m, x)
    assert plan.block16
    cfg = {"pruner_type": "block", "configs": [{"layer_set": ["layer.3.0.conv2.weight"], "sparsity": 0.75,
           "block_height": 1, "block_width": 1, "sub_rows": -1, "sub_cols": -1, "collapse_tensor": True}]}
    jp = tmp_path / "c.json"
    jp.write_text(json.dumps(cfg))
    pr = P.BlockPruner(str(jp))
    pr.generate_masks(m)
    pr.apply_masks(m)
    w = m.state_dict()["layer.3.0.conv2.weight"]
    assert 0.7 <= float((w == 0).float().mean()) <= 0.8
    plan2, after, _ = _layer1_tap(m, x)                  # (m.plan repacks, as a forward does)
    assert plan2 is plan and plan2.block16
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    _, _, stages = R.drnseg_forward(sd, "drn_c_26", x)
    ref = stages["layer1"]
    # bf16 activations through the stem and the block: the bf16 floor of test_gpu_forward (relative 0.03)
    rel = (after - ref).abs().max().item() / ref.abs().max().item()
    stale = (before - ref).abs().max().item() / ref.abs().max().item()
    print(f"layer1 after the mask: rel err vs restatement {rel:.3e} (stale weights would give {stale:.3e})")
    assert rel <= 0.03
    assert not torch.equal(after, before) and rel < stale    # stale packed weights would leave it unchanged
    _, logits = m(x.to(DEV))
    _, ref_logits, _ = R.drnseg_forward(sd, "drn_c_26", x)
    assert (logits.cpu() - ref_logits).abs().max().item() / ref_logits.abs().max().item() <= 0.03
