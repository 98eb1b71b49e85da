"""Every launch of one fine-tune step against float64 (tests/train_audit.py), and kernel-level
cases at the plan classes the fine-tune benchmark runs.

The end-to-end gates of tests/test_gpu_train.py accept a gradient rel-L2 of 1e-3 .. 2e-2 and run
shapes whose weight gradients take 1 .. 8 pixel splits; bench_finetune.py (D-54, 2 x 1024 x 768)
runs 32+ splits, the grouped reduce and conv_x6 with split-K 1, 2 and 4.  Here
  * the step's launches are recorded and each is re-computed in float64 from its own GPU inputs
    (gate: |got - ref| <= 2^-22 |ref| + a + b, train_audit.py), no element excluded;
  * the CPU tests (no gpu mark) prove the audit on synthetic records: the rounded float64 value
    passes, a missing 32-pixel chunk / border tap / accumulate, a wrong parity, an invstd 8 ulps off
    and a 4-ulp error each fail;
  * a CPU test walks D-22 and D-54 at the benchmark shape through the library's host-only plan
    queries and asserts that the kernel-level GPU cases below reach every route class found.
"""
from __future__ import annotations

import ctypes

import pytest
import torch
import torch.nn.functional as F

import train_audit as A

F64 = torch.float64
DEV = "cuda"
BENCH_SHAPE = (2, 1024, 768)        # bench_finetune.py: 2 crops of 1024 x 768


def _report(tag, figs):
    bad = A.failures(figs)
    for f in figs:
        print(f"{tag}: {f}{'  FAILED' if f in bad else ''}")
    return bad


# ----------------------------------------------------------------------------- GPU: the audit
@pytest.mark.gpu
@pytest.mark.parametrize("group", A.GROUPS)
@pytest.mark.parametrize("cfg", list(A.CONFIGS))
def test_train_launches_match_reference(cfg, group):
    """Every launch of `group` in one recorded step of `cfg`, from its own inputs.  a, b and the
    worst excess over the gate (<= 0 passes) of every compared output are printed before the verdict.

    This audit found the exact-fp32 igemm summing K >= 1024 in one fp32 chain at 5 .. 10 x torch's
    fp32 error (D-54 layer.7.0 forward, K 4608: a 1.77e-5, excess 2.69e-5); training launches now
    fold the chain every 256 k (csrc/conv_igemm.hip, profiles/train_audit/README.txt).

    Regression note (d24_fp32_1x72x40 / layer3): with the fold starting at K = 1024, the stride-1 data
    gradient of layer.3.0.conv2 (conv_igemm_kernel<f32, 128, 64, 2, 2, 3>, K = 576: one fp32 chain)
    missed the gate on one of 11520 elements: |got - ref| 2.48e-8 at |ref| 0.0233, a 1.89e-8 (the
    kernel at 5.3 x torch's fp32 error where a allows 4), excess 3.76e-10.  Training launches of
    K = 512 .. 1023 now fold every 128 k."""
    recs = A.launches(cfg, group)
    assert recs, f"no launch of {group} captured"
    cap = A.capture(cfg)
    failed = []
    for rec in recs:
        tag = f"{cfg} #{rec.index} pass {rec.step} {rec.kind} {rec.name} [{A.launch_label(rec)}]"
        if _report(tag, A.check(cap, rec)):
            failed.append((rec.index, rec.kind, rec.name))
    assert not failed, failed


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", list(A.CONFIGS))
def test_train_launches_all_audited(cfg):
    """Every record is of exactly one checked kind in one audited group; every node has its forward,
    BN, wgrad and (input node excepted) dgrad records in every pass; the parity-class launches of
    a node cover its whole destination; and the routes the runner took are the ones the host-only
    walk (train_audit.step_routes, which the class-coverage test relies on) predicts."""
    cap = A.capture(cfg)
    arch, precision, shape, passes = A.CONFIGS[cfg]
    assert [r.index for r in cap.recs] == list(range(len(cap.recs)))
    assert sum(len(A.launches(cfg, g)) for g in A.GROUPS) == len(cap.recs)
    assert {r.group for r in cap.recs} == set(A.GROUPS)
    for r in cap.recs:
        assert (r.kind in A.CHECKS) != (r.kind in A.HEAD_CHECKS), r.kind
        assert (r.name is None) == (r.kind in A.HEAD_CHECKS), (r.kind, r.name)
    for step in range(passes):
        kinds = {}
        for r in cap.recs:
            if r.step == step:
                kinds.setdefault(r.name, []).append(r)
        for k in A.HEAD_KINDS:
            assert sum(r.kind == k for r in kinds[None]) == 1, k
        for name in cap.order:
            m = cap.meta[name]
            have = [r.kind for r in kinds[name]]
            want = ["conv", "seg_nhwc", "bias_grad", "wgrad"] if m.seg else ["conv", "bn_stats", "bn_act", "bn_bwd", "wgrad"]
            for k in want:
                assert have.count(k) == 1, (name, k, have)
            dg = [r for r in kinds[name] if r.kind == "dgrad"]
            assert bool(dg) == (m.src != "input"), name
            assert len(have) == len(want) + len(dg), (name, have)
            cls = [r for r in dg if r.data["form"] == "class"]
            if cls:
                assert len(cls) == len(dg) and len({tuple(r.data["cls"]) for r in cls}) == len(cls), name
                owned = torch.zeros(m.ih, m.iw, dtype=torch.bool)
                for r in cls:
                    owned[r.data["cls"][0]::2, r.data["cls"][1]::2] = True
                assert cls[0].data["fill"] != "empty" or bool(owned.all()), name
            else:
                assert len(dg) <= 1, name
        assert A.recorded_routes(cap, step) == A.step_routes(arch, precision, shape[0], shape[2], shape[3])
    names = sorted({A.launch_label(r).split(" x")[0].split(" split-K")[0] for r in cap.recs})
    print(f"{cfg}: {len(cap.recs)} records, kernels {names}")
    if precision == "fp32x":
        forms = {r.data["form"] for r in cap.recs if r.kind == "dgrad"}
        assert "class" in forms and "s1" in forms, forms
        if arch == "drn_d_54":       # 1x1 stride-2 downsamples: classes no tap reaches stay zero-filled
            assert any(r.data["fill"] == "zeros" for r in cap.recs if r.kind == "dgrad")
    # a residual's other consumers come earlier in the graph, so in these networks the BN backward
    # always finds dres unset (test_bn_bwd_dres_accumulates covers dres_accumulate = 1); the
    # block's first conv and its downsample then accumulate onto it through the dgrad launches
    assert not any(r.kind == "bn_bwd" and r.data["dres_before"] is not None for r in cap.recs)
    assert any(r.kind == "bn_bwd" and r.data["dres"] is not None for r in cap.recs)
    assert any(r.kind == "dgrad" and r.data["fill"] == "prev" for r in cap.recs)


@pytest.mark.gpu
def test_accumulated_grads_equal_sum_of_references():
    """backward twice without zero_grad: every parameter's gradient is the sum of the two passes'
    float64 references (the accumulate = 1 paths of wgrad, dgamma / dbeta and the seg bias); the
    gate's a and b are the sums of the two launches' own."""
    cfg = "d22_fp32x_2x64x64_acc"
    cap = A.capture(cfg)
    by = {}
    for r in cap.recs:
        if r.kind in ("wgrad", "bn_bwd", "bias_grad"):
            by.setdefault((r.name, r.kind), []).append(r)
    failed = []
    checked = set()
    for (name, kind), rs in by.items():
        assert [r.step for r in rs] == [0, 1], (name, kind)
        m = cap.meta[name]
        if kind == "wgrad":
            assert rs[0].data["before"] is None and rs[1].data["before"] is not None
            t = [A.wgrad_terms(m, r.data) for r in rs]
            b = t[0][2] + t[1][2] if t[0][2] is not None else None
            outs = {"weight": (t[0][0] + t[1][0], t[0][1] + t[1][1], b)}
        elif kind == "bias_grad":
            v = [[r.data["dy"].reshape(m.n * m.oh * m.ow, -1)[:, :m.cout].to(dt).sum(0) for r in rs]
                 for dt in (F64, torch.float32)]
            outs = {"bias": (v[0][0] + v[0][1], v[1][0] + v[1][1], None)}
        else:
            rows = m.n * m.oh * m.ow
            sh = lambda q: q.reshape(rows, -1)
            t = [[A.bn_bwd_ref(sh(r.data["dz"]), sh(r.data["z"]), sh(r.data["y"]), r.data["mean"], r.data["invstd"],
                               m.gamma, m.relu, dt) for r in rs] for dt in (F64, torch.float32)]
            outs = {"gamma": (t[0][0][1] + t[0][1][1], t[1][0][1] + t[1][1][1], None),
                    "beta": (t[0][0][2] + t[0][1][2], t[1][0][2] + t[1][1][2], None)}
        for which, (r64, r32, b) in outs.items():
            key = m.keys[which]
            checked.add(key)
            a = 4.0 * float((r32.to(F64) - r64).abs().max())
            if _report(f"{cfg} {key}", [A.gate("grad after two passes", cap.params[key], r64, None, b, a=a)]):
                failed.append(key)
    assert checked == set(cap.params), set(cap.params) ^ checked
    assert not failed, failed


@pytest.mark.gpu
@pytest.mark.parametrize("rows,C", [(2 * 9 * 5, 64), (3001, 16)])
def test_bn_bwd_dres_accumulates(rows, C):
    """drnmi_bn_act_bwd_f32 with dres_accumulate = 1 and grad_accumulate = 1 (a residual value that
    already holds a gradient; the fine-tune graphs never present one), against float64."""
    from drnmi import _lib
    lib = _lib.load()
    sp = ctypes.c_void_p(_lib.stream_ptr())
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    m, g = _node(rows + C, 1, C, C, 1, 1, 0, 1, rows, 1, relu=True, res="r")
    y = torch.randn(rows, C, generator=g) * 2 + 0.3
    mean, invstd, _, _ = A.bn_stats_ref(y, [torch.zeros(C), torch.ones(C)], m.eps, m.momentum, F64)
    mean, invstd = mean.float(), invstd.float()
    res = torch.randn(rows, C, generator=g)
    z = A.bn_act_ref(y, mean, invstd, m.gamma, m.beta, res, True, torch.float32)
    dz, dres0 = torch.randn(rows, C, generator=g), torch.randn(rows, C, generator=g)
    dg0, db0 = torch.randn(C, generator=g), torch.randn(C, generator=g)
    d = lambda t: t.to(DEV).contiguous()
    dzd, dresd, dgd, dbd = d(dz), d(dres0), d(dg0), d(db0)
    keep = [d(t) for t in (z, y, mean, invstd, m.gamma)]
    ws = torch.empty(lib.drnmi_reduce_workspace_bytes(rows, C), dtype=torch.uint8, device=DEV)
    _lib.check(lib.drnmi_bn_act_bwd_f32(vp(dzd), *[vp(t) for t in keep], 1, rows, C, vp(dzd), vp(dresd), 1, vp(dgd),
                                        vp(dbd), 1, vp(ws), sp), "bn_act_bwd")
    torch.cuda.synchronize()
    rec = {"dz": dz, "z": z, "y": y, "mean": mean, "invstd": invstd, "dy": dzd.cpu(), "dres": dresd.cpu(),
           "dres_before": dres0, "dgamma": dgd.cpu(), "dbeta": dbd.cpu(), "dgamma_before": dg0, "dbeta_before": db0,
           "from_y": False}
    m.oh, m.ow, m.n = rows, 1, 1
    assert not _report(f"bn_act_bwd {rows} x {C}", A.check_bn_bwd(m, rec))


# ----------------------------------------------------------------------------- kernel-level plan classes
# (cin, cin_stride, cout, dy_stride, ks, stride, pad, dil, n, h, w, x6): the smallest pixel counts at
# which drnmi_conv_wgrad_plan gives each class of the benchmark's launches (found by a host-side
# search over the query), plus their M % 32 != 0 twins; >= 32 splits need M > 31 * 512
WGRAD_PLAN_CASES = [
    (32, 32, 19, 32, 1, 1, 0, 1, 1, 9, 64, False),          # f32, 2 splits
    (64, 64, 64, 64, 3, 1, 2, 2, 1, 21, 32, False),         # f32, ragged last split
    (64, 64, 64, 64, 3, 1, 2, 2, 1, 15, 35, False),         # ... and M % 32 != 0
    (32, 32, 19, 32, 1, 1, 0, 1, 1, 132, 128, False),       # f32, 33 splits, grouped reduce
    (64, 64, 64, 64, 3, 1, 1, 1, 1, 126, 128, False),       # f32, 32 splits, ragged, grouped reduce
    (32, 32, 64, 64, 3, 1, 1, 1, 2, 84, 95, False),         # ... and M % 32 != 0
    (64, 64, 64, 64, 3, 1, 1, 1, 2, 96, 120, True),         # split-bf16 64-tile, >= 32 splits
    (128, 128, 128, 128, 1, 1, 0, 1, 1, 9, 64, True),       # big, 2 splits
    (64, 64, 128, 128, 3, 1, 1, 1, 1, 132, 128, True),      # big, >= 32 splits, grouped reduce
    (16, 16, 16, 16, 3, 1, 1, 1, 1, 16, 64, True),          # direct, 32 wave splits, grouped reduce
    (128, 128, 128, 128, 3, 1, 1, 1, 1, 9, 64, True),       # pre, 2 splits
    (128, 128, 128, 128, 3, 1, 1, 1, 1, 21, 32, True),      # pre, ragged last split
    (128, 128, 128, 128, 3, 1, 2, 2, 1, 15, 35, True),      # ... and M % 32 != 0 (Mp padding of the dy planes)
    (128, 128, 128, 128, 3, 1, 1, 1, 2, 96, 90, True),      # pre, >= 32 splits, grouped reduce
    (128, 128, 128, 128, 3, 1, 1, 1, 1, 132, 128, True),    # ... whole splits
    (256, 256, 256, 256, 3, 1, 2, 2, 2, 96, 85, True),      # pre, 32 ragged splits, cout K > 2^19: plain reduce
]
# (n, h, w, cin, cout, ks, pad, dil, res, kernel, split-K): conv_x6 forward / stride-1 dgrad launches
# with the tile forced to the variant of that name and split count (tile id v + 6 S); >= 3 pixel tiles
X6_PLAN_CASES = [
    (2, 11, 13, 256, 256, 3, 2, 2, True, "conv_x6_kernel<3, 128, 2, 4>", 1),
    (2, 11, 13, 256, 256, 3, 2, 2, False, "conv_x6_kernel<3, 128, 2, 4>", 2),
    (1, 20, 19, 256, 256, 3, 4, 4, True, "conv_x6_kernel<3, 128, 2, 4>", 4),
    (1, 17, 19, 256, 512, 1, 0, 1, True, "conv_x6_kernel<1, 128, 2, 4>", 1),
    (1, 17, 19, 512, 256, 1, 0, 1, False, "conv_x6_kernel<1, 128, 2, 4>", 2),
    (1, 17, 19, 64, 128, 1, 0, 1, False, "conv_x6_kernel<1, 64, 2, 2>", 1),
    (2, 13, 11, 256, 128, 1, 0, 1, True, "conv_x6_kernel<1, 64, 2, 2>", 2),
    (2, 13, 11, 128, 128, 3, 1, 1, True, "conv_x6_kernel<3, 64, 2, 2>", 2),
    (1, 17, 19, 64, 64, 3, 1, 1, False, "conv_x6_kernel<3, 32, 2, 2>", 1),
    (1, 17, 19, 256, 64, 1, 0, 1, False, "conv_x6_kernel<1, 32, 2, 2>", 1),
]
# (n, ih, iw, cin, cout, ks, pad): stride-2 convs whose fp32x data gradient runs as parity-class
# launches (ks 2 / 1 kernels, y_sr row stride, asymmetric padding); odd sizes, both tile widths
S2_CLASS_CASES = [
    (2, 17, 15, 32, 64, 3, 1),       # classes of 1x1, 1x2, 2x1 and 2x2 taps -> conv_x6<1|2, 32, 2, 2>
    (1, 18, 21, 128, 256, 3, 1),     # ... -> conv_x6<1|2, 64, 2, 2>
    (2, 17, 15, 64, 128, 1, 0),      # 1x1 downsample: one class, the other three zero-filled
]


def _wgrad_case_class(case):
    from drnmi import _lib
    cin, cs, cout, dys, ks, s, p, d, n, h, w, x6 = case
    a = A.wgrad_args(n, cin, cs, cout, dys, ks, s, p, d, h, w)
    return A.wgrad_class(_lib.wgrad_plan(a, x6), n * a.ho * a.wo)


def _x6_case_args(case, tile=-1):
    from drnmi.engine import COUT_ALIGN, _round_up
    from drnmi import _lib
    n, h, w, cin, cout, ks, pad, dil, res, _, S = case
    ho, wo = h + 2 * pad - dil * (ks - 1), w + 2 * pad - dil * (ks - 1)
    k = ks * ks * cin
    a = A.conv_args(True, _lib.ALGO_IGEMM, n, h, w, cin, ho, wo, cout, _round_up(cout, COUT_ALIGN), ks, 1, pad, dil,
                    k, k, (ho * wo * cout, cout, 1), res=res, tile=tile)
    a.ws, a.ws_bytes = A.PTR, S * n * ho * wo * cout * 4
    return a


def _x6_case_tile(case):
    """The forced tile id v + 6 S whose launch is the case's kernel at its split count."""
    from drnmi import _lib
    lib = _lib.load()
    for v in range(6):
        a = _x6_case_args(case, v + 6 * case[10])
        name = lib.drnmi_conv_kernel_name(ctypes.byref(a))
        if name is not None and name.decode() == case[9]:
            return v + 6 * case[10]
    raise AssertionError(f"no conv_x6 variant gives {case[9]} for {case}")


def _s2_class_plan(ks, pad):
    """[(a, b, taps)] of a dilation-1 stride-2 conv's data-gradient parity classes (TrainRunner._s2_classes)."""
    pad_d = ks - 1 - pad
    parts = []
    for a_ in (0, 1):
        k0 = (pad_d - a_) % 2
        nh = (ks - k0 + 1) // 2 if k0 < ks else 0
        assert not nh or (a_ - pad_d + k0) // 2 == 0
        parts.append(nh)
    return [(a_, b_, max(parts[a_], parts[b_])) for a_ in (0, 1) for b_ in (0, 1) if parts[a_] and parts[b_]], pad_d


def _s2_case_routes(case):
    from drnmi import _lib
    from drnmi.engine import COUT_ALIGN, _conv_out, _round_up
    n, ih, iw, cin, cout, ks, pad = case
    oh, ow = _conv_out(ih, ks, 2, pad, 1), _conv_out(iw, ks, 2, pad, 1)
    out = []
    for (a_, b_, ksc) in _s2_class_plan(ks, pad)[0]:
        a = A.conv_args(True, _lib.ALGO_IGEMM, n, oh, ow, cout, (ih - a_ + 1) // 2, (iw - b_ + 1) // 2, cin,
                        _round_up(cin, COUT_ALIGN), ksc, 1, 0, 1, ksc * ksc * cout, ksc * ksc * cout,
                        (ih * iw * cin, 2 * cin, 1), y_sr=2 * iw * cin)
        out.append(A.conv_route(a, split=False))
    return out


def test_wgrad_plan_query():
    """drnmi_conv_wgrad_plan: the launcher's own decision.  Whole 32-pixel chunks per split, splits
    that cover M with none empty, the grouped reduce exactly at >= 32 splits of <= 2^19 outputs, the
    workspace query sized for the plan, bad geometry refused."""
    from drnmi import _lib
    lib = _lib.load()
    for case in WGRAD_PLAN_CASES:
        cin, cs, cout, dys, ks, s, p, d, n, h, w, x6 = case
        a = A.wgrad_args(n, cin, cs, cout, dys, ks, s, p, d, h, w)
        kernel, splits, per, reduce = _lib.wgrad_plan(a, x6)
        M = n * a.ho * a.wo
        assert (kernel == "wgrad_kernel<64, false>") == (not x6), case
        if kernel != "wgrad_x6_direct_kernel":
            assert per % 32 == 0 and (splits - 1) * per < M <= splits * per, (case, splits, per)
        else:
            assert splits % 4 == 0 and splits <= max(4, (M // 32 + 3) // 4 * 4), (case, splits)
        assert (reduce == "wgrad_reduce_grouped_kernel") == (splits >= 32 and cout * ks * ks * cs <= 2048 * 256), case
        nb = (lib.drnmi_conv_wgrad_workspace_bytes if x6 else lib.drnmi_conv_wgrad_f32_workspace_bytes)(ctypes.byref(a))
        assert nb >= splits * cout * ks * ks * cs * 4, case
    a = A.wgrad_args(1, 32, 32, 19, 32, 1, 1, 0, 1, 9, 64)
    a.wo += 1
    assert lib.drnmi_conv_wgrad_plan(ctypes.byref(a), 1, None, None, None, None) == -1
    a.wo -= 1
    assert lib.drnmi_conv_wgrad_plan(ctypes.byref(a), 1, None, None, None, None) == 0


def test_gpu_cases_reach_every_workload_route_class():
    """D-22 and D-54 at the benchmark shape, fp32 and fp32x: every class of weight-gradient launch
    (kernel, splits 1 / 2..31 / >= 32, reduce kernel, ragged last split, M % 32 != 0) and of conv_x6
    forward / data-gradient launch (kernel, split-K count) is reached by a kernel-level GPU case."""
    wg, cx = set(), set()
    for arch in ("drn_d_22", "drn_d_54"):
        for precision in ("fp32", "fp32x"):
            w_, c_ = A.route_classes(A.step_routes(arch, precision, *BENCH_SHAPE))
            wg |= w_
            cx |= c_
    assert len(wg) >= 12 and len(cx) >= 12, (sorted(wg), sorted(cx))
    assert any(c[1] == ">=32" and c[2] == "wgrad_reduce_grouped_kernel" for c in wg)
    got_wg = {_wgrad_case_class(c) for c in WGRAD_PLAN_CASES}
    got_cx = set()
    for c in X6_PLAN_CASES:
        assert _x6_case_tile(c) >= 6
        got_cx.add((c[9], c[10]))
    for c in S2_CLASS_CASES:
        got_cx |= set(_s2_case_routes(c))
    print(f"workload: {len(wg)} wgrad classes, {len(cx)} conv_x6 classes; cases reach {len(got_wg)} / {len(got_cx)}")
    assert not wg - got_wg, sorted(wg - got_wg)
    assert not cx - got_cx, sorted(cx - got_cx)
    # the ragged classes also with a pixel count that is no multiple of the 32-pixel chunk
    for c in wg:
        if c[3] and c[0] in ("wgrad_kernel<64, false>", "wgrad_x6_pre_kernel") and c[1] == "2..31":
            assert c[:4] + (True,) in got_wg, c


def _wgrad_node(case):
    from drnmi.engine import _conv_out
    cin, cs, cout, dys, ks, s, p, d, n, h, w, x6 = case
    return A.NodeMeta("case", "x", "y", None, False, False, n, cin, cout, ks, s, p, d, h, w, _conv_out(h, ks, s, p, d),
                      _conv_out(w, ks, s, p, d))


@pytest.mark.gpu
@pytest.mark.parametrize("case", WGRAD_PLAN_CASES, ids=lambda c: "-".join(str(int(v)) for v in c))
def test_wgrad_plan_classes_match_float64(case):
    """One weight gradient per plan class against float64, then a second launch accumulating onto
    the first; gates of train_audit.py (a from torch's fp32, b for the split-bf16 kernels)."""
    from test_gpu_train import _wgrad
    from drnmi import _lib
    cin, cs, cout, dys, ks, s, p, d, n, h, w, x6 = case
    m = _wgrad_node(case)
    g = torch.Generator().manual_seed(cin + cout + h)
    x = torch.zeros(n, h, w, cs)
    x[..., :cin] = torch.randn(n, h, w, cin, generator=g)
    dy = torch.zeros(n * m.oh * m.ow, dys)
    dy[:, :cout] = torch.randn(n * m.oh * m.ow, cout, generator=g)
    plan = _lib.wgrad_plan(A.wgrad_args(n, cin, cs, cout, dys, ks, s, p, d, h, w), x6)
    xd, dyd = x.to(DEV), dy.to(DEV)
    dw = _wgrad(dyd, xd, cin, cout, ks, s, p, d, m.oh, m.ow, x6=x6)
    dw2 = _wgrad(dyd, xd, cin, cout, ks, s, p, d, m.oh, m.ow, accumulate=dw, x6=x6)
    torch.cuda.synchronize()
    rec = {"dy": dy, "x": x, "before": None, "after": dw.cpu(), "x3": x6, "plan": plan}
    figs = A.check_wgrad(m, rec)
    rec2 = dict(rec, before=dw.cpu(), after=dw2.cpu())
    figs += A.check_wgrad(m, rec2)
    assert not _report(f"{plan} M {n * m.oh * m.ow} {A.wgrad_class(plan, n * m.oh * m.ow)}", figs)


@pytest.mark.gpu
@pytest.mark.parametrize("case", X6_PLAN_CASES, ids=lambda c: f"{c[9]}-S{c[10]}".replace(" ", ""))
def test_conv_x6_plan_classes_match_float64(case):
    """conv_x6 as the fine-tune launches it (no scale, fp32 NHWC out, residual = the accumulating
    data-gradient destination) at each tile and split-K count of the benchmark, against float64."""
    from drnmi import _lib, ops
    from drnmi.engine import split3_bf16
    n, h, w, cin, cout, ks, pad, dil, res, kernel, S = case
    g = torch.Generator().manual_seed(cin + cout + ks + S)
    x = torch.randn(n, h, w, cin, generator=g)
    wt = torch.randn(cout, cin, ks, ks, generator=g) / (cin * ks * ks) ** 0.5
    a = _x6_case_args(case, _x6_case_tile(case))
    r = torch.randn(n, a.ho, a.wo, cout, generator=g) if res else None
    wpk, k = ops.pack_conv_weight(wt.to(DEV), cin, torch.float32)
    assert k == a.k and wpk.shape == (a.cout_pad, a.k_pad)
    planes = split3_bf16(wpk)
    xd = x.to(DEV)
    y = r.to(DEV).clone() if res else torch.empty(n, a.ho, a.wo, cout, device=DEV)
    shift = torch.zeros(a.cout_pad, device=DEV)
    ws = torch.empty(a.ws_bytes, dtype=torch.uint8, device=DEV)
    a.x, a.wgt, a.shift, a.y, a.ws = xd.data_ptr(), planes.data_ptr(), shift.data_ptr(), y.data_ptr(), ws.data_ptr()
    a.res = y.data_ptr() if res else None
    assert _lib.load().drnmi_conv_kernel_name(ctypes.byref(a)).decode() == kernel
    _lib.check(_lib.load().drnmi_conv2d_bn_act(ctypes.byref(a), ctypes.c_void_p(_lib.stream_ptr())), "conv_x6")
    torch.cuda.synchronize()
    m = A.NodeMeta("case", "x", "y", None, False, False, n, cin, cout, ks, 1, pad, dil, h, w, a.ho, a.wo, weight=wt)
    v = [A._nhwc(A._conv(A._nchw(x, n, h, w, cin, dt), wt.to(dt), None, m)) + (r.to(dt) if res else 0)
         for dt in (F64, torch.float32)]
    b = A.B_REL * A._nhwc(A._conv(A._nchw(x, n, h, w, cin, F64).abs(), wt.to(F64).abs(), None, m))
    assert not _report(f"{kernel} split-K {S}", [A.gate("y", y.cpu(), v[0], v[1], b)])


@pytest.mark.gpu
@pytest.mark.parametrize("n,h,w,cin,cout,ks,pad,dil", [(1, 20, 36, 512, 512, 3, 4, 4), (2, 13, 11, 128, 128, 3, 1, 1),
                                                       (1, 17, 19, 2048, 512, 1, 0, 1), (1, 17, 19, 64, 64, 3, 1, 1),
                                                       (1, 17, 19, 32, 64, 3, 1, 1)])
def test_f32_igemm_training_plan_matches_float64(n, h, w, cin, cout, ks, pad, dil):
    """The exact-fp32 implicit GEMM as the fine-tune launches it (no scale, a workspace = the
    training plan) against float64 under the audit's gate, at the K of layer6 / layer7 (4608), of
    the 128-channel layers (1152), of a Bottleneck data gradient (2048), of the 64-channel layer3
    (576: folded every 128 k) and below the fold (288).
    One chain over K >= 1024 missed this gate at 5 .. 10 x torch's fp32 error, one over K = 576 at
    5.3 x in a D-24 step (test_train_launches_match_reference); the training plan folds the chain
    every 256 k from K = 1024 on and every 128 k from K = 512 on.  Without a workspace (inference)
    the single chain stays, and below K = 512 both plans are the same bits."""
    from drnmi import _lib, ops
    g = torch.Generator().manual_seed(cin + cout + ks)
    x = torch.relu(torch.randn(n, h, w, cin, generator=g))
    wt = torch.randn(cout, cin, ks, ks, generator=g) * (2.0 / (cin * ks * ks)) ** 0.5
    from drnmi.engine import COUT_ALIGN, _round_up
    ho, wo = h + 2 * pad - dil * (ks - 1), w + 2 * pad - dil * (ks - 1)
    wpk, k = ops.pack_conv_weight(wt.to(DEV), cin, torch.float32)
    xd = x.to(DEV)
    shift = torch.zeros(wpk.shape[0], device=DEV)
    ws = torch.empty(256, dtype=torch.uint8, device=DEV)
    outs = []
    for plan_ws in (ws, None):
        y = torch.empty(n, ho, wo, cout, device=DEV)
        a = A.conv_args(False, _lib.ALGO_IGEMM, n, h, w, cin, ho, wo, cout, wpk.shape[0], ks, 1, pad, dil, k,
                        wpk.shape[1], (ho * wo * cout, cout, 1))
        a.x, a.wgt, a.shift, a.y = xd.data_ptr(), wpk.data_ptr(), shift.data_ptr(), y.data_ptr()
        if plan_ws is not None:
            a.ws, a.ws_bytes = plan_ws.data_ptr(), plan_ws.numel()
        name = _lib.load().drnmi_conv_kernel_name(ctypes.byref(a)).decode()
        assert name.startswith("conv_igemm_kernel<f32"), name
        _lib.check(_lib.load().drnmi_conv2d_bn_act(ctypes.byref(a), ctypes.c_void_p(_lib.stream_ptr())), "igemm")
        outs.append(y)
    torch.cuda.synchronize()
    m = A.NodeMeta("case", "x", "y", None, False, False, n, cin, cout, ks, 1, pad, dil, h, w, ho, wo, weight=wt)
    v = [A._nhwc(A._conv(A._nchw(x, n, h, w, cin, dt), wt.to(dt), None, m)) for dt in (F64, torch.float32)]
    fig = A.gate("y", outs[0].cpu(), v[0], v[1])
    single = float((outs[1].cpu().double() - v[0]).abs().max())
    print(f"{name} K {k}: {fig}; single chain max error {single:.2e} = {4 * single / fig.a:.1f} x torch's")
    assert not A.failures([fig])
    assert torch.equal(outs[0], outs[1]) == (k < 512)


@pytest.mark.gpu
@pytest.mark.parametrize("case", S2_CLASS_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_s2_class_dgrad_matches_float64(case):
    """The fp32x data gradient of a stride-2 conv as parity-class launches of dy (2x2 / 1x1 tap
    kernels, y_sr strided stores, taps past the bottom / right edge read as zero), first into a fresh
    destination and then accumulating onto it, against the float64 transposed conv -- not against
    the zero-inserted conv, which is another GPU kernel."""
    from drnmi import _lib
    from drnmi.engine import COUT_ALIGN, K_ALIGN, _conv_out, _round_up
    lib = _lib.load()
    sp = ctypes.c_void_p(_lib.stream_ptr())
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    n, ih, iw, cin, cout, ks, pad = case
    oh, ow = _conv_out(ih, ks, 2, pad, 1), _conv_out(iw, ks, 2, pad, 1)
    g = torch.Generator().manual_seed(cin + cout + ks)
    wt = torch.randn(cout, cin, ks, ks, generator=g) / (cout * ks * ks) ** 0.5
    dy = torch.randn(n * oh * ow, cout, generator=g)
    classes, pad_d = _s2_class_plan(ks, pad)
    kd = ks * ks * cout
    assert kd == _round_up(kd, K_ALIGN)
    rows_d = _round_up(cin, COUT_ALIGN)
    wd = torch.empty(rows_d, kd, device=DEV)
    wtd = wt.to(DEV)
    _lib.check(lib.drnmi_pack_conv_weight(vp(wtd), cout, cin, ks, cout, rows_d, kd, 1, None, _lib.DRNMI_F32, vp(wd), sp),
               "pack dgrad")
    wdx = torch.empty(3, rows_d, kd, dtype=torch.bfloat16, device=DEV)
    _lib.check(lib.drnmi_split3_bf16(vp(wd), wd.numel(), vp(wdx), sp), "split3")
    dyd = dy.to(DEV)
    zeros = torch.zeros(rows_d, device=DEV)
    out = torch.zeros(n * ih * iw, cin, device=DEV) if len(classes) < 4 else \
        torch.full((n * ih * iw, cin), float("nan"), device=DEV)
    names = []
    snaps = []
    keep = []
    for accumulate in (False, True):
        for (a_, b_, ksc) in classes:
            kpc = ksc * ksc * cout
            planes = torch.empty(3, rows_d, kpc, dtype=torch.bfloat16, device=DEV)
            _lib.check(lib.drnmi_dgrad_s2_class_planes(vp(wdx), rows_d, kd, cout, ks, pad_d, a_, b_, ksc, vp(planes), kpc,
                                                       sp), "class planes")
            keep.append(planes)
            view = out.view(-1)[(a_ * iw + b_) * cin:]
            a = A.conv_args(True, _lib.ALGO_IGEMM, n, oh, ow, cout, (ih - a_ + 1) // 2, (iw - b_ + 1) // 2, cin, rows_d,
                            ksc, 1, 0, 1, kpc, kpc, (ih * iw * cin, 2 * cin, 1), y_sr=2 * iw * cin)
            a.x, a.wgt, a.shift, a.y = dyd.data_ptr(), planes.data_ptr(), zeros.data_ptr(), view.data_ptr()
            a.res = view.data_ptr() if accumulate else None
            names.append(lib.drnmi_conv_kernel_name(ctypes.byref(a)).decode())
            _lib.check(lib.drnmi_conv2d_bn_act(ctypes.byref(a), sp), f"class {a_}{b_}")
        snaps.append(out.cpu().reshape(n, ih, iw, cin))
    torch.cuda.synchronize()
    m = A.NodeMeta("case", "x", "y", None, False, False, n, cin, cout, ks, 2, pad, 1, ih, iw, oh, ow, weight=wt)
    c = [A._nhwc(A._dgrad(wt.to(dt), A._nchw(dy, n, oh, ow, cout, dt), m)) for dt in (F64, torch.float32)]
    b = A.B_REL * A._nhwc(A._dgrad(wt.to(F64).abs(), A._nchw(dy, n, oh, ow, cout, F64).abs(), m))
    figs = [A.gate("dx", snaps[0], c[0], c[1], b),
            A.gate("dx accumulated", snaps[1], c[0] + snaps[0].to(F64), c[1] + snaps[0], b)]
    if len(classes) < 4:
        own = torch.zeros(ih, iw, dtype=torch.bool)
        for (a_, b_, _k) in classes:
            own[a_::2, b_::2] = True
        assert not c[0][:, ~own].any()
        figs.append(A.exact("pixels no tap reaches", snaps[1][:, ~own], torch.zeros_like(snaps[1][:, ~own])))
    assert not _report(f"{sorted(set(names))}", figs)


# ----------------------------------------------------------------------------- CPU: the audit itself
def _node(seed, n, cin, cout, ks, stride, pad, dil, ih, iw, relu=True, res=None):
    from drnmi.engine import _conv_out
    g = torch.Generator().manual_seed(seed)
    m = A.NodeMeta("syn", "x", "y", res, relu, False, n, cin, cout, ks, stride, pad, dil, ih, iw,
                   _conv_out(ih, ks, stride, pad, dil), _conv_out(iw, ks, stride, pad, dil))
    m.weight = torch.randn(cout, cin, ks, ks, generator=g) * (2.0 / (cin * ks * ks)) ** 0.5
    m.gamma = torch.rand(cout, generator=g) + 0.5
    m.beta = torch.randn(cout, generator=g) * 0.2
    return m, g


def _syn_wgrad():
    m, g = _node(1, 2, 64, 64, 3, 1, 2, 2, 48, 40)
    x = torch.relu(torch.randn(2, 48, 40, 64, generator=g))
    dy = torch.randn(2 * 48 * 40, 64, generator=g) * 1e-3
    d = {"dy": dy, "x": x, "before": None, "x3": False, "plan": None}
    d["after"] = A.wgrad_terms(m, d)[0].float()
    return m, d


def test_wgrad_gate_passes_rounded_reference_and_fails_missing_chunk():
    """The fp32-rounded float64 value passes; one 32-pixel chunk missing from one split fails (at
    the benchmark's 1.5 M pixels such a chunk moves the gradient by ~5e-3 rel-L2, inside the
    end-to-end gate of 2e-2)."""
    m, d = _syn_wgrad()
    figs = A.check_wgrad(m, d)
    print(figs[0])
    assert not A.failures(figs) and 0 < figs[0].a < 1e-6
    chunk = torch.zeros_like(d["dy"])
    chunk[1024 + 64:1024 + 96] = d["dy"][1024 + 64:1024 + 96]        # third chunk of the split starting at 1024
    full = A.wgrad_terms(m, d)[0]
    part = A.wgrad_terms(m, dict(d, dy=chunk))[0]
    rel = float((part.norm() / full.norm()))
    bad = dict(d, after=(full - part).float())
    figs = A.check_wgrad(m, bad)
    print(f"missing chunk: rel-L2 {rel:.2e};", figs[0])
    assert A.failures(figs)
    # accumulate: the sum with `before` passes, the overwrite fails
    before = torch.randn(m.weight.shape, generator=torch.Generator().manual_seed(3)) * 1e-2
    acc = dict(d, before=before, after=(full + before.double()).float())
    assert not A.failures(A.check_wgrad(m, acc))
    assert A.failures(A.check_wgrad(m, dict(acc, after=d["after"])))


def test_split_bf16_term_is_derived_not_fitted():
    """b = 2^-25 (|x| conv |w|): a value off by the dropped products' bound passes a split-bf16
    launch and fails an exact-fp32 one."""
    m, d = _syn_wgrad()
    full, _, _ = A.wgrad_terms(m, d)
    _, _, b = A.wgrad_terms(m, dict(d, x3=True))
    assert b is not None and float(b.min()) > 0
    a = A.check_wgrad(m, d)[0].a
    off = (full + a + 0.9 * b).float()               # beyond a, inside a + b
    assert not A.failures(A.check_wgrad(m, dict(d, x3=True, after=off)))
    assert A.failures(A.check_wgrad(m, dict(d, x3=False, after=off)))
    assert A.failures(A.check_wgrad(m, dict(d, x3=True, after=(full + a + 2.0 ** -21 * full.abs() + 1.5 * b).float())))


def _syn_dgrad(stride=1):
    m, g = _node(2, 2, 32, 32, 3, stride, 1, 1, 10, 12)
    dy = torch.randn(2 * m.oh * m.ow, 32, generator=g)
    c = A._nhwc(A._dgrad(m.weight.double(), A._nchw(dy, 2, m.oh, m.ow, 32, F64), m))
    return m, dy, c


def test_dgrad_gate_fails_missing_centre_tap_chunk_at_corner():
    m, dy, c = _syn_dgrad()
    d = {"form": "s1", "cls": None, "fill": "empty", "dy": dy, "before": None, "after": c.float(), "x3": False}
    figs = A.check_dgrad(m, d)
    print(figs[0])
    assert not A.failures(figs)
    # dx[0, 0, 0, ci] without sum over co < 8 of dy[0, 0, 0, co] * w[co, ci, 1, 1]
    miss = c.clone()
    miss[0, 0, 0] -= dy[0, :8].double() @ m.weight[:8, :, 1, 1].double()
    figs = A.check_dgrad(m, dict(d, after=miss.float()))
    assert A.failures(figs) and figs[0].where[:3] == (0, 0, 0), figs[0]
    # a second consumer accumulates onto the first one's gradient
    before = torch.randn(c.shape, generator=torch.Generator().manual_seed(4))
    acc = dict(d, fill="prev", before=before, after=(c + before.double()).float())
    assert not A.failures(A.check_dgrad(m, acc))
    assert A.failures(A.check_dgrad(m, dict(acc, after=c.float())))


@pytest.mark.parametrize("fill", ["zeros", "empty", "prev"])
def test_dgrad_gate_fails_class_at_wrong_parity(fill):
    """A parity-class launch owns (a::2, b::2): its float64 contribution there passes; the same
    values stored at the neighbouring parity fail, and so does a touched pixel of another class."""
    m, dy, c = _syn_dgrad(stride=2)
    a_, b_ = 1, 0
    if fill == "prev":
        before = torch.randn(c.shape, generator=torch.Generator().manual_seed(5)).float()
    elif fill == "zeros":
        before = torch.zeros(c.shape)
    else:
        before = torch.full(c.shape, float("nan"))
    base = before.double() if fill != "empty" else torch.zeros(c.shape, dtype=F64)
    before[:, 0::2, 0::2] = (base + c)[:, 0::2, 0::2].float()            # class 00 already written
    good = before.clone()
    good[:, a_::2, b_::2] = (base + c)[:, a_::2, b_::2].float()
    d = {"form": "class", "cls": (a_, b_), "fill": fill, "written": [(0, 0)], "dy": dy, "before": before, "after": good,
         "x3": False}
    figs = A.check_dgrad(m, d)
    for f in figs:
        print(f)
    assert not A.failures(figs)
    wrong = before.clone()
    wrong[:, 1::2, 1::2] = (base + c)[:, a_::2, b_::2].float()            # stored at parity 11
    assert len(A.failures(A.check_dgrad(m, dict(d, after=wrong)))) >= 1
    touched = good.clone()
    touched[0, 0, 0, 3] += 1e-3                                            # a pixel of class 00
    bad = A.failures(A.check_dgrad(m, dict(d, after=touched)))
    assert len(bad) == 1 and "outside" in bad[0].what
    if fill == "zeros":        # the zero fill itself is checked at the node's first launch
        first = dict(d, written=[], before=torch.zeros(c.shape))
        first["before"][0, 1, 1, 0] = 1e-9
        assert any("zero-filled" in f.what for f in A.failures(A.check_dgrad(m, dict(first, after=first["before"]))))


def _syn_bn(res):
    m, g = _node(6, 2, 16, 32, 3, 1, 1, 1, 9, 7, relu=True, res="r" if res else None)
    rows = 2 * 9 * 7
    y = torch.randn(rows, 32, generator=g) * 2 + 0.3
    before = [torch.randn(32, generator=g) * 0.1, torch.rand(32, generator=g) + 0.5, torch.tensor(4)]
    mean, invstd, rm, rv = A.bn_stats_ref(y, before, m.eps, m.momentum, F64)
    stats = {"y": y, "mean": mean.float(), "invstd": invstd.float(), "fused": False, "before": before,
             "after": [rm.float(), rv.float(), torch.tensor(5)]}
    r = torch.randn(rows, 32, generator=g) if res else None
    z = A.bn_act_ref(y, stats["mean"], stats["invstd"], m.gamma, m.beta, r, True, F64).float()
    act = {"y": y, "mean": stats["mean"], "invstd": stats["invstd"], "res": r, "z": z}
    dz = torch.randn(rows, 32, generator=g)
    dyv, dg, db, dr = A.bn_bwd_ref(dz, z, y, stats["mean"], stats["invstd"], m.gamma, True, F64)
    dres0 = torch.randn(rows, 32, generator=g)
    bwd = {"dz": dz, "z": z, "y": y, "mean": stats["mean"], "invstd": stats["invstd"], "dy": dyv.float(),
           "dgamma": dg.float(), "dbeta": db.float(), "dgamma_before": None, "dbeta_before": None,
           "dres": (dr + dres0.double()).float() if res else None, "dres_before": dres0 if res else None,
           "from_y": not res}
    return m, stats, act, bwd, dr


def test_bn_gates_pass_rounded_reference():
    for res in (False, True):
        m, stats, act, bwd, _ = _syn_bn(res)
        for figs in (A.check_bn_stats(m, stats), A.check_bn_act(m, act), A.check_bn_bwd(m, bwd)):
            for f in figs:
                print(f)
            assert not A.failures(figs)


def test_bn_bwd_gate_fails_dres_overwritten():
    """dres must accumulate onto the gradient the residual value already has."""
    m, _, _, bwd, dr = _syn_bn(True)
    bad = A.failures(A.check_bn_bwd(m, dict(bwd, dres=dr.float())))
    assert [f.what for f in bad] == ["dres (accumulated)"]
    # a fresh dres is dz * mask bit for bit: a flipped mask element fails
    fresh = dict(bwd, dres_before=None, dres=dr.float())
    assert not A.failures(A.check_bn_bwd(m, fresh))
    flip = dr.float().clone()
    k = int(torch.nonzero(flip.reshape(-1) == 0)[0])
    flip.reshape(-1)[k] = bwd["dz"].reshape(-1)[k]
    assert [f.what for f in A.failures(A.check_bn_bwd(m, dict(fresh, dres=flip)))] == ["dres (exact)"]


def _ulps(t, k):
    """t moved by k fp32 ulps away from zero."""
    bits = t.contiguous().view(torch.int32) + k
    return bits.view(torch.float32)


def test_bn_stats_gate_fails_invstd_8_ulps():
    m, stats, _, _, _ = _syn_bn(False)
    bad = dict(stats, invstd=stats["invstd"].clone())
    bad["invstd"][5:6] = _ulps(bad["invstd"][5:6], 8)
    f = A.failures(A.check_bn_stats(m, bad))
    assert [x.what for x in f] == ["invstd"] and f[0].where == (5,)
    bad = dict(stats, after=[stats["after"][0], stats["after"][1], torch.tensor(4)])
    assert [x.what for x in A.failures(A.check_bn_stats(m, bad))] == ["num_batches_tracked (exact)"]


@pytest.mark.parametrize("kind", ["conv", "dgrad", "wgrad"])
def test_gate_fails_4_ulps_at_largest_value(kind):
    """One element 4 fp32 ulps off at the tensor's largest value.  Max-abs over the global max (the
    end-to-end metric) reads 5e-7 there and passes anything.  On small-integer operands every fp32
    order is exact, so a = 0 and the gate is its relative term alone, 2^-22 |ref| (2 .. 4 ulps): one
    ulp passes, four fail.  (On real operands a itself is >= 4 x the half ulp of torch's own
    rounding, so an error of 4 ulps at the largest value is within what two fp32 orders may differ
    by; errors there are caught from ~2^-22 |ref| + a on: profiles/train_audit/README.txt.)"""
    g = torch.Generator().manual_seed(12)
    ints = lambda *shape: torch.randint(-4, 5, shape, generator=g).float()
    m, _ = _node(11, 2, 16, 32, 3, 1, 1, 1, 9, 11)
    m.weight = ints(32, 16, 3, 3)
    x, dy = ints(2, 9, 11, 16), ints(2 * 9 * 11, 32)
    if kind == "wgrad":
        d, key, fn = {"dy": dy, "x": x, "before": None, "x3": False, "plan": None}, "after", A.check_wgrad
        d["after"] = A.wgrad_terms(m, d)[0].float()
    elif kind == "dgrad":
        c = A._nhwc(A._dgrad(m.weight.double(), A._nchw(dy, 2, 9, 11, 32, F64), m))
        d = {"form": "s1", "cls": None, "fill": "empty", "dy": dy, "before": None, "after": c.float(), "x3": False}
        key, fn = "after", A.check_dgrad
    else:
        y = A._nhwc(A._conv(A._nchw(x, 2, 9, 11, 16, F64), m.weight.double(), None, m))
        d, key, fn = {"x": x, "y": y.float().reshape(-1, 32), "x3": False}, "y", A.check_conv
    figs = fn(m, d)
    assert not A.failures(figs) and figs[0].a == 0.0
    for ulps, fails in ((1, False), (4, True)):
        t = d[key].clone()
        k = int(torch.argmax(t.abs().reshape(-1)))
        t.reshape(-1)[k:k + 1] = _ulps(t.reshape(-1)[k:k + 1], ulps)
        figs = fn(m, dict(d, **{key: t}))
        print(ulps, figs[0])
        assert bool(A.failures(figs)) == fails, (ulps, figs[0])


def test_head_and_ce_gates():
    """Head forward / backward and the CE on synthetic records: the rounded float64 values pass, log-probs
    shifted by one pixel, a gradient that ignores ignore_index and a dlog without the softmax term fail."""
    g = torch.Generator().manual_seed(8)
    logits = torch.randn(2, 19, 5, 4, generator=g) * 3
    up = torch.rand(16, 16, generator=g)
    c = 19
    lp = F.log_softmax(F.conv_transpose2d(logits.double(), A._up_weight(up, c, F64), stride=8, padding=4, groups=c), 1)
    head = {"logits": logits, "logprobs": lp.float(), "up": up}
    assert not A.failures(A.check_head(head))
    assert A.failures(A.check_head(dict(head, logprobs=torch.roll(head["logprobs"], 1, dims=3))))
    tgt = torch.randint(0, 19, (2, 40, 32), generator=g)
    tgt[torch.rand(tgt.shape, generator=g) < 0.2] = A.IGNORE
    lp32 = head["logprobs"]
    q = lp32.double().requires_grad_(True)
    loss = F.cross_entropy(q, tgt, ignore_index=A.IGNORE)
    loss.backward()
    ce = {"logprobs": lp32, "target": tgt, "loss": loss.detach().float(), "g_lp": q.grad.float()}
    assert not A.failures(A.check_ce(ce))
    q2 = lp32.double().requires_grad_(True)
    F.cross_entropy(q2, tgt.clamp(max=18)).backward()
    assert [f.what for f in A.failures(A.check_ce(dict(ce, g_lp=q2.grad.float())))] == ["g_logprobs"]
    # (the CE gradient sums to zero over the classes of a pixel, so the softmax term needs another g)
    g_lp = torch.randn(lp32.shape, generator=g) * 1e-3
    hb = {"g_lp": g_lp, "g_logits": None, "logprobs": lp32, "up": up, "grad_scale": 0.5}
    q3 = logits.double().requires_grad_(True)
    lp3 = F.log_softmax(F.conv_transpose2d(q3, A._up_weight(up, c, F64), stride=8, padding=4, groups=c), 1)
    (lp3 * g_lp.double()).sum().backward()
    hb["dlog"] = (0.5 * q3.grad).float()
    figs = A.check_head_bwd(hb)
    print(figs[0])
    assert not A.failures(figs)
    no_softmax = F.conv2d(g_lp.double(), A._up_weight(up, c, F64), stride=8, padding=4, groups=c) * 0.5
    assert A.failures(A.check_head_bwd(dict(hb, dlog=no_softmax.float())))


def test_conv_and_seg_records():
    """Forward conv (padding-channel check included), the seg bias gradient and the NCHW -> NHWC copy."""
    m, g = _node(9, 2, 3, 16, 7, 1, 3, 1, 12, 10)
    x = torch.zeros(2, 12, 10, 8)
    x[..., :3] = torch.randn(2, 12, 10, 3, generator=g)
    y = A._nhwc(A._conv(A._nchw(x, 2, 12, 10, 3, F64), m.weight.double(), None, m)).float().reshape(-1, 16)
    d = {"x": x, "y": y, "x3": False}
    assert not A.failures(A.check_conv(m, d))
    shifted = torch.roll(y.reshape(2, 12, 10, 16), 1, dims=2).reshape(-1, 16)
    assert A.failures(A.check_conv(m, dict(d, y=shifted)))
    s, g = _node(10, 1, 32, 19, 1, 1, 0, 1, 5, 6)
    s.seg, s.bias = True, torch.randn(19, generator=g)
    dlog = torch.randn(1, 19, 5, 6, generator=g)
    dy = torch.zeros(30, 32)
    dy[:, :19] = dlog.permute(0, 2, 3, 1).reshape(30, 19)
    assert not A.failures(A.check_seg_nhwc(s, {"dlog": dlog, "dy": dy}))
    junk = dy.clone()
    junk[3, 25] = 1.0
    assert A.failures(A.check_seg_nhwc(s, {"dlog": dlog, "dy": junk}))
    before = torch.randn(19, generator=g)
    bg = {"dy": dy, "before": before, "after": (dy[:, :19].double().sum(0) + before.double()).float()}
    assert not A.failures(A.check_bias_grad(s, bg))
    assert A.failures(A.check_bias_grad(s, dict(bg, after=dy[:, :19].double().sum(0).float())))
