"""Controls of the fine-tune audit's gates for fp32x2 and frozen-BN launches (tests/train_audit.py), host only.

Each control builds a record on the CPU and pairs the correctly rounded restatement, which must pass, with
one subtly wrong result, which must fail.  A three-product launch is restated as the kernels compute it
(include/drnmi.h DRNMI_F32X2): x1 = bf16(x), x2 = bf16(x - x1), the same for w, and x1 w2 + x2 w1 + x1 w1
summed in float64 and rounded to fp32; a six-product one with the three-way split and the six products
above 2^-24.  The three-product controls run at train_audit.MAX_K3, the longest sums the audit's fp32x2
configurations launch (the GPU audit asserts no launch sums more): K = 18432 for a conv (D-54's layer7: 3x3
over 2048 channels), 192 pixels for the two-plane weight gradient.
"""
from __future__ import annotations

import pytest
import torch

import train_audit as A

F64 = torch.float64
X3 = "conv_x3_kernel<3, 64, 2, 2, 1>"
X6 = "conv_x6_kernel<3, 64, 2, 2>"


def _bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


def split(t, planes):
    """The leading `planes` terms of the bf16 split of an fp32 tensor, as float64."""
    out, r = [], t.float()
    for _ in range(planes):
        p = _bf16(r)
        out.append(p.double())
        r = r - p
    return out


# the products kept, by (plane of x, plane of w), smallest first
THREE = ((0, 1), (1, 0), (0, 0))
SIX = ((0, 2), (1, 1), (2, 0), (0, 1), (1, 0), (0, 0))


def emulate(fn, a, b, pairs):
    """sum over the kept pairs (i, j) of fn(a_i, b_j) in float64, rounded to fp32."""
    planes = 1 + max(max(p) for p in pairs)
    pa, pb = split(a, planes), split(b, planes)
    return sum(fn(pa[i], pb[j]) for i, j in pairs).float()


def _node(seed, n, cin, cout, ks, pad, dil, ih, iw, relu=False, res=None, frozen=False):
    from drnmi.engine import _conv_out
    g = torch.Generator().manual_seed(seed)
    m = A.NodeMeta("syn", "x", "y", res, relu, False, n, cin, cout, ks, 1, pad, dil, ih, iw,
                   _conv_out(ih, ks, 1, pad, dil), _conv_out(iw, ks, 1, pad, dil))
    m.weight = torch.randn(cout, cin, ks, ks, generator=g) * (2.0 / (cin * ks * ks)) ** 0.5
    if frozen:
        m.frozen = True
        m.gamma = torch.rand(cout, generator=g) + 0.5
        m.beta = torch.rand(cout, generator=g) * 0.2 - 0.1
        m.rmean = torch.rand(cout, generator=g) * 0.2 - 0.1
        m.rvar = torch.rand(cout, generator=g) + 0.5
    return m, g


def _conv_rec(m, g, kernel):
    x = torch.relu(torch.randn(m.n, m.ih, m.iw, m.cin, generator=g))
    return x, {"x": x, "x3": True, "kernel": kernel, "k": m.ks * m.ks * m.cin, "split_k": 1}


def _conv_emul(m, x, pairs):
    xc = x.permute(0, 3, 1, 2).contiguous()
    y = emulate(lambda a, b: A._conv(a, b, None, m), xc, m.weight, pairs)
    return A._nhwc(y).reshape(m.n * m.oh * m.ow, m.cout)


@pytest.mark.parametrize("drop", [(1, 0), (0, 1)], ids=["x2w1", "x1w2"])
def test_three_product_conv_gate_fails_dropped_cross_product(drop):
    """A conv_x3 launch of K = 18432 (3x3 over 2048 channels, D-54's layer7): the rounded three-product value
    passes b2 = 3 x 2^-18 S; without one cross product it fails."""
    m, g = _node(21, 1, 2048, 32, 3, 2, 2, 7, 6)
    x, d = _conv_rec(m, g, X3)
    assert d["k"] == A.MAX_K3["conv"] and A.products("conv", d) == 3
    figs = A.check_conv(m, dict(d, y=_conv_emul(m, x, THREE)))
    print(figs[0])
    assert not A.failures(figs) and 0 < figs[0].ratio < A.B2_SUMMED
    figs = A.check_conv(m, dict(d, y=_conv_emul(m, x, [p for p in THREE if p != drop])))
    print(f"without x{drop[0] + 1} w{drop[1] + 1}:", figs[0])
    assert A.failures(figs) and figs[0].ratio > A.B2_SUMMED


@pytest.mark.parametrize("drop", [(1, 0), (0, 1)], ids=["dy2x1", "dy1x2"])
def test_three_product_wgrad_gate_fails_dropped_cross_product(drop):
    """The two-plane pre weight gradient over M = 192 pixels (D-54's 1/8-resolution maps of a 2 x 96 x 64
    batch), below K = 288 and so under the worst-case term 2^-15 S: still fails without a cross product."""
    m, g = _node(22, 2, 128, 128, 3, 1, 1, 12, 8)
    x = torch.relu(torch.randn(m.n, m.ih, m.iw, m.cin, generator=g))
    dy = torch.randn(m.n * m.oh * m.ow, m.cout, generator=g) * 1e-3
    d = {"dy": dy, "x": x, "before": None, "x3": True, "two": True,
         "plan": ("wgrad_x6_pre_kernel", 2, 96, "wgrad_reduce_kernel")}
    assert m.n * m.oh * m.ow == A.MAX_K3["wgrad"] and A.products("wgrad", d) == 3
    dyc = A._nchw(dy, m.n, m.oh, m.ow, m.cout, torch.float32)
    xc = x.permute(0, 3, 1, 2).contiguous()
    fn = lambda a, b: A._wgrad(b, a, m)
    figs = A.check_wgrad(m, dict(d, after=emulate(fn, dyc, xc, THREE)))
    print(figs[0])
    assert not A.failures(figs) and figs[0].b > 0
    figs = A.check_wgrad(m, dict(d, after=emulate(fn, dyc, xc, [p for p in THREE if p != drop])))
    print(f"without dy{drop[0] + 1} x{drop[1] + 1}:", figs[0])
    assert A.failures(figs)
    # the same record on another route of the same step keeps six products and the tighter term
    assert A.products("wgrad", dict(d, plan=("wgrad_kernel<128, true>", 2, 96, "wgrad_reduce_kernel"))) == 6
    assert A.products("wgrad", dict(d, two=False)) == 6


def test_split_term_is_picked_per_launch():
    """K = 288 (3x3 over 32 channels): the rounded three-product value passes as a conv_x3 launch and fails
    when the record names a six-product kernel (b2 against b); the six-product value passes under b."""
    m, g = _node(23, 2, 32, 32, 3, 1, 1, 16, 16)
    x, d3 = _conv_rec(m, g, X3)
    d6 = dict(d3, kernel=X6)
    assert d3["k"] == A.B2_MIN_K and A.products("conv", d3) == 3 and A.products("conv", d6) == 6
    y3, y6 = _conv_emul(m, x, THREE), _conv_emul(m, x, SIX)
    figs = [A.check_conv(m, dict(d, y=y))[0] for d, y in ((d3, y3), (d6, y3), (d6, y6))]
    for f in figs:
        print(f)
    assert not A.failures(figs[:1]) and A.failures(figs[1:2]) and not A.failures(figs[2:])
    assert figs[0].ratio is not None and figs[1].ratio is None
    # below K = 288 the worst case of one product takes over
    S = torch.ones(3, dtype=F64)
    assert torch.equal(A.split_term("dgrad", d3, S, 287)[0], A.B2_ONE * S)
    assert torch.equal(A.split_term("dgrad", d3, S, 288)[0], A.B2_SUMMED * S)
    assert torch.equal(A.split_term("dgrad", d6, S, 64)[0], A.B_REL * S)
    assert A.split_term("conv", dict(d3, x3=False), S, 288) == (None, None)


def _frozen_conv():
    m, g = _node(24, 2, 32, 32, 3, 1, 1, 9, 7, relu=True, res="r", frozen=True)
    x = torch.relu(torch.randn(m.n, m.ih, m.iw, m.cin, generator=g))
    rows = m.n * m.oh * m.ow
    res = torch.randn(rows, m.cout, generator=g)
    s, t, _ = A.frozen_affine(m, F64)
    conv = A._nhwc(A._conv(x.permute(0, 3, 1, 2).double(), m.weight.double(), None, m)).reshape(rows, -1)
    shift = torch.zeros(128)
    shift[:m.cout] = t.float()
    d = {"x": x, "x3": False, "kernel": "conv_igemm_kernel<f32, 128, 64, 2, 2, 3>", "k": 288, "split_k": 1,
         "shift": shift, "res": res, "relu": True}
    return m, d, conv, s, shift[:m.cout].double(), res.double()


def test_frozen_conv_gate():
    """relu(conv(x, w) * s + t + res): passes rounded; fails with t missing on one channel, with gamma in
    place of s on one channel, and with the ReLU applied before the residual."""
    m, d, conv, s, t, res = _frozen_conv()
    figs = A.check_conv(m, dict(d, y=torch.relu(conv * s + t + res).float()))
    print(figs[0])
    assert not A.failures(figs)
    c = int(torch.argmax((m.rvar - 1).abs()))            # where s and gamma differ most
    no_t = t.clone()
    no_t[c] = 0
    f = A.failures(A.check_conv(m, dict(d, y=torch.relu(conv * s + no_t + res).float())))
    assert f and f[0].where[1] == c
    sg = s.clone()
    sg[c] = m.gamma[c].double()
    f = A.failures(A.check_conv(m, dict(d, y=torch.relu(conv * sg + t + res).float())))
    assert f and f[0].where[1] == c
    assert A.failures(A.check_conv(m, dict(d, y=(torch.relu(conv * s + t) + res).float())))
    # the unfused form: y = conv(x, s o w) alone, then bn_act with mean 0, invstd 1, no gamma, beta = t
    y = (conv * s).float()
    assert not A.failures(A.check_conv(m, dict(d, y=y, shift=None, res=None, relu=False)))
    act = {"y": y, "mean": torch.zeros(128), "invstd": torch.ones(128), "res": res.float(), "beta": d["shift"],
           "z": torch.relu(y.double() + t + res).float()}
    assert not A.failures(A.check_bn_act(m, act))
    with_gamma = torch.relu(y.double() * m.gamma.double() + t + res).float()
    assert A.failures(A.check_bn_act(m, dict(act, z=with_gamma)))
    # s, t and rstd themselves, pad channels included
    s32, t32, r32 = (torch.zeros(128) for _ in range(3))
    for buf, v in zip((s32, t32, r32), A.frozen_affine(m, F64)):
        buf[:m.cout] = v.float()
    prep = {"s": s32, "t": t32, "rstd": r32}
    assert not A.failures(A.check_frozen_prepare(m, prep))
    junk = t32.clone()
    junk[m.cout + 3] = 1e-30
    assert [f.what for f in A.failures(A.check_frozen_prepare(m, dict(prep, t=junk)))] == ["t padding channels (exact)"]
    no_eps = s32.clone()
    no_eps[:m.cout] = (m.gamma.double() / m.rvar.double().sqrt()).float()
    assert [f.what for f in A.failures(A.check_frozen_prepare(m, dict(prep, s=no_eps)))] == ["s"]


def _frozen_bwd():
    m, g = _node(25, 2, 16, 32, 3, 1, 1, 9, 7, relu=True, res="r", frozen=True)
    rows = m.n * m.oh * m.ow
    z = torch.relu(torch.randn(rows, m.cout, generator=g))           # post-ReLU data: about half zeros
    dz, dres0, db0 = (torch.randn(rows, m.cout, generator=g), torch.randn(rows, m.cout, generator=g),
                      torch.randn(m.cout, generator=g))
    dr, col = A.frozen_act_bwd_ref(dz, z, True, F64)
    d = {"dz": dz, "z": z, "relu": True, "dr": dr.float(), "dres": (dr + dres0.double()).float(), "dres_before": dres0,
         "dbeta": (col + db0.double()).float(), "dbeta_before": db0, "dbeta_sum": col}
    return m, d, dr, col


def test_frozen_act_bwd_gate():
    """Passes rounded (dres and dbeta accumulated, and stored); fails when dres is overwritten where it must
    accumulate and when the mask is taken as z >= 0."""
    m, d, dr, col = _frozen_bwd()
    assert float((d["z"] == 0).float().mean()) > 0.3
    assert not A.failures(A.check_frozen_act_bwd(m, d))
    stored = dict(d, dres=dr.float(), dres_before=None, dbeta=col.float(), dbeta_before=None)
    assert not A.failures(A.check_frozen_act_bwd(m, stored))
    assert [f.what for f in A.failures(A.check_frozen_act_bwd(m, dict(d, dres=dr.float())))] == ["dres (accumulated)"]
    assert [f.what for f in A.failures(A.check_frozen_act_bwd(m, dict(d, dbeta=col.float())))] == ["dbeta (accumulated)"]
    ge = torch.where(d["z"] >= 0, d["dz"], torch.zeros(()))
    bad = A.failures(A.check_frozen_act_bwd(m, dict(stored, dr=ge, dres=ge, dbeta=ge.double().sum(0).float(),
                                                    dbeta_sum=ge.double().sum(0))))
    assert {"dr (exact)", "dres (exact)", "dbeta", "dbeta_sum"} == {f.what for f in bad}


def test_frozen_unfold_gate():
    """dw = s o G and dgamma = rstd (<G, w> - running_mean sum dr): pass rounded, stored and accumulated; fail
    when gamma.grad (or weight.grad) is stored where it must accumulate, and without the running_mean term."""
    m, g = _node(26, 1, 32, 16, 3, 1, 1, 5, 5, frozen=True)
    G = torch.randn(m.weight.shape, generator=g) * 1e-2
    dsum = torch.randn(m.cout, generator=g).double()
    s, _, rstd = (v.float() for v in A.frozen_affine(m, F64))
    dw, dg = A.frozen_unfold_ref(G, m.weight, s, rstd, m.rmean, dsum, F64)
    dw0, dg0 = torch.randn(m.weight.shape, generator=g) * 1e-2, torch.randn(m.cout, generator=g)
    d = {"g": G, "w": m.weight.clone(), "s": s, "rstd": rstd, "dbeta_sum": dsum, "dw": dw.float(), "dgamma": dg.float(),
         "dw_before": None, "dgamma_before": None}
    assert not A.failures(A.check_frozen_unfold(m, d))
    acc = dict(d, dw=(dw + dw0.double()).float(), dgamma=(dg + dg0.double()).float(), dw_before=dw0, dgamma_before=dg0)
    assert not A.failures(A.check_frozen_unfold(m, acc))
    assert [f.what for f in A.failures(A.check_frozen_unfold(m, dict(acc, dgamma=dg.float())))] == ["dgamma (accumulated)"]
    assert [f.what for f in A.failures(A.check_frozen_unfold(m, dict(acc, dw=dw.float())))] == ["dw (accumulated)"]
    no_mean = (rstd.double() * (G.double() * m.weight.double()).flatten(1).sum(1)).float()
    assert [f.what for f in A.failures(A.check_frozen_unfold(m, dict(d, dgamma=no_mean)))] == ["dgamma"]
    # gamma alone (the conv weight is not trained): the launch writes no dw
    assert [f.what for f in A.check_frozen_unfold(m, dict(d, dw=None))] == ["dgamma"]


def test_frozen_dgrad_reads_folded_weight():
    """The data gradient of a frozen step is conv^T(s o w, dr): the raw weight fails."""
    m, g = _node(27, 2, 32, 32, 3, 1, 1, 10, 12, frozen=True)
    dy = torch.randn(m.n * m.oh * m.ow, m.cout, generator=g)
    dyc = A._nchw(dy, m.n, m.oh, m.ow, m.cout, F64)
    d = {"form": "s1", "cls": None, "fill": "empty", "dy": dy, "before": None, "x3": False}
    good = A._nhwc(A._dgrad(A.folded_weight(m, F64), dyc, m)).float()
    assert not A.failures(A.check_dgrad(m, dict(d, after=good)))
    assert A.failures(A.check_dgrad(m, dict(d, after=A._nhwc(A._dgrad(m.weight.double(), dyc, m)).float())))


def test_route_walk_knows_fp32x2_and_freeze_bn():
    """step_routes: fp32x2 turns every conv_x6 launch of fp32x into conv_x3 and keeps the patch kernels and the
    weight-gradient plans; freeze_bn changes no route (the statistics request and the epilogue are not part of
    the kernel's name) -- the GPU audit compares these walks with the launches the runner made."""
    a = A.step_routes("drn_d_22", "fp32x", 1, 72, 40)
    b = A.step_routes("drn_d_22", "fp32x2", 1, 72, 40)
    assert len(a) == len(b)
    for (wa, na, ra), (wb, nb, rb) in zip(a, b):
        assert (wa, na) == (wb, nb)
        if wa == "wgrad" or not ra[0].startswith("conv_x6_kernel"):
            assert ra == rb, (na, ra, rb)
        else:
            assert rb[0].startswith("conv_x3_kernel") and ra[0].split("<")[1][0] == rb[0].split("<")[1][0], (na, ra, rb)
    assert [r[:2] for r in A.step_routes("drn_d_22", "fp32x2", 1, 72, 40, freeze_bn=True)] == [r[:2] for r in b]
