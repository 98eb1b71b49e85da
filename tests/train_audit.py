"""Teacher-forced audit of one fine-tune step against float64 -- TEST INFRASTRUCTURE.

The end-to-end fine-tune gates (tests/test_gpu_train.py) compare final gradients with a float64
oracle under a relative-L2 bound of 1e-3 .. 2e-2: a ReLU within an ulp of zero may fall either way
in fp32 and float64, so the bound has to be loose, and a weight gradient that drops one 32-pixel
chunk or a data gradient that misses one border tap fits inside it.  Here every launch of
TrainRunner.forward / TrainRunner.backward is recorded through TrainRunner.record with what it
read and wrote, and re-computed on the CPU in float64 from the launch's own GPU inputs:

  capture(cfg)         one GPU run per configuration (cached): a Capture (records + node geometry)
  check(cap, rec)      float64 reference of one record and its gates; returns the Figures measured
  step_routes(...)     host-only: the conv / wgrad routes a step takes at a shape (library queries)

Taking every launch's inputs from the GPU removes the ReLU flips: the BN backward's mask is the
GPU's own z > 0, so no element is excluded from any comparison.

Gates: |got - ref| <= 2^-22 |ref| + a (+ b), elementwise.  a = 4 x max |v32 - ref|,
v32 the same operation on the same operands through torch's CPU fp32 kernels: one valid fp32
evaluation order; the GPU's is another, the two may err in opposite directions (2), and 2 is
margin.  2^-22 |ref| is two fp32 ulps of the result (the final rounding and one more).  b, split-
bf16 launches only (conv_x6, the X6 patch kernels, drnmi_conv_wgrad_f32x3): the three-way bf16
split is exact, the products dropped are x2 w3, x3 w2 and x3 w3, bounded by (2^-27 + 2^-27 + 2^-36)
|x| |w|; b = 2^-25 (|x| conv |w|) in float64 is that bound with a factor of two.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field

import torch
import torch.nn.functional as F

from plan_audit import GROUPS, group_of

SEED = 13
IGNORE = 255
# name -> (arch, precision, input shape, passes): passes forward + backward runs without zero_grad
CONFIGS = {
    "d22_fp32_1x72x40": ("drn_d_22", "fp32", (1, 3, 72, 40), 1),
    "d22_fp32x_1x72x40": ("drn_d_22", "fp32x", (1, 3, 72, 40), 1),
    "d54_fp32_2x96x64": ("drn_d_54", "fp32", (2, 3, 96, 64), 1),
    "d54_fp32x_2x96x64": ("drn_d_54", "fp32x", (2, 3, 96, 64), 1),
    "d22_fp32x_2x64x64_acc": ("drn_d_22", "fp32x", (2, 3, 64, 64), 2),
    # two conv+BN+ReLU units in layer7 and layer8 (BasicBlock and Bottleneck trunks)
    "d24_fp32_1x72x40": ("drn_d_24", "fp32", (1, 3, 72, 40), 1),
    "d24_fp32x_1x72x40": ("drn_d_24", "fp32x", (1, 3, 72, 40), 1),
    "d56_fp32x_1x64x64": ("drn_d_56", "fp32x", (1, 3, 64, 64), 1),
}
# every kind a record may have; each has exactly one check below
NODE_KINDS = ("conv", "bn_stats", "bn_act", "seg_nhwc", "bias_grad", "bn_bwd", "wgrad", "dgrad")
HEAD_KINDS = ("head", "ce", "head_bwd")
F64 = torch.float64
EPS_REL = 2.0 ** -22
B_REL = 2.0 ** -25


# ----------------------------------------------------------------------------- records
@dataclass
class NodeMeta:
    """Geometry and parameters of one graph node (host copies, fp32)."""
    name: str
    src: str
    dst: str
    res: str | None
    relu: bool
    seg: bool
    n: int
    cin: int
    cout: int
    ks: int
    stride: int
    pad: int
    dil: int
    ih: int
    iw: int
    oh: int
    ow: int
    weight: torch.Tensor | None = None
    bias: torch.Tensor | None = None
    gamma: torch.Tensor | None = None
    beta: torch.Tensor | None = None
    eps: float = 1e-5
    momentum: float = 0.1
    keys: dict = field(default_factory=dict)    # weight / bias / gamma / beta -> parameter name


@dataclass
class Rec:
    index: int
    kind: str
    name: str | None          # node name; None for the head
    group: str
    step: int                 # forward + backward pass the record belongs to
    data: dict = field(default_factory=dict)


@dataclass
class Capture:
    cfg: str
    recs: list
    meta: dict                # node name -> NodeMeta
    order: list               # node names in graph order
    params: dict              # parameter name -> final .grad (host)


@dataclass
class Figure:
    """One compared output of one launch: a, max b, worst excess over the gate (<= 0 passes)."""
    what: str
    a: float
    b: float
    excess: float
    where: tuple
    got: float
    ref: float
    n: int

    def __str__(self):
        return (f"{self.what}: a {self.a:.2e} b {self.b:.2e} worst excess {self.excess:.2e} at {self.where} "
                f"(got {self.got:.9g}, ref {self.ref:.9g}, {self.n} elements)")


def gate(what: str, got: torch.Tensor, ref: torch.Tensor, v32: torch.Tensor | None, b: torch.Tensor | None = None,
         a: float | None = None) -> Figure:
    """|got - ref| <= 2^-22 |ref| + a (+ b) over every element; a from v32 unless given."""
    ref = ref.to(F64)
    got64 = got.to(F64)
    assert got64.shape == ref.shape, (what, tuple(got64.shape), tuple(ref.shape))
    if ref.numel() == 0:
        return Figure(what, 0.0, 0.0, 0.0, (), 0.0, 0.0, 0)
    if a is None:
        a = 4.0 * float((v32.to(F64) - ref).abs().max())
    bound = EPS_REL * ref.abs() + a
    if b is not None:
        bound = bound + b
    over = (got64 - ref).abs() - bound
    over = torch.where(torch.isfinite(got64), over, torch.full_like(over, float("inf")))
    k = int(torch.argmax(over.reshape(-1)))
    where = tuple(int(i) for i in torch.unravel_index(torch.tensor(k), over.shape)) if over.dim() else ()
    return Figure(what, a, float(b.max()) if b is not None else 0.0, float(over.reshape(-1)[k]), where,
                  float(got64.reshape(-1)[k]), float(ref.reshape(-1)[k]), ref.numel())


def exact(what: str, got: torch.Tensor, ref: torch.Tensor) -> Figure:
    """Bit-for-bit: the excess is the count of differing elements (0 passes)."""
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    if ref.numel() == 0:
        return Figure(what + " (exact)", 0.0, 0.0, 0.0, (), 0.0, 0.0, 0)
    bad = ~((got == ref) | (torch.isnan(got) & torch.isnan(ref)))
    k = int(torch.argmax(bad.reshape(-1).to(torch.uint8)))
    where = tuple(int(i) for i in torch.unravel_index(torch.tensor(k), bad.shape)) if bad.dim() else ()
    return Figure(what + " (exact)", 0.0, 0.0, float(bad.sum()), where, float(got.reshape(-1)[k]),
                  float(ref.reshape(-1)[k]), ref.numel())


# ----------------------------------------------------------------------------- references
def _nchw(t: torch.Tensor, n: int, h: int, w: int, c: int, dtype) -> torch.Tensor:
    """NHWC rows [n*h*w, stride] (or [n, h, w, stride]) -> NCHW [n, c, h, w] of the first c channels."""
    return t.reshape(n, h, w, -1)[..., :c].permute(0, 3, 1, 2).to(dtype).contiguous()


def _nhwc(t: torch.Tensor) -> torch.Tensor:
    return t.permute(0, 2, 3, 1).contiguous()


def _conv(x, w, bias, m: NodeMeta):
    return F.conv2d(x, w, bias, stride=m.stride, padding=m.pad, dilation=m.dil)


def _wgrad(x, dy, m: NodeMeta):
    return torch.nn.grad.conv2d_weight(x, (m.cout, m.cin, m.ks, m.ks), dy, stride=m.stride, padding=m.pad,
                                       dilation=m.dil)


def _dgrad(w, dy, m: NodeMeta):
    return torch.nn.grad.conv2d_input((m.n, m.cin, m.ih, m.iw), w, dy, stride=m.stride, padding=m.pad,
                                      dilation=m.dil)


def check_conv(m: NodeMeta, d: dict) -> list:
    outs = {}
    for dt in (F64, torch.float32):
        x = _nchw(d["x"], m.n, m.ih, m.iw, m.cin, dt)
        outs[dt] = _conv(x, m.weight.to(dt), m.bias.to(dt) if m.bias is not None else None, m)
    b = None
    if d["x3"]:
        b = B_REL * _conv(_nchw(d["x"], m.n, m.ih, m.iw, m.cin, F64).abs(), m.weight.to(F64).abs(), None, m)
    got = d["y"] if m.seg else _nchw(d["y"], m.n, m.oh, m.ow, m.cout, torch.float32)
    figs = [gate("y", got, outs[F64], outs[torch.float32], b)]
    if not m.seg and d["y"].reshape(m.n * m.oh * m.ow, -1).shape[1] != m.cout:
        pad = d["y"].reshape(m.n * m.oh * m.ow, -1)[:, m.cout:]
        figs.append(exact("y padding channels", pad, torch.zeros_like(pad)))
    return figs


def bn_stats_ref(y: torch.Tensor, before: list, eps: float, momentum: float, dt):
    """(mean, invstd, running_mean, running_var) of y [rows, C] in dtype dt."""
    y = y.to(dt)
    rows = y.shape[0]
    mean = y.mean(0)
    var = ((y - mean) ** 2).mean(0)
    invstd = (var + eps) ** -0.5
    unb = var * (rows / (rows - 1)) if rows > 1 else var
    rm = momentum * mean + (1 - momentum) * before[0].to(dt)
    rv = momentum * unb + (1 - momentum) * before[1].to(dt)
    return mean, invstd, rm, rv


def bn_stats_torch32(y: torch.Tensor, before: list, eps: float, momentum: float):
    """The same four through torch's own CPU fp32 batch norm (native_batch_norm in training mode)."""
    rm, rv = before[0].clone().float(), before[1].clone().float()
    _, mean, invstd = torch.native_batch_norm(y.float().t().reshape(1, y.shape[1], -1), None, None, rm, rv, True,
                                              momentum, eps)
    return mean, invstd, rm, rv


def check_bn_stats(m: NodeMeta, d: dict) -> list:
    y = d["y"].reshape(m.n * m.oh * m.ow, -1)
    r64 = bn_stats_ref(y, d["before"], m.eps, m.momentum, F64)
    r32 = bn_stats_torch32(y, d["before"], m.eps, m.momentum)
    got = (d["mean"], d["invstd"], d["after"][0], d["after"][1])
    figs = [gate(k, g, a, b) for k, g, a, b in zip(("mean", "invstd", "running_mean", "running_var"), got, r64, r32)]
    figs.append(exact("num_batches_tracked", d["after"][2], d["before"][2] + 1))
    return figs


def bn_act_ref(y, mean, invstd, gamma, beta, res, relu, dt):
    z = ((y.to(dt) - mean.to(dt)) * invstd.to(dt)) * gamma.to(dt) + beta.to(dt)
    if res is not None:
        z = z + res.to(dt)
    return torch.relu(z) if relu else z


def check_bn_act(m: NodeMeta, d: dict) -> list:
    rows = m.n * m.oh * m.ow
    y = d["y"].reshape(rows, -1)
    res = d["res"].reshape(rows, -1) if d["res"] is not None else None
    assert (res is not None) == (m.res is not None), m.name
    r = [bn_act_ref(y, d["mean"], d["invstd"], m.gamma, m.beta, res, m.relu, dt) for dt in (F64, torch.float32)]
    return [gate("z", d["z"].reshape(rows, -1), r[0], r[1])]


def _up_weight(up: torch.Tensor, c: int, dt) -> torch.Tensor:
    return up.to(dt).reshape(1, 1, 16, 16).expand(c, 1, 16, 16).contiguous()


def check_head(d: dict) -> list:
    c = d["logits"].shape[1]
    r = [F.log_softmax(F.conv_transpose2d(d["logits"].to(dt), _up_weight(d["up"], c, dt), stride=8, padding=4, groups=c),
                       1) for dt in (F64, torch.float32)]
    return [gate("logprobs", d["logprobs"], r[0], r[1])]


def check_ce(d: dict) -> list:
    outs = []
    for dt in (F64, torch.float32):
        lp = d["logprobs"].detach().to(dt, copy=True).requires_grad_(True)
        loss = F.cross_entropy(lp, d["target"], ignore_index=IGNORE)
        loss.backward()
        outs.append((loss.detach(), lp.grad))
    return [gate("loss", d["loss"], outs[0][0], outs[1][0]), gate("g_logprobs", d["g_lp"], outs[0][1], outs[1][1])]


def head_bwd_ref(g, lp, g_logits, up, scale, dt):
    c = g.shape[1]
    g, lp = g.to(dt), lp.to(dt)
    du = g - torch.exp(lp) * g.sum(1, keepdim=True)
    out = F.conv2d(du, _up_weight(up, c, dt), stride=8, padding=4, groups=c)
    if g_logits is not None:
        out = out + g_logits.to(dt)
    return out * scale


def check_head_bwd(d: dict) -> list:
    r = [head_bwd_ref(d["g_lp"], d["logprobs"], d["g_logits"], d["up"], d["grad_scale"], dt)
         for dt in (F64, torch.float32)]
    return [gate("dlog", d["dlog"], r[0], r[1])]


def check_seg_nhwc(m: NodeMeta, d: dict) -> list:
    dy = d["dy"].reshape(m.n, m.oh, m.ow, -1)
    want = torch.zeros_like(dy)
    want[..., :m.cout] = d["dlog"].permute(0, 2, 3, 1)
    return [exact("seg dy", dy, want)]


def check_bias_grad(m: NodeMeta, d: dict) -> list:
    dy = d["dy"].reshape(m.n * m.oh * m.ow, -1)[:, :m.cout]
    r = []
    for dt in (F64, torch.float32):
        v = dy.to(dt).sum(0)
        r.append(v + d["before"].to(dt) if d["before"] is not None else v)
    return [gate("bias.grad", d["after"], r[0], r[1])]


def bn_bwd_ref(dz, z, y, mean, invstd, gamma, relu, dt):
    """(dy, dgamma, dbeta, dr) with the ReLU mask taken as z > 0."""
    dr = dz.to(dt)
    if relu:
        dr = torch.where(z > 0, dr, torch.zeros_like(dr))
    rows = y.shape[0]
    yc = y.to(dt) - mean.to(dt)
    s1 = dr.sum(0)
    sx = (dr * yc).sum(0)
    is_ = invstd.to(dt)
    dgamma = is_ * sx
    dy = (gamma.to(dt) * is_) * (dr - s1 / rows - yc * (is_ * is_ * sx / rows))
    return dy, dgamma, s1, dr


def check_bn_bwd(m: NodeMeta, d: dict) -> list:
    rows = m.n * m.oh * m.ow
    sh = lambda t: t.reshape(rows, -1)
    assert d["from_y"] == (m.relu and m.res is None), m.name
    r = [bn_bwd_ref(sh(d["dz"]), sh(d["z"]), sh(d["y"]), d["mean"], d["invstd"], m.gamma, m.relu, dt)
         for dt in (F64, torch.float32)]
    figs = [gate("dy", sh(d["dy"]), r[0][0], r[1][0])]
    for i, key in ((1, "dgamma"), (2, "dbeta")):
        if d[key] is None:
            continue
        before = d[key + "_before"]
        v64, v32 = r[0][i], r[1][i]
        if before is not None:
            v64, v32 = v64 + before.to(F64), v32 + before
        figs.append(gate(key, d[key], v64, v32))
    assert (d["dres"] is not None) == (m.res is not None), m.name
    if d["dres"] is not None:
        if d["dres_before"] is None:         # dres = dz * mask: no arithmetic, so no rounding
            figs.append(exact("dres", sh(d["dres"]), r[1][3]))
        else:
            figs.append(gate("dres (accumulated)", sh(d["dres"]), r[0][3] + sh(d["dres_before"]).to(F64),
                             r[1][3] + sh(d["dres_before"])))
    return figs


def wgrad_terms(m: NodeMeta, d: dict):
    """(float64 contribution, fp32 contribution, b or None) of one wgrad launch."""
    rows = m.n * m.oh * m.ow
    dys = d["dy"].reshape(rows, -1)
    v = []
    for dt in (F64, torch.float32):
        v.append(_wgrad(_nchw(d["x"], m.n, m.ih, m.iw, m.cin, dt), _nchw(dys, m.n, m.oh, m.ow, m.cout, dt), m))
    b = None
    if d["x3"]:
        b = B_REL * _wgrad(_nchw(d["x"], m.n, m.ih, m.iw, m.cin, F64).abs(),
                           _nchw(dys, m.n, m.oh, m.ow, m.cout, F64).abs(), m)
    return v[0], v[1], b


def check_wgrad(m: NodeMeta, d: dict) -> list:
    v64, v32, b = wgrad_terms(m, d)
    if d["before"] is not None:
        v64, v32 = v64 + d["before"].to(F64), v32 + d["before"]
    return [gate("weight.grad", d["after"], v64, v32, b)]


def check_dgrad(m: NodeMeta, d: dict) -> list:
    """One data-gradient launch: this launch's contribution added to the `before` snapshot of its
    destination.  A parity-class launch (cls = (a, b)) owns the pixels (a::2, b::2); every other
    pixel must keep its `before` bits, wherever `before` is defined: a destination the step
    allocated uninitialised (fill == "empty") is defined on the classes already written."""
    rows = m.n * m.oh * m.ow
    dys = d["dy"].reshape(rows, -1)
    c = [_nhwc(_dgrad(m.weight.to(dt), _nchw(dys, m.n, m.oh, m.ow, m.cout, dt), m)) for dt in (F64, torch.float32)]
    b = None
    if d["x3"]:
        b = B_REL * _nhwc(_dgrad(m.weight.to(F64).abs(), _nchw(dys, m.n, m.oh, m.ow, m.cout, F64).abs(), m))
    after = d["after"].reshape(m.n, m.ih, m.iw, -1)
    assert after.shape[3] == m.cin, (m.name, after.shape)
    before = d["before"].reshape(after.shape) if d["before"] is not None else None
    assert (before is not None) == (d["fill"] != "empty" or d["form"] == "class"), m.name
    figs = []
    if d["form"] != "class":
        if d["fill"] == "prev":
            c = [c[0] + before.to(F64), c[1] + before]
        return [gate(f"d {m.src} ({d['form']})", after, c[0], c[1], b)]
    a_, b_ = d["cls"]
    own = torch.zeros(m.ih, m.iw, dtype=torch.bool)
    own[a_::2, b_::2] = True
    defined = torch.ones(m.ih, m.iw, dtype=torch.bool)
    if d["fill"] == "empty":
        defined[:] = False
        for (pa, pb) in d["written"]:
            defined[pa::2, pb::2] = True
    elif d["fill"] == "zeros" and not d["written"]:
        figs.append(exact("zero-filled destination", before, torch.zeros_like(before)))
    assert not (defined & own).any() or d["fill"] != "empty", (m.name, d["cls"], d["written"])
    if d["fill"] != "empty":
        c = [c[0] + before.to(F64), c[1] + before]
    sel = lambda t: t[:, a_::2, b_::2]
    figs.append(gate(f"d {m.src} class {a_}{b_}", sel(after), sel(c[0]), sel(c[1]), sel(b) if b is not None else None))
    keep = defined & ~own
    figs.append(exact(f"d {m.src} outside class {a_}{b_}", after[:, keep], before[:, keep]))
    return figs


CHECKS = {"conv": check_conv, "bn_stats": check_bn_stats, "bn_act": check_bn_act, "seg_nhwc": check_seg_nhwc,
          "bias_grad": check_bias_grad, "bn_bwd": check_bn_bwd, "wgrad": check_wgrad, "dgrad": check_dgrad}
HEAD_CHECKS = {"head": check_head, "ce": check_ce, "head_bwd": check_head_bwd}


def check(cap: Capture, rec: Rec) -> list:
    """The Figures of one record (every compared output); raises on a malformed record only."""
    if rec.kind in HEAD_CHECKS:
        return HEAD_CHECKS[rec.kind](rec.data)
    return CHECKS[rec.kind](cap.meta[rec.name], rec.data)


def failures(figs: list) -> list:
    return [f for f in figs if not f.excess <= 0]


def launch_label(rec: Rec) -> str:
    d = rec.data
    if rec.kind == "wgrad":
        k, s, per, red = d["plan"]
        return f"{k} x{s} per {per} + {red}"
    if "kernel" in d:
        return f"{d['kernel']} split-K {d['split_k']}"
    if rec.kind == "bn_stats":
        return "bn_stats_partials" if d["fused"] else "bn_stats"
    if rec.kind == "bn_bwd":
        return "bn_relu_bwd_y" if d["from_y"] else "bn_act_bwd"
    return rec.kind


# ----------------------------------------------------------------------------- capture
def _host(v):
    if torch.is_tensor(v):
        return v.detach().cpu()
    if isinstance(v, (list, tuple)) and v and all(torch.is_tensor(t) or t is None for t in v):
        return [_host(t) for t in v]
    return v


def node_meta(model, shape) -> tuple:
    """({name: NodeMeta}, [names]) of model._graph at an input shape (parameters as host fp32)."""
    from drnmi.engine import _conv_out
    n, _, h, w = shape
    shapes = {"input": (h, w)}
    meta, order = {}, []
    ids = {id(q): k for k, q in model.named_parameters()}
    for nd in model._graph.nodes:
        c = nd.conv
        ih, iw = shapes[nd.src]
        ks, s, p, d = c.kernel_size[0], c.stride[0], c.padding[0], c.dilation[0]
        oh, ow = _conv_out(ih, ks, s, p, d), _conv_out(iw, ks, s, p, d)
        shapes[nd.dst] = (oh, ow)
        t = lambda q: None if q is None else q.detach().float().cpu().clone()
        meta[nd.name] = NodeMeta(nd.name, nd.src, nd.dst, nd.res or None, bool(nd.relu), bool(nd.out_fp32_nchw), n,
                                 c.in_channels, c.out_channels, ks, s, p, d, ih, iw, oh, ow, t(c.weight), t(c.bias),
                                 t(nd.bn.weight) if nd.bn is not None else None,
                                 t(nd.bn.bias) if nd.bn is not None else None,
                                 float(nd.bn.eps) if nd.bn is not None else 0.0,
                                 float(nd.bn.momentum) if nd.bn is not None else 0.0)
        ps = {"weight": c.weight, "bias": c.bias, "gamma": nd.bn.weight if nd.bn is not None else None,
              "beta": nd.bn.bias if nd.bn is not None else None}
        meta[nd.name].keys = {k: ids[id(q)] for k, q in ps.items() if q is not None}
        order.append(nd.name)
    return meta, order


_CACHE: dict = {}


def make_inputs(shape, seed=SEED):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=g)
    t = torch.randint(0, 19, (shape[0], shape[2], shape[3]), generator=g)
    t[torch.rand(t.shape, generator=g) < 0.2] = IGNORE
    return x, t


def capture(cfg: str) -> Capture:
    """One recorded GPU run of configuration `cfg` (cached)."""
    if cfg in _CACHE:
        return _CACHE[cfg]
    from drnmi.drnseg import DRNSeg
    from drnmi.train import CrossEntropyLoss, TrainRunner
    from drnmi.weights import synth_state_dict
    arch, precision, shape, passes = CONFIGS[cfg]
    m = DRNSeg(arch, 19, pretrained=False)
    m.load_state_dict(synth_state_dict(m, SEED))
    m.set_precision(precision)
    m = m.to("cuda").train()
    meta, order = node_meta(m, shape)
    x, t = make_inputs(shape)
    recs: list = []
    step = [0]

    def hook(kind, name, items):
        recs.append(Rec(len(recs), kind, name, group_of(name), step[0], {k: _host(v) for k, v in items.items()}))

    crit = CrossEntropyLoss(ignore_index=IGNORE)
    xd, td = x.to("cuda"), t.to("cuda")
    m._train_runner = TrainRunner(m)           # as train_forward would on the first call
    m._train_runner.record = hook
    for i in range(passes):
        step[0] = i
        lp = m(xd)[0]
        lp.retain_grad()
        loss = crit(lp, td)
        loss.backward()
        head = [r for r in recs if r.kind == "head" and r.step == i][-1]
        recs.append(Rec(len(recs), "ce", None, "head", i, {"logprobs": head.data["logprobs"], "target": t,
                                                           "loss": loss.detach().cpu(), "g_lp": lp.grad.detach().cpu()}))
    torch.cuda.synchronize()
    m._train_runner.record = None
    # the classes written before each parity-class launch of the same node and pass
    seen: dict = {}
    for r in recs:
        if r.kind == "dgrad" and r.data["form"] == "class":
            done = seen.setdefault((r.step, r.name), [])
            r.data["written"] = list(done)
            done.append(tuple(r.data["cls"]))
    params = {k: p.grad.detach().cpu() for k, p in m.named_parameters() if p.grad is not None}
    cap = Capture(cfg, recs, meta, order, params)
    _CACHE[cfg] = cap
    return cap


def launches(cfg: str, group: str) -> list:
    return [r for r in capture(cfg).recs if r.group == group]


# ----------------------------------------------------------------------------- routes of a step
PTR = 0x1000        # placeholder for a present, 16-byte aligned operand: the queries read no data


def wgrad_class(plan, m_pix: int) -> tuple:
    """(kernel, split bucket, reduce kernel, ragged last split, M % 32 != 0) of a wgrad plan."""
    kernel, splits, per, reduce = plan
    bucket = "1" if splits == 1 else "2..31" if splits < 32 else ">=32"
    ragged = kernel != "wgrad_x6_direct_kernel" and m_pix % per != 0
    return (kernel, bucket, reduce, bool(ragged), m_pix % 32 != 0)


def wgrad_args(n, cin, cs, cout, dys, ks, stride, pad, dil, h, w):
    from drnmi import _lib
    from drnmi.engine import _conv_out
    a = _lib.WgradArgs()
    a.dy = a.x = a.dw = a.ws = PTR
    a.ws_bytes = 1 << 40
    a.n, a.h, a.w, a.cin, a.cin_stride = n, h, w, cin, cs
    a.ho, a.wo = _conv_out(h, ks, stride, pad, dil), _conv_out(w, ks, stride, pad, dil)
    a.cout, a.dy_stride = cout, dys
    a.ks, a.stride, a.pad, a.dil = ks, stride, pad, dil
    return a


def conv_args(x3, algo, n, h, w, cin, ho, wo, cout, cout_pad, ks, stride, pad, dil, k, k_pad, y_strides, res=False,
              y_sr=0, tile=-1):
    from drnmi import _lib
    a = _lib.ConvArgs()
    a.x = a.wgt = a.shift = a.y = PTR
    a.res = PTR if res else None
    a.y_sn, a.y_sp, a.y_sc = y_strides
    a.y_sr = y_sr
    a.n, a.h, a.w, a.cin = n, h, w, cin
    a.ho, a.wo, a.cout, a.cout_pad = ho, wo, cout, cout_pad
    a.ks, a.stride, a.pad, a.dil = ks, stride, pad, dil
    a.k, a.k_pad = k, k_pad
    a.relu = 0
    a.dtype = _lib.DRNMI_F32X3 if x3 else _lib.DRNMI_F32
    a.out_dtype = _lib.DRNMI_F32
    a.tile, a.algo = tile, algo
    return a


def conv_route(a, split=True, want_stats=False) -> tuple:
    """(kernel name, split-K count) of a training conv launch, by TrainRunner._conv's own steps."""
    from drnmi import _lib
    lib = _lib.load()
    sk = 1
    x3 = a.dtype == _lib.DRNMI_F32X3
    if x3 and a.algo == _lib.ALGO_IGEMM and split:
        nb = lib.drnmi_conv_workspace_bytes(ctypes.byref(a))
        if nb > 0:
            a.ws, a.ws_bytes = PTR, nb
            sk = max(1, nb // (4 * a.n * a.ho * a.wo * a.cout))
    if want_stats and x3 and a.algo == _lib.ALGO_IGEMM:
        if lib.drnmi_conv_stats_rows(ctypes.byref(a)) > 0:
            a.stats = PTR
    name = lib.drnmi_conv_kernel_name(ctypes.byref(a))
    return (name.decode() if name else None, sk)


def step_routes(arch: str, precision: str, n: int, h: int, w: int) -> list:
    """Every conv, wgrad and dgrad launch of one fine-tune step at [n, 3, h, w], with the route the
    library's host-only queries give it: [(what, node name, route)], what in fwd / wgrad / dgrad;
    route = (kernel, split-K) or the drnmi_conv_wgrad_plan tuple plus the pixel count.  It follows
    TrainRunner.forward / backward with the module switches at their defaults; the GPU audit checks
    it against the launches the runner really made."""
    from drnmi import _lib
    from drnmi.drnseg import DRNSeg
    from drnmi.engine import COUT_ALIGN, K_ALIGN, X6_PATCH_SHAPES, _conv_out, _pow2_at_least, _round_up
    g = DRNSeg(arch, 19, pretrained=False)._graph
    x3 = precision == "fp32x"
    cstride = {"input": 8}
    for v, c in g.channels.items():
        if v != "input":
            cstride[v] = _pow2_at_least(c)
    shapes = {"input": (h, w)}
    out = []
    for nd in g.nodes:
        c = nd.conv
        ih, iw = shapes[nd.src]
        ks, s, p, d = c.kernel_size[0], c.stride[0], c.padding[0], c.dilation[0]
        oh, ow = _conv_out(ih, ks, s, p, d), _conv_out(iw, ks, s, p, d)
        shapes[nd.dst] = (oh, ow)
        cout, cs = c.out_channels, cstride[nd.src]
        k = ks * ks * cs
        k_pad = _round_up(k, K_ALIGN)
        patch = x3 and not nd.out_fp32_nchw and (cs, cout, ks, s, d) in X6_PATCH_SHAPES
        split = x3 and (patch or (cs >= 32 and k == k_pad))
        ys = (cout * oh * ow, 1, oh * ow) if nd.out_fp32_nchw else (oh * ow * cstride[nd.dst], cstride[nd.dst], 1)
        a = conv_args(split, _lib.ALGO_PATCH if patch else _lib.ALGO_IGEMM, n, ih, iw, cs, oh, ow, cout,
                      _round_up(cout, COUT_ALIGN), ks, s, p, d, k, k_pad, ys)
        out.append(("fwd", nd.name, conv_route(a, want_stats=not nd.out_fp32_nchw)))
    have = set()
    for nd in reversed(g.nodes):
        c = nd.conv
        ih, iw = shapes[nd.src]
        oh, ow = shapes[nd.dst]
        ks, s, p, d = c.kernel_size[0], c.stride[0], c.padding[0], c.dilation[0]
        cout, cin = c.out_channels, c.in_channels
        dys = _pow2_at_least(cout) if nd.out_fp32_nchw else cstride[nd.dst]
        if nd.res:
            have.add(nd.res)
        wa = wgrad_args(n, cin, cstride[nd.src], cout, dys, ks, s, p, d, ih, iw)
        out.append(("wgrad", nd.name, _lib.wgrad_plan(wa, x3) + (n * oh * ow,)))
        if nd.src == "input":
            continue
        cs_src = cstride[nd.src]
        kd = ks * ks * dys
        kd_pad = _round_up(kd, K_ALIGN)
        rows_d = _round_up(cin, COUT_ALIGN)
        dpatch = x3 and (dys, cin, ks, 1, d) in X6_PATCH_SHAPES
        wdx = x3 and (dpatch or (dys >= 32 and kd == kd_pad))
        prev = nd.src in have
        pad_d = d * (ks - 1) - p
        classes = None
        if s == 2 and wdx and not dpatch and d == 1 and dys % 8 == 0 and kd == kd_pad:
            parts = []
            for a_ in (0, 1):
                k0 = (pad_d - a_) % 2
                nh = (ks - k0 + 1) // 2 if k0 < ks else 0
                if nh and (a_ - pad_d + k0) // 2 != 0:
                    parts = None
                    break
                parts.append(nh)
            if parts is not None:
                classes = [(a_, b_, max(parts[a_], parts[b_])) for a_ in (0, 1) for b_ in (0, 1)
                           if parts[a_] and parts[b_]]
        if classes is not None:
            for (a_, b_, ksc) in classes:
                ho_c, wo_c = (ih - a_ + 1) // 2, (iw - b_ + 1) // 2
                if ho_c <= 0 or wo_c <= 0:
                    continue
                a = conv_args(True, _lib.ALGO_IGEMM, n, oh, ow, dys, ho_c, wo_c, cin, rows_d, ksc, 1, 0, 1,
                              ksc * ksc * dys, ksc * ksc * dys, (ih * iw * cs_src, 2 * cs_src, 1), res=prev,
                              y_sr=2 * iw * cs_src)
                out.append(("dgrad", nd.name, conv_route(a, split=False)))
        else:
            hu, wu = (oh, ow) if s == 1 else (ih + 2 * p - d * (ks - 1), iw + 2 * p - d * (ks - 1))
            use_patch = dpatch and not prev
            a = conv_args(bool(wdx and (use_patch or not dpatch)), _lib.ALGO_PATCH if use_patch else _lib.ALGO_IGEMM, n,
                          hu, wu, dys, ih, iw, cin, rows_d, ks, 1, pad_d, d, kd, kd_pad, (ih * iw * cs_src, cs_src, 1),
                          res=prev)
            out.append(("dgrad", nd.name, conv_route(a)))
        have.add(nd.src)
    return out


def recorded_routes(cap: Capture, step: int = 0) -> list:
    """The routes of a captured pass in step_routes' form and order."""
    out = []
    for r in cap.recs:
        if r.step != step:
            continue
        if r.kind == "conv":
            out.append(("fwd", r.name, (r.data["kernel"], r.data["split_k"])))
        elif r.kind == "wgrad":
            m = cap.meta[r.name]
            out.append(("wgrad", r.name, tuple(r.data["plan"]) + (m.n * m.oh * m.ow,)))
        elif r.kind == "dgrad":
            out.append(("dgrad", r.name, (r.data["kernel"], r.data["split_k"])))
    return out


def route_classes(routes: list) -> tuple:
    """(wgrad classes, conv_x6 classes) of a list of routes."""
    wg = {wgrad_class(r[:4], r[4]) for what, _, r in routes if what == "wgrad"}
    cx = {r for what, _, r in routes if what != "wgrad" and r[0] and r[0].startswith("conv_x6_kernel")}
    return wg, cx
