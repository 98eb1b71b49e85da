"""numpy fp32 restatement of the quantisation-aware fine-tuning arithmetic (csrc/qat.hip, DESIGN.md
§3.7b), built on the int8 oracle: one fp32 rounding per step, rint = round half to even.

  fq(x; s)     = fl(float(quantize_i8(x, inv)) * s),   inv = fp32(1 / s) computed in double
  mask(x; s)   = rint(fl(x * inv)) in [-127, 127]      (the level was not clamped)
  fq_bwd       = dq where mask else 0, optionally added into dx with one rounding
  fq_rows(w)   = float(q) * s_row with (q, s_row) = quantize_weight_rows(w)
"""
import numpy as np

from oracle.int8_oracle import quantize_i8, quantize_weight_rows

F32 = np.float32


def scale_pair(s: float):
    """(scale, inv_scale) as the fp32 values the kernels receive from a host double s."""
    return F32(s), F32(1.0 / float(s))


def fq(x: np.ndarray, s: float) -> np.ndarray:
    s32, inv = scale_pair(s)
    return (quantize_i8(np.asarray(x, dtype=F32), inv).astype(F32) * s32).astype(F32)


def mask(x: np.ndarray, s: float) -> np.ndarray:
    _, inv = scale_pair(s)
    with np.errstate(over="ignore"):
        lvl = np.rint(np.asarray(x, dtype=F32) * inv)
    return np.abs(lvl) <= F32(127)


def fq_bwd(dq: np.ndarray, x: np.ndarray, s: float, dx: np.ndarray | None = None) -> np.ndarray:
    g = np.where(mask(x, s), np.asarray(dq, dtype=F32), F32(0)).astype(F32)
    return g if dx is None else (np.asarray(dx, dtype=F32) + g).astype(F32)


def row_codes(w: np.ndarray):
    """(int8 codes, fp32 row scales) of a [rows, cols] weight: the int8 pack's."""
    return quantize_weight_rows(np.asarray(w, dtype=F32))


def fq_rows(w: np.ndarray):
    """(shadow weight fp32 [rows, cols], row scales fp32 [rows])."""
    q, s = row_codes(w)
    return (q.astype(F32) * s[:, None]).astype(F32), s


# ---------------------------------------------------------------------------------------------
# float64 torch-CPU restatement of one fine-tune step of the specified network:
# the model's conv graph with batch-statistics BN, the fixed x8 up-convolution, LogSoftmax and the
# criterion on the log-probs; the convs in `elig` read fq(v) of their input and residual and the
# row-quantised weight, straight-through in the backward.
def net_step(model, x, target, elig=(), scales=None, levels=None, ignore_index=255):
    """Returns (loss, {parameter name: gradient}, {value: tensor NCHW}, level_diffs).

    elig: node indices on the int8 grids; scales {value: s} of the values they read.
    levels {value: integer levels, float64 NCHW}: the level of each element is taken from here (the
    recorded GPU launch: a last-bit difference of the value then cannot move it) while the
    pass-through mask is the restatement's own, |rint(v * inv)| <= 127 on its own v; level_diffs
    counts the elements whose own rounding would have chosen another level.  levels None: its own."""
    import torch
    import torch.nn.functional as F
    g = model._graph
    dt = torch.float64
    named = dict(model.named_parameters())
    leaf = {id(p): p.detach().cpu().to(dt).requires_grad_(True) for k, p in named.items() if not k.startswith("up.")}
    scales = scales or {}
    diffs = {}

    class _STE(torch.autograd.Function):
        @staticmethod
        def forward(ctx, v, lvl, s32, inv):
            own = torch.round(v * inv)
            ctx.save_for_backward(own.abs() <= 127)
            return lvl * s32

        @staticmethod
        def backward(ctx, gq):
            (m,) = ctx.saved_tensors
            return gq * m, None, None, None

    vals = {"input": x.detach().cpu().to(dt)}
    qv = {}
    for i, nd in enumerate(g.nodes):
        c = nd.conv
        rd = qv if i in elig else vals
        w = leaf[id(c.weight)]
        if i in elig:
            w32 = c.weight.detach().cpu().float().numpy()
            wq, _ = fq_rows(w32.reshape(w32.shape[0], -1))
            w = w + (torch.from_numpy(wq.reshape(w32.shape)).to(dt) - w.detach())      # d w = d w_q
        b = leaf[id(c.bias)] if c.bias is not None else None
        y = F.conv2d(rd[nd.src], w, b, c.stride, c.padding, c.dilation)
        if nd.bn is not None:
            y = F.batch_norm(y, None, None, leaf[id(nd.bn.weight)], leaf[id(nd.bn.bias)], True, 0.0, nd.bn.eps)
            if nd.res:
                y = y + rd[nd.res]
            if nd.relu:
                y = torch.relu(y)
        vals[nd.dst] = y
        if nd.dst in scales:
            s32, inv = scale_pair(scales[nd.dst])
            s32, inv = float(s32), float(inv)
            own = torch.round(y.detach() * inv).clamp(-127, 127)
            lvl = own if levels is None else levels[nd.dst]
            diffs[nd.dst] = int((own != lvl).sum())
            qv[nd.dst] = _STE.apply(y, lvl, s32, inv)
    logits = vals[g.nodes[-1].dst]
    up = model.up.weight.detach().cpu().to(dt)
    lp = F.log_softmax(F.conv_transpose2d(logits, up, None, 8, 4, 0, logits.shape[1]), dim=1)
    loss = F.cross_entropy(lp, target.cpu(), ignore_index=ignore_index)
    loss.backward()
    grads = {k: leaf[id(p)].grad for k, p in named.items() if id(p) in leaf and leaf[id(p)].grad is not None}
    return float(loss.detach()), grads, {v: t.detach() for v, t in vals.items()}, diffs
