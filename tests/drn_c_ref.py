"""Test infrastructure: CPU restatement of the reference DRN-C segmentation forward and fine-tune
step, as plain functional torch ops over a state_dict (the arch-C sibling of oracle/drn_oracle.py,
whose _bn / _conv / up_logsoftmax / _TRAIN it shares).

Pinned by tests/golden/drn_c.N.npz (tests/golden/make_drn_c_golden.py runs the reference's own
drn.drn_c_26 / drn_c_42): tests/test_drn_c.py checks max-abs 0 on logits / log-probs and exact labels.

Reference anchors:
  DRN.__init__ arch 'C'   lmodels/drn.py:121-130 (conv1 / bn1 / relu, layer1 / layer2 = BasicBlocks),
                          :144-158 (layer3-6 with the family's block; layer7 / layer8 = BasicBlocks with
                          new_level=False, residual=False, dilation 2 / 1)
  BasicBlock.forward      lmodels/drn.py:49-65 (`if self.residual: out += residual`)
  state_dict keys         layer.0.weight, layer.1.* (bn1), layer.3.* .. layer.10.* (layer1 .. layer8)
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle.drn_oracle import _TRAIN, _bn, _conv, trainable_keys, up_logsoftmax

# (block kind of layer3-6, blocks per layer) -- lmodels/drn.py:340-358
ARCHS = {
    "drn_c_26": ("basic", [1, 1, 2, 2, 2, 2, 1, 1]),
    "drn_c_42": ("basic", [1, 1, 3, 4, 6, 3, 1, 1]),
    "drn_c_58": ("bottleneck", [1, 1, 3, 4, 6, 3, 1, 1]),
}


def basic(sd, p, x, stride, dil, residual=True):
    """BasicBlock.forward (lmodels/drn.py:49-65) with its residual flag."""
    out = F.relu(_bn(sd, p + ".bn1", _conv(sd, p + ".conv1", x, stride, dil[0], dil[0])))
    out = _bn(sd, p + ".bn2", _conv(sd, p + ".conv2", out, 1, dil[1], dil[1]))
    if residual:
        res = x
        if (p + ".downsample.0.weight") in sd:
            res = _bn(sd, p + ".downsample.1", _conv(sd, p + ".downsample.0", x, stride))
        out = out + res
    return F.relu(out)


def bottleneck(sd, p, x, stride, dil, residual=True):
    """Bottleneck.forward (lmodels/drn.py:86-106): always adds the residual."""
    out = F.relu(_bn(sd, p + ".bn1", _conv(sd, p + ".conv1", x)))
    out = F.relu(_bn(sd, p + ".bn2", _conv(sd, p + ".conv2", out, stride, dil[1], dil[1])))
    out = _bn(sd, p + ".bn3", _conv(sd, p + ".conv3", out))
    res = x
    if (p + ".downsample.0.weight") in sd:
        res = _bn(sd, p + ".downsample.1", _conv(sd, p + ".downsample.0", x, stride))
    return F.relu(out + res)


def res_layer(sd, p, x, kind, nblocks, stride, dilation, new_level, residual=True):
    """_make_layer (lmodels/drn.py:177-199)."""
    blk = basic if kind == "basic" else bottleneck
    first = (1, 1) if dilation == 1 else ((dilation // 2) if new_level else dilation, dilation)
    x = blk(sd, f"{p}.0", x, stride, first, residual)
    for b in range(1, nblocks):
        x = blk(sd, f"{p}.{b}", x, 1, (dilation, dilation), residual)
    return x


def backbone(sd, arch, x, prefix="layer"):
    """DRN-C trunk through layer8 (lmodels/drn.py:216-247); returns (x, stages by DRN layer number)."""
    kind, layers = ARCHS[arch]
    stages = {}
    x = F.relu(_bn(sd, f"{prefix}.1", _conv(sd, f"{prefix}.0", x, 1, 3)))
    stages["layer0"] = x
    # (stride, dilation, new_level, block kind, residual) of layer1 .. layer8
    spec = [(1, 1, True, "basic", True), (2, 1, True, "basic", True), (2, 1, True, kind, True),
            (2, 1, True, kind, True), (1, 2, False, kind, True), (1, 4, False, kind, True),
            (1, 2, False, "basic", False), (1, 1, False, "basic", False)]
    idx = 3
    for li, (stride, dil, new_level, k, residual) in enumerate(spec):
        if layers[li] == 0:
            continue
        x = res_layer(sd, f"{prefix}.{idx}", x, k, layers[li], stride, dil, new_level, residual)
        stages[f"layer{li + 1}"] = x
        idx += 1
    return x, stages


@torch.no_grad()
def drnseg_forward(sd, arch, x):
    """(log_probs, logits, stages) of the reference DRNSeg.forward around a DRN-C trunk."""
    sd = {k: v.float() for k, v in sd.items()}
    feat, stages = backbone(sd, arch, x.float())
    logits = _conv(sd, "seg", feat, bias=True)
    return up_logsoftmax(sd, logits), logits, stages


def drnseg_train_steps(sd, arch, inputs, targets, lr=0.01, momentum=0.9, weight_decay=1e-4,
                       masks=None, ignore_index=255, dtype=torch.float32):
    """oracle.drn_oracle.drnseg_train_steps on the arch-C trunk: train-mode forward,
    CrossEntropyLoss(ignore_index) on the log-probs, SGD(momentum, weight_decay) step, masks.
    Returns (losses, grads of the LAST step, final state_dict); sd is not modified.  Parameters the
    forward never reads (the unused downsample of a residual=False block) get no gradient and are
    left out of the optimiser, as autograd leaves their .grad None in the reference loop."""
    sd = {k: v.detach().clone() for k, v in sd.items()}
    for k, v in sd.items():
        if v.is_floating_point():
            sd[k] = v.to(dtype)
    keys = trainable_keys(sd)
    params = [sd[k].requires_grad_(True) for k in keys]
    opt = torch.optim.SGD(params, lr, momentum=momentum, weight_decay=weight_decay)
    losses, grads = [], {}
    _TRAIN["on"] = True
    try:
        for x, t in zip(inputs, targets):
            feat, _ = backbone(sd, arch, x.to(dtype))
            logits = _conv(sd, "seg", feat, bias=True)
            lp = up_logsoftmax(sd, logits)
            loss = F.cross_entropy(lp, t.long(), ignore_index=ignore_index)
            opt.zero_grad()
            loss.backward()
            grads = {k: sd[k].grad.detach().clone() for k in keys if sd[k].grad is not None}
            opt.step()
            if masks:
                with torch.no_grad():
                    for k, m in masks.items():
                        sd[k].mul_(m.to(dtype))
            losses.append(float(loss.detach()))
    finally:
        _TRAIN["on"] = False
    out = {k: v.detach().clone() for k, v in sd.items()}
    return losses, grads, out
