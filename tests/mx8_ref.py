"""CPU restatement of the block-scaled e4m3 format of include/drnmi.h (DRNMI_MXF8), on torch: blocks of 32 along the
last axis, the shared exponent from amax's bits, e4m3(v * 2^-E) elements (fp8_ref.e4m3), and a float64 conv over the
dequantised operands in the style of fp8_ref.conv_f8."""
from __future__ import annotations

import torch
import torch.nn.functional as F

import fp8_ref as R


def scale_byte(amax: torch.Tensor) -> torch.Tensor:
    """fp32 amax -> the stored scale byte (int32 tensor)."""
    bits = amax.to(torch.float32).contiguous().view(torch.int32)
    return ((bits >> 23) - 8 + ((bits & 0x7FFFFF) > 0x600000).to(torch.int32)).clamp(0, 254)


def quantize(x: torch.Tensor):
    """bf16 / fp32 [..., c] -> (e4m3 bytes [..., c], scale bytes [..., c / 32])."""
    x = x.to(torch.float32)
    xb = x.reshape(*x.shape[:-1], x.shape[-1] // 32, 32)
    byte = scale_byte(xb.abs().amax(-1))
    inv = ((254 - byte) << 23).view(torch.float32)            # 2^-E
    return R.e4m3(xb * inv[..., None]).reshape(x.shape), byte.to(torch.uint8)


def dequant(q: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """(e4m3 bytes [..., c], scale bytes [..., c / 32]) -> float64 values."""
    v = R.dequant(q).reshape(*s.shape, 32) * torch.exp2(s.to(torch.float64) - 127)[..., None]
    return v.reshape(q.shape)


def conv_mx(x, w, scale, shift, cout, ks, pad, dil, relu, res=None):
    """One DRNMI_MXF8 launch.  x: fp32 / bf16 [n][h][w][cin] and w: fp32 [cout_pad][ks*ks*cin] before
    quantisation, k = (kh*ks + kw)*cin + ci; res: [n][ho][wo][cout] before quantisation, or None.
    Returns float64 NHWC tensors acc, sumabs, v, mag and scale as fp8_ref.conv_f8 does."""
    cin = x.shape[-1]
    xd = dequant(*quantize(x)).permute(0, 3, 1, 2)
    wd = dequant(*quantize(w[:cout])).view(cout, ks, ks, cin).permute(0, 3, 1, 2)
    acc = F.conv2d(xd, wd, None, 1, pad, dil).permute(0, 2, 3, 1).contiguous()
    sumabs = F.conv2d(xd.abs(), wd.abs(), None, 1, pad, dil).permute(0, 2, 3, 1).contiguous()
    sc, sh = scale[:cout].to(torch.float64), shift[:cout].to(torch.float64)
    v, mag = acc * sc + sh, (acc * sc).abs() + sh.abs()
    if res is not None:
        r = dequant(*quantize(res))
        v, mag = v + r, mag + r.abs()
    if relu:
        v = v.clamp_min(0.0)
    return {"acc": acc, "sumabs": sumabs, "v": v, "mag": mag, "scale": sc}
