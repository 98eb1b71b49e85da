"""CPU restatement of the fp8 (OCP e4m3) arithmetic of include/drnmi.h (DRNMI_F8), on torch.

  element      e4m3(v) = v.clamp(-448, 448).to(torch.float8_e4m3fn)        (bytes: .view(torch.uint8))
  quantiser    e4m3(x * inv_scale), the product one fp32 multiply
  conv         sum of the exact products of the dequantised operands, in float64 (a product of two
               e4m3 values has 8 significant bits and at most 9 x 1024 of them are added: float64
               holds every partial sum of the cases here to far below one fp32 ulp)
  epilogue     v = acc * scale[co] + shift[co]; v += f32(res) * res_scale; ReLU; then e4m3(v *
               out_scale), bf16(v) or v

The kernels run the epilogue in fp32 (one rounding per step) on an fp32 accumulator whose summation
order the hardware fixes; this file evaluates the same expression without intermediate rounding and
returns, next to it, the terms that bound the difference (conv_f8: `sumabs`, `mag`; tolerance()).
It reads a PackedNet's own nodes, scales and a Plan's own buffers (node_case), so it needs no second
model description.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

F8_MAX = 448.0
F8 = torch.float8_e4m3fn


def e4m3(v: torch.Tensor) -> torch.Tensor:
    """Values -> e4m3 bytes (uint8 tensor): clamp to +-448, then round to nearest even."""
    return v.to(torch.float32).clamp(-F8_MAX, F8_MAX).to(F8).view(torch.uint8)


def dequant(b: torch.Tensor) -> torch.Tensor:
    """e4m3 bytes -> float64 values."""
    return b.contiguous().view(F8).to(torch.float64)


def quantize(x: torch.Tensor, inv_scale: float) -> torch.Tensor:
    """drnmi_quantize_f8: bf16 / fp32 values -> e4m3 bytes of x * inv_scale (one fp32 multiply)."""
    return e4m3(x.to(torch.float32) * torch.tensor(inv_scale, dtype=torch.float32))


def e4m3_bytes_np(v) -> np.ndarray:
    """The same conversion spelled out in numpy (no torch float8): finite float32 values -> bytes.
    Normal numbers 2^e * (1 + m / 8), e = -6 .. 8 (448 = 2^8 * 1.75 is the largest; the pattern
    e = 8, m = 7 is NaN), subnormals m * 2^-9; round to nearest, ties to even."""
    v = np.clip(np.asarray(v, dtype=np.float32), -F8_MAX, F8_MAX)
    neg = np.signbit(v)
    a = np.abs(v).astype(np.float64)
    e = np.clip(np.floor(np.log2(np.maximum(a, 2.0 ** -30))), -6, 8)
    val = np.rint(a / 2.0 ** (e - 3)) * 2.0 ** (e - 3)           # np.rint: ties to even; the scaling is exact
    e2 = np.clip(np.floor(np.log2(np.maximum(val, 2.0 ** -30))), -6, 8)   # a mantissa that rounded up to 16
    normal = val >= 2.0 ** -6
    mant = np.where(normal, val / 2.0 ** e2 * 8 - 8, val * 2.0 ** 9)
    byte = np.where(normal, (e2 + 7) * 8 + mant, mant).astype(np.uint8)
    return byte | (neg.astype(np.uint8) << 7)


def pack_weights(full: torch.Tensor):
    """PackedNet._pack_q8's weight side for e4m3: fp32 [rows][k] -> (e4m3 bytes, s_w)."""
    a = full.abs().amax(dim=1)
    pos = a > 0
    inv = torch.where(pos, F8_MAX / torch.where(pos, a, torch.ones_like(a)), torch.ones_like(a))
    return e4m3(full * inv[:, None]), torch.where(pos, a / F8_MAX, torch.ones_like(a))


def conv_f8(x, wpk, scale, shift, cout, ks, stride, pad, dil, relu, res=None, res_scale=0.0, out_scale=0.0):
    """One DRNMI_F8 launch.  x: e4m3 bytes [n][h][w][cin]; wpk: e4m3 bytes [cout_pad][ks*ks*cin], k =
    (kh*ks + kw)*cin + ci; scale, shift: fp32 [cout_pad]; res: e4m3 bytes [n][ho][wo][cout] or None.
    Returns float64 NHWC tensors [n][ho][wo][cout]:
      acc     the exact sum of products,   sumabs   sum |a * b| over the same terms,
      v       the epilogue's value before the store (after ReLU),
      vq      v * out_scale (what an fp8 output converts; only with out_scale),
      mag     |acc * scale| + |shift| + |res * res_scale|: every intermediate of the fp32 epilogue is
              at most this large."""
    n, h, w, cin = x.shape
    xd = dequant(x).permute(0, 3, 1, 2)
    wd = dequant(wpk[:cout]).view(cout, ks, ks, cin).permute(0, 3, 1, 2)
    acc = F.conv2d(xd, wd, None, stride, pad, dil).permute(0, 2, 3, 1).contiguous()
    sumabs = F.conv2d(xd.abs(), wd.abs(), None, stride, pad, dil).permute(0, 2, 3, 1).contiguous()
    sc = scale[:cout].to(torch.float64)
    sh = shift[:cout].to(torch.float64)
    v = acc * sc + sh
    mag = (acc * sc).abs() + sh.abs()
    if res is not None:
        r = dequant(res) * float(np.float32(res_scale))
        v = v + r
        mag = mag + r.abs()
    if relu:
        v = v.clamp_min(0.0)
    out = {"acc": acc, "sumabs": sumabs, "v": v, "mag": mag, "scale": sc}
    if out_scale:
        out["vq"] = v * float(np.float32(out_scale))
    return out


def tolerance(ref: dict, c: float, out: str, out_scale: float = 0.0) -> torch.Tensor:
    """Bound on |kernel - ref["v"]| (out "f32" / "bf16") or on |kernel's pre-conversion value -
    ref["vq"]| (out "f8"):  c * scale[co] * sum|a b|  for the accumulator (c: the measured constant of
    the MFMA's fp32 summation, tests/test_gpu_fp8.py ACC_C), plus the fp32 epilogue's own roundings
    -- fmul, fadd, the residual's fmul and fadd, the output scaling: five steps of at most 2^-24
    relative to an intermediate no larger than `mag` -- plus, for bf16, the store's rounding (half an
    ulp: 2^-9 of the value, taken at |v| + the rest of the bound)."""
    t = c * ref["scale"].abs() * ref["sumabs"] + 5 * 2.0 ** -24 * ref["mag"]
    if out == "f8":
        return t * abs(float(np.float32(out_scale)))
    if out == "bf16":
        t = t + 2.0 ** -8 * (ref["v"].abs() + t)
    return t


def f8_interval(ref: dict, tol: torch.Tensor):
    """Rounding is monotone: a kernel whose pre-conversion value is within tol of vq stores a byte
    whose value lies in [e4m3(vq - tol), e4m3(vq + tol)].  Returns the two bounds as float64 values."""
    return dequant(e4m3(ref["vq"] - tol)), dequant(e4m3(ref["vq"] + tol))


def node_case(plan, nd):
    """The launch of PackedNet node `nd` as conv_f8 arguments, read from the plan's own buffers (a
    keep_all plan after run_backbone) and the node's packed tensors.  Returns (kwargs, out kind)."""
    from drnmi import _lib as L
    pk = plan.packed
    c = nd.conv
    n = plan.n
    ih, iw = plan.shapes[nd.src]
    oh, ow = plan.shapes[nd.dst]
    x = plan.bufs[nd.x_val].cpu().view(n, ih, iw, pk.cstride[nd.src])
    res = plan.bufs[nd.r_val].cpu().view(n, oh, ow, c.out_channels) if nd.r_val else None
    code = pk.value_code(nd.dst)
    out = "f32" if nd.out_fp32_nchw else "f8" if code == L.DRNMI_F8 else "bf16"
    kw = dict(x=x, wpk=nd.wpk.cpu(), scale=nd.scale.cpu(), shift=nd.shift.cpu(), cout=c.out_channels,
              ks=c.kernel_size[0], stride=c.stride[0], pad=c.padding[0], dil=c.dilation[0], relu=nd.relu,
              res=res, res_scale=nd.res_scale, out_scale=nd.out_scale)
    return kw, out
