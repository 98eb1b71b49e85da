"""mxfp8 (block-scaled e4m3 on v_mfma_scale_f32_16x16x128_f8f6f4; include/drnmi.h DRNMI_MXF8) on the GPU,
against tests/mx8_ref.py: the quantiser bit for bit, conv_mx_kernel within the project's fp8 accumulation
bound for every output form, and a D-22 end to end with no calibration."""
import ctypes
import itertools

import pytest
import torch

import fp8_ref as R
import mx8_ref as MX
from test_gpu_fp8 import ACC_C, FP8_AGREE

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _lib():
    from drnmi import _lib
    return _lib, _lib.load()


def _stream():
    return ctypes.c_void_p(_lib()[0].stream_ptr(torch.device(DEV)))


def _image(x):
    """drnmi_quantize_mx8 of a [..., c] tensor on the GPU -> the image, with a guard behind it."""
    L, lib = _lib()
    c, m = x.shape[-1], x.numel() // x.shape[-1]
    nbytes = lib.drnmi_mx8_image_bytes(m, c)
    img = torch.full((nbytes + 16,), 0xA5, dtype=torch.uint8, device=DEV)
    code = L.DRNMI_BF16 if x.dtype == torch.bfloat16 else L.DRNMI_F32
    L.check(lib.drnmi_quantize_mx8(x.contiguous().data_ptr(), code, m, c, img.data_ptr(), _stream()), "quantize_mx8")
    torch.cuda.synchronize()
    assert bool((img[nbytes:] == 0xA5).all()), "wrote past the image"
    return img


def _values(img, shape):
    L, lib = _lib()
    y, c = torch.empty(shape, dtype=torch.float32, device=DEV), shape[-1]
    L.check(lib.drnmi_dequantize_mx8(img.data_ptr(), y.numel() // c, c, y.data_ptr(), _stream()), "dequantize_mx8")
    torch.cuda.synchronize()
    return y.cpu()


def _data(rows: int, c: int, seed: int) -> torch.Tensor:
    """Normal values times a power of two that differs per block and per row / pixel: 2^((block + 3 row) % 7 - 3)."""
    e = (torch.arange(c // 32)[None, :] + 3 * torch.arange(rows)[:, None]) % 7 - 3
    x = torch.randn(rows, c // 32, 32, generator=torch.Generator().manual_seed(seed)) * torch.exp2(e.float())[..., None]
    return x.reshape(rows, c)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("m,c", [(1, 128), (37, 128), (1, 512), (37, 512)])
def test_quantiser_bit_for_bit(dtype, m, c):
    x = _data(m, c, 3).to(dtype).reshape(m, c // 32, 32)
    ints = torch.int16 if dtype == torch.bfloat16 else torch.int32
    for b in range(c // 32):
        for r in range(m):
            kind = (b + r) % 4
            if kind == 1:
                x[r, b] = 0                                       # an all-zero block
            elif kind >= 2:                                       # amax exactly 1.75 * 2^e, and one ulp above it
                top = torch.tensor([1.75 * 2.0 ** ((b + r) % 5 - 2)], dtype=dtype)
                blk = x[r, b].float()
                x[r, b] = (blk / blk.abs().max() * 0.5 * top.float()).to(dtype)      # the rest of the block stays below
                x[r, b, (b + r) % 32] = -top if r % 2 else (top.view(ints) + (kind - 2)).view(dtype)
    x = x.reshape(m, c)
    got = _values(_image(x.to(DEV)), (m, c))
    q, s = MX.quantize(x)
    want = MX.dequant(q, s).float()
    assert int(s.min()) == 0 and int(s.max()) < 255
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


# (ks, cin, cout, dil, (n, h, w), residual + ReLU): 1 / 2 K steps per tap and channel tiles, a ragged tile, a tile over two images
CONV_CASES = [(ks, cin, cout, dil, nhw, rr)
              for ks, cin, cout, nhw, rr in itertools.product((1, 3), (128, 256), (128, 256), ((1, 9, 13), (2, 16, 16)), (False, True))
              for dil in ((1, 2, 4) if ks == 3 else (1,))]


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "k{}_{}to{}_d{}_{}x{}x{}_{}".format(*c[:4], *c[4], "res" if c[5] else "plain"))
def test_conv_mx_against_reference(case):
    L, lib = _lib()
    ks, cin, cout, dil, (n, h, w), rr = case
    pad, k, M = dil * (ks // 2), ks * ks * cin, n * h * w
    x = _data(M, cin, 11).to(torch.bfloat16).view(n, h, w, cin)
    wgt = _data(cout, k, 12) * 0.05
    res = _data(M, cout, 13).to(torch.bfloat16).view(n, h, w, cout) if rr else None
    g = torch.Generator().manual_seed(14)
    scale, shift = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    ref = MX.conv_mx(x, wgt, scale, shift, cout, ks, pad, dil, rr, res)
    tol = R.tolerance(ref, ACC_C, "f32")

    blob = torch.empty(lib.drnmi_mx8_pack_bytes(cout, k), dtype=torch.uint8)
    L.check(lib.drnmi_mx8_pack(wgt.contiguous().data_ptr(), cout, k, blob.data_ptr(), blob.numel()), "mx8_pack")
    blob, xi, ri = blob.to(DEV), _image(x.to(DEV)), _image(res.to(DEV)) if rr else None
    sc, sh = scale.to(DEV), shift.to(DEV)
    a = L.ConvArgs()
    a.x, a.wgt, a.scale, a.shift, a.res = xi.data_ptr(), blob.data_ptr(), sc.data_ptr(), sh.data_ptr(), ri.data_ptr() if rr else None
    a.n, a.h, a.w, a.cin, a.ho, a.wo, a.cout, a.cout_pad = n, h, w, cin, h, w, cout, cout
    a.ks, a.stride, a.pad, a.dil, a.k, a.k_pad, a.relu = ks, 1, pad, dil, k, k, int(rr)
    a.dtype, a.tile, a.algo = L.DRNMI_MXF8, -1, L.ALGO_IGEMM
    a.y_sn, a.y_sp, a.y_sc = h * w * cout, cout, 1
    for out, td in (("f32", torch.float32), ("bf16", torch.bfloat16), ("mx", torch.uint8)):
        nbytes = lib.drnmi_mx8_image_bytes(M, cout) if out == "mx" else M * cout
        y = torch.full((nbytes + 16,), 0xA5 if out == "mx" else 7, dtype=td, device=DEV)
        a.y, a.out_dtype = y.data_ptr(), {"f32": L.DRNMI_F32, "bf16": L.DRNMI_BF16, "mx": L.DRNMI_MXF8}[out]
        L.check(lib.drnmi_conv2d_bn_act(ctypes.byref(a), _stream()), f"conv {out}")
        torch.cuda.synchronize()
        assert bool((y[nbytes:] == (0xA5 if out == "mx" else 7)).all()), "wrote past the output"
        if out == "mx":
            got = _values(y, (n, h, w, cout)).double()
            # half an e4m3 step (2^-4 relative, subnormal 2^(E' - 10)) at the largest shared exponent E' within tol of the amax
            blk = (ref["v"].abs() + tol).view(n, h, w, cout // 32, 32).amax(-1)
            e_max = MX.scale_byte(blk.float()).double() - 127
            step = torch.exp2(e_max - 10)[..., None].expand(n, h, w, cout // 32, 32).reshape(n, h, w, cout)
            bound = tol + torch.maximum(2.0 ** -4 * (ref["v"].abs() + tol), step)
        else:
            got = y[:M * cout].view(n, h, w, cout).double().cpu()
            bound = R.tolerance(ref, ACC_C, out)
        err = (got - ref["v"]).abs()
        print(f"{out}: max |err| {float(err.max()):.3e}, max err / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= bound).all()), out


def test_d22_end_to_end_without_calibration(golden_forward):
    from drnmi.drnseg import build
    from oracle import drn_oracle as O
    case = "d22_2x128x256"
    m = build("drn_d_22", 19, seed=int(golden_forward[case + "/meta"][0]), device=DEV).set_precision("mxfp8")
    frames = torch.from_numpy(golden_forward[case + "/frames"]).to(DEV)
    seg = m.segment(frames)                              # no calibrate_int8, no loaded state
    assert m._act_scales is None
    assert m.plan(*frames.shape[:3]).labels_path() == "nhwc"
    pred = m.predict(O.preprocess_u8(frames.cpu().numpy()).to(DEV))
    same = float((seg.long() == pred).float().mean())
    agree = float((seg.long().cpu().numpy() == golden_forward[case + "/labels"]).mean())
    print(f"mxfp8: segment() == predict() {same:.4f}, label agreement with the reference fp32 forward {agree:.4f}")
    assert same >= 0.90 and agree >= FP8_AGREE
    out, s = torch.empty_like(seg), torch.cuda.Stream()
    with torch.cuda.stream(s):
        m.segment(frames, labels=out)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            m.segment(frames, labels=out)
    for _ in range(3):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, seg)
