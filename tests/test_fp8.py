"""fp8 (OCP e4m3, include/drnmi.h DRNMI_F8) without a GPU: the API surface, the quantiser's argument
checks, the routing of fp8 launches, tests/fp8_ref.py's conversion and the reuse of the int8
activation scales by the fp8 pack."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import fp8_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from drnmi import _lib
    return _lib, _lib.load()


def test_api_surface():
    from drnmi.drnseg import DRNSeg
    L, lib = _lib()
    m = DRNSeg("drn_d_22", 19, pretrained=False)
    assert m.set_precision("fp8") is m and m.precision == "fp8"
    assert L.DRNMI_F8 == 6
    with open(os.path.join(REPO, "include", "drnmi.h")) as f:
        text = f.read()
    header = int(re.search(r"#define DRNMI_ABI_VERSION (\d+)", text).group(1))
    assert header == L.ABI_VERSION == lib.drnmi_abi_version()
    assert re.search(r"DRNMI_F8 = 6\b", text)
    with pytest.raises(ValueError):
        m.set_precision("fp4")


def test_drn_c_refuses_fp8_like_int8():
    from drnmi.drnseg import DRNSeg
    m = DRNSeg("drn_c_26", 19, pretrained=False)
    for prec in ("int8", "fp8"):
        with pytest.raises(NotImplementedError, match=f"precision '{prec}' covers the DRN-D family only"):
            m.set_precision(prec)


def test_quantize_f8_rejects_bad_args():
    """NULL pointers, n <= 0 and other dtypes are refused before any HIP call (no device needed)."""
    L, lib = _lib()
    x = np.zeros(64, np.float32)
    y = np.zeros(64, np.uint8)
    xp, yp = x.ctypes.data, y.ctypes.data
    xp, yp = xp + (-xp % 16), yp + (-yp % 16)        # (16-byte aligned addresses inside the arrays)
    assert lib.drnmi_quantize_f8(None, L.DRNMI_F32, 16, 1.0, yp, None) == -1
    assert lib.drnmi_quantize_f8(xp, L.DRNMI_F32, 16, 1.0, None, None) == -1
    assert lib.drnmi_quantize_f8(xp, L.DRNMI_F32, 0, 1.0, yp, None) == -1
    assert lib.drnmi_quantize_f8(xp, L.DRNMI_F32, -16, 1.0, yp, None) == -1
    for code in (L.DRNMI_U8, L.DRNMI_I64, L.DRNMI_I8, L.DRNMI_F32X3, L.DRNMI_F8):
        assert lib.drnmi_quantize_f8(xp, code, 16, 1.0, yp, None) == -1
    assert lib.drnmi_quantize_f8(xp, L.DRNMI_F32, 16, 0.0, yp, None) == -1
    assert lib.drnmi_quantize_f8(xp + 4, L.DRNMI_F32, 16, 1.0, yp, None) == -1


def _args(L, cin=512, cout=512, ks=3, dil=2, wo=256, ho=4, out=None, tile=-1):
    a = L.ConvArgs()
    a.scale = 1                                      # routing reads the pointers only for presence
    pad = dil * (ks // 2)
    a.n, a.h, a.w, a.cin, a.ho, a.wo, a.cout, a.cout_pad = 1, ho, wo, cin, ho, wo, cout, (cout + 127) // 128 * 128
    a.ks, a.stride, a.pad, a.dil, a.k, a.k_pad = ks, 1, pad, dil, ks * ks * cin, ks * ks * cin
    a.dtype, a.out_dtype, a.tile, a.algo = L.DRNMI_F8, L.DRNMI_F8 if out is None else out, tile, L.ALGO_IGEMM
    a.y_sn, a.y_sp, a.y_sc = ho * wo * cout, cout, 1
    return a


def test_routing_names_the_fp8_kernels():
    L, lib = _lib()

    def name(**kw):
        a = _args(L, **kw)
        nm = lib.drnmi_conv_kernel_name(ctypes.byref(a))
        assert (nm is None) == (lib.drnmi_conv_status(ctypes.byref(a)) != 0)
        return None if nm is None else nm.decode()
    assert name(wo=256) == "conv_f8_stag_kernel"
    assert name(wo=256, tile=L.TILE_STAG) == "conv_f8_stag_kernel"
    assert name(wo=24).startswith("conv_f8_kernel<3, 128, 2, 2, 128>")
    assert name(wo=24, ks=1, dil=1).startswith("conv_f8_occ2_kernel<1, 128, 1, 2, 64>")   # 1x1: two workgroups per CU
    assert name(wo=24, cin=64, cout=128).startswith("conv_f8_kernel<3, 128, 1, 4, 64>")
    for out in (L.DRNMI_BF16, L.DRNMI_F32):
        assert name(wo=256, out=out) == "conv_f8_stag_kernel"
    # nothing: cin 32, no scale, the one-wave-per-SIMD tiles, an int8 output, a strip tile off whole rows
    assert name(wo=256, cin=32) is None
    for tile in (L.TILE_W1, L.TILE_W1H):
        assert name(wo=256, tile=tile) is None
        assert name(wo=24, tile=tile) is None
    assert name(wo=256, out=L.DRNMI_I8) is None
    assert name(wo=24, tile=L.TILE_STAG) is None
    a = _args(L)
    a.scale = None
    assert lib.drnmi_conv_kernel_name(ctypes.byref(a)) is None and lib.drnmi_conv_status(ctypes.byref(a)) == -2
    # the seg-fused launch has no fp8 form either
    assert lib.drnmi_conv_stag_seg_kernel_name(ctypes.byref(_args(L))) is None
    # and the int8 and bf16 routes of the same geometry are what they were
    for dtype, want in ((L.DRNMI_I8, "conv_i8_stag_kernel"), (L.DRNMI_BF16, "conv_stag_kernel")):
        a = _args(L)
        a.dtype = a.out_dtype = dtype
        assert lib.drnmi_conv_kernel_name(ctypes.byref(a)).decode() == want


def _finite_bf16():
    bits = np.arange(1 << 16, dtype=np.uint16)
    x = torch.from_numpy(bits.view(np.int16).copy()).view(torch.bfloat16)
    return x[torch.isfinite(x.float())]


@pytest.mark.parametrize("scale", [1.0, 0.37, 2.0 ** -5])
def test_ref_quantise_matches_spelled_out_conversion(scale):
    """fp8_ref.quantize (torch's float8_e4m3fn after the clamp) against the numpy restatement of the
    format on every finite bf16 value: the saturation (1000 -> 448, not NaN), the subnormals, the ties."""
    x = _finite_bf16()
    inv = float(np.float32(1.0 / scale))
    got = R.quantize(x, inv).numpy()
    prod = (x.float() * torch.tensor(inv, dtype=torch.float32)).numpy()
    want = R.e4m3_bytes_np(prod)
    np.testing.assert_array_equal(got, want)
    assert got.max() <= 0xFE and not np.any((got & 0x7F) == 0x7F), "no NaN pattern from a finite value"
    assert R.quantize(torch.tensor([1000.0, -1e30, 448.0, 0.0]), 1.0).tolist() == [0x7E, 0xFE, 0x7E, 0x00]
    # without the clamp, values past the last rounding interval of 448 convert to NaN: the clamp is
    # part of the arithmetic
    assert torch.tensor([1000.0]).to(torch.float8_e4m3fn).view(torch.uint8).item() == 0x7F
    back = R.dequant(torch.from_numpy(got)).numpy()
    ok = np.abs(prod) <= 448
    assert np.all(np.abs(back[ok] - prod[ok].astype(np.float64)) <= np.maximum(np.abs(prod[ok]) * 2.0 ** -4, 2.0 ** -10))


def _state(m, seed=0):
    rng = np.random.default_rng(seed)
    return {"version": 1, "method": "absmax", "percentile": None,
            "scales": {v: float(rng.uniform(0.01, 0.2)) for v in m._int8_values()}}


def test_fp8_pack_reuses_the_int8_scales():
    from drnmi import _lib as L
    from drnmi.drnseg import DRNSeg
    from drnmi.engine import PackedNet, _fold_bn
    from drnmi.weights import synth_state_dict
    m = DRNSeg("drn_d_22", 19, pretrained=False)
    m.load_state_dict(synth_state_dict(m, 0))
    m.eval().load_int8_state(_state(m))
    s = m._act_scales
    cpu = torch.device("cpu")
    p8 = PackedNet(m._graph, "fp8", cpu, block_sparse=False, act_scales=s)
    pi = PackedNet(m._graph, "int8", cpu, block_sparse=False, act_scales=s)
    assert p8.i8_nodes == pi.i8_nodes and len(p8.i8_nodes) >= 10
    assert p8.quant_after == pi.quant_after
    assert {v for v, c in p8.vcode.items() if c == L.DRNMI_F8} == {v for v, c in pi.vcode.items() if c == L.DRNMI_I8}
    assert p8.value_code("q:v7") == L.DRNMI_F8 and pi.value_code("q:v7") == L.DRNMI_I8
    for i, (n8, ni) in enumerate(zip(p8.graph.nodes, pi.graph.nodes)):
        assert n8.i8 == ni.i8 == (i in p8.i8_nodes)
        assert (n8.x_val, n8.r_val) == (ni.x_val, ni.r_val)
        if not n8.i8:
            assert torch.equal(n8.wpk, ni.wpk) and n8.wpk.dtype == torch.bfloat16
            continue
        cout = n8.conv.out_channels
        w = n8.conv.weight.detach().float()
        full = torch.zeros(n8.cout_pad, n8.k_pad)
        wp = torch.zeros(cout, w.shape[2], w.shape[3], n8.cin_stride)
        wp[..., :w.shape[1]] = w.permute(0, 2, 3, 1)
        full[:cout, :n8.k] = wp.reshape(cout, n8.k)
        q, sw = R.pack_weights(full)
        assert n8.wpk.dtype == torch.uint8 and torch.equal(n8.wpk, q)
        # the same pack in int8 (oracle/int8_oracle.py quantize_weight_rows in torch's fp32 arithmetic)
        a = full.abs().amax(dim=1)
        one = torch.ones_like(a)
        qi = torch.round(full * torch.where(a > 0, 127.0 / torch.where(a > 0, a, one), one)[:, None]).clamp(-127, 127)
        swi = torch.where(a > 0, a / 127.0, one)
        assert ni.wpk.dtype == torch.int8 and torch.equal(ni.wpk, qi.to(torch.int8))
        bn = torch.ones(n8.cout_pad)
        if n8.bn is not None:
            bn[:cout] = _fold_bn(n8.bn)[0]
        s8 = s[n8.src] * 127.0 / 448.0
        assert torch.equal(n8.scale, (sw * s8 * bn).float())
        assert torch.equal(ni.scale, (swi * s[n8.src] * bn).float())
        if n8.res:
            assert n8.res_scale == s[n8.res] * 127.0 / 448.0 and ni.res_scale == s[n8.res]
        if n8.out_scale:
            assert n8.out_scale == 1.0 / (s[n8.dst] * 127.0 / 448.0) and ni.out_scale == 1.0 / s[n8.dst]
        # every weight row uses the format's full range, and dequantises to within half a step
        deq = R.dequant(n8.wpk[:cout]).float() * sw[:cout, None]
        assert float(R.dequant(n8.wpk[:cout]).abs().amax(dim=1).min()) == 448.0
        assert float((deq - full[:cout]).abs().max()) <= float(full.abs().max()) * 2.0 ** -4


def test_fp8_needs_scales_like_int8():
    from drnmi.drnseg import DRNSeg
    from drnmi.engine import PackedNet
    m = DRNSeg("drn_d_22", 19, pretrained=False).eval()
    for prec in ("int8", "fp8"):
        with pytest.raises(RuntimeError, match=f"{prec}: no calibrated activation scale"):
            PackedNet(m._graph, prec, torch.device("cpu"), block_sparse=False, act_scales=None)


def test_roofline_prices_fp8_at_the_8bit_peak():
    from drnmi import roofline
    assert roofline.kernel_peak("conv_f8_stag_kernel", "bf16") == roofline.MFMA_PEAK["int8"]
    assert roofline.kernel_peak("conv_f8_kernel<3, 128, 2, 2, 128>", "bf16") == roofline.MFMA_PEAK["int8"]
    assert roofline.kernel_peak("conv_stag_kernel", "bf16") == roofline.MFMA_PEAK["bf16"]
