"""fp32x2 without a GPU: the two-term split / three-product arithmetic restated in numpy against its
derived bound, the C ABI, and conv_x3's host-side routing answers."""
import ctypes

import numpy as np
import pytest
import torch

from drnmi import _lib


def _bf16(a):
    return torch.from_numpy(a).to(torch.bfloat16).float().numpy()


def test_three_product_bound():
    """x1 w2 + x2 w1 + x1 w1 with x1 = bf16(x), x2 = bf16(x - x1).  One product is within 2^-15 |x||w| of x w in
    the worst case (bf16 rounds to 8 bits, so x - x1 - x2 is at most 2^-17 |x| and the dropped x2 w2 at most
    2^-16 |x||w|; measured here: 2.7e-5 = 0.88 x 2^-15), not within 3 * 2^-18; the launch metric of
    tests/test_gpu_fp32x2.py, max |sum - exact| / sum |x||w| over dot products of the shortest K there (288) of
    normal data, is within 3 * 2^-18, because the products' errors carry either sign."""
    rng = np.random.default_rng(0)
    x = rng.standard_normal((4096, 288)).astype(np.float32)
    w = (rng.standard_normal((4096, 288)) / 17).astype(np.float32)
    x1, w1 = _bf16(x), _bf16(w)
    x2, w2 = _bf16(x - x1), _bf16(w - w1)
    got = x1.astype(np.float64) * w2 + x2.astype(np.float64) * w1 + x1.astype(np.float64) * w1
    exact = x.astype(np.float64) * w
    one = (np.abs(got - exact) / np.abs(exact)).max()
    r = (np.abs(got.sum(1) - exact.sum(1)) / np.abs(exact).sum(1)).max()
    print(f"one product {one:.3e} (2^-15 = {2.0 ** -15:.3e}); K = 288 dot products {r:.3e} (3 * 2^-18 = {3 * 2.0 ** -18:.3e})")
    assert 2.0 ** -24 < one <= 2.0 ** -15 and r <= 3 * 2.0 ** -18


def _args(cin, cout, ks, n=2, h=16, w=16, stride=1, dil=1, dtype=None, tile=-1):
    a = _lib.ConvArgs()
    pad = dil * (ks - 1) // 2
    a.n, a.h, a.w, a.cin, a.cout, a.cout_pad = n, h, w, cin, cout, (cout + 127) // 128 * 128
    a.ks, a.stride, a.pad, a.dil, a.k, a.k_pad = ks, stride, pad, dil, ks * ks * cin, ks * ks * cin
    a.ho = (h + 2 * pad - dil * (ks - 1) - 1) // stride + 1
    a.wo = (w + 2 * pad - dil * (ks - 1) - 1) // stride + 1
    a.y_sn, a.y_sp, a.y_sc = a.ho * a.wo * cout, cout, 1
    a.dtype, a.out_dtype, a.tile, a.algo = _lib.DRNMI_F32X2 if dtype is None else dtype, _lib.DRNMI_F32, tile, 0
    return a


@pytest.mark.parametrize("cin,cout,ks,stride,dil,tile,name", [
    (512, 512, 3, 1, 4, -1, "conv_x3_kernel<3, 64, 2, 2, 1>"), (256, 128, 1, 2, 1, -1, "conv_x3_kernel<1, 64, 2, 2, 1>"),
    (32, 48, 3, 1, 1, -1, "conv_x3_kernel<3, 32, 2, 2, 1>"), (512, 19, 1, 1, 1, -1, "conv_x3_kernel<1, 32, 2, 2, 1>"),
    (128, 128, 2, 1, 1, 0, "conv_x3_kernel<2, 64, 2, 2, 2>"), (16, 64, 3, 1, 1, -1, None), (64, 64, 7, 1, 1, -1, None)])
def test_x3_route_answers(cin, cout, ks, stride, dil, tile, name):
    lib = _lib.load()
    a = _args(cin, cout, ks, stride=stride, dil=dil, tile=tile)
    got = lib.drnmi_conv_kernel_name(ctypes.byref(a))
    assert (got.decode() if got else None) == name and (lib.drnmi_conv_status(ctypes.byref(a)) == 0) == (name is not None)
    if name is not None:
        assert lib.drnmi_conv_stats_rows(ctypes.byref(a)) == (a.n * a.ho * a.wo + 127) // 128 * 2
        a.tile = (tile if tile >= 0 else 1) + 3 * 2          # a forced two-way split: sized, and refused without it
        assert lib.drnmi_conv_workspace_bytes(ctypes.byref(a)) == 2 * a.n * a.ho * a.wo * cout * 4 * (cout % 4 == 0)


def test_dtype_code_and_precision():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from drnmi.drnseg import DRNSeg
    from drnmi.roofline import MFMA_PEAK, kernel_peak
    assert _lib.load().drnmi_conv_wgrad_f32x2 is not None
    m = DRNSeg("drn_d_22", 19, pretrained=False).eval().set_precision("fp32x2")
    with FakeTensorMode():                       # the model-handle ops' fake kernels serve an fp32x2 model
        lp, logits = torch.ops.drnmi.forward(torch.empty(1, 3, 64, 96, device="cuda"), m._handle)
        pred = torch.ops.drnmi.predict(torch.empty(1, 3, 64, 96, device="cuda"), m._handle)
    assert lp.shape == (1, 19, 64, 96) and logits.shape == (1, 19, 8, 12) and pred.shape == (1, 64, 96)
    assert _lib.DRNMI_F32X2 == 9 and MFMA_PEAK["fp32x2"] == MFMA_PEAK["bf16"] / 3
    assert kernel_peak("conv_x3_kernel<3, 64, 2, 2, 1>", "fp32x") == MFMA_PEAK["fp32x2"]
    assert DRNSeg("drn_d_22", 19, pretrained=False).set_precision("fp32x2").precision == "fp32x2"
