"""The split-K conv's host side (include/drnmi.h drnmi_conv_splitk*) and DRNSeg.set_low_latency without a GPU."""
import ctypes
import os
import re

import pytest

from drnmi import _lib as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["drnmi_conv_splitk", "drnmi_conv_splitk_status", "drnmi_conv_splitk_auto",
           "drnmi_conv_splitk_workspace_bytes", "drnmi_conv_splitk_kernel_name"]
CUS = 256                 # what the auto rule assumes without a device


def _args(n, h, w, cin, cout, ks, stride, dil):
    a = L.ConvArgs()
    pad = dil * (ks // 2)
    a.n, a.h, a.w, a.cin, a.cout, a.cout_pad = n, h, w, cin, cout, (cout + 127) // 128 * 128
    a.ho = (h + 2 * pad - dil * (ks - 1) - 1) // stride + 1
    a.wo = (w + 2 * pad - dil * (ks - 1) - 1) // stride + 1
    a.ks, a.stride, a.pad, a.dil, a.k, a.k_pad = ks, stride, pad, dil, ks * ks * cin, ks * ks * cin
    a.dtype, a.out_dtype, a.tile, a.algo = L.DRNMI_BF16, L.DRNMI_BF16, -1, L.ALGO_IGEMM
    a.y_sn, a.y_sp, a.y_sc = a.ho * a.wo * cout, cout, 1
    return a


def test_header_binding_and_library_agree():
    lib = L.load()
    header = open(os.path.join(REPO, "include", "drnmi.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\b%s\(" % name, header) and name in L.SIGNATURES and getattr(lib, name) is not None
    assert int(re.search(r"#define DRNMI_SPLITK_MAX (\d+)", header).group(1)) == 16
    assert lib.drnmi_abi_version() == L.ABI_VERSION


@pytest.mark.parametrize("shape", [(1, 38, 38, 512, 512, 3, 1, 2), (2, 9, 13, 128, 128, 3, 1, 1), (1, 16, 16, 64, 128, 1, 2, 1),
                                   (1, 9, 17, 2048, 512, 1, 1, 1), (25, 38, 38, 512, 512, 3, 1, 2), (8, 128, 256, 512, 512, 3, 1, 2)])
def test_auto_split_fills_the_part_once(shape):
    """auto: 1, or tiles x S <= 2 CUs with at least 4 K steps a part and at most DRNMI_SPLITK_MAX parts; the
    workspace is the tickets plus S partial planes; the status needs that workspace only for S > 1."""
    lib = L.load()
    a = _args(*shape)
    S = lib.drnmi_conv_splitk_auto(ctypes.byref(a))
    m, steps = a.n * a.ho * a.wo, a.k // 64
    tiles = -(-m // 64) * (a.cout_pad // 128)
    assert S >= 1 and (S == 1 or (S * tiles <= 2 * CUS and steps // S >= 4 and S <= 16))
    assert S == max(1, min(2 * CUS // tiles, steps // 4, 16))
    assert lib.drnmi_conv_splitk_status(ctypes.byref(a), 1) == 0
    assert lib.drnmi_conv_splitk_workspace_bytes(ctypes.byref(a), 1) == 0
    if steps >= 2:
        assert lib.drnmi_conv_splitk_workspace_bytes(ctypes.byref(a), 2) == -(-tiles * 4 // 256) * 256 + 2 * m * a.cout_pad * 4
        assert lib.drnmi_conv_splitk_status(ctypes.byref(a), 2) == -1                    # no workspace given
    assert lib.drnmi_conv_splitk_status(ctypes.byref(a), min(steps, 16) + 1) == -1
    assert lib.drnmi_conv_splitk_kernel_name(ctypes.byref(a), 1) == b"conv_sk_kernel<%d>" % a.ks
    a.cin, a.k, a.k_pad = 32, a.ks ** 2 * 32, a.ks ** 2 * 32
    assert lib.drnmi_conv_splitk_auto(ctypes.byref(a)) == -2 and lib.drnmi_conv_splitk_kernel_name(ctypes.byref(a), 1) is None


def test_set_low_latency_is_bf16_only():
    from drnmi.drnseg import DRNSeg
    m = DRNSeg("drn_d_22", 19, pretrained=False).eval()
    assert m.low_latency is False and m.low_latency_layers(1, 64, 64) == []
    for precision in ("fp32", "fp32x", "fp32x2", "int8", "fp8"):
        m.set_precision(precision)
        with pytest.raises(ValueError):
            m.set_low_latency(True)
        assert m.set_low_latency(False) is m
    assert m.set_precision("bf16").set_low_latency(True) is m and m.low_latency is True
    with pytest.raises(ValueError):
        m.set_precision("fp32")
    assert m.set_low_latency(False).set_precision("fp32").precision == "fp32"
