"""The fp8 conv epilogues, byte for byte: tests/golden/fp8_conv_bytes.json holds the sha256 of the raw
output buffer of each launch below as the commit that added fp8 wrote it on an MI355X, before the
int8 and fp8 epilogues were folded into one (tests/golden/make_fp8_bytes_golden.py).  The kernels have
no atomics and the inputs come from a fixed seed on the CPU, so the bytes are reproducible.  The
shapes are the smallest that reach each store form: 4-B and byte-wise stores and residual loads, the
16-B pieces with and without whole lines, the fp32 rows' partial group, bf16 and fp32 planes."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fp8_conv_bytes.json")
SLACK = 64            # bytes of 0xA5 around the output: part of the digest, so a stray write shows

# name: (h, w, cin, cout, ks, dil, residual, out, kernel prefix, y offset, res offset, tile)
#   out: "f8" / "bf16" dense NHWC, "f32" NCHW planes, "f32rows" NHWC rows of round_up(cout, 4) floats
#   offsets in bytes from a 256-B aligned allocation
CASES = {
    # M = 15: a partial pixel tile on the two-workgroups-per-CU 1x1 kernel, 64-B rows
    "1x1_64_128_f8": (3, 5, 64, 128, 1, 1, True, "f8", "conv_f8_occ2_kernel<1,", 0, 0, -1),
    "1x1_64_128_bf16": (3, 5, 64, 128, 1, 1, True, "bf16", "conv_f8_occ2_kernel<1,", 0, 0, -1),
    "1x1_64_128_f32": (3, 5, 64, 128, 1, 1, True, "f32", "conv_f8_occ2_kernel<1,", 0, 0, -1),
    # the seg rows: the partial 4-group goes whole into the row's own padding; and as planes
    "seg_512_19_rows": (3, 5, 512, 19, 1, 1, False, "f32rows", "conv_f8_occ2_kernel<1,", 0, 0, -1),
    "seg_512_19_planes": (3, 5, 512, 19, 1, 1, False, "f32", "conv_f8_occ2_kernel<1,", 0, 0, -1),
    # cout_pad 256, the byte tails of a partial group, rows of 130 B: scalar stores
    "3x3_128_130_f8": (4, 7, 128, 130, 3, 1, False, "f8", "conv_f8_kernel<3, 128, 1, 3, 128>", 0, 0, -1),
    # whole tiles, dense and 16-B aligned: 16-B pieces in whole 128-B lines; then y moved by 4 B (4-B
    # stores) and res by 1 B (byte-wise residual loads)
    "3x3_128_128_d2_x4": (3, 256, 128, 128, 3, 2, True, "f8", "conv_f8_kernel<3, 128, 1, 3, 128>", 0, 0, -1),
    "3x3_128_128_d2_y4": (3, 256, 128, 128, 3, 2, True, "f8", "conv_f8_kernel<3, 128, 1, 3, 128>", 4, 0, -1),
    "3x3_128_128_d2_res1": (3, 256, 128, 128, 3, 2, True, "f8", "conv_f8_kernel<3, 128, 1, 3, 128>", 0, 1, -1),
    # the K-64 step variant at 256 channels per tile
    "3x3_64_256": (2, 256, 64, 256, 3, 1, True, "f8", "conv_f8_kernel<3, 128, 2, 4, 64>", 0, 0, -1),
    # the strip-staged kernel, auto and forced, on its 16-B and its 4-B epilogue
    "stag_d1_x4": (2, 256, 256, 256, 3, 1, True, "f8", "conv_f8_stag_kernel", 0, 0, -1),
    "stag_d1_x4_forced": (2, 256, 256, 256, 3, 1, True, "f8", "conv_f8_stag_kernel", 0, 0, 19),
    "stag_d1_y4": (2, 256, 256, 256, 3, 1, True, "f8", "conv_f8_stag_kernel", 4, 0, -1),
    "stag_d4_x4": (2, 256, 256, 256, 3, 4, True, "f8", "conv_f8_stag_kernel", 0, 0, -1),
    "stag_d4_y4": (2, 256, 256, 256, 3, 4, True, "f8", "conv_f8_stag_kernel", 4, 0, 19),
}


def _e4m3_bytes(rng, shape):
    """Random e4m3 bytes of magnitude below 2 (no NaN, no saturation by themselves)."""
    return torch.from_numpy((rng.randint(0, 0x40, shape) | (rng.randint(0, 2, shape) << 7)).astype(np.uint8))


def _inputs(name):
    h, w, cin, cout, ks, dil, has_res = CASES[name][:7]
    rng = np.random.RandomState(sorted({c[:7] for c in CASES.values()}).index(CASES[name][:7]))
    k, cout_pad = ks * ks * cin, (cout + 127) // 128 * 128
    wt = torch.zeros(cout_pad, k, dtype=torch.uint8)
    wt[:cout] = _e4m3_bytes(rng, (cout, k))
    return {"x": _e4m3_bytes(rng, (1, h, w, cin)), "w": wt,
            "scale": torch.from_numpy(((0.5 + rng.rand(cout_pad)) / k ** 0.5).astype(np.float32)),
            "shift": torch.from_numpy((rng.randn(cout_pad) * 0.5).astype(np.float32)),
            "res": _e4m3_bytes(rng, (h * w * cout,)) if has_res else None}


def run_case(name):
    """Launches CASES[name]; the whole output buffer (slack included) as bytes on the host."""
    from drnmi import _lib as L
    lib = L.load()
    h, w, cin, cout, ks, dil, has_res, out, kernel, y_off, res_off, tile = CASES[name]
    t = _inputs(name)
    pad = dil * (ks // 2)
    a = L.ConvArgs()
    dev = {k: t[k].to(DEV) for k in ("x", "w", "scale", "shift")}
    a.x, a.wgt, a.scale, a.shift = (dev[k].data_ptr() for k in ("x", "w", "scale", "shift"))
    if has_res:
        res = torch.zeros(res_off + t["res"].numel(), dtype=torch.uint8, device=DEV)
        res[res_off:] = t["res"].to(DEV)
        a.res = res.data_ptr() + res_off
    row = (cout + 3) // 4 * 4 if out == "f32rows" else cout
    esz = {"f8": 1, "bf16": 2, "f32": 4, "f32rows": 4}[out]
    y = torch.full((SLACK + y_off + h * w * row * esz + SLACK,), 0xA5, dtype=torch.uint8, device=DEV)
    a.y = y.data_ptr() + SLACK + y_off
    if out == "f32":
        a.y_sn, a.y_sp, a.y_sc = cout * h * w, 1, h * w
    else:
        a.y_sn, a.y_sp, a.y_sc = h * w * row, row, 1
    a.out_dtype = {"f8": L.DRNMI_F8, "bf16": L.DRNMI_BF16, "f32": L.DRNMI_F32, "f32rows": L.DRNMI_F32}[out]
    a.n, a.h, a.w, a.cin, a.ho, a.wo, a.cout, a.cout_pad = 1, h, w, cin, h, w, cout, t["w"].shape[0]
    a.ks, a.stride, a.pad, a.dil, a.k, a.k_pad = ks, 1, pad, dil, ks * ks * cin, ks * ks * cin
    a.relu, a.dtype, a.tile, a.algo = 1, L.DRNMI_F8, tile, L.ALGO_IGEMM
    a.res_scale, a.out_scale = 0.75, 1.0 / 0.0123
    got = lib.drnmi_conv_kernel_name(ctypes.byref(a))
    assert got is not None and got.decode().startswith(kernel), (name, got)
    L.check(lib.drnmi_conv2d_bn_act(ctypes.byref(a), ctypes.c_void_p(L.stream_ptr(torch.device(DEV)))), name)
    torch.cuda.synchronize()
    return y.cpu().numpy()


def digest(buf):
    return hashlib.sha256(buf.tobytes()).hexdigest()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_cases_are_the_recorded_ones(golden):
    assert set(golden) == set(CASES)
    # the forced strip-staged launch is the auto-routed one
    assert golden["stag_d1_x4"] == golden["stag_d1_x4_forced"]


@pytest.mark.parametrize("name", sorted(CASES))
def test_fp8_conv_bytes(name, golden):
    buf = run_case(name)
    body = buf[SLACK:-SLACK]
    assert bool((buf[:SLACK] == 0xA5).all()) and bool((buf[-SLACK:] == 0xA5).all()), "wrote outside the output"
    if CASES[name][7] == "f8":
        code = body[CASES[name][9]:]
        assert 0.2 < float((code & 0x7F != 0).mean()) and float((code & 0x7F == 0x7E).mean()) < 0.5, "trivial output"
    assert digest(buf) == golden[name]
