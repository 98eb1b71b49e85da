"""The strip conv tiles (conv_stag*, conv_w1*, conv_w1h*) walk only a tile's live tap rows: a tap
row outside the image (output rows oh < dil and oh >= H - dil of a 3x3, pad = dil conv) is all
padding and its three K steps are left out (csrc/conv_tile.h TapWin).  The surviving steps keep
their order per accumulator, so the results must be what the full walk gives:

  bf16   bit for bit the strip tile's output (tile 18, conv_strip_kernel: it still multiplies the zero
         rows); the x2 forms, which the strip tile does not take, against conv_big's gather tile;
  seg    the seg-fused launch on both tiles: equal partial logits, and within the seg-fusion test's
         bound (2^-16 max|logit| + 1e-6: fp32 summation order) of the classifier on the stored output;
  int8   the bytes of oracle/int8_oracle.py.

Shapes: one 256-pixel tile per output row (n 1, W 256) and images so low that border rows dominate,
H in {1, 2, dil, dil + 1, 2 dil, 2 dil + 3} for dil 1, 2, 4: live rows per tile 1, 2 and 3, first
live row 0 and 1.  Random normal inputs, weights and shifts (no exactly-zero accumulator)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import int8_oracle as Q

pytestmark = pytest.mark.gpu
DEV = "cuda"
W = 256
TILE_GATHER128, TILE_GATHER256, TILE_STRIP, TILE_STAG, TILE_W1, TILE_W1H = 4, 5, 18, 19, 22, 23

GEOM = sorted({(dil, h) for dil in (1, 2, 4) for h in (1, 2, dil, dil + 1, 2 * dil, 2 * dil + 3)})
SEG_TOL = 2.0 ** -16


def _lib():
    from drnmi import _lib
    return _lib, _lib.load()


def _stream():
    from drnmi import _lib
    return ctypes.c_void_p(_lib.stream_ptr(torch.device(DEV)))


def _launch(a, what):
    L, lib = _lib()
    assert lib.drnmi_conv_kernel_name(ctypes.byref(a)) is not None, what
    L.check(lib.drnmi_conv2d_bn_act(ctypes.byref(a), _stream()), what)


# ---------------------------------------------------------------------------------------------- bf16

_BF16 = {}


def _bf16_case(dil, h, cin, cout, with_res, cin2=0):
    """Operands of one launch on the GPU (made once) and the baseline tile's output."""
    key = (dil, h, cin, cout, with_res, cin2)
    if key in _BF16:
        return _BF16[key]
    L, _ = _lib()
    g = torch.Generator().manual_seed(hash(key) % (2 ** 31))
    k = 9 * cin + cin2
    t = {"x": torch.randn(1, h, W, cin, generator=g).bfloat16().to(DEV)}
    wpk = torch.zeros(256, k)
    wpk[:cout] = torch.randn(cout, k, generator=g) / k ** 0.5
    t["w"] = wpk.bfloat16().to(DEV)
    sh = torch.zeros(256)
    sh[:cout] = torch.randn(cout, generator=g)
    t["sh"] = sh.to(DEV)
    if with_res:
        t["res"] = torch.randn(1, h, W, cout, generator=g).bfloat16().to(DEV)
    if cin2:                                         # the fused 1x1 stride-2 downsample's input
        t["x2"] = torch.randn(1, 2 * h, 2 * W, cin2, generator=g).bfloat16().to(DEV)
    a = L.ConvArgs()
    a.x, a.wgt, a.scale, a.shift = t["x"].data_ptr(), t["w"].data_ptr(), None, t["sh"].data_ptr()
    a.res = t["res"].data_ptr() if with_res else None
    a.y_sn, a.y_sp, a.y_sc = h * W * cout, cout, 1
    a.n, a.h, a.w, a.cin, a.ho, a.wo, a.cout, a.cout_pad = 1, h, W, cin, h, W, cout, 256
    a.ks, a.stride, a.pad, a.dil, a.k, a.k_pad = 3, 1, dil, dil, k, k
    a.relu, a.dtype, a.out_dtype, a.algo = 1, L.DRNMI_BF16, L.DRNMI_BF16, L.ALGO_IGEMM
    if cin2:
        a.x2, a.cin2, a.h2, a.w2, a.stride2 = t["x2"].data_ptr(), cin2, 2 * h, 2 * W, 2
    base = torch.zeros(1, h, W, cout, dtype=torch.bfloat16, device=DEV)
    a.y = base.data_ptr()
    a.tile = TILE_STRIP if not cin2 else TILE_GATHER256 if cout == 256 else TILE_GATHER128
    _launch(a, f"baseline {key}")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(base.float()).all()) and bool((base != 0).any())
    _BF16[key] = (a, t, base)
    return _BF16[key]


def _check_bf16(tile, key):
    a, _, base = _bf16_case(*key)
    y = torch.zeros_like(base)
    a.y, a.tile = y.data_ptr(), tile
    _launch(a, f"tile {tile} {key}")
    torch.cuda.synchronize()
    assert torch.equal(y.view(torch.int16), base.view(torch.int16)), (tile, key)


@pytest.mark.parametrize("dil,h", GEOM)
@pytest.mark.parametrize("tile", [TILE_STAG, TILE_W1, TILE_W1H])
def test_bf16_tiles_match_strip_tile(tile, dil, h):
    """conv_stag / conv_w1 / conv_w1h (forced) == conv_strip_kernel on the int16 view of the output,
    cin 128 and 256 (2 and 4 channel blocks), with and without a residual."""
    L, lib = _lib()
    cout = 128 if tile == TILE_W1H else 256
    for cin in (128, 256):
        for with_res in (False, True):
            key = (dil, h, cin, cout, with_res)
            a = _bf16_case(*key)[0]
            a.tile = tile
            want = {TILE_STAG: "conv_stag_kernel", TILE_W1: "conv_w1_kernel", TILE_W1H: "conv_w1h_kernel"}[tile]
            assert lib.drnmi_conv_kernel_name(ctypes.byref(a)).decode() == want
            _check_bf16(tile, key)


@pytest.mark.parametrize("h", [3, 5])
@pytest.mark.parametrize("tile,cout,name", [
    (TILE_STAG, 256, "conv_stag_x2_kernel"), (TILE_STAG, 128, "conv_stag128_x2_kernel"),
    (TILE_W1, 256, "conv_w1_x2_kernel"), (TILE_W1H, 128, "conv_w1h_x2_kernel")])
def test_bf16_x2_forms_match_gather_tile(tile, cout, name, h):
    """The x2 forms (cin2 64 at stride 2: extra K steps after the last live tap step; conv_stag's two
    keep the full walk) == conv_big's gather tile with the same fused downsample, dil 2: H 3 has
    tiles of 1 and 2 live rows, H 5 of 2 and 3."""
    L, lib = _lib()
    key = (2, h, 128, cout, False, 64)
    a = _bf16_case(*key)[0]
    a.tile = tile
    assert lib.drnmi_conv_kernel_name(ctypes.byref(a)).decode() == name
    _check_bf16(tile, key)


def test_bf16_stag128_matches_strip_tile():
    """cout 128 on the staggered tile is conv_stag128_kernel (its own instantiation)."""
    L, lib = _lib()
    for dil, h in GEOM:
        key = (dil, h, 128, 128, True)
        a = _bf16_case(*key)[0]
        a.tile = TILE_STAG
        assert lib.drnmi_conv_kernel_name(ctypes.byref(a)).decode() == "conv_stag128_kernel"
        _check_bf16(TILE_STAG, key)


@pytest.mark.parametrize("h", [3, 5])
def test_bf16_seg_fused_forms(h):
    """drnmi_conv_stag_seg at dil 1, 512 -> 512: conv_w1_seg_kernel (default) and conv_stag_seg_kernel
    (tile 19) give the same partial logits bit for bit, and block 0 + block 1 is the classifier on
    the activation the plain launch stores (strip tile), up to fp32 summation order."""
    L, lib = _lib()
    cin = cout = 512
    g = torch.Generator().manual_seed(700 + h)
    k = 9 * cin
    x = torch.randn(1, h, W, cin, generator=g).bfloat16().to(DEV)
    wpk = (torch.randn(cout, k, generator=g) / k ** 0.5).bfloat16().to(DEV)
    sh = torch.randn(cout, generator=g).to(DEV)
    segw = torch.zeros(32, cout)
    segw[:19] = torch.randn(19, cout, generator=g) / cout ** 0.5
    segw = segw.bfloat16().to(DEV)
    y = torch.zeros(1, h, W, cout, dtype=torch.bfloat16, device=DEV)
    a = L.ConvArgs()
    a.x, a.wgt, a.scale, a.shift, a.res, a.y = x.data_ptr(), wpk.data_ptr(), None, sh.data_ptr(), None, y.data_ptr()
    a.y_sn, a.y_sp, a.y_sc = h * W * cout, cout, 1
    a.n, a.h, a.w, a.cin, a.ho, a.wo, a.cout, a.cout_pad = 1, h, W, cin, h, W, cout, cout
    a.ks, a.stride, a.pad, a.dil, a.k, a.k_pad = 3, 1, 1, 1, k, k
    a.relu, a.dtype, a.out_dtype, a.algo = 1, L.DRNMI_BF16, L.DRNMI_BF16, L.ALGO_IGEMM
    a.tile = TILE_STRIP
    _launch(a, "plain conv")
    parts = {}
    for tile, name in ((-1, "conv_w1_seg_kernel"), (TILE_STAG, "conv_stag_seg_kernel")):
        a.tile = tile
        assert lib.drnmi_conv_stag_seg_kernel_name(ctypes.byref(a)).decode() == name
        part = torch.full((2, h * W, 20), float("nan"), device=DEV)
        L.check(lib.drnmi_conv_stag_seg(ctypes.byref(a), segw.data_ptr(), cout, 32, part.data_ptr(), _stream()), name)
        parts[tile] = part
    torch.cuda.synchronize()
    assert torch.equal(parts[-1].view(torch.int32), parts[TILE_STAG].view(torch.int32))
    logits = y.view(h * W, cout).double().cpu() @ segw[:19].double().cpu().T
    for part in parts.values():
        fused = (part[0, :, :19] + part[1, :, :19]).double().cpu()
        err = (fused - logits).abs().max().item()
        print(f"seg-fused H {h}: max |diff| {err:.3e} (max |logit| {logits.abs().max().item():.2f})")
        assert err <= SEG_TOL * logits.abs().max().item() + 1e-6, err


# ---------------------------------------------------------------------------------------------- int8

_I8 = {}


def _i8_case(dil, h, cin, cout, with_res):
    """One int8 launch's operands, its ConvArgs and the oracle's bytes (computed once)."""
    key = (dil, h, cin, cout, with_res)
    if key in _I8:
        return _I8[key]
    L, _ = _lib()
    rng = np.random.default_rng(abs(hash(key)) % (2 ** 31))
    k = 9 * cin
    cout_pad = (cout + 127) // 128 * 128
    x = rng.integers(-127, 128, (1, h, W, cin), dtype=np.int8)
    wpk = np.zeros((cout_pad, k), np.int8)
    wpk[:cout] = rng.integers(-127, 128, (cout, k), dtype=np.int8)
    scale = np.zeros(cout_pad, np.float32)
    shift = np.zeros(cout_pad, np.float32)
    scale[:cout] = (rng.uniform(0.5, 1.5, cout) / (np.sqrt(k) * 5400.0)).astype(np.float32)   # v ~ N(0, 1)
    shift[:cout] = rng.normal(0, 0.5, cout).astype(np.float32)
    res = rng.integers(-127, 128, (1, h, W, cout), dtype=np.int8) if with_res else None
    res_scale, out_scale = 0.011, 1.0 / 0.023
    d = {k_: torch.from_numpy(v).to(DEV) for k_, v in {"x": x, "w": wpk, "sc": scale, "sh": shift}.items()}
    if with_res:
        d["res"] = torch.from_numpy(res).to(DEV)
    d["y"] = torch.zeros((1, h, W, cout), dtype=torch.int8, device=DEV)
    a = L.ConvArgs()
    a.x, a.wgt, a.scale, a.shift = d["x"].data_ptr(), d["w"].data_ptr(), d["sc"].data_ptr(), d["sh"].data_ptr()
    a.res = d["res"].data_ptr() if with_res else None
    a.y = d["y"].data_ptr()
    a.y_sn, a.y_sp, a.y_sc, a.out_dtype = h * W * cout, cout, 1, L.DRNMI_I8
    a.n, a.h, a.w, a.cin, a.ho, a.wo, a.cout, a.cout_pad = 1, h, W, cin, h, W, cout, cout_pad
    a.ks, a.stride, a.pad, a.dil, a.k, a.k_pad = 3, 1, dil, dil, k, k
    a.relu, a.dtype, a.tile, a.algo = 1, L.DRNMI_I8, -1, L.ALGO_IGEMM
    a.res_scale, a.out_scale = res_scale, out_scale
    ref = Q.conv_i8(x, wpk, scale, shift, cout, 3, 1, dil, dil, True, res, res_scale, "i8", out_scale)
    assert np.abs(ref.astype(np.int32)).max() < 127 or (ref == 127).mean() < 0.5   # not all saturated
    _I8[key] = (a, d, ref)
    return _I8[key]


@pytest.mark.parametrize("dil,h", GEOM)
def test_i8_w1h_matches_oracle(dil, h):
    """conv_w1h_i8_kernel at cin 128: one 128-channel block, so 1, 2 or 3 live groups per tile (the odd
    counts on its odd-count walk), with and without a residual."""
    L, lib = _lib()
    for with_res in (False, True):
        a, d, ref = _i8_case(dil, h, 128, 128, with_res)
        assert lib.drnmi_conv_kernel_name(ctypes.byref(a)).decode() == "conv_w1h_i8_kernel"
        d["y"].zero_()
        _launch(a, "conv_w1h_i8")
        torch.cuda.synchronize()
        np.testing.assert_array_equal(d["y"].cpu().numpy(), ref)


@pytest.mark.parametrize("dil,h", GEOM)
def test_i8_stag_w1_and_seg_match_oracle(dil, h):
    """cin 256 -> 256 (two 128-channel blocks: even live group counts), no residual:
    conv_i8_stag_kernel (tile 19) and conv_w1_i8_kernel (tile 22) give the oracle's bytes, and the
    seg-fused launches (conv_w1_i8_seg_kernel, conv_i8_stag_seg_kernel) the exact integer partial
    logits of those bytes."""
    L, lib = _lib()
    cin = cout = 256
    a, d, ref = _i8_case(dil, h, cin, cout, False)
    for tile, name in ((TILE_STAG, "conv_i8_stag_kernel"), (TILE_W1, "conv_w1_i8_kernel")):
        a.tile = tile
        assert lib.drnmi_conv_kernel_name(ctypes.byref(a)).decode() == name
        d["y"].zero_()
        _launch(a, name)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(d["y"].cpu().numpy(), ref)
    rng = np.random.default_rng(17)
    segw = np.zeros((32, cout), np.int8)
    segw[:19] = rng.integers(-127, 128, (19, cout), dtype=np.int8)
    want = ref.reshape(h * W, cout).astype(np.int64) @ segw[:19].astype(np.int64).T
    sw = torch.from_numpy(segw).to(DEV)
    for tile, name in ((-1, "conv_w1_i8_seg_kernel"), (TILE_STAG, "conv_i8_stag_seg_kernel")):
        a.tile = tile
        assert lib.drnmi_conv_stag_seg_kernel_name(ctypes.byref(a)).decode() == name
        part = torch.full((1, h * W, 20), -(2 ** 31), dtype=torch.int32, device=DEV)
        L.check(lib.drnmi_conv_stag_seg(ctypes.byref(a), sw.data_ptr(), cout, 32, part.data_ptr(), _stream()), name)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(part[0, :, :19].cpu().numpy().astype(np.int64), want)
    a.tile = -1
