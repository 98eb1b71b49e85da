"""conv_x6 / conv_x3 and the two pre-route weight gradients, byte for byte: tests/golden/xsplit_bytes.json
holds the sha256 of what each launch below wrote, as the commit before the fp32x2 twins were folded into the
fp32x family wrote it on an MI355X (tests/golden/make_xsplit_bytes_golden.py).  Neither kernel family has
atomics, every sum has a fixed order and the inputs come from fixed seeds on the CPU, so the bytes are
reproducible.

The conv launches are tests/test_gpu_fp32x2.py's (its CASES through its _launch: y starts as NaN, the
statistics partials too, so an unwritten element changes the digest): every case on the default route under
both dtype codes, the three BN-statistics cases (y and the fp64 partials), every forced variant of both
families on the ragged cin 32 case, and K = 4608 under a forced split-K of 2 and 4 on one variant per family.
The weight gradients are the pre-route case of test_wgrad_f32x2_matches_float64 through both entries,
accumulate 0 then 1, dw between 64 B of 0xA5 and the workspace at exactly the queried size with 64 B of 0xA5
behind it (tests/test_gpu_wgrad_bytes.py's guard)."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import test_gpu_fp32x2 as T2
from drnmi import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "xsplit_bytes.json")
SLACK = 64            # bytes of 0xA5 around dw (part of the digest) and behind the workspace
STATS_CASES = ["cin32_k288_ragged", "down_1x1_s2", "res_relu"]
FAMILIES = {"x6": (_lib.DRNMI_F32X3, 6), "x3": (_lib.DRNMI_F32X2, 3)}       # dtype code, variants
SPLIT_VARIANT = {"x6": 5, "x3": 2}                                           # the 64 x 128 tile of each family
WGRAD_ENTRIES = ("drnmi_conv_wgrad_f32x3", "drnmi_conv_wgrad_f32x2")
WGRAD_CASE = (256, 256, 512, 512, 3, 1, 4, 4, 16, 16)     # cin, cs, cout, dys, ks, stride, pad, dil, h, w; n = 2


def _conv_cases():
    """name -> (family, case, _launch keywords)"""
    out = {}
    for fam, (_, num) in FAMILIES.items():
        for case in sorted(T2.CASES):
            out[f"{fam}/default/{case}"] = (fam, case, {})
        for case in STATS_CASES:
            out[f"{fam}/stats/{case}"] = (fam, case, dict(stats=True))
        for v in range(num):
            out[f"{fam}/variant{v}/cin32_k288_ragged"] = (fam, "cin32_k288_ragged", dict(tile=v))
        for s in (2, 4):
            out[f"{fam}/split{s}/k4608"] = (fam, "k4608", dict(tile=SPLIT_VARIANT[fam] + num * s, splits=s))
    return out


CONV_CASES = _conv_cases()


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def run_conv(name):
    """The digests of one conv launch: [y] or [y, partials]; y is finite everywhere (no element left NaN)."""
    from drnmi import ops
    fam, case, kw = CONV_CASES[name]
    # conv_x6's variant 0 reads 256 weight rows per plane: its launch packs to 256 rows (zero rows past cout,
    # never stored) where the others take the package's 128
    wide = (fam, kw.get("tile")) == ("x6", 0)
    keep, pack, rows = ops.COUT_ALIGN, ops.pack_conv_weight, []

    def pack_and_note(*a, **k):
        out = pack(*a, **k)
        rows.append(out[0].shape[0])
        return out

    ops.COUT_ALIGN, ops.pack_conv_weight = (256 if wide else keep), pack_and_note
    try:
        y, _, part = T2._launch(case, FAMILIES[fam][0], **kw)
    finally:
        ops.COUT_ALIGN, ops.pack_conv_weight = keep, pack
    assert rows and (not wide or rows[0] % 256 == 0), f"{name}: weights packed to {rows} rows"
    assert bool(torch.isfinite(y).all()), f"{name}: unwritten or non-finite output element"
    out = [digest(y.float().numpy())]
    if part is not None:
        p = part.cpu().numpy()
        assert bool(np.isfinite(p).all()), f"{name}: unwritten statistics partial"
        out.append(digest(p))
    return out


def run_wgrad(fn):
    """The digests of dw (slack included) after accumulate 0 and then 1 through entry `fn`."""
    cin, cs, cout, dys, ks, stride, pad, dil, h, w = WGRAD_CASE
    lib = _lib.load()
    g = torch.Generator().manual_seed(cin + cout)
    ho = (h + 2 * pad - dil * (ks - 1) - 1) // stride + 1
    wo = (w + 2 * pad - dil * (ks - 1) - 1) // stride + 1
    xd = torch.randn(2, h, w, cs, generator=g).to(DEV)
    gd = torch.randn(2, ho, wo, dys, generator=g).to(DEV)
    a = _lib.WgradArgs()
    a.n, a.h, a.w, a.cin, a.cin_stride, a.ho, a.wo, a.cout, a.dy_stride = 2, h, w, cin, cs, ho, wo, cout, dys
    a.ks, a.stride, a.pad, a.dil = ks, stride, pad, dil
    assert _lib.wgrad_plan(a, True)[0] == "wgrad_x6_pre_kernel"
    nb = lib.drnmi_conv_wgrad_workspace_bytes(ctypes.byref(a))
    assert nb > 0, nb
    ws = torch.full((nb + SLACK,), 0xA5, dtype=torch.uint8, device=DEV)
    buf = torch.full((SLACK + cout * cin * ks * ks * 4 + SLACK,), 0xA5, dtype=torch.uint8, device=DEV)
    a.dy, a.x, a.dw, a.ws, a.ws_bytes = gd.data_ptr(), xd.data_ptr(), buf.data_ptr() + SLACK, ws.data_ptr(), nb
    out = []
    for acc in (0, 1):
        a.accumulate = acc
        _lib.check(getattr(lib, fn)(ctypes.byref(a), ctypes.c_void_p(_lib.stream_ptr(torch.device(DEV)))), fn)
        torch.cuda.synchronize()
        assert bool((ws[nb:] == 0xA5).all()), f"{fn}: wrote past the queried workspace size"
        b = buf.cpu().numpy()
        assert bool((b[:SLACK] == 0xA5).all()) and bool((b[-SLACK:] == 0xA5).all()), f"{fn}: wrote outside dw"
        dw = b[SLACK:-SLACK].view(np.float32)
        assert bool(np.isfinite(dw).all()) and bool((dw != 0).all()), f"{fn}: zero or non-finite dw element"
        out.append(digest(b))
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_cases_are_the_recorded_ones(golden):
    assert set(golden) == set(CONV_CASES) | set(WGRAD_ENTRIES)
    assert all(len(golden[fn]) == 2 and golden[fn][0] != golden[fn][1] for fn in WGRAD_ENTRIES)
    assert golden[WGRAD_ENTRIES[0]] != golden[WGRAD_ENTRIES[1]]         # three products are not six
    # every variant of a family keeps each accumulator's MFMA order: the bytes of its default route
    for fam, (_, num) in FAMILIES.items():
        assert all(golden[f"{fam}/variant{v}/cin32_k288_ragged"] == golden[f"{fam}/default/cin32_k288_ragged"]
                   for v in range(num))


@pytest.mark.parametrize("name", sorted(CONV_CASES))
def test_conv_bytes(name, golden):
    assert run_conv(name) == golden[name]


@pytest.mark.parametrize("fn", WGRAD_ENTRIES)
def test_wgrad_bytes(fn, golden):
    assert run_wgrad(fn) == golden[fn]
