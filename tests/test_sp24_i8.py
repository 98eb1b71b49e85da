"""2:4 weight sparsity at int8 without a GPU: dtype DRNMI_I8_SP24 (include/drnmi.h) in header, binding and
library, the packed size, the argument checks made before any HIP call, the route and every refusal's
status, and what the engine decides on the host (off by default; which int8 nodes a pack is tried on)."""
import ctypes
import os
import re

import pytest
import torch

from drnmi import _lib, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 0x1000
ENOTSUP, EINVAL = -2, -1
SYMBOLS = ("drnmi_sp24_pack_i8_bytes", "drnmi_sp24_pack_i8", "drnmi_sp24_mma_probe_i8")


def test_dtype_8_and_symbols_under_abi_7():
    text = open(os.path.join(ROOT, "include", "drnmi.h")).read()
    assert int(re.search(r"#define DRNMI_ABI_VERSION (\d+)", text).group(1)) == 7
    assert _lib.ABI_VERSION == 7 and _lib.load().drnmi_abi_version() == 7
    assert re.search(r"DRNMI_I8_SP24 = 8\b", text) and _lib.DRNMI_I8_SP24 == 8
    lib = _lib.load()
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES and re.search(r"\b%s\(" % name, text) and hasattr(lib, name)
    assert ctypes.sizeof(_lib.ConvArgs) == lib.drnmi_conv_args_size()          # the struct did not grow


def test_pack_bytes_and_argument_checks():
    lib = _lib.load()
    assert lib.drnmi_sp24_pack_i8_bytes(512, 4608) == 512 * 4608 * 5 // 8     # half the values + 2 bits per kept value
    assert lib.drnmi_sp24_pack_i8_bytes(128, 128) == 128 * 64 + 128 * 16
    for rows, k in ((0, 128), (16, 128), (48, 128), (128, 64), (128, 192), (-128, 128), (128, 0), (128, -128)):
        assert lib.drnmi_sp24_pack_i8_bytes(rows, k) == -1
    # refused before any HIP call: NULL operands, sizes, alignment
    assert lib.drnmi_sp24_pack_i8(None, 128, 128, PTR, None, None) == EINVAL
    assert lib.drnmi_sp24_pack_i8(PTR, 128, 128, None, None, None) == EINVAL
    assert lib.drnmi_sp24_pack_i8(PTR, 100, 128, PTR, None, None) == EINVAL
    assert lib.drnmi_sp24_pack_i8(PTR, 128, 64, PTR, None, None) == EINVAL
    assert lib.drnmi_sp24_pack_i8(PTR, 128, 128, PTR + 4, None, None) == EINVAL
    for args in ((None, PTR, PTR, PTR), (PTR, None, PTR, PTR), (PTR, PTR, None, PTR), (PTR, PTR, PTR, None)):
        assert lib.drnmi_sp24_mma_probe_i8(*args, None) == EINVAL


# ----------------------------------------------------------------------------- route and status
def _args(cin=128, cout=256, ks=3, stride=1, dil=1, ho=6, wo=20, out="i8", cout_pad=None, tile=-1, **over):
    a = _lib.ConvArgs()
    pad = dil * (ks // 2)
    a.x = a.wgt = a.scale = a.shift = a.y = PTR
    a.n, a.ho, a.wo = 1, ho, wo
    a.h = (ho - 1) * stride + dil * (ks - 1) + 1 - 2 * pad
    a.w = (wo - 1) * stride + dil * (ks - 1) + 1 - 2 * pad
    a.cin, a.cout, a.ks, a.stride, a.pad, a.dil = cin, cout, ks, stride, pad, dil
    a.cout_pad = cout_pad or (cout + 127) // 128 * 128
    a.k = a.k_pad = ks * ks * cin
    a.relu, a.dtype, a.tile, a.algo = 1, _lib.DRNMI_I8_SP24, tile, _lib.ALGO_IGEMM
    a.res_scale, a.out_scale = 0.01, 40.0
    if out in ("i8", "bf16"):                # NHWC rows
        a.out_dtype, a.y_sn, a.y_sp, a.y_sc = (_lib.DRNMI_I8 if out == "i8" else _lib.DRNMI_BF16), ho * wo * cout, cout, 1
    elif out == "f32":                       # NCHW logits planes
        a.out_dtype, a.y_sn, a.y_sp, a.y_sc = _lib.DRNMI_F32, cout * ho * wo, 1, ho * wo
    else:                                    # "f32rows" / "f32slice": NHWC logits rows, or a slice of wider ones
        cs = (cout + 3) // 4 * 4 + (8 if out == "f32slice" else 0)
        a.out_dtype, a.y_sn, a.y_sp, a.y_sc = _lib.DRNMI_F32, ho * wo * cs, cs, 1
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _route(a):
    lib = _lib.load()
    name = lib.drnmi_conv_kernel_name(ctypes.byref(a))
    return lib.drnmi_conv_status(ctypes.byref(a)), None if name is None else name.decode()


@pytest.mark.parametrize("kw, tile", [
    (dict(), "128, 2"), (dict(cout=128), "128, 1"), (dict(cin=256, cout=160), "128, 2"), (dict(out="bf16"), "128, 2"),
    (dict(cin=512, cout=512, dil=4), "128, 2"), (dict(cin=512, cout=512, dil=2, wo=256, tile=_lib.SP24_GATHER), "128, 2"),
    (dict(cin=512, cout=512, dil=2, wo=256), "128, 2"),                     # auto is the gather on whole rows too
    (dict(cin=128, cout=128, wo=256), "128, 1"), (dict(wo=256, stride=2), "128, 2"), (dict(ks=1, wo=256), "128, 2"),
    (dict(ks=1, cin=256, cout=512), "128, 2"), (dict(ks=1, cin=128, cout=128, stride=2), "128, 1"),
    (dict(cin=128, cout=384), "128, 1"), (dict(stride=2, dil=2), "128, 2"), (dict(res=PTR, relu=0), "128, 2"),
    (dict(cin=128, cout=130, out="bf16", res=PTR), "128, 2"),
    (dict(ks=1, cin=512, cout=19, out="f32"), "128, 1"), (dict(ks=1, cin=512, cout=19, out="f32rows"), "128, 1"),
    (dict(ks=1, cin=512, cout=19, out="f32slice"), "128, 1"), (dict(cin=1024, cout=256, out="f32"), "128, 2"),
    (dict(cout=128, cout_pad=256), "128, 1"), (dict(tile=_lib.SP24_GATHER), "128, 2"),
])
def test_accepted_shapes_name_a_sparse_int8_kernel(kw, tile):
    a = _args(**kw)
    status, name = _route(a)
    assert status == 0 and name == f"conv_sp24_i8_kernel<{a.ks}, {tile}>", (status, name)


@pytest.mark.parametrize("kw", [dict(wo=256), dict(cin=256, cout=160, wo=512, dil=4),
                                dict(cin=512, cout=512, dil=2, wo=256, ho=1, res=PTR), dict(wo=256, out="f32")])
def test_whole_rows_take_the_strip_form_when_forced(kw):
    assert _route(_args(tile=_lib.SP24_STRIP, **kw)) == (0, "conv_sp24_i8_strip_kernel")
    assert _route(_args(**kw))[1] == "conv_sp24_i8_kernel<3, 128, 2>"


@pytest.mark.parametrize("kw, want", [
    (dict(x2=PTR, cin2=64, h2=6, w2=20, stride2=1), ENOTSUP),
    (dict(unit_mask=PTR), ENOTSUP),
    (dict(scale=None), ENOTSUP),                          # the int8 contract: a scale
    (dict(cin=64), ENOTSUP),                              # below one K step: stays dense int8
    (dict(cin=96), EINVAL),                               # not a power of two
    (dict(ks=7), ENOTSUP),
    (dict(k_pad=9 * 128 + 128), ENOTSUP),                 # k_pad != k
    (dict(cout=100, cout_pad=104), ENOTSUP),              # cout_pad % 128
    (dict(out_dtype=_lib.DRNMI_F8), EINVAL),
    (dict(out_dtype=_lib.DRNMI_U8), EINVAL),
    (dict(algo=_lib.ALGO_PATCH), EINVAL),
    (dict(tile=_lib.TILE_STAG), EINVAL),                  # tile is enum drnmi_sp24_tile: a foreign id
    (dict(tile=2), EINVAL),
    (dict(tile=_lib.SP24_STRIP), ENOTSUP),                # strip form forced on wo % 256 != 0
    (dict(tile=_lib.SP24_STRIP, wo=256, ks=1), ENOTSUP),
    (dict(tile=_lib.SP24_STRIP, wo=256, stride=2), ENOTSUP),
    (dict(tile=_lib.SP24_STRIP, wo=256, cout=128), ENOTSUP),      # the strip form is the 256-channel tile's
    (dict(tile=_lib.SP24_STRIP, wo=512, dil=8), ENOTSUP),         # the strip buffer holds 256 + 2 * 4 rows
])
def test_refusals(kw, want):
    status, name = _route(_args(**kw))
    assert name is None
    assert status == want, (kw, status)


def test_rows_must_exist():
    assert _route(_args(cout=300, cout_pad=512)) == (0, "conv_sp24_i8_kernel<3, 128, 2>")
    status, name = _route(_args(cout=200, cout_pad=128))   # cout > cout_pad
    assert status == EINVAL and name is None


def test_seg_fused_entry_refuses_dtype_8():
    lib = _lib.load()
    a = _args(cin=512, cout=512, dil=2, wo=256, ho=2)
    assert lib.drnmi_conv_stag_seg_kernel_name(ctypes.byref(a)) is None
    assert lib.drnmi_conv_stag_seg(ctypes.byref(a), PTR, 512, 32, PTR, None) == ENOTSUP
    a.dtype = _lib.DRNMI_I8                                  # the same launch in dense int8 has the fused form
    assert lib.drnmi_conv_stag_seg_kernel_name(ctypes.byref(a)) is not None


def test_other_dtypes_cannot_reach_the_sparse_int8_rows():
    for dtype in (_lib.DRNMI_F32, _lib.DRNMI_BF16, _lib.DRNMI_I8, _lib.DRNMI_F32X3, _lib.DRNMI_F8, _lib.DRNMI_BF16_SP24):
        for tile in list(range(-1, 24)):
            for kw in (dict(), dict(ks=1, cin=256, cout=512), dict(cin=512, cout=512, wo=256, dil=2), dict(out="bf16")):
                for scale in (PTR, None):
                    _, name = _route(_args(dtype=dtype, tile=tile, scale=scale, **kw))
                    assert name is None or "sp24_i8" not in name, (dtype, tile, kw, name)


# ----------------------------------------------------------------------------- the engine, host side
def _d22():
    from drnmi.drnseg import DRNSeg
    from drnmi.weights import synth_state_dict
    m = DRNSeg("drn_d_22", 19, pretrained=False)
    m.load_state_dict(synth_state_dict(m, 0))
    return m.eval()


def _signature(pk):
    lib = _lib.load()
    plan = engine.Plan(pk, 1, 64, 128)
    out = []
    for src, labels_only in (("nchw", False), ("u8", True)):
        for l in plan.launches(src, labels_only):
            a = plan.args[l.row]
            out.append((l.row, l.kind, l.nodes, l.kernel_name(lib), None if a is None else a.dtype))
    return out


def test_off_by_default_and_host_side_candidates(monkeypatch):
    m = _d22()
    cpu = torch.device("cpu")
    scales = {v: 0.05 for v in m._graph.channels}          # a constant scale for every value a calibration would give
    absent = engine.PackedNet(m._graph, "int8", cpu, block_sparse=False, act_scales=scales)
    off = engine.PackedNet(m._graph, "int8", cpu, block_sparse=False, act_scales=scales, sparse24=False)
    assert absent.sparse24 is False and absent.sparse24_layers() == off.sparse24_layers() == []
    assert all(nd.wsp is None for nd in off.graph.nodes)
    sig = _signature(off)
    assert sig == _signature(absent)
    assert any(s[4] == _lib.DRNMI_I8 for s in sig)
    assert not any("sp24" in (s[3] or "") for s in sig) and all(s[4] != _lib.DRNMI_I8_SP24 for s in sig)
    assert m.set_precision("fp32").set_sparse24(True).sparse24_layers() == []       # not a switch of fp32
    m.set_sparse24(False)
    # what the host decides with every eligible layer routed sparse: the int8 nodes with cin >= 128 the route
    # accepts (the pack itself, which finds this unmasked net's violations, needs the device)
    assert engine.SP24_I8_EVERY is False
    default = off.sp24_i8_candidates()
    monkeypatch.setattr(engine, "SP24_I8_EVERY", True)
    every = off.sp24_i8_candidates()
    nodes = off.graph.nodes
    assert every == [i for i, nd in enumerate(nodes) if nd.i8 and nd.cin_stride >= 128]
    assert set(default) <= set(every)
    names = [nodes[i].name for i in every]
    assert {"layer.7.0", "layer.8.0", "seg"} <= set(names)
    # fp8 shares the int8 layout and is excluded
    f8 = engine.PackedNet(m._graph, "fp8", cpu, block_sparse=False, act_scales=scales, sparse24=True)
    assert f8.sp24_i8_candidates() == [] and f8.sparse24_layers() == []


def test_roofline_prices_sparse_int8_launches_at_twice_the_int8_peak():
    from drnmi import roofline
    assert roofline.kernel_peak("conv_sp24_i8_kernel<3, 128, 2>", "bf16") == 2 * roofline.MFMA_PEAK["int8"]
    assert roofline.kernel_peak("conv_sp24_i8_strip_kernel", "bf16") == 2 * roofline.MFMA_PEAK["int8"]
    assert roofline.kernel_peak("conv_sp24_kernel<3, 128, 2>", "bf16") == 2 * roofline.MFMA_PEAK["bf16"]
    assert roofline.kernel_peak("conv_i8_stag_kernel", "bf16") == roofline.MFMA_PEAK["int8"]
