"""2:4 weight sparsity without a GPU: NMPruner's masks, the route and status of dtype DRNMI_BF16_SP24
(include/drnmi.h), the packed size, and that the switch is off by default and changes nothing when off."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from drnmi import _lib, engine
from drnmi import pruners as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 0x1000


# ----------------------------------------------------------------------------- NMPruner
class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Conv2d(8, 6, 3, bias=False)
        self.b = torch.nn.Conv2d(12, 5, 1, bias=False)
        g = torch.Generator().manual_seed(3)
        with torch.no_grad():
            self.a.weight.copy_(torch.randn(6, 8, 3, 3, generator=g))
            self.b.weight.copy_(torch.randn(5, 12, 1, 1, generator=g))


def _cfg(tmp_path, n=2, m=4, layers=("a.weight", "b.weight"), **extra):
    p = tmp_path / f"nm_{n}_{m}_{len(extra)}.json"
    p.write_text(json.dumps({"pruner_type": "nm", "configs": [dict(layer_set=list(layers), n=n, m=m, **extra)]}))
    return str(p)


def _groups(mask):
    """[cout, kh, kw, cin / 4, 4]: the groups of four consecutive input channels at fixed (out, kh, kw)."""
    co, ci, kh, kw = mask.shape
    return mask.permute(0, 2, 3, 1).reshape(co, kh, kw, ci // 4, 4)


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("static", [False, True])
def test_nm_masks_have_n_ones_per_group(tmp_path, n, static):
    net = _Net()
    pr = P.make_pruner(_cfg(tmp_path, n=n), on_gpu=False)
    assert isinstance(pr, P.NMPruner)
    pr.generate_masks(net, is_static=static)
    assert list(pr.mask_dict) == ["a.weight", "b.weight"]
    for layer, mask in pr.mask_dict.items():
        assert mask.dtype == torch.float32 and mask.shape == net.state_dict()[layer].shape
        assert bool(((mask == 0) | (mask == 1)).all())
        assert bool((_groups(mask).sum(-1) == n).all())


def test_nm_magnitude_keeps_largest_and_ties_go_low(tmp_path):
    net = _Net()
    with torch.no_grad():
        net.a.weight[0, 0:4, 0, 0] = torch.tensor([0.5, -0.5, 0.5, -0.5])      # all tied: channels 0, 1
        net.a.weight[1, 4:8, 2, 1] = torch.tensor([0.1, 0.7, -0.7, 0.7])       # three tied at the top: 1, 2
        net.a.weight[2, 0:4, 1, 1] = torch.tensor([0.0, 0.0, 0.0, 0.0])        # an empty group still keeps two
        net.a.weight[3, 0:4, 1, 1] = torch.tensor([0.2, -0.9, 0.3, 0.8])       # plain: 1, 3
    pr = P.NMPruner(_cfg(tmp_path), on_gpu=False)
    pr.generate_masks(net)
    m = pr.mask_dict["a.weight"]
    assert m[0, 0:4, 0, 0].tolist() == [1, 1, 0, 0]
    assert m[1, 4:8, 2, 1].tolist() == [0, 1, 1, 0]
    assert m[2, 0:4, 1, 1].tolist() == [1, 1, 0, 0]
    assert m[3, 0:4, 1, 1].tolist() == [0, 1, 0, 1]
    for layer, mask in pr.mask_dict.items():                                    # no dropped weight beats a kept one
        a = _groups(net.state_dict()[layer].abs())
        g = _groups(mask)
        kept_min = torch.where(g == 1, a, torch.full_like(a, float("inf"))).amin(-1)
        drop_max = torch.where(g == 0, a, torch.full_like(a, -1.0)).amax(-1)
        assert bool((kept_min >= drop_max).all())
    pr1 = P.NMPruner(_cfg(tmp_path, n=1), on_gpu=False)
    pr1.generate_masks(net)
    assert pr1.mask_dict["a.weight"][3, 0:4, 1, 1].tolist() == [0, 1, 0, 0]
    assert pr1.mask_dict["a.weight"][0, 0:4, 0, 0].tolist() == [1, 0, 0, 0]


def test_nm_static_is_reproducible_from_the_seed(tmp_path):
    net = _Net()
    masks = []
    for seed in (11, 11, 12):
        pr = P.NMPruner(_cfg(tmp_path, seed=seed), on_gpu=False)
        np.random.seed(seed * 77)              # the global generator plays no part
        pr.generate_masks(net, is_static=True)
        masks.append(torch.cat([v.flatten() for v in pr.mask_dict.values()]))
    assert torch.equal(masks[0], masks[1]) and not torch.equal(masks[0], masks[2])
    assert not torch.equal(pr.mask_dict["a.weight"][0], pr.mask_dict["a.weight"][1])    # not one pattern repeated


@pytest.mark.parametrize("n, m", [(3, 4), (0, 4), (2, 8), (4, 4), (1, 2), (True, 4)])
def test_nm_refuses_other_patterns(tmp_path, n, m):
    with pytest.raises(ValueError):
        P.make_pruner(_cfg(tmp_path, n=n, m=m), on_gpu=False)


def test_nm_refuses_cin_not_multiple_of_4(tmp_path):
    net = _Net()
    net.c = torch.nn.Conv2d(6, 4, 3, bias=False)
    pr = P.NMPruner(_cfg(tmp_path, layers=("c.weight",)), on_gpu=False)
    with pytest.raises(ValueError):
        pr.generate_masks(net)


def test_nm_masks_round_trip(tmp_path):
    net = _Net()
    pr = P.NMPruner(_cfg(tmp_path), on_gpu=False)
    pr.generate_masks(net)
    path = str(tmp_path / "masks.npz")
    pr.save_masks(path)
    back = P.NMPruner(_cfg(tmp_path), on_gpu=False)
    back.load_masks(path)
    assert list(back.mask_dict) == list(pr.mask_dict)
    for k in pr.mask_dict:
        assert torch.equal(back.mask_dict[k].cpu().float(), pr.mask_dict[k])


# ----------------------------------------------------------------------------- route and status
def _args(cin=128, cout=256, ks=3, stride=1, dil=1, ho=6, wo=20, out="bf16", cout_pad=None, tile=-1, **over):
    a = _lib.ConvArgs()
    pad = dil * (ks // 2)
    a.x = a.wgt = a.shift = a.y = PTR
    a.n, a.ho, a.wo = 1, ho, wo
    a.h = (ho - 1) * stride + dil * (ks - 1) + 1 - 2 * pad
    a.w = (wo - 1) * stride + dil * (ks - 1) + 1 - 2 * pad
    a.cin, a.cout, a.ks, a.stride, a.pad, a.dil = cin, cout, ks, stride, pad, dil
    a.cout_pad = cout_pad or (cout + 127) // 128 * 128
    a.k = a.k_pad = ks * ks * cin
    a.relu, a.dtype, a.tile, a.algo = 1, _lib.DRNMI_BF16_SP24, tile, _lib.ALGO_IGEMM
    if out == "bf16":
        a.out_dtype, a.y_sn, a.y_sp, a.y_sc = _lib.DRNMI_BF16, ho * wo * cout, cout, 1
    elif out == "f32":                       # NCHW logits planes
        a.out_dtype, a.y_sn, a.y_sp, a.y_sc = _lib.DRNMI_F32, cout * ho * wo, 1, ho * wo
    else:                                    # "f32rows": NHWC logits rows
        cs = (cout + 3) // 4 * 4
        a.out_dtype, a.y_sn, a.y_sp, a.y_sc = _lib.DRNMI_F32, ho * wo * cs, cs, 1
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _route(a):
    lib = _lib.load()
    name = lib.drnmi_conv_kernel_name(ctypes.byref(a))
    return lib.drnmi_conv_status(ctypes.byref(a)), None if name is None else name.decode()


@pytest.mark.parametrize("kw, tile", [
    (dict(), "128, 2"), (dict(cin=64, cout=128), "128, 1"), (dict(cin=256, cout=160), "128, 2"),
    (dict(cin=512, cout=512, dil=4), "128, 2"), (dict(cin=512, cout=512, dil=2, wo=256, tile=_lib.SP24_GATHER), "128, 2"),
    (dict(cin=512, cout=512, dil=2, wo=256), "128, 2"),                     # auto is the gather on whole rows too
    (dict(cin=128, cout=128, wo=256), "128, 1"), (dict(wo=256, stride=2), "128, 2"), (dict(ks=1, wo=256), "128, 2"),
    (dict(ks=1, cin=256, cout=512), "128, 2"), (dict(ks=1, cin=64, cout=128, stride=2), "128, 1"),
    (dict(cin=128, cout=384), "128, 1"), (dict(stride=2, dil=2), "128, 2"), (dict(res=PTR, relu=0), "128, 2"),
    (dict(ks=1, cin=512, cout=19, out="f32"), "128, 1"), (dict(ks=1, cin=512, cout=19, out="f32rows"), "128, 1"),
    (dict(cout=128, cout_pad=256), "128, 1"), (dict(tile=_lib.SP24_GATHER), "128, 2"),
])
def test_accepted_shapes_name_a_sparse_kernel(kw, tile):
    a = _args(**kw)
    status, name = _route(a)
    assert status == 0 and name == f"conv_sp24_kernel<{a.ks}, {tile}>", (status, name)


@pytest.mark.parametrize("kw", [dict(wo=256), dict(cin=64, cout=160, wo=512, dil=4),
                                dict(cin=512, cout=512, dil=2, wo=256, ho=1, res=PTR), dict(wo=256, out="f32")])
def test_whole_rows_take_the_strip_form_when_forced(kw):
    assert _route(_args(tile=_lib.SP24_STRIP, **kw)) == (0, "conv_sp24_strip_kernel")
    assert _route(_args(**kw))[1].startswith("conv_sp24_kernel<3, 128, 2>")


ENOTSUP, EINVAL = -2, -1


@pytest.mark.parametrize("kw, want", [
    (dict(x2=PTR, cin2=64, h2=6, w2=20, stride2=1), ENOTSUP),
    (dict(unit_mask=PTR), ENOTSUP),
    (dict(scale=PTR), ENOTSUP),
    (dict(cin=96), EINVAL),                               # not a power of two
    (dict(cin=32), ENOTSUP),                              # below one K step
    (dict(cout=100, cout_pad=104), ENOTSUP),              # cout_pad % 128
    (dict(ks=7, cin=64), ENOTSUP),
    (dict(k_pad=9 * 128 + 64), ENOTSUP),                  # k_pad != k
    (dict(out_dtype=_lib.DRNMI_I8), EINVAL),
    (dict(out_dtype=_lib.DRNMI_F8), EINVAL),
    (dict(algo=_lib.ALGO_PATCH), EINVAL),
    (dict(tile=_lib.TILE_STAG), EINVAL),                  # tile is this dtype's own variant
    (dict(tile=_lib.SP24_STRIP), ENOTSUP),                # strip form forced on wo % 256 != 0
    (dict(tile=_lib.SP24_STRIP, wo=256, cout=128), ENOTSUP),      # the strip form is the 256-channel tile's
    (dict(tile=_lib.SP24_STRIP, wo=256, ks=1), ENOTSUP),
    (dict(tile=_lib.SP24_STRIP, wo=256, stride=2), ENOTSUP),
    (dict(tile=_lib.SP24_STRIP, wo=512, dil=8), ENOTSUP),         # the strip buffer holds 256 + 2 * 4 rows
    (dict(y_sp=300), ENOTSUP),                            # bf16 output rows wider than cout
])
def test_refusals(kw, want):
    status, name = _route(_args(**kw))
    assert name is None
    assert status == want, (kw, status)


def test_rows_must_exist():
    status, name = _route(_args(cout=300, cout_pad=512))
    assert (status, name) == (0, "conv_sp24_kernel<3, 128, 2>")
    status, name = _route(_args(cout=200, cout_pad=128))   # cout > cout_pad
    assert status == EINVAL and name is None


def test_seg_fused_entry_refuses_dtype_7():
    lib = _lib.load()
    a = _args(cin=512, cout=512, dil=2, wo=256, ho=2)
    assert lib.drnmi_conv_stag_seg_kernel_name(ctypes.byref(a)) is None
    assert lib.drnmi_conv_stag_seg(ctypes.byref(a), PTR, 512, 32, PTR, None) == ENOTSUP
    a.dtype = _lib.DRNMI_BF16                                # the same launch in bf16 has the fused form
    assert lib.drnmi_conv_stag_seg_kernel_name(ctypes.byref(a)) is not None


def test_other_dtypes_cannot_reach_the_sparse_rows():
    for dtype in (_lib.DRNMI_BF16, _lib.DRNMI_F32):
        for tile in list(range(-1, 24)):
            for kw in (dict(), dict(ks=1, cin=256, cout=512), dict(cin=64, cout=128)):
                _, name = _route(_args(dtype=dtype, tile=tile, **kw))
                assert name is None or "sp24" not in name


def test_pack_bytes_and_argument_checks():
    lib = _lib.load()
    assert lib.drnmi_sp24_pack_bytes(512, 4608) == 512 * 4608 * 9 // 8       # 0.5625 x the dense 2 B / weight
    assert lib.drnmi_sp24_pack_bytes(128, 64) == 128 * 64 + 128 * 8
    for rows, k in ((0, 64), (16, 64), (128, 32), (128, 96), (-128, 64), (128, 0)):
        assert lib.drnmi_sp24_pack_bytes(rows, k) == -1
    # refused before any HIP call: NULL operands, sizes, alignment
    assert lib.drnmi_sp24_pack(None, 128, 64, PTR, None, None) == EINVAL
    assert lib.drnmi_sp24_pack(PTR, 128, 64, None, None, None) == EINVAL
    assert lib.drnmi_sp24_pack(PTR, 100, 64, PTR, None, None) == EINVAL
    assert lib.drnmi_sp24_pack(PTR, 128, 64, PTR + 4, None, None) == EINVAL
    assert lib.drnmi_sp24_mma_probe(PTR, PTR, PTR, PTR, 2, None) == EINVAL


def test_abi_7_everywhere():
    text = open(os.path.join(ROOT, "include", "drnmi.h")).read()
    assert int(re.search(r"#define DRNMI_ABI_VERSION (\d+)", text).group(1)) == 7
    assert _lib.ABI_VERSION == 7 and _lib.load().drnmi_abi_version() == 7
    assert re.search(r"DRNMI_BF16_SP24 = 7\b", text) and _lib.DRNMI_BF16_SP24 == 7
    for name in ("drnmi_sp24_pack_bytes", "drnmi_sp24_pack", "drnmi_sp24_mma_probe"):
        assert name in _lib.SIGNATURES and re.search(r"\b%s\(" % name, text)


# ----------------------------------------------------------------------------- off by default
def _plan_signature(plan):
    lib = _lib.load()
    pointers = {"x", "wgt", "scale", "shift", "res", "y", "unit_mask", "x2", "ws", "stats"}
    out = []
    for src, labels_only in (("nchw", False), ("u8", False), ("u8", True)):
        for l in plan.launches(src, labels_only):
            a = plan.args[l.row]
            fields = None if a is None else tuple(
                (f, bool(getattr(a, f)) if f in pointers else (list(getattr(a, f)) if f in ("mean", "std") else getattr(a, f)))
                for f, _ in _lib.ConvArgs._fields_)
            out.append((src, labels_only, l.row, l.kind, l.nodes, l.reads, l.writes, l.quant, l.kernel_name(lib), fields))
    return out


def test_off_by_default_changes_nothing():
    from drnmi.drnseg import DRNSeg
    from drnmi.weights import synth_state_dict
    m = DRNSeg("drn_d_22", 19, pretrained=False)
    m.load_state_dict(synth_state_dict(m, 0))
    m.eval()
    assert m.sparse24 is False
    assert m.set_precision("bf16").sparse24_layers() == []
    assert m.set_sparse24(False) is m and m.sparse24 is False
    cpu = torch.device("cpu")
    absent = engine.PackedNet(m._graph, "bf16", cpu, block_sparse=False)
    off = engine.PackedNet(m._graph, "bf16", cpu, block_sparse=False, sparse24=False)
    assert absent.sparse24 is False and absent.sparse24_layers() == off.sparse24_layers() == []
    assert all(nd.wsp is None for nd in off.graph.nodes)
    a, b = engine.Plan(absent, 1, 64, 128), engine.Plan(off, 1, 64, 128)
    sig = _plan_signature(a)
    assert sig == _plan_signature(b)
    assert not any("sp24" in s[8] for s in sig) and all(s[9] is None or dict(s[9])["dtype"] != 7 for s in sig)
    # the switch is a bf16 switch: other precisions pack nothing sparse even when it is on
    on_fp32 = engine.PackedNet(m._graph, "fp32", cpu, block_sparse=False, sparse24=True)
    assert on_fp32.sparse24_layers() == []
    assert _plan_signature(engine.Plan(on_fp32, 1, 64, 128)) == \
        _plan_signature(engine.Plan(engine.PackedNet(m._graph, "fp32", cpu, block_sparse=False), 1, 64, 128))


def test_roofline_prices_sparse_launches_at_twice_the_bf16_peak():
    from drnmi import roofline
    assert roofline.kernel_peak("conv_sp24_kernel<3, 128, 2>", "bf16") == 2 * roofline.MFMA_PEAK["bf16"]
    assert roofline.kernel_peak("conv_big_kernel<3, 128, 2, 2, 64, false, 4, false, false>", "bf16") == roofline.MFMA_PEAK["bf16"]
