"""conv_psp_kernel (include/drnmi.h DRNMI_BF16_PSP, csrc/conv_psp.hip) on the GPU against a plain float64
F.conv2d on the masked weights: bit for bit on small integers (fp32 output), under plan_audit.check_conv on
real values (bf16 output); and an SRMB-masked D-22 end to end."""
import ctypes
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import plan_audit as A
from test_srmb_sparse import psp_pack, srmb_weight

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (n, h, w, cin, cout, ks, dil, residual, relu, cb, ib, isp): 2 x 9 x 13 is two pixel tiles, the second ragged;
# cin is two K steps (128 at d / P = 16 / 32, 256 at 16 / 64 and 8 / 32, 512 at 8 / 64); cout 128 with cbh 8 is
# eight 16-row classes, cout 512 with cbh 32 four tiles of eight; ib 2 x 2 at cbh 64 gives classes of 16 and 48 rows
CASES = [
    (2, 9, 13, 128, 128, 3, 1, False, False, (8, 32), 1, 0.5),
    (2, 9, 13, 128, 128, 3, 2, True, True, (8, 32), 1, 0.5),
    (1, 8, 8, 128, 128, 1, 1, True, False, (8, 32), 1, 0.5),
    (2, 9, 13, 256, 128, 3, 4, True, True, (8, 64), 1, 0.75),
    (1, 8, 8, 256, 128, 1, 1, False, True, (8, 64), 1, 0.75),
    (2, 9, 13, 512, 128, 3, 2, False, True, (8, 64), 1, 0.875),
    (1, 8, 8, 512, 128, 1, 1, True, True, (8, 64), 1, 0.875),
    (2, 9, 13, 256, 128, 3, 1, True, True, (16, 32), 2, 0.75),
    (1, 8, 8, 128, 512, 3, 2, True, True, (32, 32), 1, 0.5),
    (1, 8, 8, 256, 512, 3, 1, False, True, (64, 32), 2, 0.75),
]
_ID = lambda c: "x".join(str(v).replace(" ", "") for v in c)


def _operands(case, integer):
    n, h, w, cin, cout, ks, dil, has_res, relu, cb, ib, isp = case
    wi = torch.from_numpy(srmb_weight(cout, cin, ks, cb, ib, isp, seed=sum(case[:7]))).view(torch.bfloat16)   # +-{1, 2, 3}
    rng = np.random.RandomState(7 + sum(case[:7]))
    bf = lambda v: torch.from_numpy(np.asarray(v, np.float32)).to(torch.bfloat16)
    if integer:
        wt, x = wi, bf(rng.randint(-4, 5, size=(n, h, w, cin)))
        shift, res = rng.randint(-8, 9, size=cout), bf(rng.randint(-8, 9, size=(n, h, w, cout)))
    else:
        wt = (wi.float() * bf(rng.rand(cout, ks * ks * cin) + 0.5).float() / (3 * np.sqrt(ks * ks * cin * (1 - isp)))).to(torch.bfloat16)
        x, shift, res = bf(rng.randn(n, h, w, cin)), rng.randn(cout) * 0.5, bf(rng.randn(n, h, w, cout))
    return x, wt.contiguous(), torch.from_numpy(np.asarray(shift, np.float32)), (res if has_res else None)


def _launch(case, x, wt, shift, res, out):
    """Pack on the host, one DRNMI_BF16_PSP launch -> [n, h, w, cout] on the host."""
    from drnmi import _lib as L
    lib = L.load()
    n, h, w, cin, cout, ks, dil, has_res, relu, cb, ib, isp = case
    variant, viol, blob = psp_pack(wt.view(torch.int16).numpy(), cin, ks)
    assert viol == 0 and L.PSP_VARIANTS[variant][1] / L.PSP_VARIANTS[variant][0] == 1 - isp
    t = {"x": x.to(DEV), "shift": shift.to(DEV), "res": res.to(DEV) if has_res else None, "blob": torch.from_numpy(blob).to(DEV)}
    a = L.ConvArgs()
    a.x, a.wgt, a.scale, a.shift = t["x"].data_ptr(), t["blob"].data_ptr(), None, t["shift"].data_ptr()
    a.res = t["res"].data_ptr() if has_res else None
    if out == "f32":                              # NCHW planes: the strided element stores
        y = torch.full((n, cout, h, w), float("nan"), device=DEV)
        a.y_sn, a.y_sp, a.y_sc, a.out_dtype = cout * h * w, 1, h * w, L.DRNMI_F32
    else:                                         # NHWC rows: the 16-B stores
        y = torch.full((n * h * w * cout + 64,), float("nan"), dtype=torch.bfloat16, device=DEV)
        a.y_sn, a.y_sp, a.y_sc, a.out_dtype = h * w * cout, cout, 1, L.DRNMI_BF16
    a.y = y.data_ptr()
    a.n, a.h, a.w, a.cin, a.ho, a.wo, a.cout, a.cout_pad = n, h, w, cin, h, w, cout, cout
    a.ks, a.stride, a.pad, a.dil, a.k, a.k_pad = ks, 1, dil * (ks // 2), dil, ks * ks * cin, ks * ks * cin
    a.relu, a.dtype, a.tile, a.algo = int(relu), L.DRNMI_BF16_PSP, variant, L.ALGO_IGEMM
    name = lib.drnmi_conv_kernel_name(ctypes.byref(a))
    P, d = L.PSP_VARIANTS[variant]
    assert name is not None and name.decode() == f"conv_psp_kernel<{ks}, {P // d}, {d}>", name
    a.tile = L.TILE_AUTO
    assert lib.drnmi_conv_kernel_name(ctypes.byref(a)) is None        # the blob's (P, d) must be named
    a.tile = variant
    L.check(lib.drnmi_conv2d_bn_act(ctypes.byref(a), ctypes.c_void_p(L.stream_ptr(torch.device(DEV)))), f"conv psp {case}")
    torch.cuda.synchronize()
    if out == "f32":
        return y.cpu().permute(0, 2, 3, 1).contiguous()
    assert bool(torch.isnan(y[n * h * w * cout:].float()).all()), "wrote past the output"
    return y[:n * h * w * cout].cpu().view(n, h, w, cout)


@pytest.mark.parametrize("case", CASES, ids=_ID)
def test_integer_exact(case):
    n, h, w, cin, cout, ks, dil, has_res, relu, cb, ib, isp = case
    x, wt, shift, res = _operands(case, integer=True)
    got = _launch(case, x, wt, shift, res, "f32")
    w4 = wt.double().view(cout, ks, ks, cin).permute(0, 3, 1, 2)
    ref = F.conv2d(x.double().permute(0, 3, 1, 2), w4, padding=dil * (ks // 2), dilation=dil).permute(0, 2, 3, 1) + shift.double()
    if has_res:
        ref = ref + res.double()
    if relu:
        ref = ref.clamp_min(0)
    assert float(ref.abs().max()) < 2 ** 24 and float(ref.abs().max()) > 16
    assert torch.equal(got, ref.float()), f"{int((got != ref.float()).sum())} of {ref.numel()} differ"


@pytest.mark.parametrize("case", CASES, ids=_ID)
def test_real_values_conv_gate(case):
    """bf16 output against float64 under tests/plan_audit.py's conv gate (4 x the error of torch's fp32 conv)."""
    n, h, w, cin, cout, ks, dil, has_res, relu, cb, ib, isp = case
    x, wt, shift, res = _operands(case, integer=False)
    got = _launch(case, x, wt, shift, res, "bf16").float().numpy()
    r = A.ConvRec(x=x.float().numpy(), wpk=wt.float().numpy(), shift=shift.numpy(), k=ks * ks * cin, k_pad=ks * ks * cin,
                  cout=cout, ks=ks, stride=1, pad=dil * (ks // 2), dil=dil, relu=relu,
                  res=res.float().numpy() if has_res else None, got=got)
    print(case, A.check_conv(r))


def test_network():
    """D-22 under the committed SRMB 50 % masks at 1 x 64 x 128: the routed set, labels against the dense bf16 run
    of the same masked model (the bf16 label gate), and bit-identity with the switch off again."""
    from drnmi import engine, pruners as P
    from drnmi.drnseg import build
    from drnmi.weights import synth_frames
    m = build("drn_d_22", 19, seed=0, device=DEV)
    pr = P.make_pruner(str(Path(__file__).parent / "golden" / "srmb_d22_1024X768_50.json"))
    np.random.seed(22)
    pr.generate_masks(m, is_static=True)
    pr.apply_masks(m)
    frames = torch.from_numpy(synth_frames(7, 1, 64, 128)).to(DEV)
    m.set_precision("bf16")
    dense = m.segment(frames).cpu()
    path = m.plan(1, 64, 128).labels_path()
    assert m.srmb_sparse_layers() == []
    m.set_srmb_sparse(True)
    routed = m.srmb_sparse_layers()
    plan = m.plan(1, 64, 128)
    pk = plan.packed
    in_block = {j for pairs in pk.block_pairs.values() for i in pairs for j in (i, i + 1)}
    sd = m.state_dict()
    want = []
    for i, nd in enumerate(pk.graph.nodes):
        c = nd.conv
        if nd.name + ".weight" not in pr.mask_dict or c.out_channels % 128 or c.stride[0] != 1 or nd.cin_stride < 64 or \
                not nd.scale_folded or nd.fused or nd.fused_into >= 0 or i in in_block or nd.unit_mask is not None:
            continue
        wq = sd[nd.name + ".weight"].permute(0, 2, 3, 1).reshape(c.out_channels, -1).to(torch.bfloat16).contiguous().cpu()
        if psp_pack(wq.view(torch.int16).numpy(), c.in_channels, c.kernel_size[0])[0] >= 0:
            want.append(nd.name)
    fused_l8 = engine.SEG_FUSE and "layer.8.0" in want
    if fused_l8:
        want.remove("layer.8.0")                  # kept dense: its epilogue takes the seg classifier
    assert routed == want and "layer.7.0" in routed and len(routed) >= 4, (routed, want)
    names = {plan.packed.graph.nodes[l.row].name: l.kernel_name(engine._lib.load()) for l in plan.launches("u8", True)}
    assert all(names[r].startswith("conv_psp_kernel<") for r in routed), names
    got = m.segment(frames).cpu()
    assert plan.labels_path() == path             # the switch costs no plan its seg fusion
    agree = (got == dense).float().mean().item()
    print(f"SRMB 50 % D-22 1x64x128: {routed}; period-sparse vs dense bf16 labels {agree:.4f}")
    assert agree >= 0.990
    m.set_srmb_sparse(False)
    assert m.srmb_sparse_layers() == [] and torch.equal(m.segment(frames).cpu(), dense)
