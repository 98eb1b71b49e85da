"""2:4 weight sparsity on v_smfmac_f32_16x16x64_bf16 (include/drnmi.h DRNMI_BF16_SP24, csrc/conv_sp24.hip)
on the GPU: the instruction's operand map, the kernel bit for bit on integer data and under
plan_audit.conv_gate on real data, the packer's violation count, and a 2:4-pruned D-22 end to end.

Whole 256-pixel output rows (borders on all four sides) run on the per-tap gather and, forced, on the
strip-staged form: the same sums in the same order, so the two agree bit for bit."""
import ctypes
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import plan_audit as A

pytestmark = pytest.mark.gpu
DEV = "cuda"

# kept positions of a group of four: the six pairs, one non-zero at each position, none
PATTERNS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3), (0,), (1,), (2,), (3,), ()]

# (n, h, w, cin, cout, ks, stride, dil, residual, relu): M = 15 (one partial tile) and 768 (three pixel
# tiles), cin 64 / 128 / 256, cout 128 / 160 (cout_pad 256, a partial channel tile) / 512 (two channel
# tiles), both kernel sizes, every dilation, both strides; then whole 256-pixel rows at dil 1 / 2 / 4
CASES = [
    (1, 3, 5, 64, 128, 3, 1, 1, False, False),
    (1, 3, 5, 128, 160, 1, 1, 1, True, True),
    (1, 3, 5, 256, 512, 3, 1, 2, True, True),
    (2, 16, 24, 64, 128, 1, 2, 1, False, True),
    (2, 16, 24, 128, 128, 3, 1, 2, True, True),
    (2, 16, 24, 256, 160, 3, 1, 4, True, False),
    (2, 16, 24, 128, 512, 3, 2, 1, False, True),
    (2, 16, 24, 256, 512, 1, 1, 1, True, True),
    (2, 16, 24, 64, 160, 3, 2, 2, False, False),
    (2, 16, 24, 256, 128, 3, 1, 1, False, True),
    (1, 2, 256, 128, 256, 3, 1, 1, True, True),
    (1, 6, 256, 64, 160, 3, 1, 4, False, True),
    (1, 6, 256, 256, 512, 3, 1, 2, True, False),
    (2, 2, 256, 128, 128, 3, 1, 1, False, True),       # whole rows on the 128-channel tile: the gather
    (1, 3, 5, 64, 512, 1, 1, 1, True, False),          # one K step (fewer than the ring's prologue) on the 256-channel tile
]


def _strip(case):
    """The launch has a strip-staged form (DRNMI_SP24_STRIP): 3x3 stride 1, whole 256-pixel rows, the 256-channel tile."""
    n, h, w, cin, cout, ks, st, dil, has_res, relu = case
    return ks == 3 and st == 1 and w % 256 == 0 and cout > 128


def _lib():
    from drnmi import _lib
    return _lib, _lib.load()


def _stream():
    from drnmi import _lib
    return ctypes.c_void_p(_lib.stream_ptr(torch.device(DEV)))


def _pattern_mask(rng, shape_groups):
    """0/1 mask [..., groups, 4] with every group's kept positions drawn from PATTERNS."""
    pid = rng.randint(0, len(PATTERNS), size=shape_groups)
    table = np.zeros((len(PATTERNS), 4), np.float32)
    for i, p in enumerate(PATTERNS):
        table[i, list(p)] = 1.0
    return table[pid], pid


def _geom(case):
    n, h, w, cin, cout, ks, st, dil, has_res, relu = case
    pad = dil * (ks // 2)
    ho = (h + 2 * pad - dil * (ks - 1) - 1) // st + 1
    wo = (w + 2 * pad - dil * (ks - 1) - 1) // st + 1
    return pad, ho, wo, (cout + 127) // 128 * 128


def _operands(case, integer):
    """x [n, h, w, cin], w [cout, ks, ks, cin] with a 2:4 pattern along cin (all eleven group patterns
    present), shift [cout_pad], res [n, ho, wo, cout]: small integers, or bf16-rounded real values."""
    n, h, w, cin, cout, ks, st, dil, has_res, relu = case
    pad, ho, wo, cout_pad = _geom(case)
    rng = np.random.RandomState(1000 + sum(case[:8]))
    mask, pid = _pattern_mask(rng, (cout, ks, ks, cin // 4))
    assert set(np.unique(pid)) == set(range(len(PATTERNS)))
    if integer:
        wv = rng.randint(1, 4, size=mask.shape) * rng.choice([-1, 1], size=mask.shape)       # {-3..3} without 0
        x = rng.randint(-4, 5, size=(n, h, w, cin))
        shift = rng.randint(-8, 9, size=cout_pad)
        res = rng.randint(-8, 9, size=(n, ho, wo, cout))
    else:
        wv = rng.randn(*mask.shape) / np.sqrt(ks * ks * cin / 2)
        wv = np.where(np.abs(wv) < 1e-3, 1e-3, wv)
        x = rng.randn(n, h, w, cin)
        shift = rng.randn(cout_pad) * 0.5
        res = rng.randn(n, ho, wo, cout)
    bf = lambda v: torch.from_numpy(np.asarray(v, np.float32)).to(torch.bfloat16)
    wt = bf((wv * mask).reshape(cout, ks, ks, cin))
    shift = torch.from_numpy(np.asarray(shift, np.float32))
    shift[cout:] = 0
    return bf(x), wt, shift, (bf(res) if has_res else None)


def _pack(wt, cout_pad):
    """dense bf16 [cout, ks, ks, cin] -> (dense packed [cout_pad, k] on the device, blob, violations)."""
    L, lib = _lib()
    cout = wt.shape[0]
    k = wt[0].numel()
    dense = torch.zeros(cout_pad, k, dtype=torch.bfloat16)
    dense[:cout] = wt.reshape(cout, k)
    dense = dense.to(DEV)
    nbytes = lib.drnmi_sp24_pack_bytes(cout_pad, k)
    assert nbytes == cout_pad * k * 9 // 8
    blob = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    cnt = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    L.check(lib.drnmi_sp24_pack(dense.data_ptr(), cout_pad, k, blob.data_ptr(), cnt.data_ptr(), _stream()), "sp24_pack")
    torch.cuda.synchronize()
    assert bool((blob[nbytes:] == 0xA5).all()), "the packer wrote past drnmi_sp24_pack_bytes"
    return dense, blob, int(cnt.item())


def _launch(case, x, blob, shift, res, out, tile=-1):
    """One DRNMI_BF16_SP24 launch -> [n, ho, wo, cout] on the host (fp32 from NCHW planes, or bf16 NHWC)."""
    L, lib = _lib()
    n, h, w, cin, cout, ks, st, dil, has_res, relu = case
    pad, ho, wo, cout_pad = _geom(case)
    t = {"x": x.to(DEV), "shift": shift.to(DEV), "res": res.to(DEV) if has_res else None}
    a = L.ConvArgs()
    a.x, a.wgt, a.scale, a.shift = t["x"].data_ptr(), blob.data_ptr(), None, t["shift"].data_ptr()
    a.res = t["res"].data_ptr() if has_res else None
    if out == "f32":
        y = torch.full((n, cout, ho, wo), float("nan"), device=DEV)
        a.y_sn, a.y_sp, a.y_sc, a.out_dtype = cout * ho * wo, 1, ho * wo, L.DRNMI_F32
    else:
        y = torch.full((n * ho * wo * cout + 64,), float("nan"), dtype=torch.bfloat16, device=DEV)
        a.y_sn, a.y_sp, a.y_sc, a.out_dtype = ho * wo * cout, cout, 1, L.DRNMI_BF16
    a.y = y.data_ptr()
    a.n, a.h, a.w, a.cin, a.ho, a.wo, a.cout, a.cout_pad = n, h, w, cin, ho, wo, cout, cout_pad
    a.ks, a.stride, a.pad, a.dil, a.k, a.k_pad = ks, st, pad, dil, ks * ks * cin, ks * ks * cin
    a.relu, a.dtype, a.tile, a.algo = int(relu), L.DRNMI_BF16_SP24, tile, L.ALGO_IGEMM
    name = lib.drnmi_conv_kernel_name(ctypes.byref(a))
    want = "conv_sp24_strip_kernel" if tile == L.SP24_STRIP else "conv_sp24_kernel<"
    assert name is not None and name.decode().startswith(want), (name, case, tile)
    L.check(lib.drnmi_conv2d_bn_act(ctypes.byref(a), _stream()), f"conv sp24 {case} {out}")
    torch.cuda.synchronize()
    if out == "f32":
        return y.cpu().permute(0, 2, 3, 1).contiguous()
    assert bool(torch.isnan(y[n * ho * wo * cout:].float()).all()), "wrote past the output"
    return y[:n * ho * wo * cout].cpu().view(n, ho, wo, cout)


def test_operand_map():
    """One v_smfmac_f32_16x16x64_bf16 against the CPU product, operands laid out by the map in
    include/drnmi.h (DRNMI_BF16_SP24): A 16 x 64 with a 2:4 pattern (every group pattern), B 64 x 16,
    integer-valued and asymmetric in every coordinate; both ABID halves, the other half inverted."""
    L, lib = _lib()
    rng = np.random.RandomState(24)
    mask, pid = _pattern_mask(rng, (16, 16))
    assert set(np.unique(pid)) == set(range(len(PATTERNS)))
    i, k, n = np.arange(16)[:, None], np.arange(64)[None, :], np.arange(16)[None, :]
    a_dense = ((1 + (3 * i + 5 * k) % 7) * np.where((i + k) % 3 == 0, -1, 1)) * mask.reshape(16, 64)   # |a| <= 7
    b_dense = (1 + (2 * np.arange(64)[:, None] + 7 * n) % 9) * np.where((np.arange(64)[:, None] + 2 * n) % 5 == 0, -1, 1)
    want = torch.from_numpy((a_dense @ b_dense).astype(np.float32))                                    # |sum| <= 64 * 63 < 2^24
    a_l = np.zeros((64, 8), np.float32)
    b_l = np.zeros((64, 16), np.float32)
    idx = np.zeros(64, np.uint32)
    for lane in range(64):
        fr, fq = lane & 15, lane >> 4
        for g in range(4):
            grp = a_dense[fr, 16 * fq + 4 * g:16 * fq + 4 * g + 4]
            pos = [p for p in range(4) if grp[p] != 0]
            pos = sorted(pos + [p for p in (3, 2, 1, 0) if p not in pos][:2 - len(pos)])
            for s, p in enumerate(pos):
                a_l[lane, 2 * g + s] = grp[p]
                idx[lane] |= np.uint32(p << (2 * (2 * g + s)))
        for e in range(16):
            b_l[lane, e] = b_dense[32 * (e // 8) + 8 * fq + e % 8, fr]
    a_t = torch.from_numpy(a_l).to(torch.bfloat16).to(DEV)
    b_t = torch.from_numpy(b_l).to(torch.bfloat16).to(DEV)
    for abid in (0, 1):
        word = idx | ((~idx & np.uint32(0xffff)) << np.uint32(16)) if abid == 0 else (idx << np.uint32(16)) | (~idx & np.uint32(0xffff))
        i_t = torch.from_numpy(word.view(np.int32).copy()).to(DEV)
        d = torch.full((64, 4), float("nan"), device=DEV)
        L.check(lib.drnmi_sp24_mma_probe(a_t.data_ptr(), b_t.data_ptr(), i_t.data_ptr(), d.data_ptr(), abid, _stream()), "probe")
        torch.cuda.synchronize()
        got = d.cpu().view(4, 16, 4).permute(0, 2, 1).reshape(16, 16)      # lane (fq, fr), reg r -> row 4 fq + r, column fr
        assert torch.equal(got, want), f"abid {abid}"


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(int(v)) for v in c))
def test_integer_exact(case):
    n, h, w, cin, cout, ks, st, dil, has_res, relu = case
    pad, ho, wo, cout_pad = _geom(case)
    x, wt, shift, res = _operands(case, integer=True)
    _, blob, viol = _pack(wt, cout_pad)
    assert viol == 0
    got = _launch(case, x, blob, shift, res, "f32")
    ref = F.conv2d(x.double().permute(0, 3, 1, 2), wt.double().permute(0, 3, 1, 2), stride=st, padding=pad, dilation=dil)
    ref = ref.permute(0, 2, 3, 1) + shift[:cout].double()
    if has_res:
        ref = ref + res.double()
    if relu:
        ref = ref.clamp_min(0)
    assert float(ref.abs().max()) <= 2304 * 12
    assert torch.equal(got, ref.float()), f"{int((got != ref.float()).sum())} of {ref.numel()} differ"
    if _strip(case):
        strip = _launch(case, x, blob, shift, res, "f32", tile=_lib()[0].SP24_STRIP)
        assert torch.equal(strip, ref.float()), "strip-staged form"


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(int(v)) for v in c))
def test_real_values_conv_gate(case):
    """bf16 output against float64 under tests/plan_audit.py's conv_gate, a = 4 x max |torch fp32 conv - float64|."""
    n, h, w, cin, cout, ks, st, dil, has_res, relu = case
    pad, ho, wo, cout_pad = _geom(case)
    x, wt, shift, res = _operands(case, integer=False)
    dense, blob, viol = _pack(wt, cout_pad)
    assert viol == 0
    got = _launch(case, x, blob, shift, res, "bf16").float().numpy()
    r = A.ConvRec(x=x.float().numpy(), wpk=dense.cpu().float().numpy(), shift=shift.numpy(), k=ks * ks * cin,
                  k_pad=ks * ks * cin, cout=cout, ks=ks, stride=st, pad=pad, dil=dil, relu=relu,
                  res=res.float().numpy() if has_res else None, got=got)
    st_ = A.check_conv(r)
    print(case, st_)
    if _strip(case):
        strip = _launch(case, x, blob, shift, res, "bf16", tile=_lib()[0].SP24_STRIP).float().numpy()
        assert np.array_equal(strip, got), "strip and gather forms differ"


def test_pack_counts_violations():
    rng = np.random.RandomState(5)
    mask, _ = _pattern_mask(rng, (128, 3, 3, 32))
    w = (rng.randint(1, 4, size=mask.shape) * mask).reshape(128, 3, 3, 128).astype(np.float32)
    wt = torch.from_numpy(w).to(torch.bfloat16)
    assert _pack(wt, 128)[2] == 0
    wt[77, 1, 2, 40:44] = torch.tensor([1.0, 0.0, -2.0, 3.0]).to(torch.bfloat16)       # one group of three
    assert _pack(wt, 128)[2] == 1
    wt[3, 0, 0, 0:4] = 1.0                                                               # and one of four
    assert _pack(wt, 128)[2] == 2
    wt[5, 0, 0, 4:8] = torch.tensor([-0.0, 0.0, 1.0, 2.0]).to(torch.bfloat16)           # -0 is a zero
    assert _pack(wt, 128)[2] == 2


# ----------------------------------------------------------------------------- network
_NET = {}


def _masked_d22(tmp_path_factory):
    """D-22 with NMPruner 2:4 magnitude masks applied to every conv with cin >= 64 (shared by the tests below)."""
    if "m" not in _NET:
        from drnmi import pruners as P
        from drnmi.drnseg import build
        from drnmi.weights import synth_frames
        m = build("drn_d_22", 19, seed=0, device=DEV)
        layers = [nd.name + ".weight" for nd in m._graph.nodes if nd.conv.in_channels >= 64]
        cfg = tmp_path_factory.mktemp("sp24") / "nm.json"
        cfg.write_text(json.dumps({"pruner_type": "nm", "configs": [{"layer_set": layers, "n": 2, "m": 4}]}))
        pr = P.make_pruner(str(cfg))
        pr.generate_masks(m)
        pr.apply_masks(m)
        _NET.update(m=m, layers=layers, frames=torch.from_numpy(synth_frames(7, 2, 128, 256)).to(DEV))
    return _NET["m"], _NET["layers"], _NET["frames"]


def test_network_sparse_launches_and_labels(tmp_path_factory):
    m, layers, frames = _masked_d22(tmp_path_factory)
    L, lib = _lib()
    try:
        ref = m.set_precision("fp32").segment(frames).cpu()
        m.set_precision("bf16")
        assert m.sparse24_layers() == []                              # off by default
        dense = m.segment(frames).cpu()
        m.set_sparse24(True)
        sparse = m.sparse24_layers()
        nodes = m._graph.nodes
        # eligible: pruned, cin >= 64, BN scale folded (the dense launch is one of the LDS-DMA kernels that
        # take scale = NULL), not the conv a 1x1 downsample is folded into (nor that downsample), not part
        # of the fused 64-channel block
        plan = m.plan(2, 128, 256)
        pk = plan.packed
        in_block = {j for i in pk.block_pairs[64] for j in (i, i + 1)}
        want = [nd.name for i, nd in enumerate(pk.graph.nodes)
                if nd.name + ".weight" in layers and nd.scale_folded and not nd.fused and nd.fused_into < 0
                and i not in in_block]
        assert sparse == want and len(sparse) >= 10, (sparse, want)
        assert "layer.8.0" in sparse and "layer.7.0" in sparse and "seg" in sparse
        labels = torch.empty(2, *plan.out_hw, dtype=torch.uint8, device=DEV)
        by_row = {l.row: l for l in plan.launches("u8", True)}
        ins, outs, names = {}, {}, {}

        def hook(i, nd, start):
            if nd is None or nd.name not in sparse:
                return
            torch.cuda.synchronize()
            if start:
                names[i] = by_row[i].kernel_name(lib)
                ins[i] = {v: plan.bufs[v].cpu().clone() for v in by_row[i].reads}
            else:
                outs[i] = plan.bufs[by_row[i].writes[0]].cpu().clone()
        m.timing_hook = hook
        try:
            got = m.segment(frames, labels=labels).cpu()
        finally:
            m.timing_hook = None
        assert plan.labels_path() == "nhwc"                           # a sparse layer8: the separate seg conv
        assert sorted(pk.graph.nodes[i].name for i in names) == sorted(sparse)
        assert all(k.startswith("conv_sp24_kernel<") for k in names.values()), names
        n = 2
        for i in sorted(names):
            nd = pk.graph.nodes[i]
            c = nd.conv
            ih, iw = plan.shapes[nd.src]
            oh, ow = plan.shapes[nd.dst]
            cout = c.out_channels
            if nd.out_fp32_nchw:
                o = outs[i].view(n, oh, ow, plan.seg_cs)[..., :cout].float().numpy()
            else:
                o = outs[i].view(n, oh, ow, cout).float().numpy()
            r = A.ConvRec(x=ins[i][nd.x_val].float().numpy().reshape(n, ih, iw, nd.cin_stride), wpk=nd.wpk.cpu().float().numpy(),
                          shift=nd.shift.cpu().numpy(), k=nd.k, k_pad=nd.k_pad, cout=cout, ks=c.kernel_size[0],
                          stride=c.stride[0], pad=c.padding[0], dil=c.dilation[0], relu=bool(nd.relu),
                          res=ins[i][nd.r_val].float().numpy().reshape(n, oh, ow, cout) if nd.r_val else None, got=o)
            print(nd.name, names[i], A.check_conv(r))
        agree = (got == ref).float().mean().item()
        print(f"2:4 D-22 2x128x256: sparse vs fp32 {agree:.4f}, dense bf16 vs fp32 {(dense == ref).float().mean().item():.4f}, "
              f"sparse vs dense bf16 {(got == dense).float().mean().item():.4f}")
        assert agree >= 0.990
    finally:
        m.timing_hook = None
        m.set_sparse24(False).set_precision("fp32")


def test_network_violation_keeps_layer_dense(tmp_path_factory):
    m, layers, frames = _masked_d22(tmp_path_factory)
    w = m.state_dict()["layer.7.0.weight"]
    saved = w[9, 4:8, 1, 1].clone()
    try:
        m.set_precision("bf16").set_sparse24(True)
        assert "layer.7.0" in m.sparse24_layers()
        with torch.no_grad():
            w[9, 4:8, 1, 1] = torch.tensor([0.5, 0.25, -0.5, 0.0], device=w.device)    # three non-zeros in one group
        got = m.sparse24_layers()
        assert "layer.7.0" not in got and "layer.8.0" in got
        plan = m.plan(2, 128, 256)
        i = [nd.name for nd in plan.packed.graph.nodes].index("layer.7.0")
        assert plan.args[i].dtype == _lib()[0].DRNMI_BF16
    finally:
        with torch.no_grad():
            w[9, 4:8, 1, 1] = saved
        m.set_sparse24(False).set_precision("fp32")


def test_network_graph_capture(tmp_path_factory):
    m, layers, frames = _masked_d22(tmp_path_factory)
    from drnmi.drnseg import INFO_MEAN, INFO_STD
    from drnmi.weights import synth_frames
    mean, std = [float(v) for v in INFO_MEAN], [float(v) for v in INFO_STD]
    frames = frames.clone()

    def step():
        return torch.ops.drnmi.segment(frames, m._handle, mean, std, False)

    try:
        m.set_precision("bf16").set_sparse24(True)
        s = torch.cuda.Stream()                  # warm-up off the capture: packing, plan buffers, attributes
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                step()
        torch.cuda.current_stream().wait_stream(s)
        assert m.sparse24_layers()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = step()
        for seed in (4, 11):
            frames.copy_(torch.from_numpy(synth_frames(seed, 2, 128, 256)).to(DEV))
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(captured, step())
        assert len(captured.unique()) > 1
    finally:
        m.set_sparse24(False).set_precision("fp32")
