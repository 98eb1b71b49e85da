"""2:4 weight sparsity at int8 on v_smfmac_i32_16x16x128_i8 (include/drnmi.h DRNMI_I8_SP24,
csrc/conv_sp24_i8.hip) on the GPU: the instruction's operand map, the packer, every launch bit for bit
against oracle/int8_oracle.conv_i8 on the dense masked weights, and a 2:4-pruned, calibrated D-22 whose
labels must equal the dense int8 network's.

int32 accumulation is exact, so nothing here has a tolerance."""
import ctypes
import json

import numpy as np
import pytest
import torch

from oracle import int8_oracle as Q
from test_gpu_sp24 import PATTERNS, _pattern_mask

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _lib():
    from drnmi import _lib
    return _lib, _lib.load()


def _stream():
    from drnmi import _lib
    return ctypes.c_void_p(_lib.stream_ptr(torch.device(DEV)))


def _nonzero_i8(rng, shape):
    """Full-range int8 without 0 and -128."""
    return (rng.randint(1, 128, size=shape) * rng.choice([-1, 1], size=shape)).astype(np.int8)


# ----------------------------------------------------------------------------- the instruction
def test_operand_map():
    """One v_smfmac_i32_16x16x128_i8 against the integer product, operands laid out by the map in
    include/drnmi.h (DRNMI_I8_SP24): A 16 x 128 with a 2:4 pattern (every group pattern), B 128 x 16,
    full-range int8.  The 16 kept values of a lane take 2 bits each: the index register has no unused
    field to invert (ABID selects nothing at this width)."""
    L, lib = _lib()
    rng = np.random.RandomState(24)
    mask, pid = _pattern_mask(rng, (16, 32))
    assert set(np.unique(pid)) == set(range(len(PATTERNS)))
    a_dense = _nonzero_i8(rng, (16, 128)).astype(np.int64) * mask.reshape(16, 128).astype(np.int64)
    b_dense = rng.randint(-127, 128, size=(128, 16)).astype(np.int64)
    want = torch.from_numpy((a_dense @ b_dense).astype(np.int32))           # |sum| <= 64 * 127 * 127 < 2^31
    a_l = np.zeros((64, 16), np.int8)
    b_l = np.zeros((64, 32), np.int8)
    idx = np.zeros(64, np.uint32)
    for lane in range(64):
        fr, fq = lane & 15, lane >> 4
        for g in range(8):
            grp = a_dense[fr, 32 * fq + 4 * g:32 * fq + 4 * g + 4]
            pos = [p for p in range(4) if grp[p] != 0]
            pos = sorted(pos + [p for p in (3, 2, 1, 0) if p not in pos][:2 - len(pos)])
            for s, p in enumerate(pos):
                a_l[lane, 2 * g + s] = grp[p]
                idx[lane] |= np.uint32(p << (2 * (2 * g + s)))
        for e in range(32):
            b_l[lane, e] = b_dense[64 * (e // 16) + 16 * fq + e % 16, fr]
    a_t, b_t = torch.from_numpy(a_l).to(DEV), torch.from_numpy(b_l).to(DEV)
    i_t = torch.from_numpy(idx.view(np.int32).copy()).to(DEV)
    d = torch.full((64, 4), -(2 ** 31), dtype=torch.int32, device=DEV)
    L.check(lib.drnmi_sp24_mma_probe_i8(a_t.data_ptr(), b_t.data_ptr(), i_t.data_ptr(), d.data_ptr(), _stream()), "probe")
    torch.cuda.synchronize()
    got = d.cpu().view(4, 16, 4).permute(0, 2, 1).reshape(16, 16)          # lane (fq, fr), reg r -> row 4 fq + r, column fr
    assert torch.equal(got, want), f"{int((got != want).sum())} of 256 differ"


# ----------------------------------------------------------------------------- the packer
def _pack(wpk):
    """dense int8 [cout_pad, k] (numpy) -> (blob on the device, violations); checks the size and a guard tail."""
    L, lib = _lib()
    rows, k = wpk.shape
    dense = torch.tensor(wpk, device=DEV)
    nbytes = lib.drnmi_sp24_pack_i8_bytes(rows, k)
    assert nbytes == rows * k * 5 // 8
    blob = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    cnt = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    L.check(lib.drnmi_sp24_pack_i8(dense.data_ptr(), rows, k, blob.data_ptr(), cnt.data_ptr(), _stream()), "sp24_pack_i8")
    torch.cuda.synchronize()
    assert bool((blob[nbytes:] == 0xA5).all()), "the packer wrote past drnmi_sp24_pack_i8_bytes"
    return blob, int(cnt.item())


def test_pack_counts_violations():
    rng = np.random.RandomState(5)
    mask, _ = _pattern_mask(rng, (128, 3, 3, 32))
    w = (_nonzero_i8(rng, mask.shape) * mask.astype(np.int8)).reshape(128, 3, 3, 128)
    assert _pack(w.reshape(128, -1))[1] == 0                   # violations starts from the -7 sentinel: reset by the call
    w[77, 1, 2, 40:44] = [1, 0, -2, 3]                         # one group of three
    assert _pack(w.reshape(128, -1))[1] == 1
    w[3, 0, 0, 0:4] = 1                                        # and one of four
    assert _pack(w.reshape(128, -1))[1] == 2
    w[5, 0, 0, 4:8] = [0, 0, 1, -128]                          # zero is no violation
    assert _pack(w.reshape(128, -1))[1] == 2
    w[77, 1, 2, 40:44] = [1, 0, 0, 3]
    w[3, 0, 0, 0:4] = [0, 0, 0, 0]
    assert _pack(w.reshape(128, -1))[1] == 0                   # and the count does not carry over


# ----------------------------------------------------------------------------- one launch
# (n, h, w, cin, cout, ks, stride, dil, residual, output): the smallest shapes that reach each path
CASES = [
    (1, 3, 5, 128, 128, 3, 1, 1, False, "i8"),              # one partial pixel tile
    (1, 3, 5, 128, 512, 1, 1, 1, False, "f32"),             # one K step (fewer than the ring prologue), 256-channel tile
    (1, 3, 5, 256, 160, 3, 1, 2, True, "bf16"),             # partial channel tile (cout_pad 256)
    (2, 16, 24, 128, 130, 3, 1, 1, True, "bf16"),           # cout % 4 != 0
    (2, 16, 24, 256, 512, 3, 2, 1, False, "i8"),            # stride 2
    (2, 16, 24, 512, 256, 1, 2, 1, False, "i8"),            # 1x1 stride 2
    (2, 16, 24, 128, 512, 3, 1, 4, True, "f32"),            # dilation 4, fp32 planes
    (1, 10, 10, 512, 19, 1, 1, 1, False, "f32rows20"),      # labels-head rows
    (1, 10, 10, 512, 19, 1, 1, 1, False, "f32slice28"),     # a channel slice: the other channels keep the sentinel
    (1, 2, 256, 128, 256, 3, 1, 1, True, "i8"),             # whole 256-pixel rows (also the strip form)
    (1, 6, 256, 256, 512, 3, 1, 2, False, "bf16"),
    (1, 6, 256, 128, 256, 3, 1, 4, False, "i8"),
    (2, 2, 256, 128, 128, 3, 1, 1, False, "i8"),            # whole rows on the 128-channel tile
]
RES_SCALE, OUT_SCALE = 0.011, 1.0 / 0.023
_REF = {}


def _strip(case):
    n, h, w, cin, cout, ks, st, dil, has_res, out = case
    return ks == 3 and st == 1 and w % 256 == 0 and cout > 128


def _geom(case):
    n, h, w, cin, cout, ks, st, dil, has_res, out = case
    pad = dil * (ks // 2)
    ho = (h + 2 * pad - dil * (ks - 1) - 1) // st + 1
    wo = (w + 2 * pad - dil * (ks - 1) - 1) // st + 1
    return pad, ho, wo, (cout + 127) // 128 * 128


def _operands(case):
    """x and w uniform in [-127, 127], w times a 2:4 pattern mask (all eleven group patterns present); the
    scale keeps v ~ N(0, 1) with half of the products zero.  Computed once per case, with the oracle's output."""
    if case in _REF:
        return _REF[case]
    n, h, w, cin, cout, ks, st, dil, has_res, out = case
    pad, ho, wo, cout_pad = _geom(case)
    rng = np.random.RandomState(2000 + CASES.index(case))
    k = ks * ks * cin
    mask, pid = _pattern_mask(rng, (cout, ks, ks, cin // 4))
    assert set(np.unique(pid)) == set(range(len(PATTERNS)))
    x = rng.randint(-127, 128, size=(n, h, w, cin)).astype(np.int8)
    wpk = np.zeros((cout_pad, k), np.int8)
    wpk[:cout] = (rng.randint(-127, 128, size=mask.shape) * mask).astype(np.int8).reshape(cout, k)
    scale = np.zeros(cout_pad, np.float32)
    shift = np.zeros(cout_pad, np.float32)
    scale[:cout] = (rng.uniform(0.5, 1.5, cout) / (np.sqrt(k / 2) * 5400.0)).astype(np.float32)
    shift[:cout] = rng.normal(0, 0.5, cout).astype(np.float32)
    res = rng.randint(-127, 128, size=(n, ho, wo, cout)).astype(np.int8) if has_res else None
    relu = (not out.startswith("f32")) or has_res
    ref = Q.conv_i8(x, wpk, scale, shift, cout, ks, st, pad, dil, relu, res, RES_SCALE,
                    "f32" if out.startswith("f32") else out, OUT_SCALE)
    if out == "i8":
        assert (ref == 127).mean() < 0.5
    for v in (x, wpk, scale, shift, ref) + ((res,) if has_res else ()):
        v.setflags(write=False)
    _REF[case] = (x, wpk, scale, shift, res, relu, ref)
    return _REF[case]


def _launch(case, blob, tile=-1):
    """One DRNMI_I8_SP24 launch -> the output as the oracle returns it; checks that nothing outside it is written."""
    L, lib = _lib()
    n, h, w, cin, cout, ks, st, dil, has_res, out = case
    pad, ho, wo, cout_pad = _geom(case)
    x, wpk, scale, shift, res, relu, ref = _operands(case)
    t = {"x": torch.tensor(x, device=DEV), "sc": torch.tensor(scale, device=DEV), "sh": torch.tensor(shift, device=DEV),
         "res": torch.tensor(res, device=DEV) if has_res else None}
    a = L.ConvArgs()
    a.x, a.wgt, a.scale, a.shift = t["x"].data_ptr(), blob.data_ptr(), t["sc"].data_ptr(), t["sh"].data_ptr()
    a.res = t["res"].data_ptr() if has_res else None
    numel = n * ho * wo * cout
    if out == "f32":
        y = torch.full((numel + 64,), float("nan"), device=DEV)
        a.y_sn, a.y_sp, a.y_sc, a.out_dtype = cout * ho * wo, 1, ho * wo, L.DRNMI_F32
    elif out.startswith("f32"):
        ysp = int(out[len("f32rows"):] if out.startswith("f32rows") else out[len("f32slice"):])
        numel = n * ho * wo * ysp
        y = torch.full((numel + 64,), 7.0, device=DEV)
        a.y_sn, a.y_sp, a.y_sc, a.out_dtype = ho * wo * ysp, ysp, 1, L.DRNMI_F32
    elif out == "bf16":
        y = torch.full((numel + 64,), float("nan"), dtype=torch.bfloat16, device=DEV)
        a.y_sn, a.y_sp, a.y_sc, a.out_dtype = ho * wo * cout, cout, 1, L.DRNMI_BF16
    else:
        y = torch.full((numel + 64,), -128, dtype=torch.int8, device=DEV)        # outputs are clamped to +-127
        a.y_sn, a.y_sp, a.y_sc, a.out_dtype = ho * wo * cout, cout, 1, L.DRNMI_I8
    a.y = y.data_ptr()
    a.n, a.h, a.w, a.cin, a.ho, a.wo, a.cout, a.cout_pad = n, h, w, cin, ho, wo, cout, cout_pad
    a.ks, a.stride, a.pad, a.dil, a.k, a.k_pad = ks, st, pad, dil, ks * ks * cin, ks * ks * cin
    a.relu, a.dtype, a.tile, a.algo = int(relu), L.DRNMI_I8_SP24, tile, L.ALGO_IGEMM
    a.res_scale, a.out_scale = RES_SCALE, OUT_SCALE
    name = lib.drnmi_conv_kernel_name(ctypes.byref(a))
    tile_name = "128, 2" if cout_pad % 256 == 0 and cout > 128 else "128, 1"
    want = "conv_sp24_i8_strip_kernel" if tile == L.SP24_STRIP else f"conv_sp24_i8_kernel<{ks}, {tile_name}>"
    assert name is not None and name.decode() == want, (name, case, tile)
    L.check(lib.drnmi_conv2d_bn_act(ctypes.byref(a), _stream()), f"conv sp24 i8 {case}")
    torch.cuda.synchronize()
    tail, body = y[numel:].cpu(), y[:numel].cpu()
    if out == "i8":
        assert bool((tail == -128).all()), "wrote past the output"
        return body.numpy().reshape(n, ho, wo, cout)
    if out == "bf16":
        assert bool(torch.isnan(tail.float()).all()), "wrote past the output"
        return body.view(torch.int16).numpy().view(np.uint16).reshape(n, ho, wo, cout)
    if out == "f32":
        assert bool(torch.isnan(tail).all()), "wrote past the output"
        return body.numpy().reshape(n, cout, ho, wo).transpose(0, 2, 3, 1)
    assert bool((tail == 7.0).all()), "wrote past the output"
    got = body.numpy().reshape(n, ho, wo, -1)
    if out.startswith("f32slice"):
        assert bool((got[..., cout:] == 7.0).all()), "a wider buffer's other channels were touched"
    return got[..., :cout]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_conv_matches_int8_oracle(case):
    x, wpk, scale, shift, res, relu, ref = _operands(case)
    blob, viol = _pack(wpk)
    assert viol == 0
    np.testing.assert_array_equal(_launch(case, blob), ref)
    if _strip(case):
        np.testing.assert_array_equal(_launch(case, blob, tile=_lib()[0].SP24_STRIP), ref, err_msg="strip-staged form")


# ----------------------------------------------------------------------------- network
_NET = {}


def _masked_int8_d22(tmp_path_factory):
    """D-22 with NMPruner 2:4 magnitude masks on every conv with cin >= 64, calibrated for int8 (shared below)."""
    if "m" not in _NET:
        from drnmi import pruners as P
        from drnmi.drnseg import build
        from drnmi.weights import synth_frames
        m = build("drn_d_22", 19, seed=0, device=DEV)
        layers = [nd.name + ".weight" for nd in m._graph.nodes if nd.conv.in_channels >= 64]
        cfg = tmp_path_factory.mktemp("sp24_i8") / "nm.json"
        cfg.write_text(json.dumps({"pruner_type": "nm", "configs": [{"layer_set": layers, "n": 2, "m": 4}]}))
        pr = P.make_pruner(str(cfg))
        pr.generate_masks(m)
        pr.apply_masks(m)
        frames = torch.from_numpy(synth_frames(7, 2, 128, 256)).to(DEV)
        m.calibrate_int8(frames)
        _NET.update(m=m, frames=frames)
    return _NET["m"], _NET["frames"]


def _norm():
    from drnmi.drnseg import INFO_MEAN, INFO_STD
    return INFO_MEAN, INFO_STD


def test_network_every_eligible_layer_sparse(tmp_path_factory, monkeypatch):
    from drnmi import engine
    m, frames = _masked_int8_d22(tmp_path_factory)
    L, lib = _lib()
    n, h, w = frames.shape[:3]
    try:
        m.set_precision("int8")
        assert m.sparse24_layers() == []                              # off by default
        dense = m.segment(frames).cpu()
        assert len(dense.unique()) > 1
        monkeypatch.setattr(engine, "SP24_I8_EVERY", True)
        m.set_sparse24(True)
        sparse = m.sparse24_layers()
        plan = m.plan(n, h, w, keep_all=True)
        pk = plan.packed
        want = [pk.graph.nodes[i].name for i in pk.sp24_i8_candidates()]
        assert want == [nd.name for nd in pk.graph.nodes if nd.i8 and nd.cin_stride >= 128]
        assert sparse == want and len(sparse) >= 10, (sparse, want)
        assert {"layer.7.0", "layer.8.0", "seg"} <= set(sparse)
        # every launch, all activations kept: sparse launches name the sparse kernel and equal conv_i8 on the
        # dense masked wpk from their own inputs, bit for bit
        names = {l.row: l.kernel_name(lib) for l in plan.launches("u8", False)}
        stream = L.stream_ptr(torch.device(DEV))
        plan.ingest_u8(frames, *_norm(), False, stream)
        plan.run_backbone(stream)
        torch.cuda.synchronize()
        for i, nd in enumerate(pk.graph.nodes):
            if nd.name not in sparse:
                assert "sp24" not in (names.get(i) or "")
                continue
            assert names[i].startswith("conv_sp24_i8_kernel<"), (nd.name, names[i])
            assert plan.args[i].dtype == L.DRNMI_I8_SP24
            c = nd.conv
            ih, iw = plan.shapes[nd.src]
            oh, ow = plan.shapes[nd.dst]
            x = plan.bufs[nd.x_val].cpu().numpy().reshape(n, ih, iw, pk.cstride[nd.src])
            res = plan.bufs[nd.r_val].cpu().numpy().reshape(n, oh, ow, c.out_channels) if nd.r_val else None
            out = "f32" if nd.out_fp32_nchw else ("i8" if pk.value_code(nd.dst) == L.DRNMI_I8 else "bf16")
            ref = Q.conv_i8(x, nd.wpk.cpu().numpy(), nd.scale.cpu().numpy(), nd.shift.cpu().numpy(), c.out_channels,
                            c.kernel_size[0], c.stride[0], c.padding[0], c.dilation[0], nd.relu, res, nd.res_scale,
                            out, nd.out_scale)
            got = plan.bufs[nd.dst].cpu().numpy()
            if out == "f32":
                got = got.transpose(0, 2, 3, 1)
            elif out == "bf16":
                got = got.view(np.uint16).reshape(ref.shape)
            else:
                got = got.reshape(ref.shape)
            np.testing.assert_array_equal(got, ref, err_msg=nd.name)
        got = m.segment(frames).cpu()
        lplan = m.plan(n, h, w)
        assert lplan.labels_path() == "nhwc"                          # a sparse layer8: the separate seg conv
        lnames = {l.row: l.kernel_name(lib) for l in lplan.launches("u8", True)}
        assert sorted(lplan.packed.graph.nodes[i].name for i, k in lnames.items() if k and "sp24" in k) == sorted(sparse)
        assert torch.equal(got, dense)
        assert len(got.unique()) > 1
    finally:
        m.set_sparse24(False).set_precision("fp32")


def test_network_default_route_same_labels(tmp_path_factory):
    from drnmi import engine
    m, frames = _masked_int8_d22(tmp_path_factory)
    try:
        assert engine.SP24_I8_EVERY is False
        dense = m.set_precision("int8").segment(frames).cpu()
        m.set_sparse24(True)
        pk = m.plan(*frames.shape[:3]).packed
        assert m.sparse24_layers() == [pk.graph.nodes[i].name for i in pk.sp24_i8_candidates()]
        assert torch.equal(m.segment(frames).cpu(), dense)
        assert len(dense.unique()) > 1
    finally:
        m.set_sparse24(False).set_precision("fp32")


def test_network_violation_keeps_layer_dense(tmp_path_factory, monkeypatch):
    from drnmi import engine
    m, frames = _masked_int8_d22(tmp_path_factory)
    w = m.state_dict()["layer.7.0.weight"]
    saved = w[9, 4:8, 1, 1].clone()
    try:
        monkeypatch.setattr(engine, "SP24_I8_EVERY", True)
        m.set_precision("int8").set_sparse24(True)
        assert "layer.7.0" in m.sparse24_layers()
        big = float(w[9].abs().max())
        with torch.no_grad():
            w[9, 4:8, 1, 1] = torch.tensor([0.5, 0.25, -0.5, 0.0], device=w.device) * big   # three int8 non-zeros in one group
        got = m.sparse24_layers()
        assert "layer.7.0" not in got and "layer.8.0" in got
        plan = m.plan(2, 128, 256)
        i = [nd.name for nd in plan.packed.graph.nodes].index("layer.7.0")
        assert plan.args[i].dtype == _lib()[0].DRNMI_I8
    finally:
        with torch.no_grad():
            w[9, 4:8, 1, 1] = saved
        m.set_sparse24(False).set_precision("fp32")


def test_network_graph_capture(tmp_path_factory, monkeypatch):
    from drnmi import engine
    from drnmi.drnseg import INFO_MEAN, INFO_STD
    from drnmi.weights import synth_frames
    m, frames = _masked_int8_d22(tmp_path_factory)
    mean, std = [float(v) for v in INFO_MEAN], [float(v) for v in INFO_STD]
    frames = frames.clone()

    def step():
        return torch.ops.drnmi.segment(frames, m._handle, mean, std, False)

    try:
        monkeypatch.setattr(engine, "SP24_I8_EVERY", True)
        m.set_precision("int8").set_sparse24(True)
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
