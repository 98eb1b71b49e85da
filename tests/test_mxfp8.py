"""mxfp8 (block-scaled e4m3, include/drnmi.h DRNMI_MXF8) on the host: the precision is accepted with no
calibration, a D-22 packs and routes to conv_mx_kernel on the layers int8_layout selects, and the routing
refuses what the kernel has no form for."""
import ctypes

import pytest
import torch


def _probe(L, cin=256, cout=256, ks=3, dil=2, out=None):
    a = L.ConvArgs()
    a.scale = 1                                      # routing reads the pointers only for presence
    pad = dil * (ks // 2)
    a.n, a.h, a.w, a.cin, a.ho, a.wo, a.cout, a.cout_pad = 1, 9, 13, cin, 9, 13, cout, (cout + 127) // 128 * 128
    a.ks, a.stride, a.pad, a.dil, a.k, a.k_pad = ks, 1, pad, dil, ks * ks * cin, ks * ks * cin
    a.dtype, a.out_dtype, a.tile, a.algo = L.DRNMI_MXF8, L.DRNMI_MXF8 if out is None else out, -1, L.ALGO_IGEMM
    a.y_sn, a.y_sp, a.y_sc = 9 * 13 * cout, cout, 1
    return a


def test_routing():
    from drnmi import _lib as L
    lib = L.load()
    for ks in (1, 3):
        for out in (L.DRNMI_MXF8, L.DRNMI_BF16, L.DRNMI_F32):
            a = _probe(L, ks=ks, out=out)
            assert lib.drnmi_conv_status(ctypes.byref(a)) == 0
            assert lib.drnmi_conv_kernel_name(ctypes.byref(a)).decode() == f"conv_mx_kernel<{ks}>"
    refused = {"x2": dict(x2=1, cin2=64, h2=9, w2=13, stride2=1, k=9 * 256 + 64, k_pad=9 * 256 + 64), "unit_mask": dict(unit_mask=1),
               "scale": dict(scale=None), "stride": dict(stride=2, ho=5, wo=7, y_sn=35 * 256), "tile": dict(tile=L.TILE_STAG)}
    for what, fields in refused.items():
        a = _probe(L)
        for k, v in fields.items():
            setattr(a, k, v)
        assert lib.drnmi_conv_status(ctypes.byref(a)) == -2 and lib.drnmi_conv_kernel_name(ctypes.byref(a)) is None, what
    assert lib.drnmi_conv_status(ctypes.byref(_probe(L, cin=64))) == -2
    assert lib.drnmi_conv_status(ctypes.byref(_probe(L, out=L.DRNMI_F8))) == -1
    assert lib.drnmi_conv_stag_seg_kernel_name(ctypes.byref(_probe(L, cin=512, cout=512))) is None
    assert lib.drnmi_mx8_image_bytes(37, 128) == 37 * 132 + 12 and lib.drnmi_mx8_image_bytes(37, 48) == -1
    assert lib.drnmi_mx8_pack_bytes(128, 1152) == 128 * 1152 // 32 * 33 and lib.drnmi_mx8_pack_bytes(64, 1152) == -1


def test_d22_packs_and_routes_without_calibration():
    from drnmi import _lib as L
    from drnmi.drnseg import DRNSeg
    from drnmi.engine import PackedNet, _probe_args, channel_strides, int8_layout
    from drnmi.weights import synth_state_dict
    lib = L.load()
    m = DRNSeg("drn_d_22", 19, pretrained=False)
    m.load_state_dict(synth_state_dict(m, 0))
    assert m.eval().set_precision("mxfp8") is m and m._act_scales is None
    with pytest.raises(NotImplementedError, match="precision 'mxfp8' covers the DRN-D family only"):
        DRNSeg("drn_c_26", 19, pretrained=False).set_precision("mxfp8")
    pk = PackedNet(m._graph, "mxfp8", torch.device("cpu"), block_sparse=False, act_scales=None)
    cs = channel_strides(m._graph)
    elig, _, _ = int8_layout(m._graph, cs)
    want = {i for i in elig if cs[m._graph.nodes[i].src] >= 128 and m._graph.nodes[i].conv.stride[0] == 1}
    assert pk.i8_nodes == want and len(want) >= 10
    for i, nd in enumerate(pk.graph.nodes):
        assert nd.i8 == (i in want)
        if not nd.i8:
            continue
        assert nd.wpk.dtype == torch.uint8 and nd.wpk.numel() == lib.drnmi_mx8_pack_bytes(nd.cout_pad, nd.k_pad)
        a = _probe_args(nd, nd.cin_stride, nd.k, nd.k_pad)
        a.scale, a.dtype = 1, L.DRNMI_MXF8
        a.out_dtype = pk.value_code(nd.dst)
        if nd.out_fp32_nchw:
            a.out_dtype, a.y_sp, a.y_sc = L.DRNMI_F32, 1, a.ho * a.wo
        a.y_sn = a.ho * a.wo * a.cout
        assert lib.drnmi_conv_kernel_name(ctypes.byref(a)).decode() == f"conv_mx_kernel<{a.ks}>", nd.name
    # the image values: written and read by MX launches only; one bf16 value gets an image copy
    assert all(c == L.DRNMI_MXF8 for c in pk.vcode.values()) and sum(len(v) for v in pk.quant_after.values()) == 1
