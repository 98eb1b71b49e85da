"""conv_x3 (fp32x2, three products) against conv_x6 (fp32x, six) on the fine-tune step's dominant
launches (D-54 at 2 x 1024 x 768: the 1/8-resolution 3x3 and 1x1 convs, layer3's 1x1s and the seg conv),
as the train path launches them (a workspace, so the planned split-K): HIP-event time per launch, rounds
alternating the configurations, median and min - max over the rounds.  Configurations: x6 auto, x3 auto and
the forced x3 variants 0 / 1 / 2 (unsplit).  Also prints max |y_x3 - y_x6| / max |y_x6|.
python scripts/x3_micro.py [out.json]"""
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "video-seg-model-compress_amd"))
import torch  # noqa: E402

from drnmi import _lib, ops  # noqa: E402
from drnmi.engine import split3_bf16  # noqa: E402

DEV = "cuda"
SHAPES = [  # name, n, h, w, cin, cout, ks, stride, pad, dil, res
    ("3x3 512 d4", 2, 128, 96, 512, 512, 3, 1, 4, 4, False),
    ("3x3 256 d2", 2, 128, 96, 256, 256, 3, 1, 2, 2, False),
    ("3x3 128 d1 1/4", 2, 256, 192, 128, 128, 3, 1, 1, 1, False),
    ("3x3 64 d1 1/4", 2, 256, 192, 64, 64, 3, 1, 1, 1, False),
    ("1x1 1024-256", 2, 128, 96, 1024, 256, 1, 1, 0, 1, False),
    ("1x1 256-1024 +res", 2, 128, 96, 256, 1024, 1, 1, 0, 1, True),
    ("1x1 2048-512", 2, 128, 96, 2048, 512, 1, 1, 0, 1, False),
    ("1x1 512-2048 +res", 2, 128, 96, 512, 2048, 1, 1, 0, 1, True),
    ("1x1 256-64 1/4", 2, 256, 192, 256, 64, 1, 1, 0, 1, False),
    ("1x1 64-256 1/4 +res", 2, 256, 192, 64, 256, 1, 1, 0, 1, True),
    ("seg 1x1 512-19", 2, 128, 96, 512, 19, 1, 1, 0, 1, False),
]
CONFIGS = [("x6 auto", _lib.DRNMI_F32X3, -1), ("x3 auto", _lib.DRNMI_F32X2, -1), ("x3 v0", _lib.DRNMI_F32X2, 0),
           ("x3 v1", _lib.DRNMI_F32X2, 1), ("x3 v2", _lib.DRNMI_F32X2, 2)]
ROUNDS, REPS = 5, 20
lib = _lib.load()
st = ctypes.c_void_p(_lib.stream_ptr())
results = []
for name, n, h, w, cin, cout, ks, s, pad, dil, res in SHAPES:
    g = torch.Generator(device=DEV).manual_seed(cin + cout + ks)
    xd = torch.randn(n, h, w, cin, device=DEV, generator=g)
    wt = torch.randn(cout, cin, ks, ks, device=DEV, generator=g) / (cin * ks * ks) ** 0.5
    ho = (h + 2 * pad - dil * (ks - 1) - 1) // s + 1
    wo = (w + 2 * pad - dil * (ks - 1) - 1) // s + 1
    rd = torch.randn(n, ho, wo, cout, device=DEV, generator=g) if res else None
    wpk, k = ops.pack_conv_weight(wt, cin, torch.float32)
    planes = split3_bf16(wpk)
    shp = torch.randn(wpk.shape[0], device=DEV, generator=g)
    runs = []
    for label, dtype, tile in CONFIGS:
        y = torch.empty(n, ho, wo, cout, device=DEV)
        a = _lib.ConvArgs()
        a.x, a.wgt, a.scale, a.shift = xd.data_ptr(), planes.data_ptr(), None, shp.data_ptr()
        a.res, a.y = rd.data_ptr() if res else None, y.data_ptr()
        a.y_sn, a.y_sp, a.y_sc = ho * wo * cout, cout, 1
        a.n, a.h, a.w, a.cin, a.ho, a.wo, a.cout, a.cout_pad = n, h, w, cin, ho, wo, cout, wpk.shape[0]
        a.ks, a.stride, a.pad, a.dil, a.k, a.k_pad = ks, s, pad, dil, k, wpk.shape[1]
        a.relu, a.dtype, a.out_dtype, a.tile, a.algo = 1, dtype, _lib.DRNMI_F32, tile, _lib.ALGO_IGEMM
        nb = lib.drnmi_conv_workspace_bytes(ctypes.byref(a))
        ws = torch.empty(max(nb, 256), dtype=torch.uint8, device=DEV)
        a.ws, a.ws_bytes = ws.data_ptr(), ws.numel()
        kn = lib.drnmi_conv_kernel_name(ctypes.byref(a))
        if kn is None:
            continue
        for _ in range(5):                                # warm-up: code objects, the LDS attribute
            _lib.check(lib.drnmi_conv2d_bn_act(ctypes.byref(a), st), label)
        runs.append({"config": label, "kernel": kn.decode(), "split_k": max(1, nb // (4 * n * ho * wo * cout)),
                     "a": a, "keep": (y, ws), "us": []})
    for _ in range(ROUNDS):                               # alternate the configurations
        for r in runs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPS):
                _lib.check(lib.drnmi_conv2d_bn_act(ctypes.byref(r["a"]), st), r["config"])
            e1.record()
            torch.cuda.synchronize()
            r["us"].append(e0.elapsed_time(e1) / REPS * 1e3)
    y6 = runs[0]["keep"][0]
    flops = 2.0 * n * ho * wo * cout * cin * ks * ks
    for r in runs:
        med = statistics.median(r["us"])
        d = float((r["keep"][0] - y6).abs().max() / y6.abs().max())
        print(f"{name:22s} {r['config']:8s} {r['kernel']:34s} S{r['split_k']} {med:8.1f} us ({min(r['us']):.1f} - "
              f"{max(r['us']):.1f})  {flops / med / 1e6:6.1f} TF  vs x6 {d:.1e}", flush=True)
        results.append({"shape": name, "config": r["config"], "kernel": r["kernel"], "split_k": r["split_k"],
                        "us_median": med, "us_min": min(r["us"]), "us_max": max(r["us"]), "diff_vs_x6": d})
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(results, f, indent=1)
