"""Diagnostic: the weight-gradient kernels on fine-tune shapes of the benchmark (2 crops of 1024 x 768),
timed with HIP events; run under rocprofv3 --pmc for counters.

    python scripts/wgrad_micro.py [--precision fp32|fp32x|both] [--repeats N]

The 1/8-resolution D-54 shapes take the 128-tile / pre kernel in fp32x; the two 1/4-resolution
64-channel shapes take the 64-tile kernels (64 -> 128 in fp32x: the 128-tile).  DRNMI_LIB selects
another build of the library (an A/B against a parent build)."""
import argparse
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "video-seg-model-compress_amd"))
import torch  # noqa: E402

from drnmi import _lib  # noqa: E402

SHAPES = [  # name, cin, cout, ks, dil, h, w
    ("layer7.0 conv1 2048->512 d2", 2048, 512, 3, 2, 128, 96),
    ("layer6 conv2 512->512 d4", 512, 512, 3, 4, 128, 96),
    ("layer5 conv3 256->1024 1x1", 256, 1024, 1, 1, 128, 96),
    ("layer3 conv2 64->64 3x3", 64, 64, 3, 1, 256, 192),
    ("layer4 conv1 64->128 3x3", 64, 128, 3, 1, 256, 192),
]
ap = argparse.ArgumentParser()
ap.add_argument("--precision", choices=["fp32", "fp32x", "both"], default="fp32x")
ap.add_argument("--repeats", type=int, default=5)
opt = ap.parse_args()
lib = _lib.load()
n = 2
for precision in (["fp32", "fp32x"] if opt.precision == "both" else [opt.precision]):
    x6 = precision == "fp32x"
    fn = lib.drnmi_conv_wgrad_f32x3 if x6 else lib.drnmi_conv_wgrad_f32
    for name, cin, cout, ks, dil, h, w in SHAPES:
        pad = dil * (ks // 2)
        x = torch.randn(n * h * w, cin, device="cuda")
        dy = torch.randn(n * h * w, cout, device="cuda")
        dw = torch.empty(cout, cin, ks, ks, device="cuda")
        a = _lib.WgradArgs()
        a.dy, a.x, a.dw = dy.data_ptr(), x.data_ptr(), dw.data_ptr()
        a.n, a.h, a.w, a.cin, a.cin_stride = n, h, w, cin, cin
        a.ho, a.wo, a.cout, a.dy_stride = h, w, cout, cout
        a.ks, a.stride, a.pad, a.dil = ks, 1, pad, dil
        a.accumulate = 0
        nb = lib.drnmi_conv_wgrad_workspace_bytes(ctypes.byref(a))
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
        a.ws, a.ws_bytes = ws.data_ptr(), nb
        sp = ctypes.c_void_p(_lib.stream_ptr())
        kernel = _lib.wgrad_plan(a, x6)[0]
        for _ in range(2):
            _lib.check(fn(ctypes.byref(a), sp), "wgrad")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(opt.repeats + 1)]
        ev[0].record()
        for i in range(opt.repeats):
            _lib.check(fn(ctypes.byref(a), sp), "wgrad")
            ev[i + 1].record()
        torch.cuda.synchronize()
        us = statistics.median(ev[i].elapsed_time(ev[i + 1]) for i in range(opt.repeats)) * 1e3
        fl = 2.0 * n * h * w * cout * cin * ks * ks
        print(f"{precision:5s} {name:32s} {us:8.1f} us/call at the median of {opt.repeats} (incl. reduce) "
              f"{fl / us / 1e6:6.1f} TF  ws {nb / 2**20:.0f} MiB  {kernel}", flush=True)
