"""fp8 against int8 and bf16, measured in one process with the three precisions interleaved
(hipEvents around every repeat; warm-up first; REPS timed repeats each, median and minimum printed):

  * the conv kernels on four DRN-D-22 shapes at 8 x 128 x 256 (layer5-8's resolution for 8 x 1024 x
    2048 frames): 512 -> 512 3x3 dilation 2 and 4, 128 -> 128 3x3, the layer6.0 1x1 downsample --
    each launched as the engine launches it (bf16: scale folded, bf16 in / out; int8 / fp8: 8-bit in
    and out, scale * acc + shift), auto-routed; microseconds and TFLOP/s;
  * one segment() step of D-22 on 8 x 1024 x 2048 uint8 frames: frames/s;
  * label quality at 2 x 1024 x 2048 on the synthetic weights and frames of the tests: agreement
    and mIoU of the bf16, int8 and fp8 labels against the fp32 engine's labels.

python scripts/fp8_micro.py [--reps 20] [--skip-net]      (profiles/fp8/README.txt records a run)
"""
import argparse
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "video-seg-model-compress_amd"))
import torch  # noqa: E402

from drnmi import _lib as L  # noqa: E402

DEV = "cuda"
PRECS = ("bf16", "int8", "fp8")
SHAPES = [  # name, cin, cout, ks, dil at n x h x w = 8 x 128 x 256, stride 1
    ("512->512 3x3 d2 (dominant)", 512, 512, 3, 2),
    ("512->512 3x3 d4", 512, 512, 3, 4),
    ("128->128 3x3", 128, 128, 3, 1),
    ("layer6.0 downsample 256->512 1x1", 256, 512, 1, 1),
]
N, H, W = 8, 128, 256


def conv_args(prec, cin, cout, ks, dil, keep):
    """drnmi_conv_args of one launch in `prec` on random operands (kept alive in `keep`)."""
    pad = dil * (ks // 2)
    k = ks * ks * cin
    cout_pad = (cout + 127) // 128 * 128
    a = L.ConvArgs()
    g = torch.Generator(device=DEV).manual_seed(1)
    if prec == "bf16":
        x = torch.randn(N * H * W * cin, device=DEV, generator=g).bfloat16()
        w = (torch.randn(cout_pad * k, device=DEV, generator=g) * k ** -0.5).bfloat16()
        y = torch.empty(N * H * W * cout, dtype=torch.bfloat16, device=DEV)
        code, scale = L.DRNMI_BF16, None
    else:
        # random bytes; fp8: exponent field at most 7 (|v| <= 1.875), so no NaN pattern and no overflow
        x = torch.randint(0, 256, (N * H * W * cin,), device=DEV, generator=g, dtype=torch.uint8)
        w = torch.randint(0, 256, (cout_pad * k,), device=DEV, generator=g, dtype=torch.uint8)
        if prec == "fp8":
            x, w = x & 0xBF, w & 0xBF
        y = torch.empty(N * H * W * cout, dtype=torch.uint8, device=DEV)
        code = L.DRNMI_I8 if prec == "int8" else L.DRNMI_F8
        scale = torch.full((cout_pad,), 1e-3, device=DEV)
    shift = torch.zeros(cout_pad, device=DEV)
    keep += [x, w, y, scale, shift]
    a.x, a.wgt, a.y, a.shift = x.data_ptr(), w.data_ptr(), y.data_ptr(), shift.data_ptr()
    a.scale = scale.data_ptr() if scale is not None else None
    a.n, a.h, a.w, a.cin, a.ho, a.wo, a.cout, a.cout_pad = N, H, W, cin, H, W, cout, cout_pad
    a.ks, a.stride, a.pad, a.dil, a.k, a.k_pad = ks, 1, pad, dil, k, k
    a.y_sn, a.y_sp, a.y_sc = H * W * cout, cout, 1
    a.relu, a.dtype, a.out_dtype, a.tile, a.algo = 1, code, code, -1, L.ALGO_IGEMM
    a.res_scale, a.out_scale = 0.0, 1.0
    return a


def timed(fn, reps, warmup=3):
    """fn() -> nothing, `reps` rounds over the callables in `fn` (a dict), interleaved."""
    for f in fn.values():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fn}
    for _ in range(reps):
        for k, f in fn.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return ms


def miou(pred, truth, classes=19):
    cm = torch.bincount(truth.flatten().long() * classes + pred.flatten().long(), minlength=classes * classes)
    cm = cm.view(classes, classes).double()
    inter = cm.diag()
    union = cm.sum(0) + cm.sum(1) - inter
    present = cm.sum(1) > 0
    return float((inter[present] / union[present]).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-net", action="store_true")
    opt = ap.parse_args()
    lib = L.load()
    stream = ctypes.c_void_p(L.stream_ptr(torch.device(DEV)))
    print(f"device {torch.cuda.get_device_name(0)}; {opt.reps} timed repeats per figure, precisions interleaved")
    print("--- conv kernels, 8 x 128 x 256, stride 1: median us (min us) TFLOP/s at the median, kernel")
    for name, cin, cout, ks, dil in SHAPES:
        keep, fn, args = [], {}, {}
        for p in PRECS:
            a = args[p] = conv_args(p, cin, cout, ks, dil, keep)
            fn[p] = lambda a=a: L.check(lib.drnmi_conv2d_bn_act(ctypes.byref(a), stream), "conv")
        ms = timed(fn, opt.reps)
        flops = 2.0 * N * H * W * cout * cin * ks * ks
        for p in PRECS:
            med, lo = statistics.median(ms[p]) * 1e3, min(ms[p]) * 1e3
            print(f"{name:34s} {p:5s} {med:8.1f} us ({lo:8.1f}) {flops / med / 1e6:7.1f} TF  "
                  f"{lib.drnmi_conv_kernel_name(ctypes.byref(args[p])).decode()}", flush=True)
    if opt.skip_net:
        return
    from drnmi.drnseg import build
    from drnmi.weights import synth_frames
    models = {p: build("drn_d_22", 19, seed=0, device=DEV) for p in ("fp32",) + PRECS}
    small = torch.from_numpy(synth_frames(100, 2, 1024, 2048)).to(DEV)
    state = None
    for p in ("int8", "fp8"):
        if state is None:
            models[p].calibrate_int8(small[:1])
            state = models[p].int8_state()
        else:
            models[p].load_int8_state(state)
    for p, m in models.items():
        m.set_precision(p)
    print("--- label quality, D-22, 2 x 1024 x 2048, synthetic weights (seed 0) and frames (seed 100), absmax scales "
          "of frame 0; against the fp32 engine's labels")
    truth = models["fp32"].segment(small)
    for p in PRECS:
        lab = models[p].segment(small)
        print(f"{p:5s} agreement {float((lab == truth).float().mean()):.4f}  mIoU {100 * miou(lab, truth):.1f}", flush=True)
    del models["fp32"], truth
    torch.cuda.empty_cache()
    g = torch.Generator(device=DEV).manual_seed(5)
    frames = torch.randint(0, 256, (8, 1024, 2048, 3), dtype=torch.uint8, device=DEV, generator=g)
    out = {p: torch.empty(8, 1024, 2048, dtype=torch.uint8, device=DEV) for p in PRECS}
    fn = {p: (lambda p=p: models[p].segment(frames, labels=out[p])) for p in PRECS}
    ms = timed(fn, opt.reps)
    print("--- segment() step, D-22, 8 x 1024 x 2048 uint8 frames: median ms (min ms) frames/s at the median")
    for p in PRECS:
        med, lo = statistics.median(ms[p]), min(ms[p])
        print(f"{p:5s} {med:7.3f} ms ({lo:7.3f})  {8e3 / med:7.1f} frames/s", flush=True)
        plan = [pl for k, pl in models[p]._plans.items() if k[:4] == (p, 8, 1024, 2048)][0]
        names = {}
        for l in plan.launches("u8", plan.labels_path() != "nchw"):
            nm = l.kernel_name(lib).split("<")[0]
            names[nm] = names.get(nm, 0) + 1
        print("      launches: " + ", ".join(f"{v} x {k}" for k, v in sorted(names.items())), flush=True)


if __name__ == "__main__":
    main()
