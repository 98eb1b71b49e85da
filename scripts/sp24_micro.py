"""2:4 weight sparsity (DRNMI_BF16_SP24, csrc/conv_sp24.hip) against the dense bf16 kernels, measured in
one process with the arms interleaved (HIP events around every repeat; warm-up first; medians and minima
of --reps timed repeats; operand buffers rotated over ROT copies so no repeat finds its inputs in cache):

  1. issue rate: a register-only loop of back-to-back MFMAs, one wave per SIMD on every CU,
     v_smfmac_f32_16x16x64_bf16 against v_mfma_f32_16x16x32_bf16: ns and cycles per instruction;
  2. kernel times on D-22's shapes at 8 x 128 x 256 (layer5-8's resolution for 8 x 1024 x 2048 frames):
     the sparse kernel (every form the route offers) against the kernel the dense launch is routed to;
  3. segment() step of the 2:4-masked D-22 on 8 x 1024 x 2048 frames, switch off against on, and labels;
  4. accumulation error of an fp32-output launch, max |acc - acc64| / sum |a b|, sparse next to dense on
     the same operands (information, not a gate).

python scripts/sp24_micro.py [--reps 20] [--skip-net]      (profiles/sp24/README.txt records a run)
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "video-seg-model-compress_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from drnmi import _lib as L  # noqa: E402

DEV = "cuda"
ROT = 3
SHAPES = [  # name, cin, cout, ks, dil at n x h x w = 8 x 128 x 256, stride 1
    ("512->512 3x3 d2", 512, 512, 3, 2),
    ("512->512 3x3 d4", 512, 512, 3, 4),
    ("256->256 3x3 d2", 256, 256, 3, 2),
    ("128->128 3x3", 128, 128, 3, 1),
    ("256->512 1x1", 256, 512, 1, 1),
]
N, H, W = 8, 128, 256


def sparse_weight(cout_pad, k, gen):
    """bf16 [cout_pad, k] with the two largest of every four consecutive columns kept."""
    w = torch.randn(cout_pad, k // 4, 4, device=DEV, generator=gen) * k ** -0.5
    keep = w.abs().argsort(dim=-1, descending=True)[..., :2]
    m = torch.zeros_like(w).scatter_(-1, keep, 1.0)
    return (w * m).reshape(cout_pad, k).bfloat16().contiguous()


def pack(lib, dense, stream):
    rows, k = dense.shape
    blob = torch.empty(lib.drnmi_sp24_pack_bytes(rows, k), dtype=torch.uint8, device=DEV)
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    L.check(lib.drnmi_sp24_pack(dense.data_ptr(), rows, k, blob.data_ptr(), cnt.data_ptr(), stream), "sp24_pack")
    assert int(cnt.item()) == 0
    return blob


def conv_args(x, wgt, y, shift, n, h, w, cin, cout, ks, dil, dtype, tile=-1, f32=False):
    a = L.ConvArgs()
    cout_pad = (cout + 127) // 128 * 128
    a.x, a.wgt, a.y, a.shift, a.scale = x.data_ptr(), wgt.data_ptr(), y.data_ptr(), shift.data_ptr(), None
    a.n, a.h, a.w, a.cin, a.ho, a.wo, a.cout, a.cout_pad = n, h, w, cin, h, w, cout, cout_pad
    a.ks, a.stride, a.pad, a.dil, a.k, a.k_pad = ks, 1, dil * (ks // 2), dil, ks * ks * cin, ks * ks * cin
    a.y_sn, a.y_sp, a.y_sc = h * w * cout, cout, 1
    a.relu, a.dtype, a.out_dtype, a.tile, a.algo = 0 if f32 else 1, dtype, L.DRNMI_F32 if f32 else L.DRNMI_BF16, tile, L.ALGO_IGEMM
    return a


def timed(fn, reps, warmup=3):
    """`reps` rounds over the callables of `fn` (a dict), interleaved; each gets the round number."""
    for f in fn.values():
        for i in range(warmup):
            f(i)
    torch.cuda.synchronize()
    ms = {k: [] for k in fn}
    for i in range(reps):
        for k, f in fn.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f(i)
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return ms


def issue_rate(lib, stream, reps):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    iters = 1 << 16
    sink = torch.empty(cus * 256, device=DEV)
    fn = {name: (lambda i, s=s: L.check(lib.drnmi_sp24_issue_probe(s, iters, cus, sink.data_ptr(), stream), "issue"))
          for name, s in (("dense v_mfma_f32_16x16x32_bf16", 0), ("sparse v_smfmac_f32_16x16x64_bf16", 1))}
    ms = timed(fn, reps)
    print(f"--- issue rate: {cus} workgroups x 4 waves (one per SIMD), {iters} x 8 MFMAs per wave on 8 accumulators")
    med = {}
    for name, v in ms.items():
        med[name] = statistics.median(v)
        ns = med[name] * 1e6 / (iters * 8)
        print(f"{name:36s} {med[name]:8.3f} ms ({min(v):8.3f})  {ns:6.3f} ns / MFMA / SIMD", flush=True)
    d, s = med["dense v_mfma_f32_16x16x32_bf16"], med["sparse v_smfmac_f32_16x16x64_bf16"]
    pf = {k: f * 4 * cus / (v * 1e-3 / (iters * 8)) / 1e15 for (k, v), f in zip(med.items(), (16384, 32768))}
    print(f"sparse / dense time per instruction {s / d:.3f}; whole chip, dense-equivalent: dense loop "
          f"{pf['dense v_mfma_f32_16x16x32_bf16']:.2f} PFLOP/s, sparse loop {pf['sparse v_smfmac_f32_16x16x64_bf16']:.2f} PFLOP/s "
          f"(the clock under each loop is not read: ns, not cycles)", flush=True)


def kernels(lib, stream, reps, strip=True):
    print(f"--- conv kernels, {N} x {H} x {W}, stride 1, bf16 in / out: median us (min us), dense-equivalent TFLOP/s at "
          f"the median, kernel; {ROT} rotated operand sets")
    gen = torch.Generator(device=DEV).manual_seed(1)
    for name, cin, cout, ks, dil in SHAPES:
        k = ks * ks * cin
        cout_pad = (cout + 127) // 128 * 128
        dense = sparse_weight(cout_pad, k, gen)
        blob = pack(lib, dense, stream)
        shift = torch.zeros(cout_pad, device=DEV)
        xs = [torch.randn(N * H * W * cin, device=DEV, generator=gen).bfloat16() for _ in range(ROT)]
        ys = [torch.empty(N * H * W * cout, dtype=torch.bfloat16, device=DEV) for _ in range(ROT)]
        arms = {"dense": (dense, L.DRNMI_BF16, -1), "sp24 gather": (blob, L.DRNMI_BF16_SP24, L.SP24_GATHER),
                "sp24 strip": (blob, L.DRNMI_BF16_SP24, L.SP24_STRIP)}
        if not strip:
            del arms["sp24 strip"]
        args, fn = {}, {}
        for arm, (wgt, dtype, tile) in arms.items():
            aa = [conv_args(xs[r], wgt, ys[r], shift, N, H, W, cin, cout, ks, dil, dtype, tile) for r in range(ROT)]
            if lib.drnmi_conv_kernel_name(ctypes.byref(aa[0])) is None:
                continue                                    # the route has no such form for this shape
            args[arm] = aa
            fn[arm] = lambda i, aa=aa: L.check(lib.drnmi_conv2d_bn_act(ctypes.byref(aa[i % ROT]), stream), "conv")
        ms = timed(fn, reps)
        flops = 2.0 * N * H * W * cout * k
        for arm in fn:
            med, lo = statistics.median(ms[arm]) * 1e3, min(ms[arm]) * 1e3
            print(f"{name:18s} {arm:12s} {med:8.1f} us ({lo:8.1f}) {flops / med / 1e6:7.1f} TF  "
                  f"{lib.drnmi_conv_kernel_name(ctypes.byref(args[arm][0])).decode()}", flush=True)
        del xs, ys


def accumulation(lib, stream):
    print("--- accumulation error, fp32 output, 1 x 16 x 256, shift 0: max |acc - acc64| / sum |a b|, same operands")
    gen = torch.Generator(device=DEV).manual_seed(2)
    n, h, w = 1, 16, 256
    for name, cin, cout, ks, dil in SHAPES:
        k = ks * ks * cin
        cout_pad = (cout + 127) // 128 * 128
        dense = sparse_weight(cout_pad, k, gen)
        blob = pack(lib, dense, stream)
        shift = torch.zeros(cout_pad, device=DEV)
        x = torch.randn(n, h, w, cin, device=DEV, generator=gen).bfloat16()
        cols = F.unfold(x.double().permute(0, 3, 1, 2), ks, dilation=dil, padding=dil * (ks // 2))   # [n, cin*ks*ks, hw]
        cols = cols.view(n, cin, ks * ks, h * w).permute(0, 3, 2, 1).reshape(n * h * w, k)           # k = tap * cin + ci
        wd = dense[:cout].double()
        acc64 = cols @ wd.t()
        mag = cols.abs() @ wd.abs().t()
        for arm, wgt, dtype in (("dense", dense, L.DRNMI_BF16), ("sp24", blob, L.DRNMI_BF16_SP24)):
            y = torch.empty(n * h * w, cout, device=DEV)
            a = conv_args(x, wgt, y, shift, n, h, w, cin, cout, ks, dil, dtype, f32=True)
            L.check(lib.drnmi_conv2d_bn_act(ctypes.byref(a), stream), "conv")
            torch.cuda.synchronize()
            err = float(((y.double() - acc64).abs() / mag.clamp_min(1e-30)).max())
            print(f"{name:18s} {arm:6s} {err:.3e}  {lib.drnmi_conv_kernel_name(ctypes.byref(a)).decode()}", flush=True)


def network(lib, reps):
    from drnmi import pruners as P
    from drnmi.drnseg import build
    from drnmi.weights import synth_frames
    m = build("drn_d_22", 19, seed=0, device=DEV)
    layers = [nd.name + ".weight" for nd in m._graph.nodes if nd.conv.in_channels >= 64]
    with tempfile.TemporaryDirectory() as d:
        cfg = os.path.join(d, "nm.json")
        with open(cfg, "w") as f:
            json.dump({"pruner_type": "nm", "configs": [{"layer_set": layers, "n": 2, "m": 4}]}, f)
        pr = P.make_pruner(cfg)
        pr.generate_masks(m)
        pr.apply_masks(m)
    small = torch.from_numpy(synth_frames(100, 2, 1024, 2048)).to(DEV)
    truth = m.set_precision("fp32").segment(small)
    m.set_precision("bf16")
    off = m.segment(small)
    on = m.set_sparse24(True).segment(small)
    print(f"--- 2:4-masked D-22 ({len(layers)} masked convs, {len(m.sparse24_layers())} launched sparse: "
          f"{', '.join(m.sparse24_layers())})")
    print(f"labels at 2 x 1024 x 2048 against the fp32 engine: switch off {float((off == truth).float().mean()):.4f}, "
          f"on {float((on == truth).float().mean()):.4f}; on against off {float((on == off).float().mean()):.4f}")
    del truth, off, on, small
    models = {"off": m.set_sparse24(False), "on": None}
    m2 = build("drn_d_22", 19, seed=0, device=DEV)
    m2.load_state_dict(m.state_dict())
    models["on"] = m2.set_precision("bf16").set_sparse24(True)
    g = torch.Generator(device=DEV).manual_seed(5)
    frames = [torch.randint(0, 256, (8, 1024, 2048, 3), dtype=torch.uint8, device=DEV, generator=g) for _ in range(ROT)]
    out = {k: torch.empty(8, 1024, 2048, dtype=torch.uint8, device=DEV) for k in models}
    fn = {k: (lambda i, k=k: models[k].segment(frames[i % ROT], labels=out[k])) for k in models}
    ms = timed(fn, reps)
    print("segment() step, 8 x 1024 x 2048 uint8 frames: median ms (min ms) frames/s at the median")
    for k in models:
        med, lo = statistics.median(ms[k]), min(ms[k])
        print(f"switch {k:3s} {med:7.3f} ms ({lo:7.3f})  {8e3 / med:7.1f} frames/s", flush=True)
    # per launch, one timed pass each with the timing hook (HIP events around every launch)
    for k, mm in models.items():
        plan = [pl for key, pl in mm._plans.items() if key[:4] == ("bf16", 8, 1024, 2048)][0]
        ev = {}

        def hook(i, nd, start):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            ev.setdefault(i, []).append(e)
        mm.timing_hook = hook
        acc = {}
        for r in range(5):
            ev.clear()
            mm.segment(frames[r % ROT], labels=out[k])
            torch.cuda.synchronize()
            for i, (e0, e1) in ev.items():
                acc.setdefault(i, []).append(e0.elapsed_time(e1) * 1e3)
        mm.timing_hook = None
        names = {l.row: l.kernel_name(lib) for l in plan.launches("u8", plan.labels_path() != "nchw")}
        nodes = plan.packed.graph.nodes
        print(f"per launch, switch {k} (median of 5 hooked steps, us):")
        for i in sorted(acc):
            nm = nodes[i].name if i < len(nodes) else "head"
            print(f"  {nm:24s} {statistics.median(acc[i]):8.1f}  {names.get(i, 'head')}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-net", action="store_true")
    ap.add_argument("--no-strip", action="store_true", help="leave the forced strip-staged arm out")
    opt = ap.parse_args()
    lib = L.load()
    stream = ctypes.c_void_p(L.stream_ptr(torch.device(DEV)))
    print(f"device {torch.cuda.get_device_name(0)}; {opt.reps} timed repeats per figure, arms interleaved")
    issue_rate(lib, stream, opt.reps)
    kernels(lib, stream, opt.reps, not opt.no_strip)
    accumulation(lib, stream)
    if not opt.skip_net:
        network(lib, opt.reps)


if __name__ == "__main__":
    main()
