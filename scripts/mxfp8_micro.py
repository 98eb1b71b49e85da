"""mxfp8 against bf16 / int8 / fp8 in ONE process with alternating rounds (scripts/fp8_micro.py's method):
frames/s of a D-22 segment() step at 8 x 1024 x 2048, the dominant 512 -> 512 3x3 launch of each precision,
and label agreement / mIoU against the fp32 engine at 2 x 1024 x 2048.  The int8 / fp8 scales come from
calibration frames disjoint from the test frames; mxfp8 has none.

    python scripts/mxfp8_micro.py [--rounds 5] [--steps 10] > profiles/mxfp8/micro.log
"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "video-seg-model-compress_amd"), REPO]
PRECS = ("bf16", "int8", "fp8", "mxfp8")


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def miou(lab, ref, classes=19):
    hist = np.bincount(ref.ravel().astype(np.int64) * classes + lab.ravel(), minlength=classes * classes).reshape(classes, classes)
    inter, union = np.diag(hist), hist.sum(0) + hist.sum(1) - np.diag(hist)
    return float((inter[union > 0] / union[union > 0]).mean() * 100)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    args = ap.parse_args()
    from drnmi.drnseg import build
    from drnmi.weights import synth_frames
    dev = torch.device("cuda", 0)
    m = build("drn_d_22", 19, seed=0, device=dev)
    m.calibrate_int8(torch.from_numpy(synth_frames(7, 2, 1024, 2048)).to(dev))      # calibration frames: seed 7
    big = torch.from_numpy(synth_frames(100, 8, 1024, 2048)).to(dev)                # test frames: seeds 100, 200
    pair = torch.from_numpy(synth_frames(200, 2, 1024, 2048)).to(dev)

    # --- the step, interleaved: every round times each precision once, in rotating order
    step = {p: [] for p in PRECS}
    for p in PRECS:
        m.set_precision(p).segment(big)                                             # pack, plan, warm up
    for r in range(args.rounds):
        for p in PRECS[r % 4:] + PRECS[:r % 4]:
            m.set_precision(p)
            m.segment(big)
            step[p].append(timed(lambda: m.segment(big), args.steps))
    for p in PRECS:
        ms = sorted(step[p])
        print(f"segment() 8x1024x2048 {p:6s}: median {8e3 / ms[len(ms) // 2]:8.1f} frames/s  (rounds: "
              + " ".join(f"{8e3 / t:.1f}" for t in step[p]) + ")")

    # --- the dominant launch: D-22's 512 -> 512 3x3 dilation-2 conv (layer7), per precision, interleaved
    conv = {p: [] for p in PRECS}
    rows = {}
    for p in PRECS:
        plan = m.set_precision(p).plan(8, 1024, 2048)
        ls = [l for l in plan.launches("u8", True) if plan.packed.graph.nodes[l.row].name == "layer.7.0"]
        rows[p] = (plan, ls[0])
    import ctypes
    from drnmi import _lib
    lib, stream = _lib.load(), ctypes.c_void_p(_lib.stream_ptr(dev))
    for r in range(args.rounds):
        for p in PRECS[r % 4:] + PRECS[:r % 4]:
            plan, l = rows[p]
            l.issue(lib, stream)
            conv[p].append(timed(lambda: l.issue(lib, stream), 20) * 1e3)
    for p in PRECS:
        us = sorted(conv[p])
        print(f"layer.7.0 512->512 3x3 d2 {p:6s}: median {us[len(us) // 2]:7.1f} us  {rows[p][1].kernel_name(lib)}")

    # --- labels against the fp32 engine
    ref = m.set_precision("fp32").segment(pair).cpu().numpy()
    for p in PRECS:
        lab = m.set_precision(p).segment(pair).cpu().numpy()
        print(f"labels vs fp32 engine 2x1024x2048 {p:6s}: agreement {float((lab == ref).mean()):.4f}, mIoU {miou(lab, ref):.1f}")


if __name__ == "__main__":
    main()
