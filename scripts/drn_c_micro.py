"""DRN-C-26 bf16 segment() with the fused 16-channel BasicBlock (drnmi_basic_block16) on and off:
step times of both plans interleaved on one device, and the per-launch table of each (HIP events
through DRNSeg.timing_hook).  python scripts/drn_c_micro.py [--batch 8 --height 1024 --width 2048]"""
import argparse
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "video-seg-model-compress_amd"), REPO]

from drnmi import _lib, engine  # noqa: E402
from drnmi.drnseg import build  # noqa: E402
from drnmi.weights import synth_frames  # noqa: E402


def make(fuse, n, h, w):
    engine.FUSE_BLOCK16 = fuse                       # read when the weights are packed
    m = build("drn_c_26", 19, seed=6, precision="bf16")
    plan = m.plan(n, h, w)
    assert bool(plan.block16) == fuse
    return m, plan


def launch_names(plan):
    """Kernel name per hook index of the segment() path (the head last)."""
    lib = _lib.load()
    names = [""] * len(plan.args)
    for l in plan.launches("u8", plan.labels_path() != "nchw"):
        names[l.row] = l.kernel_name(lib)
    return names + ["head"]


def step_time(m, frames, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        m.segment(frames)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def launch_table(m, plan, frames, reps):
    names = launch_names(plan)
    evs = []
    m.timing_hook = lambda i, nd, before: (evs.append((i, before, torch.cuda.Event(enable_timing=True))), evs[-1][2].record())
    for _ in range(reps):
        m.segment(frames)
    torch.cuda.synchronize()
    m.timing_hook = None
    tot, pend = {}, {}
    for i, before, ev in evs:
        if before:
            pend[i] = ev
        else:
            tot[i] = tot.get(i, 0.0) + pend.pop(i).elapsed_time(ev) * 1e3 / reps
    nodes = plan.packed.graph.nodes
    return [(i, nodes[i].name if i < len(nodes) else "head", names[i], us) for i, us in sorted(tot.items())]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    n, h, w = args.batch, args.height, args.width
    frames = torch.from_numpy(synth_frames(106, n, h, w)).cuda()
    nets = {"fused": make(True, n, h, w), "two launches": make(False, n, h, w)}
    labels = {}
    for k, (m, _) in nets.items():
        for _ in range(3):
            labels[k] = m.segment(frames)
    torch.cuda.synchronize()
    agree = (labels["fused"] == labels["two launches"]).float().mean().item()
    print(f"drn_c_26 bf16 segment {n} x {h} x {w}; labels fused vs two launches agree {agree:.5f}")
    times = {k: [] for k in nets}
    for _ in range(args.runs):
        for k, (m, _) in nets.items():
            times[k].append(step_time(m, frames, args.steps))
    for k, ts in times.items():
        print(f"step ms [{k}]: " + ", ".join(f"{t:.3f}" for t in ts) + f"  (fps {n * 1e3 / min(ts):.1f} at best)")
    px = n * h * w
    for k, (m, plan) in nets.items():
        print(f"\nper-launch table [{k}] (us, HIP events, mean of 5 instrumented steps)")
        for i, name, kern, us in launch_table(m, plan, frames, 5):
            extra = ""
            if kern == "block16_kernel":
                extra = f"   {64 * px / us * 1e-3:.0f} GB/s of the 64 B/pixel floor"
            print(f"  {i:3d} {name:26s} {kern:58s} {us:9.1f}{extra}")


if __name__ == "__main__":
    main()
