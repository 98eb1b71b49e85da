"""Single small frames: the default bf16 route against the low-latency mode (DRNSeg.set_low_latency,
csrc/conv_sk.hip), measured in one process with the two arms alternated.

For every (model, n x h x w) case, uint8 frames through segment():
  1. per call, a captured graph of segment() replayed (the GPU's time for the launch list, no host
     enqueue in it) and the eager call (what a per-frame Python loop pays), --rounds rounds of --reps
     repeats, a median per round, the arms alternated repeat by repeat;
  2. per launch, HIP events around every launch of one eager call (median of --reps calls): each launch
     the mode routes to conv_sk_kernel against the default launch that computes the same nodes (an
     unfolded block's conv2 + downsample against the default conv2 with the downsample folded in).

The mode "gains" where its median is below the default's by more than the spread (max - min) of the
default's rounds.  On a build without the mode only the default arm runs (the baseline table).

python scripts/low_latency_micro.py [--reps 20] [--rounds 3] [--json out.json]   (profiles/low_latency/)
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "video-seg-model-compress_amd"))
import torch  # noqa: E402

from drnmi import _lib as L  # noqa: E402
from drnmi.drnseg import build  # noqa: E402

DEV = "cuda"
CASES = [("drn_d_22", 1, 300, 300), ("drn_d_22", 1, 512, 512), ("drn_d_22", 1, 360, 640),
         ("drn_d_22", 25, 300, 300), ("drn_d_54", 1, 300, 300)]


def alternated(fn, reps, rounds, warmup=5):
    """{arm: [median ms of each round]} of the callables of `fn`, alternated repeat by repeat."""
    for f in fn.values():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    med = {k: [] for k in fn}
    for _ in range(rounds):
        ms = {k: [] for k in fn}
        for _ in range(reps):
            for k, f in fn.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1))
        for k in fn:
            med[k].append(statistics.median(ms[k]))
    return med


def captured(m, frames, labels):
    """A captured graph of m.segment(frames, labels=labels)."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            m.segment(frames, labels=labels)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        m.segment(frames, labels=labels)
    return g


def launch_times(m, frames, labels, reps):
    """[(node names of the launch, kernel name, median us)] in launch order, from events around every launch."""
    n, h, w = frames.shape[:3]
    plan = m.plan(n, h, w)
    lib = L.load()
    nodes = plan.packed.graph.nodes
    ls = plan.launches("u8" if plan.stem_u8 is not None else "nchw", plan.labels_path() != "nchw")
    by_row = {l.row: l for l in ls}
    runs = []
    for _ in range(reps):
        ev = []
        m.timing_hook = lambda i, nd, before: ev.append((i, before, torch.cuda.Event(enable_timing=True))) or ev[-1][2].record()
        m.segment(frames, labels=labels)
        m.timing_hook = None
        torch.cuda.synchronize()
        t = {}
        for (i, b0, e0), (j, b1, e1) in zip(ev[0::2], ev[1::2]):
            assert i == j and b0 and not b1
            t[i] = e0.elapsed_time(e1) * 1e3
        runs.append(t)
    out = []
    for row, l in by_row.items():
        out.append((tuple(nodes[k].name for k in l.nodes), l.kernel_name(lib), statistics.median(r[row] for r in runs)))
    return out


def case(name, n, h, w, reps, rounds):
    g = torch.Generator(device=DEV).manual_seed(11)
    frames = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device=DEV, generator=g)
    arms = {"default": build(name, 19, seed=0, device=DEV, precision="bf16")}
    if hasattr(arms["default"], "set_low_latency"):
        arms["low_latency"] = build(name, 19, seed=0, device=DEV, precision="bf16").set_low_latency(True)
    labels = {k: m.segment(frames) for k, m in arms.items()}
    torch.cuda.synchronize()
    row = {"model": name, "shape": [n, h, w]}
    if len(arms) == 2:
        row["routed"] = arms["low_latency"].low_latency_layers(n, h, w)
        row["label_agreement"] = float((labels["default"] == labels["low_latency"]).float().mean())
    graphs = {k: captured(m, frames, labels[k]) for k, m in arms.items()}
    for what, fn in (("graph", {k: g_.replay for k, g_ in graphs.items()}),
                     ("eager", {k: (lambda m=m, k=k: m.segment(frames, labels=labels[k])) for k, m in arms.items()})):
        med = alternated(fn, reps, rounds)
        d = med["default"]
        row[what] = {k: {"ms": statistics.median(v), "rounds_ms": v} for k, v in med.items()}
        row[what]["default_spread_ms"] = max(d) - min(d)
        line = "  ".join(f"{k} {statistics.median(v):7.3f} ms ({' '.join(f'{t:.3f}' for t in v)})" for k, v in med.items())
        print(f"{name} {n}x{h}x{w} {what:5s} per call: {line}  default spread {max(d) - min(d):.3f} ms", flush=True)
        if len(arms) == 2:
            gain = statistics.median(d) - statistics.median(med["low_latency"])
            row[what]["gains"] = gain > max(d) - min(d)
            print(f"    low latency {'GAINS' if row[what]['gains'] else 'no gain'}: {gain:+.3f} ms per call, "
                  f"{statistics.median(med['low_latency']) / n:.3f} vs {statistics.median(d) / n:.3f} ms per frame")
    times = {k: launch_times(m, frames, labels[k], reps) for k, m in arms.items()}
    row["launches"] = {k: [{"nodes": a, "kernel": b, "us": c} for a, b, c in v] for k, v in times.items()}
    if len(arms) == 2:
        sk = [t for t in times["low_latency"] if t[1].startswith("conv_sk")]
        node_ll = {nm: t for t in times["low_latency"] for nm in t[0]}
        row["routed_launches"] = []
        for nodes_d, kern_d, us_d in times["default"]:
            if not any(nm in t[0] for t in sk for nm in nodes_d):
                continue
            parts = {id(node_ll[nm]): node_ll[nm] for nm in nodes_d}.values()
            us_l = sum(t[2] for t in parts)
            row["routed_launches"].append({"nodes": nodes_d, "default": kern_d, "default_us": us_d, "low_latency_us": us_l,
                                           "kernels": [t[1] for t in parts]})
            print(f"    {' + '.join(nodes_d):44s} {us_d:7.1f} us {kern_d:34s} -> {us_l:7.1f} us "
                  f"{' + '.join(t[1] for t in parts)}", flush=True)
    else:
        for nodes_d, kern_d, us_d in times["default"]:
            print(f"    {' + '.join(nodes_d):44s} {us_d:7.1f} us {kern_d}")
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None, help="also write the tables to this file")
    opt = ap.parse_args()
    assert opt.rounds >= 3
    L.load()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    print(f"device {torch.cuda.get_device_name(0)}, {cus} CUs; {opt.rounds} rounds x {opt.reps} repeats per figure, arms alternated")
    result = {"cus": cus, "cases": [case(*c, opt.reps, opt.rounds) for c in CASES]}
    if opt.json:
        with open(opt.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
