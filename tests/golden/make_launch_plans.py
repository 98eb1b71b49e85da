"""Records the launch sequence of Plan.run_backbone into launch_plans.json.gz, without a GPU.

A Plan is built on torch.device("cpu") and run with drnmi._lib.load swapped for a Recorder: every
call goes to the real library except the launch entry points (ENTRY), which are written down and
answered with 0.  Per launch: the timing_hook index it ran under, its entry point, the kernel name
the library gives for its arguments, what it reads and writes (each pointer as the name of what it
points at: the plan.bufs key it means (class Names), "<node>.<field>" for packed weights,
"front_pack", "block pack (c, i)", "stem_u8_w", "frames") and a hash over every other field of its
drnmi_conv_args and its scalar arguments.  Per plan: the hook call sequence of each mode, both
roofline.launch_work tables, sorted(plan.bufs) and the plan's public attributes.  The file is
line-oriented JSON (one launch, one case per line; zcat shows it), gzipped to keep it small.

The file is generated from the commit BEFORE a change to the plan and committed unchanged;
tests/test_launch_plan.py reruns record_group() on the tree under test and compares.  Only
run_backbone, ingest_u8, the hook, launch_work and the plan's public attributes are used.

    python tests/golden/make_launch_plans.py [--tree path/to/checkout] [--commit id] [--fixture q8|gpu]

--fixture q8 writes launch_plans_q8.json.gz (groups_q8(): fp8, mxfp8, fp32x2, also without a GPU);
--fixture gpu, on an MI355X, launch_plans_gpu.json.gz (GPU_CASES: the routes that pack on the device
and the low-latency rule; tests/test_gpu_launch_routes.py).  There the plans live on the device and
the recorder still answers every launch, the split-K one included: no conv runs.
"""
import argparse
import ctypes
import gzip
import hashlib
import io
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ENTRY = ("drnmi_conv2d_bn_act", "drnmi_stem_layer1", "drnmi_video_front_u8", "drnmi_basic_block64",
         "drnmi_basic_block16", "drnmi_conv_stag_seg", "drnmi_conv_splitk",
         "drnmi_quantize_i8", "drnmi_quantize_f8", "drnmi_quantize_mx8")
QUANTIZE = ENTRY[-3:]
FIXED_NAMES = {"drnmi_video_front_u8": "front3_kernel", "drnmi_basic_block64": "block64_kernel",
               "drnmi_basic_block16": "block16_kernel"}
POINTER_FIELDS = ("x", "wgt", "scale", "shift", "res", "y", "unit_mask", "x2", "ws", "stats")
FRAMES = {"1x64x2048": (1, 64, 2048), "2x72x136": (2, 72, 136)}
SEEDS = {"drn_d_22": 3, "drn_d_54": 5, "drn_c_26": 6, "drn_c_58": 9}
FLAGS = ("FUSE_FRONT", "FUSE_STEM", "FUSE_BLOCK64", "FUSE_DOWNSAMPLE", "SEG_FUSE", "LABELS_NHWC", "FUSE_BLOCK16")
MEAN, STD = (0.29, 0.33, 0.28), (0.18, 0.19, 0.18)


def groups():
    """{group: [(case name, arch, classes, precision, keep_all, frame, flag switched off)]}; a group
    shares one model."""
    out = {}
    for arch in SEEDS:
        for precision in ("bf16", "fp32", "fp32x") + (("int8",) if "_d_" in arch else ()):
            out[f"{arch}/{precision}"] = [(f"{arch}/{precision}/{'keep_all' if keep else 'fused'}/{fr}", arch, 19,
                                           precision, keep, fr, None)
                                          for keep in (False, True) for fr in FRAMES]
    extra = [(f"drn_d_22/bf16/fused/1x64x2048/{f}=0", "drn_d_22", 19, "bf16", False, "1x64x2048", f) for f in FLAGS[:6]]
    extra.append(("drn_d_22x21/bf16/fused/1x64x2048", "drn_d_22", 21, "bf16", False, "1x64x2048", None))
    extra.append(("drn_c_26/bf16/fused/1x64x2048/FUSE_BLOCK16=0", "drn_c_26", 19, "bf16", False, "1x64x2048", "FUSE_BLOCK16"))
    out["switches"] = extra
    return out


def groups_q8():
    """The same for launch_plans_q8.json.gz: the precisions launch_plans.json.gz does not hold."""
    return {f"drn_d_22/{precision}": [(f"drn_d_22/{precision}/{'keep_all' if keep else 'fused'}/{fr}", "drn_d_22", 19,
                                       precision, keep, fr, None)
                                      for keep in (False, True) for fr in FRAMES]
            for precision in ("fp8", "mxfp8", "fp32x2")}


# launch_plans_gpu.json.gz: the routes whose packers run on the device or need pinned memory, and the
# low-latency rule, which reads the CU count.  case -> (the test file whose model it takes, precision,
# the switches set on it); every plan is D-22 at GPU_FRAME, built by DRNSeg.plan
GPU_FRAME = "1x64x2048"
GPU_CASES = {"sparse24/bf16": ("sp24", "bf16", ("sparse24",)),
             "sparse24/int8": ("sp24", "int8", ("sparse24",)),
             "block_sparse": ("sparse", "bf16", ("block_sparse",)),
             "srmb_sparse": ("srmb", "bf16", ("srmb_sparse",)),
             "low_latency": ("low_latency", "bf16", ("low_latency",)),
             "srmb_sparse+sparse24": ("srmb", "bf16", ("srmb_sparse", "sparse24"))}


def digest(obj) -> str:
    return hashlib.sha1(json.dumps(obj, sort_keys=True).encode()).hexdigest()[:10]


def num(x):
    """Integral floats as ints (exact below 2^53): shorter, and == the float they came from."""
    return int(x) if float(x).is_integer() else float(x)


class Recorder:
    """The library with the launch entry points replaced by a log: calls = [(entry, arguments)]."""

    def __init__(self, lib):
        self.lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if name not in ENTRY:
            return fn

        def record(*args):
            self.calls.append((name, args))
            return 0
        return record


class Names:
    """address -> name of what lives there.  Activation buffers are pooled (Plan.__init__), and which
    of two free buffers of one size a value gets follows the iteration order of a set of strings,
    so it differs from process to process: "the first plan.bufs key with that address" is not
    reproducible.  A buffer is named by the value the launch means instead: of the plan.bufs keys at
    that address, a launch under hook index `row` writes the first one produced at or after `row`
    and reads the last one produced before it (a "q:<v>" copy counts as produced with v).  Any other
    wiring -- a wrong buffer, or one overwritten before its last reader -- gives another name."""

    def __init__(self, plan, frames):
        self.fixed, self.alias = {}, {}
        pk = plan.packed
        self.producer = {nd.dst: i for i, nd in enumerate(pk.graph.nodes)}
        for k, t in plan.bufs.items():
            self.alias.setdefault(t.data_ptr(), []).append(k)

        def put(t, name):
            if t is not None:
                self.fixed.setdefault(t.data_ptr(), name)
        put(frames, "frames")
        for nd in pk.graph.nodes:
            for f in ("wpk", "scale", "shift", "unit_mask", "wsp", "wps"):
                put(getattr(nd, f), f"{nd.name}.{f}")
            if nd.fused:
                put(nd.fused["wpk"], f"{nd.name}.fused.wpk")
                put(nd.fused["shift"], f"{nd.name}.fused.shift")
        put(pk.stem_u8_w, "stem_u8_w")
        put(plan.front_pack_t, "front_pack")
        put(plan.sk_ws, "sk_ws")
        for c, packs in ((64, plan.block64), (16, plan.block16)):
            for i, t in packs.items():
                put(t, f"block pack ({c}, {i})")

    def __call__(self, p, row=0, write=False):
        a = _addr(p)
        if a == 0:
            return None
        keys = self.alias.get(a)
        if keys is None:
            return self.fixed.get(a, "UNKNOWN")
        made = sorted((self.producer.get(k[2:] if k.startswith("q:") else k, -1), k) for k in keys)
        if len(made) == 1:
            return made[0][1]
        pick = [k for at, k in made if at >= row] if write else [k for at, k in made if at < row][::-1]
        return pick[0] if pick else "UNKNOWN"


def _addr(p):
    p = getattr(p, "value", p)
    return int(p) if p else 0


def dump_args(a, names, row) -> dict:
    """Every field of one drnmi_conv_args of a launch under hook index `row`: pointers by name,
    arrays as lists."""
    out = {}
    for f, _ in type(a)._fields_:
        v = getattr(a, f)
        out[f] = names(v, row, f == "y") if f in POINTER_FIELDS else list(v) if hasattr(v, "__len__") else v
    return out


def describe(lib, entry, args, names, row) -> dict:
    """One recorded call under hook index `row` as {entry, kernel, reads, writes, hash, addr: (reads,
    writes) addresses}."""
    structs = [x._obj for x in args if hasattr(x, "_obj")]
    rest = [x for x in args if not hasattr(x, "_obj")][:-1]           # (the last argument is the stream)
    dumps = [dump_args(a, names, row) for a in structs]

    def io(a):
        return [p for p in (a.x, a.res, a.x2) if p]
    if entry == "drnmi_conv2d_bn_act":
        kernel = lib.drnmi_conv_kernel_name(ctypes.byref(structs[0]))
        reads, writes, extra = io(structs[0]), [structs[0].y], []
    elif entry == "drnmi_stem_layer1":
        kernel = lib.drnmi_stem_layer1_kernel_name(ctypes.byref(structs[0]), ctypes.byref(structs[1]))
        reads, writes, extra = [structs[0].x], [structs[1].y], []
    elif entry == "drnmi_conv_stag_seg":
        kernel = lib.drnmi_conv_stag_seg_kernel_name(ctypes.byref(structs[0]))
        seg_w, k_pad, rows, part = rest
        reads, writes, extra = io(structs[0]), [part], [names(seg_w), k_pad, rows]
    elif entry == "drnmi_conv_splitk":
        kernel = lib.drnmi_conv_splitk_kernel_name(ctypes.byref(structs[0]), rest[0])
        reads, writes, extra = io(structs[0]), [structs[0].y], [rest[0]]
    elif entry == "drnmi_quantize_i8":
        src, code, dst, numel, inv = rest
        kernel, reads, writes, extra = b"", [src], [dst], [code, numel, float(inv)]
    elif entry == "drnmi_quantize_f8":
        src, code, numel, inv, dst = rest
        kernel, reads, writes, extra = b"", [src], [dst], [code, numel, float(inv)]
    elif entry == "drnmi_quantize_mx8":
        src, code, m, c, dst = rest
        kernel, reads, writes, extra = b"", [src], [dst], [code, m, c]
    else:                                                             # front, block64, block16
        x, pack, y, n, h, w = rest
        kernel, reads, writes, extra = FIXED_NAMES[entry].encode(), [x], [y], [names(pack), n, h, w]
    return {"entry": entry[len("drnmi_"):], "kernel": None if kernel is None else kernel.decode(),
            # (a quantise call reads what the launch before it produced: its own row or, a fused block, the next)
            "reads": [names(p, row + 2 if entry in QUANTIZE else row) for p in reads],
            "writes": [names(p, row, True) for p in writes],
            "hash": digest([dumps, extra]), "addr": ([_addr(p) for p in reads], [_addr(p) for p in writes]),
            "dump": [dumps, extra]}


def record_mode(plan, engine, _lib, src, labels_only, frames):
    """One run_backbone of `plan` under the recorder: (hook sequence, [described launches])."""
    real = _lib.load()
    rec = Recorder(real)
    nodes = plan.packed.graph.nodes
    hooks, at = [], []

    def hook(i, nd, before):
        assert nd is nodes[i]
        hooks.append(i if before else -1 - i)
        at.append(len(rec.calls))
    keep = _lib.load
    _lib.load = lambda *a: rec
    try:
        if src == "u8":
            plan.ingest_u8(frames, MEAN, STD, False, 0)
            assert plan.src == "u8"
        else:
            plan.src = "nchw"
        plan.run_backbone(0, hook, labels_only=labels_only)
    finally:
        _lib.load = keep
    names = Names(plan, frames)
    out, idx = [], None
    for k, (entry, args) in enumerate(rec.calls):
        # the index of the hook pair that brackets this call, or (quantise) of the pair before it
        opened = [h for h, n_ in zip(hooks, at) if n_ <= k]
        idx = opened[-1] if opened[-1] >= 0 else -1 - opened[-1]
        assert (opened[-1] >= 0) == (entry not in QUANTIZE), (entry, opened[-1])
        d = describe(real, entry, args, names, idx)
        d["index"] = idx
        out.append(d)
    return hooks, out


def attributes(plan, names) -> dict:
    """The plan's public attributes, pointers by name, arg structs as hashes of their dump."""
    def h(a, row):
        return None if a is None else digest(dump_args(a, names, row))
    sf = plan.seg_fused
    if sf is not None:
        sf = {k: names(v) if k in ("seg_w", "bias", "scale") else v for k, v in sf.items()}
    return {"args": [h(a, i) for i, a in enumerate(plan.args)], "skip": sorted(plan.skip),
            "block64": {str(i): names(t.data_ptr()) for i, t in plan.block64.items()},
            "block16": {str(i): names(t.data_ptr()) for i, t in plan.block16.items()},
            "stem_fused": bool(plan.stem_fused), "front_fused": bool(plan.front_fused), "stem_u8": h(plan.stem_u8, 0),
            "seg_idx": plan.seg_idx, "seg_nhwc_args": h(plan.seg_nhwc_args, plan.seg_idx), "seg_fused": sf,
            "labels_path": plan.labels_path(), "labels_path_torch_up": plan.labels_path(True),
            "front_pack_t": None if plan.front_pack_t is None else names(plan.front_pack_t.data_ptr()),
            "_reads_of": [sorted(plan._reads_of[i]) for i in range(len(plan.args))],
            "fuse": plan.fuse, "keep_all": plan.keep_all, "SEG_NHWC_CS": plan.SEG_NHWC_CS,
            "seg_classes": plan.seg_classes, "seg_cs": plan.seg_cs}


def record_plan(plan, engine, _lib, roofline, table):
    """Everything recorded of one plan; `table` collects the distinct launches of the file
    ("index entry kernel reads -> writes #hash" strings, referenced by position).  Returns
    (json-able case, {mode: raw launches}) -- the raw launches carry addresses and full dumps."""
    import torch
    frames = torch.zeros(plan.n, plan.h, plan.w, 3, dtype=torch.uint8)
    modes = [("nchw/full", "nchw", False), ("u8/full", "u8", False)]
    case, raw = {"modes": {}}, {}
    for mode, src, lo in modes + [("u8/labels", "u8", True)]:
        if lo and plan.labels_path() == "nchw":
            continue
        hooks, launches = record_mode(plan, engine, _lib, src, lo, frames)
        raw[mode] = launches
        refs = []
        for d in launches:
            s = "%d %s %s %s -> %s #%s" % (d["index"], d["entry"], d["kernel"], ",".join(map(str, d["reads"])),
                                          ",".join(map(str, d["writes"])), d["hash"])
            if s not in table:
                table[s] = len(table)
            refs.append(table[s])
        case["modes"][mode] = {"hooks": hooks, "launches": refs}
    names = Names(plan, frames)
    nodes = plan.packed.graph.nodes
    for video in (True, False):
        rows = roofline.launch_work(plan, video)
        assert [r[0] for r in rows] == [nd.name for nd in nodes] + ["head"]
        case["launch_work_video" if video else "launch_work"] = [[num(f), num(b)] for _, f, b in rows]
    case["bufs"] = sorted(plan.bufs)
    case["attrs"] = attributes(plan, names)
    return case, raw


_MODELS = {}


def model(arch, classes):
    import torch  # noqa: F401
    from drnmi.drnseg import DRNSeg
    from drnmi.weights import synth_state_dict
    if (arch, classes) not in _MODELS:
        m = DRNSeg(arch, classes, pretrained=False)
        m.load_state_dict(synth_state_dict(m, SEEDS[arch]))
        _MODELS[(arch, classes)] = m.eval()
    return _MODELS[(arch, classes)]


def build_plan(spec, packs=None):
    """(plan, packed) of one case; PackedNets are shared through `packs` where no switch is off."""
    import torch
    from drnmi import engine
    _, arch, classes, precision, keep_all, frame, off = spec
    graph = model(arch, classes)._graph
    key = (arch, classes, precision, off if off not in ("SEG_FUSE", "LABELS_NHWC", "FUSE_STEM") else None)
    scales = {v: 0.05 for v in graph.channels} if precision in ("int8", "fp8") else None
    if off:
        assert getattr(engine, off) is True
        setattr(engine, off, False)
    try:
        packed = None if packs is None else packs.get(key)
        if packed is None:
            packed = engine.PackedNet(graph, precision, torch.device("cpu"), block_sparse=False, act_scales=scales)
            if packs is not None:
                packs[key] = packed
        return engine.Plan(packed, *FRAMES[frame], keep_all=keep_all), packed
    finally:
        if off and off != "LABELS_NHWC":
            setattr(engine, off, True)


def record_group(specs, table, on_plan=None):
    """{case name: case} of one group.  LABELS_NHWC is read when a step runs, so it stays off until
    its case is recorded.  on_plan(spec, plan, case, raw) sees each plan while it is live."""
    from drnmi import _lib, engine, roofline
    out, packs = {}, {}
    for spec in specs:
        try:
            plan, _ = build_plan(spec, packs)
            case, raw = record_plan(plan, engine, _lib, roofline, table)
            out[spec[0]] = case
            if on_plan is not None:
                on_plan(spec, plan, case, raw)
        finally:
            engine.LABELS_NHWC = True
    return out


def gpu_model(kind):
    """The D-22 of a GPU case on the device, prepared as tests/test_gpu_<kind>.py prepares its own
    ("sp24": test_gpu_sp24.py's masks and test_gpu_sp24_i8.py's calibration on them)."""
    if kind in _MODELS:
        return _MODELS[kind]
    import tempfile
    import numpy as np
    import torch
    from drnmi import pruners as P
    from drnmi.drnseg import DRNSeg, build
    from drnmi.weights import synth_frames, synth_state_dict

    def pruner(cfg, **kw):
        with tempfile.TemporaryDirectory() as d:
            with open(os.path.join(d, "cfg.json"), "w") as f:
                json.dump(cfg, f)
            return P.make_pruner(f.name, **kw)
    np.random.seed(22)
    if kind == "sparse":                          # pruned_model("drn_d_22", 2, block_cfg(probe, 16, 32, 0.5))
        m = DRNSeg("drn_d_22", 19, pretrained=False)
        m.load_state_dict(synth_state_dict(m, 2))
        layers = [k for k, v in m.state_dict().items() if k.startswith("layer.") and k.endswith(".weight")
                  and v.dim() == 4 and v.shape[1] >= 16 and v.shape[0] % 16 == 0 and v.shape[1] % 32 == 0]
        pr = pruner({"pruner_type": "block", "configs": [{"layer_set": layers, "sparsity": 0.5, "block_height": 16,
                                                          "block_width": 32, "sub_rows": -1, "sub_cols": -1,
                                                          "collapse_tensor": False}]}, on_gpu=False)
        pr.generate_masks(m, is_static=False)
        with torch.no_grad():
            sd = m.state_dict()
            for k, mk in pr.mask_dict.items():
                sd[k].mul_(mk)
        m = m.to("cuda").eval()
    else:
        m = build("drn_d_22", 19, seed=0, device="cuda")
        if kind == "sp24":
            layers = [nd.name + ".weight" for nd in m._graph.nodes if nd.conv.in_channels >= 64]
            pr = pruner({"pruner_type": "nm", "configs": [{"layer_set": layers, "n": 2, "m": 4}]})
            pr.generate_masks(m)
            pr.apply_masks(m)
            m.calibrate_int8(torch.from_numpy(synth_frames(7, 2, 128, 256)).to("cuda"))
        elif kind == "srmb":
            pr = P.make_pruner(os.path.join(HERE, "srmb_d22_1024X768_50.json"))
            pr.generate_masks(m, is_static=True)
            pr.apply_masks(m)
    _MODELS[kind] = m
    return m


def record_gpu_case(name, table, on_plan=None):
    """One case of GPU_CASES, recorded like the CPU ones (no launch reaches the device), plus what
    the routes say of themselves."""
    from drnmi import _lib, engine, roofline
    kind, precision, switches = GPU_CASES[name]
    m = gpu_model(kind)
    floor = engine.SPARSE_MIN_ZERO_UNITS
    if "block_sparse" in switches:
        engine.SPARSE_MIN_ZERO_UNITS = 0.05       # every layer with any zero unit (tests/test_gpu_sparse.py)
    try:
        m.set_precision(precision)
        for s in switches:
            getattr(m, "set_" + s)(True)
        plan = m.plan(*FRAMES[GPU_FRAME])
        case, raw = record_plan(plan, engine, _lib, roofline, table)
        case["routes"] = {"sparse24_layers": plan.packed.sparse24_layers(),
                          "srmb_sparse_layers": plan.packed.srmb_sparse_layers(),
                          "unit_mask": [nd.name for nd in plan.packed.graph.nodes if nd.unit_mask is not None],
                          "sk": {str(i): S for i, S in sorted(plan.sk.items())}, "unfold": sorted(plan.unfold)}
        if on_plan is not None:
            on_plan(name, plan, case, raw)
    finally:
        engine.SPARSE_MIN_ZERO_UNITS = floor
        for s in switches:
            getattr(m, "set_" + s)(False)
        m.set_precision("fp32")
    return case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(HERE)), help="checkout to record (built)")
    ap.add_argument("--commit", default="", help="commit id of that checkout, written into the file")
    ap.add_argument("--fixture", default="", choices=("", "q8", "gpu"), help="launch_plans_<fixture>.json.gz (gpu: on an MI355X)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    out = args.out or os.path.join(HERE, "launch_plans%s.json.gz" % ("_" + args.fixture if args.fixture else ""))
    sys.path.insert(0, os.path.join(os.path.abspath(args.tree), "video-seg-model-compress_amd"))
    table, cases, head = {}, {}, {"recorded_from": args.commit}
    if args.fixture == "gpu":
        import torch
        head["cus"] = torch.cuda.get_device_properties(0).multi_processor_count
        for name in GPU_CASES:
            cases[name] = record_gpu_case(name, table)
            print(name, len(table), "distinct launches", cases[name]["routes"])
    else:
        for g, specs in (groups_q8() if args.fixture == "q8" else groups()).items():
            cases.update(record_group(specs, table))
            print(g, len(table), "distinct launches")
    # (mtime 0 and no file name in the header: the same recording gives the same bytes)
    with open(out, "wb") as raw, gzip.GzipFile("", "wb", 9, raw, 0) as gz, io.TextIOWrapper(gz) as f:
        f.write("{%s,\n" % ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in head.items()))
        f.write('"launch_table": [\n')
        f.write(",\n".join(json.dumps(s) for s in table))
        f.write('\n],\n"cases": {\n')
        f.write(",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in cases.items()))
        f.write("\n}}\n")
    print(len(cases), "cases,", len(table), "distinct launches,", os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
