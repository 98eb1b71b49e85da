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

    python tests/golden/make_launch_plans.py [--tree path/to/checkout]
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
         "drnmi_basic_block16", "drnmi_conv_stag_seg", "drnmi_quantize_i8")
FIXED_NAMES = {"drnmi_video_front_u8": "front3_kernel", "drnmi_basic_block64": "block64_kernel",
               "drnmi_basic_block16": "block16_kernel", "drnmi_quantize_i8": ""}
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
            for f in ("wpk", "scale", "shift", "unit_mask"):
                put(getattr(nd, f), f"{nd.name}.{f}")
            if nd.fused:
                put(nd.fused["wpk"], f"{nd.name}.fused.wpk")
                put(nd.fused["shift"], f"{nd.name}.fused.shift")
        put(pk.stem_u8_w, "stem_u8_w")
        put(plan.front_pack_t, "front_pack")
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
    elif entry == "drnmi_quantize_i8":
        src, code, dst, numel, inv = rest
        kernel, reads, writes, extra = b"", [src], [dst], [code, numel, float(inv)]
    else:                                                             # front, block64, block16
        x, pack, y, n, h, w = rest
        kernel, reads, writes, extra = FIXED_NAMES[entry].encode(), [x], [y], [names(pack), n, h, w]
    return {"entry": entry[len("drnmi_"):], "kernel": None if kernel is None else kernel.decode(),
            # (a quantise call reads what the launch before it produced: its own row or, a fused block, the next)
            "reads": [names(p, row + 2 if entry == "drnmi_quantize_i8" else row) for p in reads],
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
        assert (opened[-1] >= 0) == (entry != "drnmi_quantize_i8"), (entry, opened[-1])
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
    scales = {v: 0.05 for v in graph.channels} if precision == "int8" else None
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(HERE)), help="checkout to record (built)")
    ap.add_argument("--commit", default="", help="commit id of that checkout, written into the file")
    ap.add_argument("--out", default=os.path.join(HERE, "launch_plans.json.gz"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.abspath(args.tree), "video-seg-model-compress_amd"))
    table, cases = {}, {}
    for g, specs in groups().items():
        cases.update(record_group(specs, table))
        print(g, len(table), "distinct launches")
    doc = {"recorded_from": args.commit, "launch_table": list(table), "cases": cases}
    # (mtime 0 and no file name in the header: the same recording gives the same bytes)
    with open(args.out, "wb") as raw, gzip.GzipFile("", "wb", 9, raw, 0) as gz, io.TextIOWrapper(gz) as f:
        f.write('{"recorded_from": %s,\n"launch_table": [\n' % json.dumps(args.commit))
        f.write(",\n".join(json.dumps(s) for s in doc["launch_table"]))
        f.write('\n],\n"cases": {\n')
        f.write(",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in cases.items()))
        f.write("\n}}\n")
    print(len(cases), "cases,", len(table), "distinct launches,", os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
