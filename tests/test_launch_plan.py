"""Plan.launches against the launch sequences recorded before the plan said what it launches.

tests/golden/launch_plans.json.gz was written by tests/golden/make_launch_plans.py on the commit
before Plan.launches existed (its "recorded_from"): every C call of run_backbone on CPU-built plans,
with the hook indices, kernel names, buffers by name and a hash of every other argument, plus
launch_work and the plan's public attributes.  Here the same recorder runs on this tree and must
see the same thing, and the Launch list must describe exactly the calls the recorder saw.  No GPU:
the launch entry points are answered by the recorder."""
from __future__ import annotations

import gzip
import json
import os
import sys

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import make_launch_plans as G  # noqa: E402

from drnmi import _lib, engine, roofline  # noqa: E402

KIND_OF = {"conv2d_bn_act": "conv", "stem_layer1": "stem_layer1", "video_front_u8": "front",
           "basic_block64": "block64", "basic_block16": "block16", "conv_stag_seg": "conv_seg"}
MODES = {"nchw/full": ("nchw", False), "u8/full": ("u8", False), "u8/labels": ("u8", True)}
_DOC = {}


def golden():
    if not _DOC:
        with gzip.open(os.path.join(GOLDEN, "launch_plans.json.gz"), "rt") as f:
            _DOC.update(json.load(f))
    return _DOC


def resolved(case: dict, table: list) -> dict:
    """The case with its launch references replaced by the launch strings."""
    out = dict(case)
    out["modes"] = {m: {"hooks": v["hooks"], "launches": [table[r] for r in v["launches"]]}
                    for m, v in case["modes"].items()}
    return out


def check_launch_list(plan, raw: dict):
    """plan.launches(src, labels_only) is the recorded call sequence: rows, kinds, kernel names,
    buffers read and written, the quantise calls after each; and it partitions the nodes."""
    lib = _lib.load()
    bufs = plan.bufs
    buf_addrs = {t.data_ptr() for t in bufs.values()}
    nodes = plan.packed.graph.nodes
    for mode, calls in raw.items():
        launches = plan.launches(*MODES[mode])
        seen = [d for d in calls if d["entry"] != "quantize_i8"]
        assert [(l.row, l.kind) for l in launches] == [(d["index"], KIND_OF[d["entry"]]) for d in seen], mode
        for l, d in zip(launches, seen):
            assert l.kernel_name(lib) == (d["kernel"] or ""), (mode, l.row)
            assert l.row in l.nodes
            assert [bufs[k].data_ptr() for k in l.writes] == d["addr"][1], (mode, l.row, l.writes)
            assert {bufs[k].data_ptr() for k in l.reads} == {a for a in d["addr"][0] if a in buf_addrs}, (mode, l.row)
            if any(a not in buf_addrs for a in d["addr"][0]):       # the caller's frames
                assert l.row == 0 and l.reads == () and MODES[mode][0] == "u8"
        quant = [(d["index"], d["addr"]) for d in calls if d["entry"] == "quantize_i8"]
        assert quant == [(l.row, ([bufs[v].data_ptr()], [bufs["q:" + v].data_ptr()])) for l in launches for v in l.quant]
        assert sorted(k for l in launches for k in l.nodes) == list(range(len(nodes))), mode
        for i, nd in enumerate(nodes):
            if i in plan.skip:                    # a folded downsample runs in its block's last conv
                assert [l.row for l in launches if i in l.nodes] == [nd.fused_into]


def check_refresh(plan, name: str):
    """After a repack the plan records as the same case again, on the new weight tensors (the old
    ones are kept alive, so no address can repeat), from rebuilt launch lists."""
    before = {m: plan.launches(*sm) for m, sm in MODES.items()}
    old = [t for nd in plan.packed.graph.nodes
           for t in (nd.wpk, nd.scale, nd.shift) + ((nd.fused["wpk"], nd.fused["shift"]) if nd.fused else ())]
    old_wgt = [a.wgt for a in plan.args if a is not None]
    plan.packed.pack()
    plan.refresh_weight_ptrs()
    assert all(a != b for a, b in zip(old_wgt, [a.wgt for a in plan.args if a is not None]))
    table = {}
    case, raw = G.record_plan(plan, engine, _lib, roofline, table)
    assert resolved(case, list(table)) == resolved(golden()["cases"][name], golden()["launch_table"])
    for m, sm in MODES.items():
        assert plan.launches(*sm) is not before[m]
    check_launch_list(plan, raw)
    del old


def check_live_args(plan):
    """A launch reads the plan's own arg structs when it runs: a tile forced on plan.args[j] after the
    launch list was built reaches the next run (tests/test_gpu_head_nhwc.py relies on it)."""
    import torch
    frames = torch.zeros(plan.n, plan.h, plan.w, 3, dtype=torch.uint8)
    launches = plan.launches("nchw", False)
    j = [l for l in launches if l.kind == "conv"][-2].row
    plan.args[j].tile = 19
    try:
        _, calls = G.record_mode(plan, engine, _lib, "nchw", False, frames)
        assert plan.launches("nchw", False) is launches
        tiles = {d["index"]: d["dump"][0][0]["tile"] for d in calls if d["entry"] == "conv2d_bn_act"}
        assert tiles[j] == 19 and all(t == -1 for i, t in tiles.items() if i != j)
    finally:
        plan.args[j].tile = -1


def test_fixture_covers_the_cases():
    doc = golden()
    assert doc["recorded_from"]
    assert list(doc["cases"]) == [spec[0] for specs in G.groups().values() for spec in specs]


@pytest.mark.parametrize("group", list(G.groups()))
def test_launches_equal_the_recorded_plan(group):
    doc = golden()
    table, seen = {}, []

    def on_plan(spec, plan, case, raw):
        check_launch_list(plan, raw)
        if not seen:                              # once per group: the repack and the live arg structs
            check_live_args(plan)
            check_refresh(plan, spec[0])
        seen.append(spec[0])

    cases = G.record_group(G.groups()[group], table, on_plan)
    for name, case in cases.items():
        assert resolved(case, list(table)) == resolved(doc["cases"][name], doc["launch_table"]), name
    assert seen == list(cases)
