"""The opt-in routes whose packing needs the device (2:4 in bf16 and int8, block-sparse unit masks,
the period-sparse pack, their precedence) and the low-latency rule, which reads the CU count,
against tests/golden/launch_plans_gpu.json.gz: D-22 plans at 1 x 64 x 2048 recorded by
tests/golden/make_launch_plans.py --fixture gpu on an MI355X, on the commit before the engine said
once which nodes are free for a route.  The recorder answers every launch entry point, so no conv
runs here: a case packs weights and builds one plan."""
from __future__ import annotations

import pytest
import torch

from test_launch_plan import G, check_launch_list, golden, resolved

pytestmark = pytest.mark.gpu
FIXTURE = "launch_plans_gpu.json.gz"


def test_fixture_covers_the_cases():
    doc = golden(FIXTURE)
    assert doc["recorded_from"] and list(doc["cases"]) == list(G.GPU_CASES)


@pytest.mark.parametrize("name", list(G.GPU_CASES))
def test_routes_equal_the_recorded_plan(name):
    doc = golden(FIXTURE)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if "low_latency" in G.GPU_CASES[name][2] and cus != doc["cus"]:
        pytest.skip(f"the low-latency rule reads the CU count: recorded on {doc['cus']} CUs, this device has {cus}")
    table, seen = {}, []

    def on_plan(_, plan, case, raw):
        check_launch_list(plan, raw)
        seen.append(plan)

    case = G.record_gpu_case(name, table, on_plan)
    assert seen and case["routes"] == doc["cases"][name]["routes"]
    assert resolved(case, list(table)) == resolved(doc["cases"][name], doc["launch_table"])
