"""The weight-gradient launch plans and workspace sizes are pinned against the commit before the
64- and 128-tile kernels were folded into one template and the workspace layout into one function:
for every row of tests/wgrad_grid.py, tests/golden/wgrad_plans.npz
(tests/golden/make_wgrad_plans_golden.py) holds what drnmi_conv_wgrad_plan and the two workspace
queries gave at that commit.  They must reproduce it exactly.  Host-only: no launch, no GPU (without a
device the plan's CU count is the MI355X's 256)."""
import os
import sys

import numpy as np
import pytest

import train_audit as A
import wgrad_grid
from drnmi import _lib
from test_gpu_train_audit import WGRAD_PLAN_CASES

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
FIELDS = ("status", "kernel", "splits", "pix_per_split", "reduce", "bytes", "bytes_f32")


@pytest.fixture(scope="module")
def table():
    z = np.load(os.path.join(GOLDEN, "wgrad_plans.npz"), allow_pickle=False)
    return wgrad_grid.rows(WGRAD_PLAN_CASES), {f: z[f] for f in FIELDS}, str(z["sha256"])


def test_grid_is_the_recorded_one(table):
    grid, gold, sha = table
    assert len(grid) <= 100000 and wgrad_grid.digest(grid) == sha
    assert all(len(gold[f]) == len(grid) for f in FIELDS)
    assert not gold["status"].any()                     # every row is a geometry the library accepts
    rows = {tuple(r) for r in grid.tolist()}
    for c in list(WGRAD_PLAN_CASES) + wgrad_grid.EDGE_CASES:
        assert tuple(int(v) for v in c) in rows, c
    # all five kernel codes, each with the reduce kernels it can meet; both reduce kernels
    assert set(gold["kernel"].tolist()) == set(range(len(_lib.WGRAD_KERNELS)))
    assert set(gold["reduce"].tolist()) == set(range(len(_lib.WGRAD_REDUCES)))
    cs, cout, ks, m_over = grid[:, 1], grid[:, 2], grid[:, 4], gold["splits"] * gold["pix_per_split"]
    assert (gold["bytes"] >= gold["splits"].astype(np.int64) * cout * ks * ks * cs * 4).all()
    assert (gold["bytes"] >= gold["bytes_f32"]).all() and (m_over > 0).all()
    assert {16, 19, 32, 130, 200} <= set(cout.tolist()) and (grid[:, 0] < cs).any()
    assert gold["splits"].min() == 1 and gold["splits"].max() > 32


def test_plans_match_the_parent_commit(table):
    from make_wgrad_plans_golden import query
    grid, gold, _ = table
    got = query(_lib.load(), grid)
    bad = [(i, grid[i].tolist(), {f: (int(gold[f][i]), int(got[f][i])) for f in FIELDS if gold[f][i] != got[f][i]})
           for i in np.nonzero(np.any([gold[f] != got[f] for f in FIELDS], axis=0))[0]]
    assert not bad, f"{len(bad)} of {len(grid)} rows differ; first (golden, got): {bad[:5]}"


def test_grid_holds_the_benchmark_steps_launches(table):
    """Every weight gradient train_audit.step_routes lists for D-22 and D-54 at the benchmark shape,
    fp32 and fp32x, is a row of the grid, and its recorded plan is the one the walk reports."""
    grid, gold, _ = table
    index = {tuple(r): i for i, r in enumerate(grid.tolist())}
    seen = 0
    for arch in ("drn_d_22", "drn_d_54"):
        geo = dict(wgrad_grid.step_rows(arch, *wgrad_grid.BENCH_SHAPE))
        for precision in ("fp32", "fp32x"):
            for what, name, route in A.step_routes(arch, precision, *wgrad_grid.BENCH_SHAPE):
                if what != "wgrad":
                    continue
                i = index[geo[name] + (int(precision == "fp32x"),)]
                want = (_lib.WGRAD_KERNELS[gold["kernel"][i]], int(gold["splits"][i]), int(gold["pix_per_split"][i]),
                        _lib.WGRAD_REDUCES[gold["reduce"][i]])
                assert route[:4] == want, (arch, precision, name, route, want)
                seen += 1
    assert seen >= 2 * (22 + 54)
