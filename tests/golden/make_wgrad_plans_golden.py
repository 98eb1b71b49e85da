"""Records wgrad_plans.npz: for every row of tests/wgrad_grid.py the launch plan of the library it is
run against (drnmi_conv_wgrad_plan: kernel code, splits, pixels per split, reduce kernel) and both
workspace sizes (drnmi_conv_wgrad_workspace_bytes, drnmi_conv_wgrad_f32_workspace_bytes; -1 where the
geometry is refused).  The three queries are host-only; run it on a host WITHOUT a GPU, where the
plan's CU count is the 256 of the MI355X, on the commit before the weight-gradient tiles were folded.

    python tests/golden/make_wgrad_plans_golden.py [path/to/libdrnmi.so]
"""
import collections
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (REPO, os.path.join(REPO, "video-seg-model-compress_amd"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)


def query(lib, grid):
    """(status, kernel, splits, pix_per_split, reduce, bytes, bytes_f32) arrays of the grid's rows."""
    import wgrad_grid
    n = len(grid)
    out = {"status": np.zeros(n, np.int8), "kernel": np.zeros(n, np.uint8), "splits": np.zeros(n, np.int32),
           "pix_per_split": np.zeros(n, np.int64), "reduce": np.zeros(n, np.uint8), "bytes": np.zeros(n, np.int64),
           "bytes_f32": np.zeros(n, np.int64)}
    k, s, r, per = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64()
    for i, row in enumerate(grid):
        a = wgrad_grid.args_of(row)
        k.value = s.value = r.value = per.value = 0
        out["status"][i] = lib.drnmi_conv_wgrad_plan(ctypes.byref(a), int(row[11]), ctypes.byref(k), ctypes.byref(s),
                                                     ctypes.byref(per), ctypes.byref(r))
        out["kernel"][i], out["splits"][i], out["pix_per_split"][i], out["reduce"][i] = k.value, s.value, per.value, r.value
        out["bytes"][i] = lib.drnmi_conv_wgrad_workspace_bytes(ctypes.byref(a))
        out["bytes_f32"][i] = lib.drnmi_conv_wgrad_f32_workspace_bytes(ctypes.byref(a))
    return out


def main():
    import torch
    if torch.cuda.is_available():
        sys.exit("make_wgrad_plans_golden.py: a GPU is visible; the plan depends on its CU count, record on a GPU-less host")
    from drnmi import _lib
    import wgrad_grid
    from test_gpu_train_audit import WGRAD_PLAN_CASES
    lib = _lib.load(sys.argv[1] if len(sys.argv) > 1 else None)
    grid = wgrad_grid.rows(WGRAD_PLAN_CASES)
    got = query(lib, grid)
    np.savez_compressed(os.path.join(HERE, "wgrad_plans.npz"), sha256=np.array(wgrad_grid.digest(grid)), **got)
    hist = collections.Counter((int(k), int(r)) for k, r, st in zip(got["kernel"], got["reduce"], got["status"]) if st == 0)
    for (k, r), c in sorted(hist.items()):
        print(f"{c:7d}  {_lib.WGRAD_KERNELS[k]} + {_lib.WGRAD_REDUCES[r]}")
    print(len(grid), "rows,", int((got["status"] != 0).sum()), "refused")


if __name__ == "__main__":
    main()
