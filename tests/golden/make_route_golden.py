"""Records the conv routing table of the library it is run against into conv_routes.npz (or, with the
table name "conv_routes_f8", the fp8 rows of route_grid.grid_f8() into conv_routes_f8.npz): for every
row of tests/route_grid.py the kernel name (drnmi_conv_kernel_name / drnmi_conv_stag_seg_kernel_name)
and the status of the launch entry point (drnmi_conv2d_bn_act / drnmi_conv_stag_seg): 0 when the
call got as far as a launch, else the negative drnmi_status it refused with.

Run once, on the commit before the routing refactor (conv_routes_f8: the commit that added fp8,
before the 8-bit families were folded), on a host WITHOUT a GPU: the launch entry
points are called with placeholder pointers, which is safe only where a launch attempt fails with
hipErrorNoDevice before anything runs.  The script refuses to run when a GPU is visible.

    python tests/golden/make_route_golden.py [conv_routes | conv_routes_f8] [path/to/libdrnmi.so]
"""
import collections
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(REPO, "video-seg-model-compress_amd"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)


def main():
    import torch
    if torch.cuda.is_available():
        sys.exit("make_route_golden.py: a GPU is visible; this tool calls launch entry points with placeholder "
                 "pointers and runs on GPU-less hosts only")
    from drnmi import _lib
    import route_grid
    from drnmi.build import LIB_PATH
    table = sys.argv[1] if len(sys.argv) > 1 else "conv_routes"
    grids = {"conv_routes": route_grid.grid, "conv_routes_f8": route_grid.grid_f8}
    if table not in grids:
        sys.exit(f"make_route_golden.py: unknown table {table!r}; one of {sorted(grids)}")
    lib = ctypes.CDLL(sys.argv[2] if len(sys.argv) > 2 else LIB_PATH)     # only the four entry points used here
    for f in ("drnmi_conv_kernel_name", "drnmi_conv_stag_seg_kernel_name", "drnmi_conv2d_bn_act", "drnmi_conv_stag_seg"):
        getattr(lib, f).restype, getattr(lib, f).argtypes = _lib.SIGNATURES[f]
    args, entry = grids[table]()
    names, index, status = [""], np.zeros(len(args), np.uint8), np.zeros(len(args), np.int8)
    base, size = args.ctypes.data, args.dtype.itemsize
    seg_w, partials = ctypes.c_void_p(route_grid.PTR), ctypes.c_void_p(route_grid.PTR)
    for i in range(len(args)):
        a = ctypes.cast(base + i * size, ctypes.POINTER(_lib.ConvArgs))
        if entry[i]:
            name = lib.drnmi_conv_stag_seg_kernel_name(a)
            rc = lib.drnmi_conv_stag_seg(a, seg_w, int(args["cout"][i]), 32, partials, None)
        else:
            name = lib.drnmi_conv_kernel_name(a)
            rc = lib.drnmi_conv2d_bn_act(a, None)
        name = "" if name is None else name.decode()
        if name not in names:
            names.append(name)
        index[i] = names.index(name)
        status[i] = rc if rc < 0 else 0
    np.savez_compressed(os.path.join(HERE, table + ".npz"), names=np.array(names), name_index=index,
                        status=status, sha256=np.array(route_grid.digest(args, entry)))
    hist = collections.Counter()
    for i in range(len(args)):
        hist[(names[index[i]], "launch" if status[i] == 0 else "refused")] += 1
    for n in names[1:]:
        print(f"{hist[(n, 'launch')]:7d} launch {hist[(n, 'refused')]:7d} refused  {n}")
    print(f"{hist[('', 'launch')]:7d} launch {hist[('', 'refused')]:7d} refused  (no name)")
    print(len(args), "rows,", len(names) - 1, "names; a name with 0 launch rows is a gap in the grid")


if __name__ == "__main__":
    main()
