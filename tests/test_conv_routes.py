"""The conv routing table is pinned against the commit before the routing refactor: for every row
of tests/route_grid.py, tests/golden/conv_routes.npz (tests/golden/make_route_golden.py) holds the
kernel name and the launch entry point's status that commit gave.  The fp8 rows (route_grid.grid_f8,
tests/golden/conv_routes_f8.npz) are pinned the same way against the commit that added fp8, before
the int8 and fp8 families were folded into one.  The name and status queries
must reproduce them: the status exactly, the name wherever the launch was accepted, and no name
wherever it was refused.  No launch entry point is called."""
import ctypes
import os

import numpy as np
import pytest

import route_grid
from drnmi import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TABLES = {"conv_routes": (route_grid.grid, 150000), "conv_routes_f8": (route_grid.grid_f8, 30000)}
# every fp8 kernel the route can reach.  The 1x1s all take the two-workgroups-per-CU tile (q8_variant:
# cout_pad % 128 == 0 always holds) and no tile id picks a variant, so the four KS = 1 rows of
# conv_f8_kernel and the KS = 3 row of conv_f8_occ2_kernel are dead table entries, as the same five
# rows of the int8 table are
F8_NAMES = {"conv_f8_kernel<3, 128, 2, 2, 128>", "conv_f8_kernel<3, 128, 1, 3, 128>", "conv_f8_kernel<3, 128, 2, 4, 64>",
            "conv_f8_kernel<3, 128, 1, 4, 64>", "conv_f8_occ2_kernel<1, 128, 1, 2, 64>", "conv_f8_stag_kernel"}


def _load(which):
    args, entry = TABLES[which][0]()
    z = np.load(os.path.join(GOLDEN, which + ".npz"), allow_pickle=False)
    return args, entry, [str(n) for n in z["names"]], z["name_index"], z["status"], str(z["sha256"]), which


@pytest.fixture(scope="module")
def table():
    return _load("conv_routes")


@pytest.fixture(scope="module")
def table_f8():
    return _load("conv_routes_f8")


def _query(lib, args, entry):
    """(name or None, status or None) per row; the seg-fused entry has no status query."""
    base, size = args.ctypes.data, args.dtype.itemsize
    names, status = [], []
    for i in range(len(args)):
        a = ctypes.cast(base + i * size, ctypes.POINTER(_lib.ConvArgs))
        if entry[i]:
            name, st = lib.drnmi_conv_stag_seg_kernel_name(a), None
        else:
            name, st = lib.drnmi_conv_kernel_name(a), lib.drnmi_conv_status(a)
        names.append(None if name is None else name.decode())
        status.append(st)
    return names, status


def _check_grid(table):
    args, entry, names, index, status, sha, which = table
    assert len(args) <= TABLES[which][1]
    assert route_grid.digest(args, entry) == sha
    assert len(index) == len(status) == len(args)
    # every kernel name of the table is reached by a row that launches
    assert {names[i] for i in np.unique(index[status == 0])} == set(names[1:])
    if which == "conv_routes_f8":
        assert set(names[1:]) == F8_NAMES
        assert set(np.unique(status[entry == 1])) == {-2}          # no seg-fused fp8 form


def _check_routes(table):
    args, entry, names, index, status, _, _ = table
    lib = _lib.load()
    got_names, got_status = _query(lib, args, entry)
    probes = args.copy()                     # the engine's probes leave the data pointers NULL
    for f in route_grid.DATA_POINTERS:
        probes[f] = 0
    probe_names, probe_status = _query(lib, probes, entry)
    bad = []
    for i in range(len(args)):
        want_name = names[index[i]] if status[i] == 0 else None
        ok = got_names[i] == want_name and probe_names[i] == want_name
        if not entry[i]:
            ok = ok and got_status[i] == status[i] and probe_status[i] == status[i] and \
                (got_names[i] is None) == (got_status[i] < 0)
        if not ok:
            bad.append((i, int(entry[i]), want_name, int(status[i]), got_names[i], got_status[i], probe_names[i],
                        probe_status[i]))
    assert not bad, f"{len(bad)} of {len(args)} rows differ; first: {bad[:5]}"


def test_grid_is_the_recorded_one(table):
    _check_grid(table)


def test_routes_match_the_parent_commit(table):
    _check_routes(table)


def test_f8_grid_is_the_recorded_one(table_f8):
    _check_grid(table_f8)


def test_f8_routes_match_the_parent_commit(table_f8):
    _check_routes(table_f8)
