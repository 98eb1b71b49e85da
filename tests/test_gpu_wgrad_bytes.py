"""The weight gradient, byte for byte: tests/golden/wgrad_bytes.json holds the sha256 of the raw dw
buffer of each launch below as the commit before the 64- and 128-tile kernels were folded into one
template wrote it on an MI355X (tests/golden/make_wgrad_bytes_golden.py).  The weight gradient has no
atomics and every sum has a fixed order, and the inputs come from a fixed seed on the CPU, so the bytes
are reproducible.  Each case is recorded twice: accumulate = 0, then accumulate = 1 onto that result.

The cases are WGRAD_PLAN_CASES (the smallest shapes that reach each kernel, split bucket, reduce
kernel, ragged last split and M % 32 != 0 class) and wgrad_grid.EDGE_CASES (rows past cout in a
128-tile's second row block, the 64-tile's row skip at cout 19, the element-wise dy loads at a
dy_stride tail).  The workspace is allocated at exactly the queried size with 64 B of 0xA5 behind it:
partials or dy planes laid out past what the query sized would land there."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import train_audit as A
import wgrad_grid
from test_gpu_train_audit import WGRAD_PLAN_CASES

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wgrad_bytes.json")
SLACK = 64            # bytes of 0xA5 around dw (part of the digest) and behind the workspace


def _name(case):
    return "-".join(str(int(v)) for v in case)


CASES = {_name(c): tuple(int(v) for v in c) for c in list(WGRAD_PLAN_CASES) + wgrad_grid.EDGE_CASES}
assert len(CASES) == len(WGRAD_PLAN_CASES) + len(wgrad_grid.EDGE_CASES)
# the kernel (DRNMI_WGRAD_* of include/drnmi.h) each edge case is there for: BIG, X6, F32
EDGE_KERNELS = dict(zip((_name(c) for c in wgrad_grid.EDGE_CASES), (2, 1, 0)))


def _inputs(name):
    cin, cs, cout, dys, ks, s, p, d, n, h, w, _ = CASES[name]
    a = A.wgrad_args(n, cin, cs, cout, dys, ks, s, p, d, h, w)
    g = torch.Generator().manual_seed(sorted(CASES).index(name))
    x = torch.zeros(n, h, w, cs)
    x[..., :cin] = torch.randn(n, h, w, cin, generator=g)
    dy = torch.zeros(n * a.ho * a.wo, dys)
    dy[:, :cout] = torch.randn(n * a.ho * a.wo, cout, generator=g)
    return a, x, dy


def run_case(name):
    """Launches CASES[name] twice (accumulate 0, then 1 onto the result); the whole dw buffer (slack
    included) after each launch as bytes on the host, and the plan's kernel code."""
    from drnmi import _lib
    lib = _lib.load()
    cin, cout, ks, x6 = CASES[name][0], CASES[name][2], CASES[name][4], CASES[name][11]
    a, x, dy = _inputs(name)
    kernel = ctypes.c_int32(-1)
    _lib.check(lib.drnmi_conv_wgrad_plan(ctypes.byref(a), x6, ctypes.byref(kernel), None, None, None), "wgrad plan")
    xd, dyd = x.to(DEV), dy.to(DEV)
    nb = (lib.drnmi_conv_wgrad_workspace_bytes if x6 else lib.drnmi_conv_wgrad_f32_workspace_bytes)(ctypes.byref(a))
    assert nb > 0, nb
    ws = torch.full((nb + SLACK,), 0xA5, dtype=torch.uint8, device=DEV)
    buf = torch.full((SLACK + cout * cin * ks * ks * 4 + SLACK,), 0xA5, dtype=torch.uint8, device=DEV)
    a.dy, a.x, a.dw, a.ws, a.ws_bytes = dyd.data_ptr(), xd.data_ptr(), buf.data_ptr() + SLACK, ws.data_ptr(), nb
    fn = lib.drnmi_conv_wgrad_f32x3 if x6 else lib.drnmi_conv_wgrad_f32
    out = []
    for acc in (0, 1):
        a.accumulate = acc
        _lib.check(fn(ctypes.byref(a), ctypes.c_void_p(_lib.stream_ptr(torch.device(DEV)))), name)
        torch.cuda.synchronize()
        assert bool((ws[nb:] == 0xA5).all()), f"{name}: wrote past the queried workspace size"
        out.append(buf.cpu().numpy())
    return out, kernel.value


def check_case(name, bufs, kernel):
    """The conditions on the recorded data: slack intact, every dw element finite and nonzero (a
    zeroed or skipped tile cannot hash equal by accident), the edge cases on their kernels."""
    for buf in bufs:
        assert bool((buf[:SLACK] == 0xA5).all()) and bool((buf[-SLACK:] == 0xA5).all()), f"{name}: wrote outside dw"
        dw = buf[SLACK:-SLACK].view(np.float32)
        assert bool(np.isfinite(dw).all()) and bool((dw != 0).all()), f"{name}: zero or non-finite dw element"
    assert kernel == EDGE_KERNELS.get(name, kernel), f"{name}: kernel code {kernel}"


def digest(buf):
    return hashlib.sha256(buf.tobytes()).hexdigest()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_cases_are_the_recorded_ones(golden):
    assert set(golden) == set(CASES)
    assert all(len(v) == 2 and v[0] != v[1] for v in golden.values())


@pytest.mark.parametrize("name", sorted(CASES))
def test_wgrad_bytes(name, golden):
    bufs, kernel = run_case(name)
    check_case(name, bufs, kernel)
    assert [digest(b) for b in bufs] == golden[name]
