"""The deterministic grid of weight-gradient geometries behind tests/test_wgrad_plans.py and
tests/golden/make_wgrad_plans_golden.py: a pure function of nothing (no randomness, no library call).

rows() returns an int64 array [rows][12] of (cin, cin_stride, cout, dy_stride, ks, stride, pad, dil,
n, h, w, x6), the column order of test_gpu_train_audit.WGRAD_PLAN_CASES:
  * a full product over channel strides 8 .. 512 (cin = the stride and cin < the stride), cout with
    16, 19, 32, 130 and 200 among them, dy_stride = cout rounded up to 4 and to a power of two,
    ks 1 / 3 / 7, stride 1 / 2, dilation 1 / 2 / 4 and pixel counts from under one 512-pixel split to
    over 32 of them (M % 32 != 0 and wo % 32 == 0 both included), for both arithmetics;
  * every row of WGRAD_PLAN_CASES and the three edge cases of tests/test_gpu_wgrad_bytes.py;
  * every weight gradient of one DRN-D-22 and one DRN-D-54 fine-tune step at the benchmark shape.
"""
import hashlib
import itertools

import numpy as np

COLUMNS = ("cin", "cin_stride", "cout", "dy_stride", "ks", "stride", "pad", "dil", "n", "h", "w", "x6")
BENCH_SHAPE = (2, 1024, 768)        # bench_finetune.py: 2 crops of 1024 x 768
# (n, h, w): M = 360 (under one split) .. 1.5 M (the cap of 512 splits); odd sizes, wo % 32 == 0
PIXELS = [(1, 9, 40), (1, 9, 64), (1, 21, 32), (1, 15, 35), (2, 33, 47), (1, 64, 64), (1, 126, 128), (2, 84, 95),
          (2, 96, 120), (1, 132, 128), (2, 256, 192), (2, 1024, 768)]
# the edges the fold of the two tiles touches (tests/test_gpu_wgrad_bytes.py runs them)
EDGE_CASES = [
    (128, 128, 200, 256, 1, 1, 0, 1, 1, 9, 64, True),      # 128-tile, rows past cout in the second row block
    (64, 64, 19, 32, 1, 1, 0, 1, 1, 9, 40, True),          # split-bf16 64-tile, row skip at cout 19
    (64, 64, 60, 60, 3, 1, 1, 1, 1, 9, 40, False),         # 64-tile, element-wise dy loads at the dy_stride tail
]


def _pow2_at_least(c):
    p = 8
    while p < c:
        p *= 2
    return p


def product_rows():
    out = []
    for cs, part, cout, dpow, ks, (s, d), (n, h, w), x6 in itertools.product(
            [8, 16, 32, 64, 128, 256, 512], [0, 1], [16, 19, 32, 60, 64, 128, 130, 200, 256, 512], [0, 1], [1, 3, 7],
            [(1, 1), (2, 1), (1, 2), (1, 4)], PIXELS, [0, 1]):
        cin = cs if not part else (3 if cs == 8 else cs * 3 // 4)
        dys = _pow2_at_least(cout) if dpow else (cout + 3) // 4 * 4
        out.append((cin, cs, cout, dys, ks, s, d * (ks - 1) // 2, d, n, h, w, x6))
    return out


def step_rows(arch, n, h, w):
    """(node name, row without x6) of every weight gradient of one fine-tune step, in backward order
    (the geometry train_audit.step_routes gives drnmi_conv_wgrad_plan)."""
    from drnmi.drnseg import DRNSeg
    from drnmi.engine import _conv_out
    g = DRNSeg(arch, 19, pretrained=False)._graph
    cstride = {v: _pow2_at_least(c) for v, c in g.channels.items()}
    cstride["input"] = 8
    shapes = {"input": (h, w)}
    for nd in g.nodes:
        c = nd.conv
        ih, iw = shapes[nd.src]
        ks, s, p, d = c.kernel_size[0], c.stride[0], c.padding[0], c.dilation[0]
        shapes[nd.dst] = (_conv_out(ih, ks, s, p, d), _conv_out(iw, ks, s, p, d))
    out = []
    for nd in reversed(g.nodes):
        c = nd.conv
        ih, iw = shapes[nd.src]
        dys = _pow2_at_least(c.out_channels) if nd.out_fp32_nchw else cstride[nd.dst]
        out.append((nd.name, (c.in_channels, cstride[nd.src], c.out_channels, dys, c.kernel_size[0], c.stride[0],
                              c.padding[0], c.dilation[0], n, ih, iw)))
    return out


def rows(plan_cases):
    """The whole grid; `plan_cases` = test_gpu_train_audit.WGRAD_PLAN_CASES."""
    out = product_rows() + [tuple(int(v) for v in c) for c in plan_cases] + [tuple(int(v) for v in c) for c in EDGE_CASES]
    for arch in ("drn_d_22", "drn_d_54"):
        for _, r in step_rows(arch, *BENCH_SHAPE):
            out += [r + (0,), r + (1,)]
    return np.array(out, dtype=np.int64)


def args_of(row):
    """drnmi_wgrad_args of a row, with placeholder pointers (the plan queries read no data)."""
    import train_audit as A
    cin, cs, cout, dys, ks, s, p, d, n, h, w, _ = (int(v) for v in row)
    return A.wgrad_args(n, cin, cs, cout, dys, ks, s, p, d, h, w)


def digest(rows_):
    return hashlib.sha256(np.ascontiguousarray(rows_, dtype=np.int64).tobytes()).hexdigest()
