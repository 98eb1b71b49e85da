"""The deterministic grid of drnmi_conv_args behind tests/test_conv_routes.py and
tests/golden/make_route_golden.py: a pure function of nothing (no randomness, no library call).

grid() returns (args, entry): a numpy record array with the layout of drnmi_conv_args and, per
row, 0 for drnmi_conv2d_bn_act / drnmi_conv_kernel_name or 1 for the seg-fused entry
(drnmi_conv_stag_seg / drnmi_conv_stag_seg_kernel_name).  The four data pointers x, wgt, shift, y
hold the placeholder PTR (nothing dereferences them: no row is ever launched by the test).

The grid is a concatenation of full products over small value sets ("cores": every tile id over
clean shapes, the auto route over every shape) and of lattice samples of much larger products
(every optional operand, output layout and padding convention against every shape): row i of a
lattice takes the mixed-radix digits of (i * STEP) mod N, STEP a prime, which visits distinct
rows of the product and spreads over all pairs of dimensions.
"""
import hashlib
import itertools

import numpy as np

from drnmi import _lib

ARGS = np.dtype(_lib.ConvArgs)
PTR = 0x1000                 # placeholder for a present, 16-B aligned operand
STEP = 2654435761            # prime: coprime with every product of small dimension sizes
F32, BF16, I8, F32X3, F8 = _lib.DRNMI_F32, _lib.DRNMI_BF16, _lib.DRNMI_I8, _lib.DRNMI_F32X3, _lib.DRNMI_F8
DATA_POINTERS = ("x", "wgt", "shift", "y")

# (x2 channels, k_pad convention): k_pad == k, or k rounded up to whole 64-column weight steps
X2K = [(0, 0), (0, 1), (32, 0), (32, 1), (64, 0), (64, 1)]
# (ws, ws_bytes): none, a workspace, a misaligned one, one too small for any split
WS = [(0, 0), (PTR, 1 << 40), (PTR + 8, 1 << 40), (PTR, 16)]
DEFAULTS = dict(dtype=BF16, algo=0, ks=3, cin=64, cout=64, stride=1, dil=1, wo=16, x2k=0, res=0, scale=0, mask=0,
                ws=0, stats=0, ysr=0, out=0, cpad=128, tile=-1, src_u8=0, pad0=0, seg=0, odt=-1)


def product(**dims):
    """Every combination of the given values (a dict of equally long int64 arrays)."""
    keys = list(dims)
    cols = np.array(list(itertools.product(*[range(len(dims[k])) for k in keys])), dtype=np.int64)
    return {k: np.asarray(dims[k], dtype=np.int64)[cols[:, i]] for i, k in enumerate(keys)}


def lattice(rows, **dims):
    """`rows` distinct combinations of the given values, spread over their whole product."""
    keys = list(dims)
    total = int(np.prod([len(dims[k]) for k in keys], dtype=object))
    assert rows <= total
    idx = [(i * STEP) % total for i in range(rows)]
    out = {}
    for k in reversed(keys):
        n = len(dims[k])
        out[k] = np.asarray(dims[k], dtype=np.int64)[np.array([j % n for j in idx])]
        idx = [j // n for j in idx]
    return out


def build(d):
    """drnmi_conv_args records of the rows described by `d` (missing keys: DEFAULTS)."""
    n = len(next(iter(d.values())))
    g = {k: np.asarray(d[k], dtype=np.int64) if k in d else np.full(n, v, dtype=np.int64) for k, v in DEFAULTS.items()}
    a = np.zeros(n, dtype=ARGS)
    ks, cin, cout, stride, dil, wo = g["ks"], g["cin"], g["cout"], g["stride"], g["dil"], g["wo"]
    ho = np.full(n, 2, dtype=np.int64)
    pad = np.where(g["pad0"] != 0, 0, dil * (ks - 1) // 2)
    x2 = np.array([X2K[i][0] for i in g["x2k"]])
    kpad64 = np.array([X2K[i][1] for i in g["x2k"]])
    for f in DATA_POINTERS:
        a[f] = PTR
    a["n"], a["ho"], a["wo"] = 1, ho, wo
    a["h"] = (ho - 1) * stride + dil * (ks - 1) + 1 - 2 * pad
    a["w"] = (wo - 1) * stride + dil * (ks - 1) + 1 - 2 * pad
    a["cin"], a["cout"], a["ks"], a["stride"], a["pad"], a["dil"] = cin, cout, ks, stride, pad, dil
    a["cout_pad"] = (cout + g["cpad"] - 1) // g["cpad"] * g["cpad"]
    k = np.where(g["src_u8"] != 0, 224, ks * ks * cin + x2)     # the uint8 stem's k = kh*32 + kw*4 + c
    a["k"] = k
    a["k_pad"] = np.where(kpad64 != 0, (k + 63) // 64 * 64, k)
    a["relu"], a["dtype"], a["tile"], a["algo"], a["src_u8"] = 1, g["dtype"], g["tile"], g["algo"], g["src_u8"]
    a["res_scale"], a["out_scale"] = 1.0, 1.0
    a["scale"], a["res"], a["unit_mask"] = g["scale"] * PTR, g["res"] * PTR, g["mask"] * PTR
    a["x2"] = np.where(x2 != 0, PTR, 0)
    a["cin2"], a["h2"], a["w2"], a["stride2"] = x2, np.where(x2 != 0, 2 * ho, 0), np.where(x2 != 0, 2 * wo, 0), \
        np.where(x2 != 0, 2, 0)
    a["ws"] = np.array([WS[i][0] for i in g["ws"]])
    a["ws_bytes"] = np.array([WS[i][1] for i in g["ws"]])
    a["stats"] = g["stats"]
    # output: 0 dense NHWC in the net's own type, 1 NCHW fp32, 2 NHWC rows padded to whole float4s
    # (odt >= 0: that out_dtype whatever the layout)
    native = np.select([g["dtype"] == BF16, g["dtype"] == I8, g["dtype"] == F8], [BF16, I8, F8], F32)
    out = g["out"]
    row = np.where(out == 2, (cout + 4) // 4 * 4, cout)
    a["out_dtype"] = np.where(g["odt"] >= 0, g["odt"], np.where(out == 1, F32, native))
    a["y_sp"] = np.where(out == 1, 1, row)
    a["y_sc"] = np.where(out == 1, ho * wo, 1)
    a["y_sn"] = np.where(out == 1, cout * ho * wo, row * ho * wo)
    # a row-strided class launch of a stride-2 data gradient: every other pixel of every other row
    ysr = g["ysr"] != 0
    a["y_sp"] = np.where(ysr, 2 * cout, a["y_sp"])
    a["y_sr"] = np.where(ysr, 4 * wo * cout, 0)
    a["y_sn"] = np.where(ysr, 4 * wo * cout * ho, a["y_sn"])
    return a, g["seg"].astype(np.uint8)


def _parts():
    sd = [(1, 1), (2, 1), (1, 2), (1, 4)]                      # (stride, dil)

    def with_sd(d, key="sd"):
        pairs = np.array(sd)[d.pop(key)]
        d["stride"], d["dil"] = pairs[:, 0], pairs[:, 1]
        return d
    # auto route, every shape, clean operands
    yield with_sd(product(dtype=[F32, BF16, I8, F32X3], ks=[1, 2, 3, 7], cin=[8, 16, 32, 64, 128, 256, 512],
                          cout=[16, 19, 32, 64, 128, 150, 256, 512], sd=[0, 1, 2, 3], wo=[16, 256],
                          x2k=[0, 4], scale=[0, 1]))
    # auto route, every optional operand / layout / padding convention
    yield with_sd(lattice(24900, dtype=[F32, BF16, I8, F32X3], ks=[1, 3, 3, 1, 2, 7],
                          cin=[8, 16, 32, 64, 64, 128, 128, 256, 512], cout=[16, 19, 32, 64, 128, 150, 256, 512],
                          sd=[0, 0, 1, 2, 3], wo=[16, 128, 256], x2k=[0, 0, 1, 2, 3, 4, 5], res=[0, 1], scale=[0, 1],
                          mask=[0, 0, 1], ws=[0, 1, 2, 3], stats=[0, 0, PTR, PTR + 4], ysr=[0, 0, 0, 1],
                          out=[0, 0, 1, 2], cpad=[128, 128, 256, 16]))
    # every LDS-DMA tile id over the bf16 / int8 shapes
    for scale, res in ((0, 0), (1, 0), (0, 1)):
        yield with_sd(product(tile=list(range(4, 26)), dtype=[BF16, I8], ks=[1, 3], cin=[32, 64, 128, 512],
                              cout=[19, 128, 256], sd=[0, 1, 2], wo=[16, 256], x2k=[0, 3, 4], scale=[scale],
                              res=[res]))
    # the 64-channel row-walk / halo kernels, auto and forced
    yield product(tile=[-1, 17, 20, 21], cin=[32, 64], cout=[64, 128], stride=[1, 2], x2k=[0, 2, 3, 4, 5],
                  scale=[0, 1], res=[0, 1], wo=[16])
    # every tile id against the optional operands
    yield with_sd(lattice(10000, tile=list(range(0, 26)), dtype=[F32, BF16, BF16, I8, F32X3], ks=[1, 3, 3, 7],
                          cin=[32, 64, 128, 256, 512], cout=[19, 64, 128, 256, 512], sd=[0, 0, 1, 2, 3],
                          wo=[16, 128, 256], x2k=[0, 0, 1, 2, 3, 4, 5], res=[0, 1], scale=[0, 1], mask=[0, 1],
                          ws=[0, 1], stats=[0, 0, PTR], out=[0, 0, 1, 2], cpad=[128, 256, 16]))
    # the register-staged tiles 0..3
    yield product(tile=[0, 1, 2, 3], dtype=[F32, BF16, I8, F32X3], ks=[1, 2, 3, 7], cin=[8, 32, 128],
                  cout=[16, 19, 64, 150], stride=[1, 2], x2k=[0, 1, 4], cpad=[128, 16])
    # fp32x: variants, forced splits (tile / 6 partitions of variant tile % 6), workspaces, statistics
    yield lattice(8000, dtype=[F32X3], tile=[-1, -1, 0, 1, 2, 3, 4, 5, 9, 13, 16, 24], ks=[1, 2, 3],
                  cin=[32, 128, 512], cout=[19, 64, 128, 256, 512], stride=[1, 2], wo=[16, 256], ws=[0, 1, 2, 3],
                  stats=[0, PTR, PTR + 4], ysr=[0, 0, 1], res=[0, 1], out=[0, 0, 2])
    # the LDS-patch kernels
    for cin, cout, ks, stride in ((4, 16, 7, 1), (8, 16, 7, 1), (16, 16, 3, 1), (16, 32, 3, 2), (32, 64, 3, 2),
                                  (64, 64, 3, 1)):
        yield product(algo=[1], dtype=[F32, BF16, I8, F32X3], src_u8=[0, 1], cin=[cin], cout=[cout], ks=[ks],
                      stride=[stride], wo=[16, 128], x2k=[0, 1, 4], res=[0, 1], out=[0, 1], pad0=[0, 1])
    # the seg-fused entry, on the 256- / 512-channel rows
    yield with_sd(product(seg=[1], dtype=[F32, BF16, I8], tile=[-1, 19, 22], ks=[1, 3], cin=[256, 512],
                          cout=[256, 512], sd=[0, 1, 2, 3], wo=[16, 256], x2k=[0, 4], scale=[0, 1],
                          res=[0, 1], out=[0, 1]))


def _parts_f8():
    """DRNMI_F8 over the axes the int8 rows above use, plus every out_dtype (I8: refusals)."""
    sd = np.array([(1, 1), (2, 1), (1, 2), (1, 4)])

    def with_sd(d):
        pairs = sd[d.pop("sd")]
        d["stride"], d["dil"] = pairs[:, 0], pairs[:, 1]
        return d
    # auto route, every shape (cin: non-powers of two are refusals), clean operands
    yield with_sd(product(dtype=[F8], ks=[1, 2, 3, 7], cin=[8, 16, 32, 64, 96, 128, 192, 256, 512],
                          cout=[16, 19, 32, 64, 128, 130, 150, 256, 512], sd=[0, 1, 2, 3], wo=[16, 256],
                          scale=[0, 1]))
    # every tile id and auto over the shapes fp8 runs
    yield with_sd(product(dtype=[F8], tile=[-1] + list(range(0, 26)), ks=[1, 3], cin=[64, 128, 256, 512],
                          cout=[19, 128, 130, 256, 512], sd=[0, 2], wo=[16, 256], scale=[1], res=[0, 1]))
    # every tile id against every optional operand, out_dtype, layout and padding convention
    yield with_sd(lattice(12000, dtype=[F8], tile=[-1, -1, -1] + list(range(0, 26)), ks=[1, 3, 3, 7],
                          cin=[32, 64, 128, 192, 256, 512], cout=[19, 64, 128, 130, 256, 512], sd=[0, 0, 1, 2, 3],
                          wo=[16, 128, 256], x2k=[0, 0, 0, 1, 2, 4], res=[0, 1], scale=[0, 1, 1], mask=[0, 0, 1],
                          odt=[F32, BF16, F8, F8, I8], out=[0, 0, 1, 2], cpad=[128, 256, 16]))
    # the seg-fused entry (no fp8 form: refusals)
    yield with_sd(product(seg=[1], dtype=[F8], tile=[-1, 19, 22], ks=[1, 3], cin=[256, 512], cout=[256, 512],
                          sd=[0, 1, 2, 3], wo=[16, 256], scale=[0, 1], res=[0, 1], out=[0, 1]))


def grid(parts=_parts):
    parts = [build(d) for d in parts()]
    # into zeroed memory: np.concatenate copies field by field and leaves the record's four padding
    # bytes as it finds them, and digest() reads them
    args = np.zeros(sum(len(p[0]) for p in parts), dtype=ARGS)
    np.concatenate([p[0] for p in parts], out=args)
    return args, np.concatenate([p[1] for p in parts])


def grid_f8():
    return grid(_parts_f8)


def digest(args, entry):
    return hashlib.sha256(args.tobytes() + entry.tobytes()).hexdigest()
