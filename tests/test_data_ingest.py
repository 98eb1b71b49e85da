"""Fine-tune data path, host side (no GPU): the restatement of the reference's RandomCrop /
pad_reflection / RandomHorizontalFlip in drnmi.data against tensors the reference produced
(tests/golden/ingest.npz, made by tests/golden/make_ingest_golden.py), the C-ABI's argument checks
and the fake kernel of torch.ops.drnmi.train_ingest."""
import ctypes
import random

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

from drnmi import _lib, torch_ops  # noqa: F401  (registers the ops)
from drnmi.data import TrainIngest, draw_params, extend_1d, index_maps

import ingest_ref

CASES, MEAN, STD = ingest_ref.load_cases()
IDS = [f"{c['name']}-seed{c['seed']}" for c in CASES]


def _pads(size, target):
    lead = (target - size) // 2 if size < target else 0
    return lead, (target - size - lead if size < target else 0)


def test_fixture_has_the_cases():
    names = {c["name"] for c in CASES}
    assert names == {"a", "b", "c", "d", "e", "f", "g7", "g3"}
    assert {c["params"][2] for c in CASES} == {True, False}
    assert sorted(c["params"][2] for c in CASES if c["name"] == "a") == [False, True]


def test_extend_1d_examples():
    assert extend_1d(4, 2, 3) == [2, 1, 0, 1, 2, 3, 3, 2, 1]
    assert extend_1d(3, 4, 5) == [0, 1, 2, 1, 0, 1, 2, 2, 1, 1, 2, 2]
    assert extend_1d(5, 0, 0) == [0, 1, 2, 3, 4]
    assert extend_1d(1, 0, 0) == [0]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_extend_1d_matches_reference_padding(case):
    """The reference's pad_reflection of an index image is the outer combination of the two 1-D maps."""
    h, w = case["lab"].shape
    tw, th = case["crop"]
    rows = np.asarray(extend_1d(h, *_pads(h, th)))
    cols = np.asarray(extend_1d(w, *_pads(w, tw)))
    assert np.array_equal(case["padidx"], rows[:, None] * w + cols[None, :])


@pytest.mark.parametrize("n,lo,hi", [(1, 1, 0), (1, 0, 2), (1, 3, 3)])
def test_extend_1d_length_one_raises(n, lo, hi):
    with pytest.raises(ValueError):
        extend_1d(n, lo, hi)
    with pytest.raises(ValueError):
        index_maps(1, 4, (4, 3), 0, 0, False)          # h = 1 padded to th = 3


class _CountingRng:
    """Delegates to a random.Random (a subclass that overrides random() would change how
    randint draws) and records the calls."""

    def __init__(self, seed):
        self.rng = random.Random(seed)
        self.calls = []

    def randint(self, a, b):
        self.calls.append("randint")
        return self.rng.randint(a, b)

    def random(self):
        self.calls.append("random")
        return self.rng.random()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_draw_params_reproduces_reference_draws(case):
    h, w = case["lab"].shape
    rng = _CountingRng(case["seed"])
    assert draw_params(w, h, case["crop"], True, rng) == case["params"]
    tw, th = case["crop"]
    no_crop_draw = w <= tw and h <= th                    # the padded size equals the crop (b, d, f)
    assert no_crop_draw == (case["name"] in ("b", "d", "f"))
    assert rng.calls == (["random"] if no_crop_draw else ["randint", "randint", "random"])
    # the module-level generator is the default source, as in the reference
    random.seed(case["seed"])
    assert draw_params(w, h, case["crop"]) == case["params"]
    # flip=False (the validation list) draws nothing for the flip
    rng = _CountingRng(case["seed"])
    x1, y1, fl = draw_params(w, h, case["crop"], False, rng)
    assert (x1, y1, fl) == (case["params"][0], case["params"][1], False) and "random" not in rng.calls


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_ingest_ref_equals_reference_tensors(case):
    """numpy gather through index_maps + fp32 normalise == the reference's tensors, bit for bit."""
    h, w = case["lab"].shape
    rowmap, colmap = index_maps(h, w, case["crop"], *case["params"])
    assert rowmap.dtype == np.int32 and colmap.dtype == np.int32
    assert rowmap.shape == (case["crop"][1],) and colmap.shape == (case["crop"][0],)
    out, tgt = ingest_ref.ingest_ref(case["img"], case["lab"], rowmap, colmap, MEAN, STD)
    assert out.dtype == np.float32 and out.shape == case["out"].shape
    assert np.array_equal(out.view(np.uint32), case["out"].view(np.uint32))
    assert tgt.dtype == np.int64 and np.array_equal(tgt, case["tgt"])
    out2, tgt2 = ingest_ref.ingest_ref(case["img"], None, rowmap, colmap, MEAN, STD)
    assert tgt2 is None and np.array_equal(out2, out)


def test_normalise_is_totensor_then_normalize_on_every_byte():
    """The fp32 sequence of ingest_ref on all 256 byte values and 3 channels equals
    img.float().div(255) followed by sub_(m).div_(s) (data_transforms.py:249, :120-121)."""
    img = np.stack([np.arange(256, dtype=np.uint8).reshape(16, 16)] * 3, axis=-1)
    out, _ = ingest_ref.ingest_ref(img, None, np.arange(16, dtype=np.int32), np.arange(16, dtype=np.int32), MEAN, STD)
    t = torch.from_numpy(img).permute(2, 0, 1).contiguous().float().div(255)
    for c, m, s in zip(t, torch.FloatTensor(MEAN), torch.FloatTensor(STD)):
        c.sub_(m).div_(s)
    assert np.array_equal(out.view(np.uint32), t.numpy().view(np.uint32))


def test_index_map_encoding():
    rowmap, colmap = index_maps(3, 4, (13, 12), 0, 0, False)
    assert colmap.tolist() == [~v for v in extend_1d(4, 4, 5)[:4]] + [0, 1, 2, 3] + [~v for v in extend_1d(4, 4, 5)[8:]]
    assert (rowmap[:4] < 0).all() and (rowmap[4:7] == [0, 1, 2]).all() and (rowmap[7:] < 0).all()
    _, flipped = index_maps(3, 4, (13, 12), 0, 0, True)
    assert flipped.tolist() == colmap.tolist()[::-1]
    with pytest.raises(ValueError):
        index_maps(10, 12, (8, 6), 5, 0, False)           # x1 beyond W - tw


def test_tables_layout():
    ing = TrainIngest((8, 6), rng=random.Random(3))
    tab, params = ing.tables([(10, 12), (9, 20)])
    assert tab.dtype == np.int32 and tab.shape == (2 * (6 + 8),) and len(params) == 2
    chk = random.Random(3)
    assert params == [draw_params(12, 10, (8, 6), True, chk), draw_params(20, 9, (8, 6), True, chk)]
    r1, c1 = index_maps(9, 20, (8, 6), *params[1])
    assert np.array_equal(tab[6:12], r1) and np.array_equal(tab[12 + 8:], c1)
    with pytest.raises(ValueError):
        ing.tables([(10, 12)], params=[(0, 0, False), (0, 0, False)])


def test_cpu_tensors_raise():
    ing = TrainIngest((8, 6))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ing(torch.zeros(1, 10, 12, 3, dtype=torch.uint8), torch.zeros(1, 10, 12, dtype=torch.uint8))
    with pytest.raises(NotImplementedError):              # no CPU kernel registered for the raw op
        torch.ops.drnmi.train_ingest(torch.zeros(1, 10, 12, 3, dtype=torch.uint8), None,
                                     torch.zeros(1, 6, dtype=torch.int32), torch.zeros(1, 8, dtype=torch.int32),
                                     list(MEAN), list(STD))
    from drnmi.train import accuracy
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        accuracy(torch.zeros(1, 19, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64))


def test_fake_kernel_shapes():
    with FakeTensorMode():
        img = torch.empty(3, 40, 48, 3, dtype=torch.uint8, device="cuda")
        lab = torch.empty(3, 40, 48, dtype=torch.uint8, device="cuda")
        rm = torch.empty(3, 17, dtype=torch.int32, device="cuda")
        cm = torch.empty(3, 23, dtype=torch.int32, device="cuda")
        x, t = torch.ops.drnmi.train_ingest(img, lab, rm, cm, list(MEAN), list(STD))
        x2, t2 = torch.ops.drnmi.train_ingest(img, None, rm, cm, list(MEAN), list(STD))
    assert x.shape == (3, 3, 17, 23) and x.dtype == torch.float32
    assert t.shape == (3, 17, 23) and t.dtype == torch.int64
    assert x2.shape == (3, 3, 17, 23) and t2.numel() == 0 and t2.dtype == torch.int64


# ---------------------------------------------------------------- C-ABI argument checks, no device
_F3 = ctypes.c_float * 3
_M, _S = _F3(*MEAN), _F3(*STD)
_GOOD = dict(images=0x10000, labels=0x20000, n=1, h=4, w=4, rowmap=0x30000, colmap=0x40000, th=2, tw=2,
             mean=_M, std=_S, out=0x50000, target=0x60000)


def _ingest(**kw):
    a = dict(_GOOD, **kw)
    return _lib.load().drnmi_train_ingest_u8(a["images"], a["labels"], a["n"], a["h"], a["w"], a["rowmap"], a["colmap"],
                                             a["th"], a["tw"], a["mean"], a["std"], a["out"], a["target"], None)


@pytest.mark.parametrize("bad", [
    dict(images=None), dict(rowmap=None), dict(colmap=None), dict(out=None), dict(mean=None), dict(std=None),
    dict(labels=None), dict(target=None),                      # labels and target go together
    dict(n=0), dict(h=0), dict(w=0), dict(th=0), dict(tw=0), dict(n=-1), dict(h=-3), dict(tw=-2),
    dict(out=0x50008), dict(out=0x50004), dict(target=0x60004), dict(target=0x60001),
    dict(n=1025, h=1 << 15, w=1 << 15),                         # n * h * w above 2^40
    dict(n=1025, th=1 << 15, tw=1 << 15),                       # n * th * tw above 2^40
    dict(h=(1 << 31) - 1, w=(1 << 31) - 1),
], ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_train_ingest_einval_without_gpu(bad):
    assert _ingest(**bad) == -1


@pytest.mark.parametrize("args", [
    (None, 0x2000, 1, 19, 16, 255, 0x3000), (0x1000, None, 1, 19, 16, 255, 0x3000),
    (0x1000, 0x2000, 1, 19, 16, 255, None), (0x1000, 0x2000, 0, 19, 16, 255, 0x3000),
    (0x1000, 0x2000, 1, 0, 16, 255, 0x3000), (0x1000, 0x2000, 1, 19, 0, 255, 0x3000),
    (0x1000, 0x2000, -1, 19, 16, 255, 0x3000), (0x1000, 0x2000, 1, -19, 16, 255, 0x3000),
    (0x1000, 0x2000, 1, 19, -16, 255, 0x3000),
])
def test_pixel_accuracy_einval_without_gpu(args):
    assert _lib.load().drnmi_pixel_accuracy_f32(*args, None) == -1
