"""Fine-tune data path on the GPU (csrc/ingest.hip): drnmi_train_ingest_u8 through TrainIngest and
torch.ops.drnmi.train_ingest against the reference's tensors (tests/golden/ingest.npz) and the numpy
restatement tests/ingest_ref.py, bit for bit; drnmi_pixel_accuracy_f32 / drnmi.train.accuracy
against torch on the same device; drnmi.evaluate.validate against the same loop written out."""
import functools
import math
import random

import numpy as np
import pytest
import torch

import ingest_ref
from drnmi import _lib, torch_ops  # noqa: F401  (registers torch.ops.drnmi.*)
from drnmi.data import TrainIngest, draw_params, index_maps

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES, MEAN, STD = ingest_ref.load_cases()
IDS = [f"{c['name']}-seed{c['seed']}" for c in CASES]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(inp, tgt, want_out, want_tgt):
    got = inp.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == want_out.shape
    assert np.array_equal(_bits(got), _bits(want_out))
    if want_tgt is None:
        assert tgt is None
    else:
        assert tgt.dtype == torch.int64 and np.array_equal(tgt.cpu().numpy(), want_tgt)


# ---------------------------------------------------------------- fixture cases
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fixture_cases_bit_identical(case):
    """TrainIngest with the seed's draws (the module-level generator, as the reference) gives the
    reference's tensors."""
    img = torch.from_numpy(case["img"]).to(DEV)[None]
    lab = torch.from_numpy(case["lab"]).to(DEV)[None]
    random.seed(case["seed"])
    inp, tgt = TrainIngest(case["crop"], MEAN, STD)(img, lab)
    _same(inp[0], tgt[0], case["out"], case["tgt"])
    inp2, tgt2 = TrainIngest(case["crop"], MEAN, STD)(img, lab, params=[case["params"]])
    assert torch.equal(inp, inp2) and torch.equal(tgt, tgt2)


def test_every_byte_value():
    """All 256 byte values in each channel, identity tables: the kernel's division, subtraction,
    division equals ingest_ref (which the CPU tests pin against ToTensor + Normalize)."""
    img = np.stack([np.arange(256, dtype=np.uint8).reshape(16, 16)] * 3, axis=-1)
    ident = np.arange(16, dtype=np.int32)
    want, _ = ingest_ref.ingest_ref(img, None, ident, ident, MEAN, STD)
    inp, tgt = TrainIngest(16, MEAN, STD)(torch.from_numpy(img).to(DEV)[None], None, params=[(0, 0, False)])
    _same(inp[0], tgt, want, None)


# ---------------------------------------------------------------- random cases
@functools.lru_cache(maxsize=None)
def _random_case(k):
    """n, images, labels, crop, params and the ingest_ref tensors of seeded case k (shared)."""
    rng = np.random.default_rng(1000 + k)
    n = 1 + k % 3
    h, w = int(rng.integers(2, 41)), int(rng.integers(2, 49))
    tw, th = int(rng.integers(1, 57)), int(rng.integers(1, 49))
    if k % 2 == 0:
        tw = max(4, tw // 4 * 4)                 # the 16-byte store path; odd k: mostly the scalar one
    img = rng.integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)
    lab = rng.integers(0, 256, size=(n, h, w), dtype=np.uint8)
    draws = random.Random(k)
    params = [draw_params(w, h, (tw, th), True, draws) for _ in range(n)]
    outs, tgts = [], []
    for i in range(n):
        r, c = index_maps(h, w, (tw, th), *params[i])
        o, t = ingest_ref.ingest_ref(img[i], lab[i], r, c, MEAN, STD)
        outs.append(o)
        tgts.append(t)
    return img, lab, (tw, th), params, np.stack(outs), np.stack(tgts)


@pytest.mark.parametrize("k", range(20))
def test_random_cases_bit_identical(k):
    img, lab, crop, params, want_out, want_tgt = _random_case(k)
    inp, tgt = TrainIngest(crop, MEAN, STD)(torch.from_numpy(img).to(DEV), torch.from_numpy(lab).to(DEV), params=params)
    _same(inp, tgt, want_out, want_tgt)


def test_draws_follow_the_generator():
    """Without params the batch's draws are draw_params from the given generator, in batch order."""
    img, lab, crop, _, _, _ = _random_case(2)
    n, h, w = lab.shape
    chk = random.Random(77)
    params = [draw_params(w, h, crop, True, chk) for _ in range(n)]
    a = TrainIngest(crop, MEAN, STD, rng=random.Random(77))(torch.from_numpy(img).to(DEV), torch.from_numpy(lab).to(DEV))
    b = TrainIngest(crop, MEAN, STD)(torch.from_numpy(img).to(DEV), torch.from_numpy(lab).to(DEV), params=params)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_list_of_differently_sized_images():
    rng = np.random.default_rng(5)
    sizes = [(10, 12), (40, 48), (7, 31), (2, 2)]
    for crop in [(16, 9), (7, 5)]:              # th * tw = 144: aligned slices; 35: slices off the 16-byte grid
        imgs = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in sizes]
        labs = [rng.integers(0, 256, size=(h, w), dtype=np.uint8) for h, w in sizes]
        draws = random.Random(9)
        params = [draw_params(w, h, crop, True, draws) for h, w in sizes]
        inp, tgt = TrainIngest(crop, MEAN, STD)([torch.from_numpy(a).to(DEV) for a in imgs],
                                                [torch.from_numpy(a).to(DEV) for a in labs], params=params)
        assert inp.shape == (4, 3, crop[1], crop[0]) and tgt.shape == (4, crop[1], crop[0])
        for i, (h, w) in enumerate(sizes):
            o, t = ingest_ref.ingest_ref(imgs[i], labs[i], *index_maps(h, w, crop, *params[i]), MEAN, STD)
            _same(inp[i], tgt[i], o, t)


def test_labels_none():
    img, _, crop, params, want_out, _ = _random_case(4)
    inp, tgt = TrainIngest(crop, MEAN, STD)(torch.from_numpy(img).to(DEV), None, params=params)
    _same(inp, tgt, want_out, None)
    lst, tgt = TrainIngest(crop, MEAN, STD)([torch.from_numpy(a).to(DEV) for a in img], None, params=params)
    _same(lst, tgt, want_out, None)


@pytest.mark.parametrize("crop", [(16, 11), (13, 11)])
def test_flipped_next_to_unflipped(crop):
    rng = np.random.default_rng(6)
    img = rng.integers(0, 256, size=(2, 20, 30, 3), dtype=np.uint8)
    lab = rng.integers(0, 256, size=(2, 20, 30), dtype=np.uint8)
    params = [(3, 2, True), (3, 2, False)]
    inp, tgt = TrainIngest(crop, MEAN, STD)(torch.from_numpy(img).to(DEV), torch.from_numpy(lab).to(DEV), params=params)
    for i in range(2):
        o, t = ingest_ref.ingest_ref(img[i], lab[i], *index_maps(20, 30, crop, *params[i]), MEAN, STD)
        _same(inp[i], tgt[i], o, t)
    # the same source in both samples: the flipped one is the mirror image
    two = torch.from_numpy(np.stack([img[0], img[0]])).to(DEV)
    inp, _ = TrainIngest(crop, MEAN, STD)(two, None, params=params)
    assert torch.equal(inp[0], inp[1].flip(-1))


@pytest.mark.parametrize("crop", [(16, 9), (7, 5)])
def test_nothing_outside_the_outputs_is_written(crop):
    tw, th = crop
    img, lab = _random_case(1)[:2]
    n, h, w = lab.shape
    params = [(0, 0, i % 2 == 1) for i in range(n)]
    tabs = [index_maps(h, w, crop, *p) for p in params]
    rm = torch.from_numpy(np.stack([t[0] for t in tabs])).to(DEV)
    cm = torch.from_numpy(np.stack([t[1] for t in tabs])).to(DEV)
    guard = 64
    obuf = torch.full((guard + n * 3 * th * tw + guard,), -7.0, dtype=torch.float32, device=DEV)
    tbuf = torch.full((guard + n * th * tw + guard,), -7, dtype=torch.int64, device=DEV)
    out = obuf[guard:guard + n * 3 * th * tw].view(n, 3, th, tw)
    tgt = tbuf[guard:guard + n * th * tw].view(n, th, tw)
    torch_ops.train_ingest_into(torch.from_numpy(img).to(DEV), torch.from_numpy(lab).to(DEV), rm, cm, list(MEAN),
                                list(STD), out, tgt)
    for i in range(n):
        o, t = ingest_ref.ingest_ref(img[i], lab[i], *tabs[i], MEAN, STD)
        _same(out[i], tgt[i], o, t)
    for buf, size in ((obuf, n * 3 * th * tw), (tbuf, n * th * tw)):
        assert (buf[:guard] == -7).all() and (buf[guard + size:] == -7).all()


# ---------------------------------------------------------------- clamping
def test_out_of_range_tables_are_clamped():
    """The clamp's contract: any table content reads inside the images; the output is ingest_ref on
    the clamped table."""
    rng = np.random.default_rng(8)
    n, h, w, th, tw = 2, 9, 11, 6, 8
    img = rng.integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)
    lab = rng.integers(0, 256, size=(n, h, w), dtype=np.uint8)
    big = np.array([h + 5, 10 ** 6, 2 ** 31 - 1, ~(h + 100), ~(10 ** 6), -2 ** 31], dtype=np.int64)
    rm = np.stack([np.resize(big, th), np.resize(big[::-1], th)]).astype(np.int32)
    bigc = np.array([w, w + 7, 10 ** 9, 2 ** 31 - 1, ~w, ~(10 ** 9), -2 ** 31, ~(w + 1)], dtype=np.int64)
    cm = np.stack([np.resize(bigc, tw), np.resize(bigc[::-1], tw)]).astype(np.int32)
    for t, size in ((rm, h), (cm, w)):
        assert ((np.where(t < 0, ~t, t)) >= size).all()          # every entry is out of range
    inp, tgt = torch.ops.drnmi.train_ingest(torch.from_numpy(img).to(DEV), torch.from_numpy(lab).to(DEV),
                                            torch.from_numpy(rm).to(DEV), torch.from_numpy(cm).to(DEV),
                                            list(MEAN), list(STD))
    torch.cuda.synchronize()
    for i in range(n):
        o, t = ingest_ref.ingest_ref(img[i], lab[i], rm[i], cm[i], MEAN, STD)
        _same(inp[i], tgt[i], o, t)


# ---------------------------------------------------------------- graph capture
def test_graph_capture_replays_with_new_tables():
    img, lab, crop, params, want_out, want_tgt = _random_case(8)
    n, h, w = lab.shape
    tw, th = crop

    def tables(ps):
        tabs = [index_maps(h, w, crop, *p) for p in ps]
        return (torch.from_numpy(np.stack([t[0] for t in tabs])).to(DEV),
                torch.from_numpy(np.stack([t[1] for t in tabs])).to(DEV))

    dimg, dlab = torch.from_numpy(img).to(DEV), torch.from_numpy(lab).to(DEV)
    rm, cm = tables(params)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        torch.ops.drnmi.train_ingest(dimg, dlab, rm, cm, list(MEAN), list(STD))
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        inp, tgt = torch.ops.drnmi.train_ingest(dimg, dlab, rm, cm, list(MEAN), list(STD))
    g.replay()
    _same(inp, tgt, want_out, want_tgt)
    draws = random.Random(123)
    new = [draw_params(w, h, crop, True, draws) for _ in range(n)]
    assert new != params
    rm2, cm2 = tables(new)
    rm.copy_(rm2)
    cm.copy_(cm2)
    g.replay()
    for i in range(n):
        o, t = ingest_ref.ingest_ref(img[i], lab[i], *index_maps(h, w, crop, *new[i]), MEAN, STD)
        _same(inp[i], tgt[i], o, t)


# ---------------------------------------------------------------- pixel accuracy
ACC_SHAPES = [(2, 19, 111), (1, 1, 5), (3, 150, 1000), (2, 19, 64)]       # the last: every target 255


@functools.lru_cache(maxsize=None)
def _acc_case(shape):
    n, c, hw = shape
    g = torch.Generator().manual_seed(n * 100000 + c * 1000 + hw)
    lp = torch.randn(n, c, hw, generator=g)                               # continuous: no ties
    arg = lp.argmax(1)
    tgt = torch.where(torch.rand(n, hw, generator=g) < 0.5, arg, torch.randint(0, c, (n, hw), generator=g))
    u = torch.rand(n, hw, generator=g)
    tgt = torch.where(u < 0.2, torch.full_like(tgt, 255), tgt)
    tgt = torch.where((u >= 0.2) & (u < 0.25), torch.full_like(tgt, c + 3), tgt)     # out of range: counted, never right
    tgt = torch.where((u >= 0.25) & (u < 0.3), torch.full_like(tgt, -1), tgt)
    if shape == ACC_SHAPES[-1]:
        tgt = torch.full_like(tgt, 255)
    return lp.to(DEV), tgt.to(DEV)


def _ref_accuracy(output, target):
    """utils.accuracy (utils.py:267-277), restated."""
    _, pred = output.max(1)
    pred = pred.view(1, -1)
    target = target.view(1, -1)
    correct = pred.eq(target)
    correct = correct[target != 255]
    correct = correct.view(-1)
    return correct.float().sum(0).mul(100.0 / correct.size(0))


@pytest.mark.parametrize("shape", ACC_SHAPES, ids=str)
def test_pixel_accuracy_counts(shape):
    n, c, hw = shape
    lp, tgt = _acc_case(shape)
    valid = tgt != 255
    want = [int(valid.sum()), int(((lp.argmax(1) == tgt) & valid).sum())]
    counts = torch.zeros(2, dtype=torch.int64, device=DEV)
    lib = _lib.load()
    for rep in (1, 2):                                                     # accumulates, never cleared
        _lib.check(lib.drnmi_pixel_accuracy_f32(lp.data_ptr(), tgt.data_ptr(), n, c, hw, 255, counts.data_ptr(),
                                                _lib.stream_ptr(lp.device)), "pixel_accuracy")
        assert counts.tolist() == [rep * want[0], rep * want[1]]
    if shape != ACC_SHAPES[-1]:
        assert 0 < want[1] < want[0] < n * hw or c == 1


@pytest.mark.parametrize("shape", ACC_SHAPES, ids=str)
def test_accuracy_score(shape):
    from drnmi.train import accuracy
    lp, tgt = _acc_case(shape)
    got = accuracy(lp, tgt)
    assert got.dtype == torch.float32 and got.dim() == 0 and got.is_cuda
    if shape == ACC_SHAPES[-1]:
        assert math.isnan(float(got))
        return
    want = float(_ref_accuracy(lp, tgt))
    print(f"accuracy {shape}: got {float(got)!r} want {want!r}")
    assert abs(float(got) - want) <= 1.6e-5                                # two fp32 ulps at 100
    n, c, hw = shape
    if hw % 3 == 0:                                                        # [n, c, h, w] scores, [n, h, w] targets
        got4 = accuracy(lp.view(n, c, 3, hw // 3), tgt.view(n, 3, hw // 3))
        assert float(got4) == float(got)


# ---------------------------------------------------------------- validate
class _Writer:
    def __init__(self):
        self.scalars = []

    def add_scalar(self, tag, value, step):
        self.scalars.append((tag, value, step))


def test_validate_matches_written_out_loop():
    from drnmi.drnseg import build
    from drnmi.evaluate import validate
    from drnmi.train import CrossEntropyLoss, accuracy
    model = build("drn_d_22", 19, seed=0, device=torch.device(DEV, 0), precision="fp32")
    criterion = CrossEntropyLoss(ignore_index=255)
    g = torch.Generator().manual_seed(3)
    loader = []
    for _ in range(2):
        x = torch.randn(2, 3, 32, 64, generator=g)
        t = torch.randint(0, 19, (2, 32, 64), generator=g)
        t[torch.rand(2, 32, 64, generator=g) < 0.1] = 255
        loader.append((x, t))

    model.eval()
    loss_sum, score_sum, count = 0.0, torch.zeros((), device=DEV), 0
    with torch.no_grad():
        for x, t in loader:
            out = model(x.to(DEV))[0]
            tv = t.to(DEV).long()
            loss_sum += criterion(out, tv).item() * x.size(0)
            score_sum += accuracy(out, tv) * x.size(0)
            count += x.size(0)
    want_loss, want_score = loss_sum / count, float(score_sum / count)

    w = _Writer()
    got = validate(loader, model, criterion, 4, w, None, eval_score=accuracy, print_freq=1)
    assert w.scalars == [("Loss/Eval", want_loss, 4)]                     # same kernels, same weighting: equal
    assert abs(got - want_score) <= 1.6e-5 and 0.0 <= got <= 100.0
    w2 = _Writer()
    assert validate(loader, model, criterion, writer=w2) == 0             # no eval_score
    assert w2.scalars == [("Loss/Eval", want_loss, 0)]
    assert not model.training
