"""The labels-only video head on NHWC logits for 1 .. 256 classes on the GPU: drnmi_up8_labels_nhwc_wide
(csrc/head_wide.hip up8_labels_wide_tile_kernel) and DRNSeg.segment() routed through it.

The reference in every kernel case is drnmi_up8_logsoftmax_argmax, labels only, on the NCHW copy of
the same values, compared with torch.equal: the labels are the same bits, not close ones.  The
padding columns c .. cs - 1 of the NHWC rows are NaN in every case.  Shapes are the smallest at
which borders, tile seams and partial tiles can go wrong: (1, 12, 37) is 13 x 38 windows, more than
one tile in each direction with a partial last tile in both for each of the kernel's tile shapes
(8 x 16 windows up to 32 classes, 4 x 16 up to 80, 4 x 8 above)."""
import ctypes
import functools

import pytest
import torch

from drnmi import _lib, drnseg, engine
from drnmi.drnseg import INFO_MEAN, INFO_STD
from drnmi.weights import bilinear_up_kernel, synth_frames
from oracle import drn_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
CLASS_COUNTS = [1, 2, 19, 20, 32, 33, 64, 65, 80, 81, 150, 255, 256]   # mask-word and tile-shape boundaries
SHAPES = [(1, 1, 1), (1, 1, 7), (1, 6, 1), (2, 9, 5), (1, 12, 37)]
DTYPES = [torch.uint8, torch.int64]


@functools.lru_cache(maxsize=None)
def _up_plane():
    return torch.from_numpy(bilinear_up_kernel(16)).float().contiguous().to(DEV)


def _code(dt):
    return _lib.DRNMI_I64 if dt == torch.int64 else _lib.DRNMI_U8


def _reference(logits, dt=torch.uint8):
    """Labels of drnmi_up8_logsoftmax_argmax without log-probs on NCHW device logits."""
    n, c, h, w = logits.shape
    lab = torch.empty(n, 8 * h, 8 * w, dtype=dt, device=DEV)
    _lib.check(_lib.load().drnmi_up8_logsoftmax_argmax(
        logits.data_ptr(), _up_plane().data_ptr(), None, lab.data_ptr(), _code(dt), n, c, h, w,
        ctypes.c_void_p(_lib.stream_ptr())), "nchw head")
    return lab


def _nhwc(logits, cs=None):
    n, c, h, w = logits.shape
    cs = cs or (c + 3) // 4 * 4
    rows = torch.full((n, h, w, cs), float("nan"), device=DEV)
    rows[..., :c] = logits.permute(0, 2, 3, 1)
    return rows, cs


def _wide(logits, dt=torch.uint8, cs=None, stats=False):
    """drnmi_up8_labels_nhwc_wide (stats: its counting twin, returns (labels, [fast windows, candidate
    pixels, fallback pixels])) on the NHWC form of NCHW device logits."""
    n, c, h, w = logits.shape
    rows, cs = _nhwc(logits, cs)
    lab = torch.empty(n, 8 * h, 8 * w, dtype=dt, device=DEV)
    st = ctypes.c_void_p(_lib.stream_ptr())
    lib = _lib.load()
    if not stats:
        _lib.check(lib.drnmi_up8_labels_nhwc_wide(rows.data_ptr(), cs, _up_plane().data_ptr(), lab.data_ptr(), _code(dt),
                                                  n, c, h, w, st), "wide nhwc head")
        return lab
    counts = torch.zeros(3, dtype=torch.int64, device=DEV)
    _lib.check(lib.drnmi_up8_labels_nhwc_wide_stats(rows.data_ptr(), cs, _up_plane().data_ptr(), lab.data_ptr(),
                                                    _code(dt), n, c, h, w, st, counts.data_ptr()), "wide nhwc head, stats")
    return lab, [int(v) for v in counts.cpu()]


def _check_counts(counts, logits):
    """Every pixel is counted exactly once: 64 per fast window, or as a candidate or a fallback pixel."""
    n, _, h, w = logits.shape
    assert counts[0] * 64 + counts[1] + counts[2] == n * 8 * h * 8 * w, counts


@functools.lru_cache(maxsize=None)
def _random_logits(c, shape):
    n, h, w = shape
    g = torch.Generator().manual_seed(1000 * c + 31 * h + w)
    return (torch.randn(n, c, h, w, generator=g) * 3.0).to(DEV)


@functools.lru_cache(maxsize=None)
def _blocky_logits(c, shape, block=4):
    """One class raised by 8 over block x block low-resolution pixels (block >= 3: windows whose four
    taps agree), the others randn."""
    n, h, w = shape
    g = torch.Generator().manual_seed(77 * c + h + w)
    x = torch.randn(n, c, h, w, generator=g)
    top = torch.randint(0, c, (n, (h + block - 1) // block, (w + block - 1) // block), generator=g)
    top = top.repeat_interleave(block, 1).repeat_interleave(block, 2)[:, :h, :w]
    x.scatter_add_(1, top.unsqueeze(1), torch.full((n, 1, h, w), 8.0))
    return x.to(DEV)


# ------------------------------------------------------------------ the kernel against the NCHW head
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("c", CLASS_COUNTS)
def test_random_logits_match_the_nchw_head(c, shape):
    """i.i.d. randn * 3: almost every window is slow (candidates, some fallbacks)."""
    logits = _random_logits(c, shape)
    for dt in DTYPES:
        ref = _reference(logits, dt)
        got = _wide(logits, dt)
        assert got.dtype == dt and torch.equal(got, ref)
        got_s, counts = _wide(logits, dt, stats=True)
        assert torch.equal(got_s, ref)               # the counting twin returns the same labels
        _check_counts(counts, logits)


@pytest.mark.parametrize("c,cs", [(64, 72), (150, 160), (19, 20), (1, 12)])
def test_wider_rows_and_nan_padding(c, cs):
    """Rows wider than round_up(c, 4): the padding columns (NaN here) are never read into a decision."""
    logits = _random_logits(c, (2, 9, 5))
    ref = _reference(logits)
    assert torch.equal(_wide(logits, cs=cs), ref)
    rows, _ = _nhwc(logits, cs)
    rows[..., c:] = float("inf")                     # nor is +inf
    lab = torch.empty_like(ref)
    _lib.check(_lib.load().drnmi_up8_labels_nhwc_wide(rows.data_ptr(), cs, _up_plane().data_ptr(), lab.data_ptr(),
                                                      _lib.DRNMI_U8, 2, c, 9, 5, ctypes.c_void_p(_lib.stream_ptr())),
               "wide nhwc head")
    assert torch.equal(lab, ref)


@pytest.mark.parametrize("shape", SHAPES)
def test_19_classes_match_the_19_class_kernels(shape):
    """c = 19: against the tiled 19-class kernel on the same NHWC rows (and, above, the oct kernel)."""
    n, h, w = shape
    for logits in (_random_logits(19, shape), _blocky_logits(19, shape)):
        rows, cs = _nhwc(logits)
        for dt in DTYPES:
            lab = torch.empty(n, 8 * h, 8 * w, dtype=dt, device=DEV)
            _lib.check(_lib.load().drnmi_up8_labels_nhwc(rows.data_ptr(), cs, _up_plane().data_ptr(), lab.data_ptr(),
                                                         _code(dt), n, 19, h, w, ctypes.c_void_p(_lib.stream_ptr())),
                       "19-class nhwc head")
            assert torch.equal(_wide(logits, dt), lab)
            assert torch.equal(lab, _reference(logits, dt))


@pytest.mark.parametrize("shape", [(2, 9, 5), (1, 12, 37)])
@pytest.mark.parametrize("c", [2, 19, 20, 32, 33, 64, 65, 150, 255, 256])
def test_blocky_maps_take_every_path(c, shape):
    """Blocks of one raised class: fast windows inside the blocks, candidate pixels on their seams."""
    logits = _blocky_logits(c, shape)
    for dt in DTYPES:
        ref = _reference(logits, dt)
        got, counts = _wide(logits, dt, stats=True)
        assert torch.equal(got, ref)
        assert torch.equal(_wide(logits, dt), ref)
        assert counts[0] > 0 and counts[1] > 0, counts
        _check_counts(counts, logits)


@pytest.mark.parametrize("c", [2, 33, 150, 256])
def test_exact_ties_give_the_lower_class(c):
    """Two classes identical everywhere and on top: the lower index, through the fallback."""
    shape = (1, 12, 37)
    lo, hi = (0, c - 1) if c != 150 else (41, 97)    # c = 2, 33, 256: class 0 against class c - 1
    logits = _random_logits(c, shape).clone()
    logits[:, lo] = logits[:, lo].abs() + 20.0
    logits[:, hi] = logits[:, lo]
    got, counts = _wide(logits, stats=True)
    assert torch.equal(got, _reference(logits))
    assert bool((got == lo).all())
    assert counts[2] > 0 and counts[0] == 0 and counts[1] == 0   # every pixel's top two are 0 apart
    _check_counts(counts, logits)


def test_near_tie_takes_the_lower_class():
    """test_wide_head_near_tie_takes_the_lower_class at 150 classes: two classes one ulp apart round to
    one log-prob (a quarter ulp of lse ~ log 2), so the lower index wins although its logit is lower."""
    c = 150
    logits = torch.full((1, c, 2, 2), -30.0)
    logits[:, 7] = 0.2
    logits[:, 31] = torch.nextafter(torch.tensor(0.2), torch.tensor(1.0))
    logits = logits.to(DEV)
    ref = _reference(logits)
    got, counts = _wide(logits, stats=True)
    assert torch.equal(got, ref)
    # the one interior window's 64 pixels have their top two within 2^-26: none is decided over the
    # candidates; the 192 border pixels take the full path anyway
    assert counts[2] > 0 and counts == [0, 0, 256]
    centre = got[0, 4:12, 4:12]                  # all four taps valid: weights sum to 1
    assert bool(((centre == 7) | (centre == 31)).all()) and bool((centre == 7).any())


@pytest.mark.parametrize("c", [20, 150])
@pytest.mark.parametrize("kind", ["random", "blocky"])
def test_a_class_at_minus_infinity(c, kind):
    """-inf everywhere (every window takes the full path) and in part of the image (the windows that
    touch it do; a clamped -inf tap under a zero weight gives the reference's NaN row)."""
    shape = (1, 12, 37)
    base = _random_logits(c, shape) if kind == "random" else _blocky_logits(c, shape)
    everywhere = base.clone()
    everywhere[:, 3] = float("-inf")
    got, counts = _wide(everywhere, stats=True)
    assert torch.equal(got, _reference(everywhere))
    assert counts[0] == 0 and counts[1] == 0
    _check_counts(counts, everywhere)
    partly = base.clone()
    partly[:, 3, :5, :20] = float("-inf")
    partly[:, c - 1, 8:, 30:] = float("-inf")
    got, counts = _wide(partly, stats=True)
    assert torch.equal(got, _reference(partly))
    assert counts[1] > 0 and counts[2] > 0
    _check_counts(counts, partly)


@pytest.mark.parametrize("c", [20, 150, 256])
def test_huge_magnitudes(c):
    """Logits of +-1e30 mixed with ordinary ones."""
    shape = (1, 12, 37)
    logits = _blocky_logits(c, shape).clone()
    g = torch.Generator().manual_seed(5 + c)
    big = torch.rand(logits.shape, generator=g).to(DEV)
    logits[big < 0.02] = 1e30
    logits[big > 0.98] = -1e30
    logits[:, :, 6:, 20:] = _blocky_logits(c, shape)[:, :, 6:, 20:]      # and a quiet corner
    got, counts = _wide(logits, stats=True)
    assert torch.equal(got, _reference(logits))
    assert torch.equal(_wide(logits, torch.int64), _reference(logits, torch.int64))
    _check_counts(counts, logits)


def test_against_the_cpu_oracle():
    """oracle/drn_oracle.py's head in float64 on the CPU, wherever its top-2 margin exceeds 1e-4.  On
    this seed the oracle leaves 0 of the 5760 pixels out (cap: 1e-3 of them)."""
    c, shape = 150, (2, 9, 5)
    logits = _random_logits(c, shape)
    upw = torch.from_numpy(bilinear_up_kernel(16)).double().expand(c, 1, 16, 16).contiguous()
    ref = O.up_logsoftmax({"up.weight": upw}, logits.cpu().double())
    srt = ref.sort(dim=1).values
    margin = srt[:, -1] - srt[:, -2]
    excluded = int((margin <= 1e-4).sum())
    print(f"oracle pixels with a float64 top-2 margin <= 1e-4: {excluded} of {margin.numel()}")
    assert excluded <= 1e-3 * margin.numel()
    got = _wide(logits, torch.int64).cpu()
    assert not bool(((got != O.labels_of(ref)) & (margin > 1e-4)).any())


# ------------------------------------------------------------------ DRNSeg.segment(), 150 classes
CLASSES = 150


@pytest.fixture(scope="module")
def model():
    m = drnseg.build("drn_d_22", CLASSES, seed=4, device=torch.device(DEV), precision="bf16")
    frames = torch.from_numpy(synth_frames(4, 2, 72, 40)).to(DEV)
    return m, frames


def _both_paths(m, frames, **kw):
    """segment() with the NHWC labels path off (the reference route) and on."""
    old = engine.LABELS_NHWC
    try:
        engine.LABELS_NHWC = False
        ref = m.segment(frames, INFO_MEAN, INFO_STD, False, **kw)
        ref = tuple(t.clone() for t in ref) if isinstance(ref, tuple) else ref.clone()
        engine.LABELS_NHWC = True
        got = m.segment(frames, INFO_MEAN, INFO_STD, False, **kw)
    finally:
        engine.LABELS_NHWC = old
    return ref, got


def test_segment_bf16_150_classes_takes_the_nhwc_path(model):
    m, frames = model
    m.set_precision("bf16")
    ref, got = _both_paths(m, frames)
    plan = m.plan(2, 72, 40)
    assert plan.labels_path() == "nhwc" and plan.seg_fused is None
    assert plan.labels_path(use_torch_up=True) == "nchw"
    assert got.dtype == torch.uint8 and got.shape == (2, 72, 40)
    assert torch.equal(got, ref) and len(got.unique()) > 1
    for dt in DTYPES:
        buf = torch.full((2, 72, 40), 99, dtype=dt, device=DEV)
        ref_b, got_b = _both_paths(m, frames, labels=buf)
        assert got_b is buf and torch.equal(got_b.long(), ref.long()) and torch.equal(ref_b.long(), ref.long())
    (lab_r, img_r), (lab, img) = _both_paths(m, frames, render="color")
    assert torch.equal(lab, ref) and torch.equal(lab_r, ref) and torch.equal(img, img_r)
    old = engine.LABELS_NHWC
    try:
        engine.LABELS_NHWC = False
        assert plan.labels_path() == "nchw"
    finally:
        engine.LABELS_NHWC = old


def test_segment_int8_150_classes(model):
    """The int8 seg conv (512 -> 150) runs on the int8 tile, which writes the NHWC rows."""
    m, frames = model
    m.set_precision("bf16").calibrate_int8(frames)
    m.set_precision("int8")
    try:
        ref, got = _both_paths(m, frames)
        path = m.plan(2, 72, 40).labels_path()
    finally:
        m.set_precision("bf16")
    assert path == "nhwc"
    assert torch.equal(got, ref) and len(got.unique()) > 1


@pytest.mark.parametrize("precision", ["fp32", "fp32x"])
def test_fp32_plans_keep_the_logits_planes(model, precision):
    m, frames = model
    m.set_precision(precision)
    try:
        path = m.plan(2, 72, 40).labels_path()
        ref, got = _both_paths(m, frames)
    finally:
        m.set_precision("bf16")
    assert path == "nchw" and torch.equal(got, ref)


def test_segment_bf16_21_classes():
    m = drnseg.build("drn_d_22", 21, seed=6, device=torch.device(DEV), precision="bf16")
    frames = torch.from_numpy(synth_frames(6, 2, 72, 40)).to(DEV)
    ref, got = _both_paths(m, frames)
    assert m.plan(2, 72, 40).labels_path() == "nhwc"
    assert torch.equal(got, ref) and len(got.unique()) > 1


def test_segment_graph_capture_150_classes(model):
    m, _ = model
    m.set_precision("bf16")
    frames = torch.from_numpy(synth_frames(4, 1, 72, 40)).to(DEV)
    assert m.plan(1, 72, 40).labels_path() == "nhwc"
    mean, std = [0.29, 0.33, 0.29], [0.18, 0.19, 0.18]

    def step():
        return torch.ops.drnmi.segment(frames, m._handle, mean, std, False)

    s = torch.cuda.Stream()                      # warm-up off the capture: packing, plan buffers
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for seed in (4, 11):
        frames.copy_(torch.from_numpy(synth_frames(seed, 1, 72, 40)).to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured, step())
    assert len(captured.unique()) > 1
