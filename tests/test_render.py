"""Rendering of label maps (drnmi.palette, drnmi_render_labels, torch.ops.drnmi.render_labels /
segment_render): the CPU-only checks -- palette data against the recorded fixture, argument
validation before any HIP call, the fake kernels' shapes, and the blend contract itself."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import render_ref as R
from conftest import GOLDEN
from drnmi import _lib, palette, torch_ops  # noqa: F401  (torch_ops registers the ops)
from drnmi.drnseg import DRNSeg


def test_palettes_equal_the_recorded_fixture():
    with open(os.path.join(GOLDEN, "palettes.json")) as f:
        rec = json.load(f)
    for name, shape in (("CITYSCAPE_PALETTE", (20, 3)), ("TRIPLET_PALETTE", (3, 4))):
        ours = getattr(palette, name)
        assert ours.dtype == np.uint8 and ours.shape == shape
        assert np.array_equal(ours, np.asarray(rec[name], dtype=np.uint8)), name
    assert palette.palette_for(3) is palette.TRIPLET_PALETTE
    assert palette.palette_for(19) is palette.CITYSCAPE_PALETTE


def test_as_device_palette_shapes():
    p = palette.as_device_palette(palette.CITYSCAPE_PALETTE, "cpu")
    assert p.dtype == torch.uint8 and tuple(p.shape) == (20, 3) and p.is_contiguous()
    assert np.array_equal(p.numpy(), palette.CITYSCAPE_PALETTE)
    t = palette.as_device_palette(palette.TRIPLET_PALETTE, "cpu")          # the alpha column is dropped
    assert tuple(t.shape) == (3, 3) and t.is_contiguous()
    assert np.array_equal(t.numpy(), palette.TRIPLET_PALETTE[:, :3])
    assert palette.as_device_palette(palette.TRIPLET_PALETTE, "cpu") is t  # host tables upload once
    lst = palette.as_device_palette([[1, 2, 3], [4, 5, 6]], "cpu")
    assert lst.tolist() == [[1, 2, 3], [4, 5, 6]]
    ten = torch.arange(12, dtype=torch.int64).reshape(3, 4)
    assert palette.as_device_palette(ten, "cpu").tolist() == [[0, 1, 2], [4, 5, 6], [8, 9, 10]]
    ready = torch.zeros(256, 3, dtype=torch.uint8)
    assert palette.as_device_palette(ready, "cpu").data_ptr() == ready.data_ptr()   # already in device form: no copy
    for bad in (np.zeros((20,), np.uint8), np.zeros((20, 2), np.uint8), np.zeros((0, 3), np.uint8),
                np.zeros((257, 3), np.uint8), np.zeros((2, 3), np.float32), [[0, 0, 256]], [[-1, 0, 0]],
                torch.zeros(2, 3)):
        with pytest.raises(ValueError):
            palette.as_device_palette(bad, "cpu")


def test_render_labels_argument_validation_without_gpu():
    """Every rejected argument returns DRNMI_EINVAL before any HIP call (safe with no device)."""
    lib = _lib.load()
    U8, I64 = _lib.DRNMI_U8, _lib.DRNMI_I64
    p = 0x1000                                    # never dereferenced: all of these fail validation

    def call(labels=p, dtype=U8, n=1, lh=8, lw=8, frames=p, pal=p, P=20, a=154, swap=0, out=p, oh=8, ow=8):
        return lib.drnmi_render_labels(labels, dtype, n, lh, lw, frames, pal, P, a, swap, out, oh, ow, None)

    assert call(labels=None) == -1
    assert call(pal=None) == -1
    assert call(out=None) == -1
    for dtype in (_lib.DRNMI_F32, _lib.DRNMI_BF16, _lib.DRNMI_I8, -1, 6):
        assert call(dtype=dtype) == -1
    for P in (0, -1, 257):
        assert call(P=P) == -1
    assert call(oh=9) == -1 and call(ow=9) == -1                      # output outside the label map
    for kw in ({"n": 0}, {"n": -1}, {"lh": 0}, {"lw": 0}, {"oh": 0}, {"ow": 0}, {"oh": -1}, {"ow": -3}):
        assert call(**kw) == -1, kw
    for a in (-1, 257, 1 << 20):
        assert call(a=a) == -1
    # n * lh * lw beyond what the 64-bit offsets are bounded to (2^40 elements), int64 labels too
    big = 2 ** 31 - 1
    assert call(n=big, lh=big, lw=big, oh=1, ow=1) == -1
    assert call(n=2, lh=1 << 20, lw=1 << 20, oh=1, ow=1) == -1
    assert call(dtype=I64, n=1 << 11, lh=1 << 15, lw=1 << 15, oh=1, ow=1) == -1


def test_ops_registered():
    assert hasattr(torch.ops.drnmi, "render_labels") and hasattr(torch.ops.drnmi, "segment_render")


@pytest.mark.parametrize("h,w,lh,lw", [(60, 100, 64, 104), (64, 96, 64, 96), (300, 300, 304, 304)])
def test_fake_kernels_give_the_documented_shapes(h, w, lh, lw):
    m = DRNSeg("drn_d_22", 19, pretrained=False).eval()
    with FakeTensorMode():
        frames = torch.empty(2, h, w, 3, dtype=torch.uint8, device="cuda")
        pal = torch.empty(20, 3, dtype=torch.uint8, device="cuda")
        for overlay in (False, True):
            lab, img = torch.ops.drnmi.segment_render(frames, m._handle, [0.3, 0.3, 0.3], [0.2, 0.2, 0.2], False,
                                                      pal, 154, overlay)
            assert tuple(lab.shape) == (2, lh, lw) and lab.dtype == torch.uint8
            assert tuple(img.shape) == (2, h, w, 3) and img.dtype == torch.uint8
        for dtype in (torch.uint8, torch.int64):
            labels = torch.empty(2, lh, lw, dtype=dtype, device="cuda")
            col = torch.ops.drnmi.render_labels(labels, pal, None, 0, False, lh, lw)
            ov = torch.ops.drnmi.render_labels(labels, pal, frames, 154, True, h, w)
            assert tuple(col.shape) == (2, lh, lw, 3) and col.dtype == torch.uint8
            assert tuple(ov.shape) == (2, h, w, 3) and ov.dtype == torch.uint8


def test_cpu_tensors_have_no_kernel():
    with pytest.raises(NotImplementedError):
        torch.ops.drnmi.render_labels(torch.zeros(1, 8, 8, dtype=torch.uint8), torch.zeros(20, 3, dtype=torch.uint8),
                                      None, 0, False, 8, 8)
    from drnmi import ops
    with pytest.raises(ValueError):
        ops.render_labels(torch.zeros(1, 8, 8, dtype=torch.uint8))
    m = DRNSeg("drn_d_22", 19, pretrained=False).eval()
    with pytest.raises(ValueError, match="render must be"):
        m.segment(torch.zeros(1, 64, 64, 3, dtype=torch.uint8), render="rgba")


def test_blend_contract_endpoints():
    """alpha = 0 returns the frame and alpha = 1 the colour, for all 256 x 256 value pairs."""
    f, c = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    assert R.alpha_q8(0.0) == 0 and R.alpha_q8(1.0) == 256 and R.alpha_q8(0.6) == 154
    assert np.array_equal(R.blend(f, c, R.alpha_q8(0.0)), f)
    assert np.array_equal(R.blend(f, c, R.alpha_q8(1.0)), c)
    mid = R.blend(f, c, 128).astype(np.int64)                       # a half blend rounds half up
    assert np.array_equal(mid, (f.astype(np.int64) + c + 1) >> 1)


def test_render_ref_clamp_crop_and_swap():
    pal = palette.CITYSCAPE_PALETTE
    lab = np.array([[[0, 19, 200], [255, 18, 1]]], dtype=np.uint8)
    img = R.render_ref(lab, pal)
    assert img.shape == (1, 2, 3, 3)
    assert np.array_equal(img[0, 0, 1], pal[19]) and np.array_equal(img[0, 0, 2], pal[19])
    assert np.array_equal(img[0, 1, 0], pal[19]) and np.array_equal(img[0, 1, 1], pal[18])
    assert np.array_equal(R.render_ref(lab, pal, out_hw=(1, 2)), img[:, :1, :2])
    assert np.array_equal(R.render_ref(lab, pal, bgr=True), img[..., ::-1])
    frames = np.full((1, 1, 2, 3), 100, np.uint8)
    ov = R.render_ref(lab, pal, frames, alpha=0.6)
    assert ov.shape == (1, 1, 2, 3)
    assert ov[0, 0, 0].tolist() == [(100 * 102 + int(v) * 154 + 128) >> 8 for v in pal[0]]
    assert np.array_equal(R.render_ref(lab, palette.TRIPLET_PALETTE)[0, 0], palette.TRIPLET_PALETTE[[0, 2, 2], :3])
