"""33 .. 256 segmentation classes (ADE20K has 150): the checks that need no GPU -- argument
validation of the C entry points before any launch, the generic palette, and the fake kernels'
shapes for a 150-class model."""
import ctypes

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

from drnmi import _lib, palette, torch_ops  # noqa: F401  (torch_ops registers the ops)
from drnmi.drnseg import DRNSeg

U8, I64 = _lib.DRNMI_U8, _lib.DRNMI_I64
OK, EINVAL, ENOTSUP = 0, -1, -2                   # drnmi_status (include/drnmi.h)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def dummy():
    buf = (ctypes.c_uint8 * 64)()                    # never dereferenced: every call returns before a launch
    return ctypes.addressof(buf)


@pytest.mark.parametrize("nclass", [33, 150, 256])
def test_confusion_matrix_accepts_up_to_256_classes(lib, dummy, nclass):
    # npix == 0 returns after the argument checks and before any launch
    assert lib.drnmi_confusion_matrix(dummy, U8, dummy, U8, 0, nclass, dummy, None) == OK


def test_confusion_matrix_refuses_257_classes(lib, dummy):
    assert lib.drnmi_confusion_matrix(dummy, U8, dummy, U8, 0, 257, dummy, None) == ENOTSUP
    assert lib.drnmi_confusion_matrix(dummy, U8, dummy, U8, 0, 0, dummy, None) == ENOTSUP
    assert lib.drnmi_confusion_matrix(None, U8, dummy, U8, 0, 150, dummy, None) == EINVAL


def test_wide_head_entry_validates(lib, dummy):
    f = lib.drnmi_up8_logsoftmax_argmax_wide
    assert f(None, dummy, dummy, dummy, U8, 1, 150, 4, 4, None) == EINVAL
    assert f(dummy, dummy, dummy, dummy, U8, 1, 257, 4, 4, None) == ENOTSUP
    assert f(dummy, dummy, dummy, dummy, U8, 1, 0, 4, 4, None) == ENOTSUP
    assert f(dummy, dummy, dummy, dummy, 99, 1, 150, 4, 4, None) == EINVAL
    # float4 log-prob stores and packed label stores: misaligned outputs are refused, not written
    assert f(dummy, dummy, dummy + 4, dummy, U8, 1, 150, 4, 4, None) == EINVAL
    assert f(dummy, dummy, dummy, dummy + 1, U8, 1, 150, 4, 4, None) == EINVAL
    assert f(dummy, dummy, dummy, dummy + 4, I64, 1, 150, 4, 4, None) == EINVAL


def test_head_entries_refuse_only_above_256(lib, dummy):
    assert lib.drnmi_up8_logsoftmax_argmax(dummy, dummy, dummy, dummy, U8, 1, 257, 4, 4, None) == ENOTSUP
    assert lib.drnmi_up8_bilinear_logsoftmax_argmax(dummy, dummy, dummy, U8, 1, 257, 4, 4, None) == ENOTSUP
    # 33 .. 256 passes the class check: the next refusal is the batch limit, EINVAL, not ENOTSUP
    for c in (33, 150, 256):
        assert lib.drnmi_up8_logsoftmax_argmax(dummy, dummy, dummy, dummy, U8, 70000, c, 4, 4, None) == EINVAL
        assert lib.drnmi_up8_bilinear_logsoftmax_argmax(dummy, dummy, dummy, U8, 70000, c, 4, 4, None) == EINVAL


def test_generic_palette():
    p = palette.palette_for(150)
    assert p.shape == (150, 3) and p.dtype == np.uint8
    assert tuple(p[0]) == (0, 0, 0)
    assert len(np.unique(p, axis=0)) == 150
    g = palette.generic_palette(256)
    assert g.shape == (256, 3) and g.dtype == np.uint8
    assert len(np.unique(g, axis=0)) == 256
    np.testing.assert_array_equal(g[:150], p)                     # deterministic, a prefix for fewer classes
    np.testing.assert_array_equal(g[[1, 2, 4, 8, 255]], [[128, 0, 0], [0, 128, 0], [0, 0, 128], [64, 0, 0],
                                                         [224, 224, 192]])
    assert "generic_palette" in palette.__all__
    for bad in (0, 257):
        with pytest.raises(ValueError):
            palette.generic_palette(bad)


def test_small_class_counts_keep_the_reference_tables():
    assert palette.palette_for(19) is palette.CITYSCAPE_PALETTE
    assert palette.palette_for(20) is palette.CITYSCAPE_PALETTE
    assert palette.palette_for(3) is palette.TRIPLET_PALETTE
    assert palette.palette_for(21).shape == (21, 3)


@pytest.mark.parametrize("h,w,oh,ow", [(72, 40, 72, 40), (97, 61, 104, 64)])
def test_fake_shapes_150_classes(h, w, oh, ow):
    m = DRNSeg("drn_d_22", 150, pretrained=False).eval()
    with FakeTensorMode():
        lab = torch.ops.drnmi.segment(torch.empty(2, h, w, 3, dtype=torch.uint8, device="cuda"), m._handle,
                                      [0.3, 0.3, 0.3], [0.2, 0.2, 0.2], False)
        lp, logits = torch.ops.drnmi.forward(torch.empty(2, 3, h, w, device="cuda"), m._handle)
        pred = torch.ops.drnmi.predict(torch.empty(2, 3, h, w, device="cuda"), m._handle)
        hl, hlp = torch.ops.drnmi.up8_logsoftmax_argmax(torch.empty(2, 150, oh // 8, ow // 8, device="cuda"),
                                                        torch.empty(16, 16, device="cuda"), True, True)
    assert lab.shape == (2, oh, ow) and lab.dtype == torch.uint8
    assert lp.shape == (2, 150, oh, ow) and logits.shape == (2, 150, oh // 8, ow // 8)
    assert pred.shape == (2, oh, ow) and pred.dtype == torch.int64
    assert hlp.shape == (2, 150, oh, ow) and hlp.dtype == torch.float32
    assert hl.shape == (2, oh, ow) and hl.dtype == torch.uint8
