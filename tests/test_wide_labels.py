"""The labels-only video head on NHWC logits for 1 .. 256 classes (drnmi_up8_labels_nhwc_wide and its
counting twin, csrc/head_wide.hip up8_labels_wide_tile_kernel): the checks that need no GPU -- the
symbols and their bindings, and the refusals the entry points make before any HIP call."""
import ctypes

import pytest

from drnmi import _lib

U8, I64 = _lib.DRNMI_U8, _lib.DRNMI_I64
OK, EINVAL, ENOTSUP = 0, -1, -2                   # drnmi_status (include/drnmi.h)
ENTRIES = ("drnmi_up8_labels_nhwc_wide", "drnmi_up8_labels_nhwc_wide_stats")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def dummy():
    buf = (ctypes.c_uint8 * 96)()                    # never dereferenced: every call returns before a launch
    return (ctypes.addressof(buf) + 15) & ~15        # 16-byte aligned


def _call(lib, entry, logits, cs, up_w, labels, dtype, n, c, h, w, stats):
    f = getattr(lib, entry)
    if entry.endswith("_stats"):
        return f(logits, cs, up_w, labels, dtype, n, c, h, w, None, stats)
    return f(logits, cs, up_w, labels, dtype, n, c, h, w, None)


def test_symbols_exist_and_are_bound(lib):
    for entry in ENTRIES:
        assert entry in _lib.SIGNATURES
        assert getattr(lib, entry).restype is ctypes.c_int
    assert len(_lib.SIGNATURES["drnmi_up8_labels_nhwc_wide"][1]) == 10
    assert len(_lib.SIGNATURES["drnmi_up8_labels_nhwc_wide_stats"][1]) == 11


@pytest.mark.parametrize("entry", ENTRIES)
def test_refusals_before_any_hip_call(lib, dummy, entry):
    d = dummy

    def f(logits=d, cs=152, up_w=d, labels=d, dtype=U8, n=1, c=150, h=4, w=4, stats=d):
        return _call(lib, entry, logits, cs, up_w, labels, dtype, n, c, h, w, stats)

    assert f(c=0, cs=4) == ENOTSUP
    assert f(c=257, cs=260) == ENOTSUP
    assert f(c=-3, cs=4) == ENOTSUP
    assert f(cs=148) == EINVAL                       # cs < c
    assert f(cs=149) == EINVAL
    assert f(cs=154) == EINVAL                       # cs % 4 != 0
    assert f(dtype=99) == EINVAL
    assert f(logits=None) == EINVAL
    assert f(up_w=None) == EINVAL
    assert f(labels=None) == EINVAL
    for zero in ("n", "h", "w"):
        assert f(**{zero: 0}) == EINVAL
        assert f(**{zero: -1}) == EINVAL
    assert f(logits=d + 4) == EINVAL                 # float4 row reads
    assert f(logits=d + 8) == EINVAL
    assert f(labels=d + 1) == EINVAL                 # packed 4-label stores
    assert f(labels=d + 2) == EINVAL
    assert f(labels=d + 4, dtype=I64) == EINVAL
    assert f(n=70000) == EINVAL                      # grid.z
    assert f(h=70000) == EINVAL                      # grid.y
    if entry.endswith("_stats"):
        assert f(stats=None) == EINVAL
        assert f(stats=d + 4) == EINVAL


def test_the_19_class_entry_is_unchanged(lib, dummy):
    f = lib.drnmi_up8_labels_nhwc
    assert f(dummy, 24, dummy, dummy, U8, 1, 21, 4, 4, None) == ENOTSUP
    assert f(dummy, 20, dummy, dummy, U8, 1, 20, 4, 4, None) == ENOTSUP
    assert f(dummy, 18, dummy, dummy, U8, 1, 19, 4, 4, None) == EINVAL
