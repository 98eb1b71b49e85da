"""The 2:4 sparse conv, byte for byte: tests/golden/sp24_bytes.json holds the sha256 of the output of
each launch below as the commit before conv_big_body moved to its header and the launchers onto
launch_lds wrote it on an MI355X (tests/golden/make_sp24_bytes_golden.py).  The kernels have no atomics and every sum has a fixed
order, and the operands come from NumPy RandomState seeds, so the bytes are reproducible.

The cases are tests/test_gpu_sp24.py::CASES with the real-valued operands of _operands(case,
integer=False), each into both output layouts (fp32 NCHW planes; bf16 NHWC, whose NaN guard tail
_launch checks) on the per-tap gather and, where _strip(case) holds, on the forced strip-staged form.
What is hashed is what _launch hands back: every output element, in NHWC order."""
import hashlib
import json
import os

import pytest
import torch

import test_gpu_sp24 as S

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sp24_bytes.json")


def _name(case):
    return "x".join(str(int(v)) for v in case)


CASES = {_name(c): c for c in S.CASES}
assert len(CASES) == len(S.CASES)


def forms(case):
    """(key, out, tile) of every launch recorded for a case."""
    f = [("f32", "f32", -1), ("bf16", "bf16", -1)]
    if S._strip(case):
        strip = S._lib()[0].SP24_STRIP
        f += [("f32_strip", "f32", strip), ("bf16_strip", "bf16", strip)]
    return f


def digest(t):
    t = t.contiguous()
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    return hashlib.sha256(t.numpy().tobytes()).hexdigest()


def run_case(name):
    """{form: sha256 of the output} of CASES[name]; every element finite (a skipped store leaves NaN)."""
    case = CASES[name]
    x, wt, shift, res = S._operands(case, integer=False)
    _, blob, viol = S._pack(wt, S._geom(case)[3])
    assert viol == 0
    out = {}
    for key, layout, tile in forms(case):
        y = S._launch(case, x, blob, shift, res, layout, tile=tile)
        assert bool(torch.isfinite(y.float()).all()), f"{name} {key}: non-finite output element"
        out[key] = digest(y)
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_cases_are_the_recorded_ones(golden):
    assert set(golden) == set(CASES)
    for name, rec in golden.items():
        want = {"f32", "bf16"} | ({"f32_strip", "bf16_strip"} if S._strip(CASES[name]) else set())
        assert set(rec) == want, name
        if S._strip(CASES[name]):        # the strip form adds in the gather's order: the same bytes
            assert rec["f32_strip"] == rec["f32"] and rec["bf16_strip"] == rec["bf16"], name


@pytest.mark.parametrize("name", sorted(CASES))
def test_sp24_bytes(name, golden):
    assert run_case(name) == golden[name]
