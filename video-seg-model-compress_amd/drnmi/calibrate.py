"""int8 activation scales from an exact |x| histogram (host side, numpy fp64, no GPU).

drnmi_abs_histogram (include/drnmi.h, csrc/quant.hip) counts a bf16 activation buffer into
HIST_BINS = 32768 bins, one per representable bf16 magnitude: bin b holds the elements whose
|x| has the bf16 bit pattern b.  Bins from 0x7f80 up are inf / NaN.  The histogram of a bf16
tensor is its exact distribution of |x|, so every statistic below is exact, over any number
of batches accumulated into the same counters.

  bin_values()                                   the 32768 magnitudes as float64
  scale_from_histogram(hist, method, percentile) "absmax" | "percentile" | "mse" -> scale
  quant_sse(hist, scale)                         sum of squared int8 round-trip errors

The quantiser modelled here is the engine's own (quantize_kernel in csrc/quant.hip, the conv
epilogues): q = clamp(rint(float32(x) * float32(1 / scale)), -127, 127), one fp32 multiply,
round-half-even; the dequantised value is scale * q.
"""
from __future__ import annotations

import math

import numpy as np

HIST_BINS = 32768            # include/drnmi.h DRNMI_HIST_BINS
FIRST_NONFINITE_BIN = 0x7f80
METHODS = ("absmax", "percentile", "mse")
MSE_OCTAVES = 4              # "mse" searches clip values down to absmax / 2^4

_BIN_VALUES = None


def bin_values() -> np.ndarray:
    """float64 [32768]: bin b's magnitude, the value of the bf16 bit pattern b (inf / NaN from
    0x7f80 up).  A copy: callers may write to it."""
    global _BIN_VALUES
    if _BIN_VALUES is None:
        bits = np.arange(HIST_BINS, dtype=np.uint32) << np.uint32(16)
        with np.errstate(invalid="ignore"):           # (the NaN bins)
            _BIN_VALUES = bits.view(np.float32).astype(np.float64)
    return _BIN_VALUES.copy()


def _counts(hist) -> np.ndarray:
    h = np.asarray(hist)
    if h.shape != (HIST_BINS,):
        raise ValueError(f"histogram must have shape ({HIST_BINS},), got {h.shape}")
    if h.dtype.kind not in "iu":
        raise ValueError("histogram counters must be integers")
    if h.dtype.kind == "i" and (h < 0).any():
        raise ValueError("negative histogram counter")
    return h.astype(np.int64, copy=False)


def _absmax_value(h: np.ndarray) -> float:
    nz = np.flatnonzero(h[:FIRST_NONFINITE_BIN])
    return float(bin_values()[nz[-1]]) if nz.size else 0.0


def _round_trip_sq_err(v: np.ndarray, scale: float) -> np.ndarray:
    """(v - scale * q(v))^2 in fp64 for magnitudes v (float64, exactly bf16), q as the engine."""
    inv = np.float32(1.0 / scale)
    q = np.clip(np.rint(v.astype(np.float32) * inv), np.float32(-127.0), np.float32(127.0)).astype(np.float64)
    e = v - scale * q
    return e * e


def quant_sse(hist, scale: float) -> float:
    """sum_b hist[b] * (v_b - scale * q(v_b))^2 over the finite bins: the squared error of
    quantising the histogrammed tensor to int8 at `scale` and back."""
    scale = float(scale)
    if not (math.isfinite(scale) and scale > 0.0):
        raise ValueError("scale must be finite and positive")
    h = _counts(hist)[:FIRST_NONFINITE_BIN]
    nz = np.flatnonzero(h)
    if nz.size == 0:
        return 0.0
    v = bin_values()[nz]
    return float(np.sum(_round_trip_sq_err(v, scale) * h[nz].astype(np.float64)))


def scale_from_histogram(hist, method: str = "absmax", percentile: float = 99.99) -> float:
    """Per-tensor symmetric int8 scale (dequantised value = scale * q) from an |x| histogram.

    "absmax":     the largest finite magnitude present / 127 (on a bf16 tensor exactly
                  drnmi_absmax / 127); 1.0 for an all-zero tensor.
    "percentile": v / 127 for the smallest magnitude v with at least ceil(percentile / 100 * N)
                  of the N finite elements (zeros included) at or below it; 1.0 if v == 0.
    "mse":        the clip value v among the magnitudes present in [absmax / 16, absmax] whose
                  scale v / 127 has the smallest quant_sse; ties go to the larger clip.
    Only finite bins are used; "percentile" and "mse" refuse a histogram that counted inf / NaN."""
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}, got {method!r}")
    h = _counts(hist)
    if method != "absmax" and h[FIRST_NONFINITE_BIN:].any():
        raise ValueError(f"{int(h[FIRST_NONFINITE_BIN:].sum())} inf/NaN activations in the histogram: "
                         f"no {method} scale")
    amax = _absmax_value(h)
    if method == "absmax":
        return amax / 127.0 if amax > 0.0 else 1.0
    h = h[:FIRST_NONFINITE_BIN]
    vals = bin_values()[:FIRST_NONFINITE_BIN]
    if method == "percentile":
        p = float(percentile)
        if not 0.0 <= p <= 100.0:
            raise ValueError("percentile must be in [0, 100]")
        total = int(h.sum())
        need = min(math.ceil(p / 100.0 * total), total)
        v = float(vals[int(np.searchsorted(np.cumsum(h), need, side="left"))]) if total else 0.0
        return v / 127.0 if v > 0.0 else 1.0
    if amax == 0.0:
        return 1.0
    nz = np.flatnonzero(h)
    v = vals[nz]
    cnt = h[nz].astype(np.float64)
    cands = v[v >= amax / 2.0 ** MSE_OCTAVES]         # ascending; absmax is the last
    best_cost, best_v = None, None
    for c in cands:
        cost = float(np.sum(_round_trip_sq_err(v, float(c) / 127.0) * cnt))
        if best_cost is None or cost <= best_cost:    # <=: a tie goes to the larger clip
            best_cost, best_v = cost, float(c)
    return best_v / 127.0


__all__ = ["HIST_BINS", "METHODS", "bin_values", "scale_from_histogram", "quant_sse"]
