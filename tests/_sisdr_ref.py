"""fp64 numpy restatement of include/cse_sisdr.h: SI-SDR, SI-SIR and SI-SAR of
one cell.  Test infrastructure only; it shares no code with the device.

The header leaves one freedom, the order of the fp64 sums.  `order` picks one:
"fsum" (math.fsum of the rounded products: the correctly rounded sum, what the
tests compare the device with), "sequential", "reversed", "blocks" (sums of 64
consecutive products, then a pairwise tree over the block sums) and "pairwise"
(numpy's own sum).  tools/sisdr_tolerance.py measures how far they lie apart.
"""

import math

import numpy as np

ORDERS = ("fsum", "sequential", "reversed", "blocks", "pairwise")
NAMES = ("sisdr", "sisir", "sisar")


def test_signal(y, length, lag=0, clip=False):
    """The cell's test signal as cse_stoi_cells defines it: f32 y[n - lag], zero
    outside [0, length), clipped to [-1, 1] when clip, widened to f64."""
    y = np.asarray(y, dtype=np.float32)[:length]
    if clip:
        y = np.clip(y, np.float32(-1.0), np.float32(1.0))
    out = np.zeros(length, dtype=np.float64)
    lag = int(lag)
    lo, hi = max(0, lag), min(length, length + lag)
    if hi > lo:
        out[lo:hi] = y[lo - lag:hi - lag].astype(np.float64)
    return out


test_signal.__test__ = False  # a helper, not a test


def _tree(x):
    x = list(x)
    while len(x) > 1:
        x = [x[i] + x[i + 1] if i + 1 < len(x) else x[i] for i in range(0, len(x), 2)]
    return x[0] if x else np.float64(0.0)


def total(x, order="fsum"):
    """The sum of the f64 array x in the given order, as np.float64."""
    x = np.asarray(x, dtype=np.float64)
    if order == "fsum":
        return np.float64(math.fsum(x.tolist()))
    if order == "sequential":
        return np.float64(np.add.accumulate(x)[-1]) if len(x) else np.float64(0.0)
    if order == "reversed":
        return np.float64(np.add.accumulate(x[::-1])[-1]) if len(x) else np.float64(0.0)
    if order == "blocks":
        return np.float64(_tree([np.add.accumulate(x[i:i + 64])[-1] for i in range(0, len(x), 64)]))
    if order == "pairwise":
        return np.float64(np.sum(x))
    raise ValueError(order)


def _centred(ab, a, b, length):
    """<a,b> - (A * B) / len: one multiplication, one division, one subtraction."""
    p = np.float64(a) * np.float64(b)
    q = p / np.float64(length)
    return np.float64(ab) - q


def _pos(x):
    """max(x, 0) as the header defines it: x when x > 0, else 0."""
    return x if x > 0.0 else np.float64(0.0)


def finish(ys, yv, yy, ss, vv, sv, with_noise=True):
    """The header's chain from the six (centred) sums: (sisdr, sisir, sisar);
    without interference the last two are NaN."""
    with np.errstate(all="ignore"):
        ys, yv, yy, ss, vv, sv = (np.float64(t) for t in (ys, yv, yy, ss, vv, sv))
        a = ys / ss
        et = a * ys
        r2 = _pos(yy - et)
        sisdr = np.float64(10.0) * np.log10(et / r2)
        if not with_noise:
            return float(sisdr), math.nan, math.nan
        rv = yv - a * sv
        ei = np.float64(0.0) if vv == 0.0 else rv * rv / vv
        ea = _pos(r2 - ei)
        sisir = np.float64(10.0) * np.log10(et / ei)
        sisar = np.float64(10.0) * np.log10(et / ea)
    return float(sisdr), float(sisir), float(sisar)


def scores(clean, y, noisy=None, lag=0, clip=False, zero_mean=True, order="fsum"):
    """(sisdr, sisir, sisar) of the f32 cell output y against clean (f64); the
    interference is noisy - clean, one fp64 subtraction (noisy None: SI-SDR
    alone, the other two NaN)."""
    s = np.asarray(clean, dtype=np.float64)
    L = len(s)
    t = test_signal(y, L, lag, clip)
    with_noise = noisy is not None
    v = np.asarray(noisy, dtype=np.float64) - s if with_noise else np.zeros(L)
    ss, vv, sv = total(s * s, order), total(v * v, order), total(s * v, order)
    ys, yv, yy = total(t * s, order), total(t * v, order), total(t * t, order)
    if zero_mean:
        S, V, Y = total(s, order), total(v, order), total(t, order)
        ss, vv, sv = _centred(ss, S, S, L), _centred(vv, V, V, L), _centred(sv, S, V, L)
        ys, yv, yy = _centred(ys, Y, S, L), _centred(yv, Y, V, L), _centred(yy, Y, Y, L)
    return finish(ys, yv, yy, ss, vv, sv, with_noise)


def same_class(a, b):
    """Whether two values that are not both finite are the same NaN / +inf / -inf."""
    if a != a or b != b:
        return a != a and b != b
    return a == b
