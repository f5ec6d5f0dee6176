"""numpy restatement of include/cse_lpc.h: the log-likelihood ratio (LLR) and the
LPC cepstrum distance (CEP), Loizou's comp_llr / comp_cep with the header's
three stated differences (exactly-silent clean frames left out, the guarded
Levinson-Durbin recursion, the clamp of a frame's LLR to [0, 2]).

Written from the header, not from the kernel: the quadratic forms go through
the explicit Toeplitz matrix, the selection is a sort.

dtype= runs everything from the windowed sample on in that format: np.float64 is
the specification, np.longdouble measures the specification's own rounding,
np.float32 is the all-f32 evaluation the header rules out.  store= is the format
a frame's two values are kept in before the n95 smallest are averaged: None
keeps dtype; np.float32 with dtype=np.float64 is what the header's precision
paragraph says of the device, and its distance to plain f64 is the yardstick of
tests/test_gpu_lpc.py's tolerance (tools/lpc_tolerance.py).
"""

import numpy as np

from _segsnr_ref import test_signal

LLR_MAX, CEP_MAX = 2.0, 10.0


def constants(sr):
    """(W, hop, P) of a supported rate."""
    if sr not in (16000, 8000):
        raise NotImplementedError(f"LLR/CEP: sample rate {sr} not supported (16000, 8000)")
    W = int(round(0.03 * sr))
    return W, W // 4, 16 if sr == 16000 else 10


def window(W, dtype=np.float64):
    pi = dtype(4) * np.arctan(dtype(1))
    i = np.arange(W).astype(dtype)
    return (dtype(0.5) * (dtype(1) - np.cos(dtype(2) * pi * (i + dtype(1)) / dtype(W + 1)))).astype(dtype)


def n95(ja):
    """round(0.95 Ja), half up, in integers."""
    return (19 * int(ja) + 10) // 20


def autocorr(f, P):
    """R[:, k] = sum_{i < W - k} f[:, i] f[:, i + k], k = 0..P, of frames f [n, W]."""
    W = f.shape[1]
    return np.stack([np.sum(f[:, :W - k] * f[:, k:], axis=1) for k in range(P + 1)], axis=1)


def levinson(R):
    """The monic predictors A [n, P + 1] of the autocorrelations R [n, P + 1],
    with the header's guard: a frame's recursion stops at step i when
    E_{i-1} > 0 or |k_i| < 1 is false, its coefficients of order >= i stay 0."""
    n, P1 = R.shape
    A = np.zeros_like(R)
    A[:, 0] = 1
    E = R[:, 0].copy()
    go = np.ones(n, dtype=bool)
    with np.errstate(all="ignore"):
        for i in range(1, P1):
            s = R[:, i].copy()
            for j in range(1, i):
                s = s + A[:, j] * R[:, i - j]
            k = -s / E
            go = go & (E > 0) & (np.abs(k) < 1)
            new = A.copy()
            for j in range(1, i):
                new[:, j] = A[:, j] + k * A[:, i - j]
            new[:, i] = k
            A = np.where(go[:, None], new, A)
            E = np.where(go, (1 - k * k) * E, E)
    return A


def toeplitz_form(R, A):
    """A T(R) A^T per frame, T(R)[a, b] = R[|a - b|]."""
    P1 = R.shape[1]
    idx = np.abs(np.arange(P1)[:, None] - np.arange(P1)[None, :])
    T = R[:, idx]  # [n, P1, P1]
    return np.sum(A[:, :, None] * T * A[:, None, :], axis=(1, 2))


def cepstrum(A):
    """c[:, 1..P] of the predictors A (column 0 unused)."""
    P1 = A.shape[1]
    c = np.zeros_like(A)
    c[:, 1] = -A[:, 1]
    for n in range(2, P1):
        s = np.zeros_like(A[:, 0])
        for k in range(1, n):
            s = s + k * c[:, k] * A[:, n - k]
        c[:, n] = -(A[:, n] + s / n)
    return c


def frame_values(x, y, sr, lag=0, clip=False, dtype=np.float64):
    """(llr, cep) of every non-silent frame, [Ja] each, in dtype; None when J < 1."""
    W, hop, P = constants(sr)
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    y = test_signal(y, n, lag, clip)
    J = n // hop - 4
    if J < 1:
        return None
    idx = np.arange(J)[:, None] * hop + np.arange(W)[None, :]
    xs = x[idx]
    keep = xs.any(axis=1)  # silent: all W clean samples exactly 0 (from the f64 samples)
    w = window(W, dtype)
    xf = xs[keep].astype(dtype) * w
    yf = y[idx][keep].astype(dtype) * w
    Rx, Ry = autocorr(xf, P), autocorr(yf, P)
    Ax, Ay = levinson(Rx), levinson(Ry)
    with np.errstate(all="ignore"):
        ratio = toeplitz_form(Rx, Ay) / toeplitz_form(Rx, Ax)
        ok = np.isfinite(ratio) & (ratio > 0)
        llr = np.where(ok, np.log(np.where(ok, ratio, 1)), dtype(LLR_MAX))
        llr = np.minimum(np.maximum(llr, 0), dtype(LLR_MAX)).astype(dtype)
        d = np.sum((cepstrum(Ax)[:, 1:] - cepstrum(Ay)[:, 1:]) ** 2, axis=1)
        cep = (dtype(10) / np.log(dtype(10))) * np.sqrt(2 * d)
        cep = np.where(np.isfinite(cep), np.minimum(cep, dtype(CEP_MAX)), dtype(CEP_MAX)).astype(dtype)
    return llr, cep


def trimmed_mean(v, store=None):
    """Mean of the n95 smallest of the frame values v, kept in `store` (None:
    as they are), accumulated in f64 (longdouble values: in longdouble)."""
    if store is not None:
        v = v.astype(store)
    acc = np.longdouble if v.dtype == np.longdouble else np.float64
    k = n95(len(v))
    return np.sum(np.sort(v)[:k].astype(acc)) / acc(k)


def scores(x, y, sr, lag=0, clip=False, dtype=np.float64, store=None, exact=False):
    """(LLR, CEP); NaN for both when J < 1 or Ja = 0.  exact=True returns them
    in the accumulation format (longdouble runs) instead of Python floats."""
    fv = frame_values(x, y, sr, lag, clip, dtype)
    if fv is None or len(fv[0]) == 0:
        return float("nan"), float("nan")
    out = trimmed_mean(fv[0], store), trimmed_mean(fv[1], store)
    return out if exact else (float(out[0]), float(out[1]))


def llr(x, y, sr, **kw):
    return scores(x, y, sr, **kw)[0]


def cep(x, y, sr, **kw):
    return scores(x, y, sr, **kw)[1]
