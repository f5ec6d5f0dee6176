"""numpy restatement of include/cse_csii.h: the three-level coherence speech
intelligibility index (Kates & Arehart 2005) and I3.  Frames, window, filters
and the test signal are tests/_segsnr_ref.py's.

dtype=np.float64 is the specification.  dtype=np.float32 runs the test signal's
side in f32 from the windowed frame on (scipy.fft on complex64, f32 sums of
Pxy and Pyy, f32 band sums and logarithms), with the clean side made in f64 and
X and Pxx kept as f32, MSC and 1 - MSC formed in f64 from the f32 sums and kept
as f32, and the sums over bands, the mean over frames and I3 in f64, as the
header's precision paragraph says of the device.  That variant is the CPU
stand-in for the device's precision: the tolerance of tests/test_gpu_csii.py is
derived from its distance to f64 (tools/csii_tolerance.py).
"""

import numpy as np
import scipy.fft

from _segsnr_ref import constants, filter_table, test_signal, window

LEVELS = ("high", "mid", "low")
A = np.array([0.003, 0.003, 0.003, 0.007, 0.010, 0.016, 0.016, 0.017, 0.017, 0.022, 0.027, 0.028,
              0.030, 0.032, 0.034, 0.035, 0.037, 0.036, 0.036, 0.033, 0.030, 0.029, 0.027, 0.026,
              0.026])
TINY = 2.0 ** -100
NAN = float("nan")


def levels(x, sr):
    """(code[J] with 0 high, 1 mid, 2 low, 3 none; n_L[3]; the smallest relative
    distance of any a_j to a threshold, inf when there is nothing to compare)."""
    W, hop, _, _ = constants(sr)
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    J = max(n // hop - 4, 0)
    code = np.full(J, 3, dtype=np.int64)
    S = float(np.sum(x * x))
    if J < 1 or S == 0.0:
        return code, np.zeros(3, dtype=np.int64), float("inf")
    s = np.array([np.sum(x[j * hop:j * hop + W] ** 2) for j in range(J)])
    a, b = s * n, S * W
    code[a >= 0.001 * b] = 2
    code[a >= 0.1 * b] = 1
    code[a >= b] = 0
    thr = np.array([b, 0.1 * b, 0.001 * b])
    margin = float(np.min(np.abs(a[:, None] - thr[None, :]) / thr[None, :]))
    return code, np.array([(code == L).sum() for L in range(3)], dtype=np.int64), margin


def i3_of(mid, low):
    if mid != mid or low != low:
        return NAN
    return float(1.0 / (1.0 + np.exp(-(-3.47 + 1.84 * low + 9.99 * mid))))


def csii(x, y, sr, lag=0, clip=False, dtype=np.float64, details=False):
    """(CSII_high, CSII_mid, CSII_low, I3); with details=True also n_L[3] and the
    level margin."""
    W, hop, nfft, H = constants(sr)
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    code, n_l, margin = levels(x, sr)
    J = len(code)
    out = [NAN, NAN, NAN]
    if J >= 1:
        y = test_signal(y, n, lag, clip)
        w = window(W)
        f32 = dtype == np.float32
        ctype = np.complex64 if f32 else np.complex128
        F = filter_table(sr).astype(dtype)
        for L in range(3):
            idx = np.flatnonzero(code == L)
            if len(idx) == 0:
                continue
            fx = np.stack([x[j * hop:j * hop + W] * w for j in idx])
            fy = np.stack([y[j * hop:j * hop + W] * w for j in idx]).astype(dtype)
            X = scipy.fft.fft(fx, nfft, axis=1)[:, :H]
            Y = scipy.fft.fft(fy.astype(ctype), nfft, axis=1)[:, :H]
            assert Y.dtype == ctype
            pxx = np.sum(X.real ** 2 + X.imag ** 2, axis=0).astype(dtype)
            X = X.astype(ctype)
            py = (Y.real * Y.real + Y.imag * Y.imag).astype(dtype)   # [n, H]
            pxy = np.sum(X * np.conj(Y), axis=0, dtype=ctype)
            pyy = np.sum(py, axis=0, dtype=dtype)
            den = pxx.astype(np.float64) * pyy.astype(np.float64)
            num = pxy.real.astype(np.float64) ** 2 + pxy.imag.astype(np.float64) ** 2
            with np.errstate(invalid="ignore", divide="ignore"):
                msc = np.where(den == 0.0, 0.0, np.minimum(num / den, 1.0))
            omm = (1.0 - msc).astype(dtype)
            msc = msc.astype(dtype)
            bn = (msc[None, :] * py) @ F.T       # [n, 25]
            bd = (omm[None, :] * py) @ F.T
            assert bn.dtype == dtype and bd.dtype == dtype
            with np.errstate(over="ignore"):
                q = bn / np.maximum(bd, dtype(TINY))
            sdr = np.clip(dtype(10.0) * np.log10(np.maximum(q, dtype(TINY))), dtype(-15.0),
                          dtype(15.0))
            T = ((sdr + dtype(15.0)) / dtype(30.0)).astype(dtype)
            c = (T.astype(np.float64) * A[None, :]).sum(axis=1) / A.sum()
            out[L] = float(np.mean(c))
    res = (out[0], out[1], out[2], i3_of(out[1], out[2]))
    return (res, n_l, margin) if details else res
