"""numpy restatement of include/cse_wss.h: the weighted spectral slope distance
(Klatt 1982; Loizou's comp_wss as pysepm's wss restates it, nearest-peak quirk
included), with the header's one difference: exactly-silent clean frames are
left out.  Frames, window, filters and the test signal are tests/_segsnr_ref.py's.

Every function takes dtype=: np.float64 is the specification; np.float32 runs
the test signal's side in f32 from the windowed frame on (scipy.fft on
complex64), with the clean side (E_x, Wx) made in f64 and kept as f32, the
frame's two sums and the mean over frames accumulated in f64 and a frame's
value stored as f32, as the header's precision paragraph says of the device.
That variant is the CPU stand-in for the device's precision: the tolerance of
tests/test_gpu_wss.py is derived from its distance to f64
(tools/wss_tolerance.py).
"""

import numpy as np
import scipy.fft

from _segsnr_ref import constants, filter_table, test_signal, window

NBANDS = 25
KMAX, KLOC = 20.0, 1.0
E_FLOOR = 1e-10


def n95(ja):
    """Frames averaged of ja kept ones: round(0.95 ja), half up, in integers."""
    return (19 * int(ja) + 10) // 20


def nearest_peak(E):
    """P[24] of the band energies E[25]: the header's rule."""
    E = np.asarray(E)
    s = E[1:] - E[:-1]
    P = np.empty(NBANDS - 1, dtype=E.dtype)
    for i in range(NBANDS - 1):
        n = i
        if s[i] > 0:
            while n < NBANDS - 1 and s[n] > 0:
                n += 1
            P[i] = E[n - 1]
        else:
            while n >= 0 and s[n] <= 0:
                n -= 1
            P[i] = E[n + 1]
    return P


def nearest_peak_matlab(E):
    """The same rule as a literal transcription of comp_wss's 1-based loops."""
    num_crit = NBANDS
    energy = {k + 1: v for k, v in enumerate(np.asarray(E))}        # energy(1..25)
    slope = {i: energy[i + 1] - energy[i] for i in range(1, num_crit)}  # slope(1..24)
    loc_peak = {}
    for i in range(1, num_crit):            # for i = 1:num_crit-1
        if slope[i] > 0:                    # search to the right
            n = i
            while n < num_crit and slope[n] > 0:
                n = n + 1
            loc_peak[i] = energy[n - 1]
        else:                               # search to the left
            n = i
            while n > 0 and slope[n] <= 0:
                n = n - 1
            loc_peak[i] = energy[n + 1]
    return np.array([loc_peak[i] for i in range(1, num_crit)], dtype=np.asarray(E).dtype)


def band_energies(f, F, nfft, H, dtype=np.float64):
    """E[25] in dB of the windowed frame f (already of `dtype`)."""
    ctype = np.complex64 if dtype == np.float32 else np.complex128
    Z = scipy.fft.fft(f.astype(ctype), nfft)[:H]
    S = (Z.real * Z.real + Z.imag * Z.imag).astype(dtype)
    e = F @ S
    return (dtype(10.0) * np.log10(np.maximum(e, dtype(E_FLOOR)))).astype(dtype)


def weights(E):
    """W[24] = Wmax Wloc of the band energies E[25], in E's precision."""
    t = E.dtype.type
    P = nearest_peak(E)
    wmax = t(KMAX) / (t(KMAX) + (E.max() - E[:-1]))
    wloc = t(KLOC) / (t(KLOC) + (P - E[:-1]))
    return wmax * wloc


def frame_values(x, y, sr, lag=0, clip=False, dtype=np.float64):
    """The WSS value of every non-silent frame, [Ja]; None when J < 1."""
    W, hop, nfft, H = constants(sr)
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    y = test_signal(y, n, lag, clip)
    J = n // hop - 4
    if J < 1:
        return None
    w = window(W)
    F64 = filter_table(sr)
    F = F64.astype(dtype)
    out = []
    for j in range(J):
        xs = x[j * hop:j * hop + W]
        if not xs.any():  # silent: all W clean samples exactly 0 (from the f64 samples)
            continue
        # the clean side is made once per signal in f64 (cse_wss_prepare) and kept
        # as f32: E_x, from which sx follows in `dtype`, and Wx
        Ex64 = band_energies(xs * w, F64, nfft, H)
        Ex = Ex64.astype(dtype)
        Wx = weights(Ex64).astype(dtype)
        sx = Ex[1:] - Ex[:-1]
        # the test side runs in `dtype` from the windowed frame on
        yf = (y[j * hop:j * hop + W] * w).astype(dtype)
        Ey = band_energies(yf, F, nfft, H, dtype)
        Wy = weights(Ey)
        sy = Ey[1:] - Ey[:-1]
        Wt = dtype(0.5) * (Wx + Wy)
        d = sx - sy
        num = np.sum((Wt * (d * d)).astype(np.float64))
        den = np.sum(Wt.astype(np.float64))
        v = num / den
        out.append(float(np.float32(v)) if dtype == np.float32 else v)
    return np.asarray(out, dtype=np.float64)


def wss(x, y, sr, lag=0, clip=False, dtype=np.float64):
    """The cell score: the mean of the n95 smallest frame values; NaN when
    J < 1 or Ja = 0."""
    fv = frame_values(x, y, sr, lag, clip, dtype)
    if fv is None or len(fv) == 0:
        return float("nan")
    return float(np.mean(np.sort(fv)[:n95(len(fv))]))
