"""numpy restatement of include/cse_ncm.h: the normalized covariance measure
(NCM) and its signal-dependent band-importance form.  Frames, window, filters
and the test signal are tests/_segsnr_ref.py's; the articulation-index weights
are tests/_csii_ref.py's.

dtype=np.float64 is the specification.  dtype=np.float32 runs the test signal's
side in f32 from the windowed frame through the band envelope e_j[i]
(scipy.fft on complex64, f32 powers, f32 band sums, f32 square root); the clean
side, the envelope samples E_m, the running sums and everything after them are
f64, as the header's precision paragraph says of the device.  That variant is
the CPU stand-in for the device's precision: the tolerance of
tests/test_gpu_ncm.py is derived from its distance to f64
(tools/ncm_tolerance.py).

envelopes() makes the envelope samples of both signals; score_from_envelopes()
is everything after them, so that the dead-band and zero-clean rules can be
tested with hand-made envelopes.
"""

import numpy as np
import scipy.fft

from _csii_ref import A
from _segsnr_ref import constants, filter_table, test_signal, window

NAN = float("nan")
TINY = 2.0 ** -100
DEAD = 2.0 ** -40          # vx > DEAD sxx, vy > DEAD syy: the band moves
MARGIN = 2.0 ** -30        # what every GPU input keeps: v / s is 0 or at least this
G = 0.5 * (1.0 - np.cos(2.0 * np.pi * (np.arange(8) + 1.0) / 9.0))


def frame_counts(n, sr):
    """(J, M) of a clip of n samples; M = 0 when J < 8."""
    _, hop, _, _ = constants(sr)
    J = max(n // hop - 4, 0)
    return J, ((J - 8) // 4 + 1 if J >= 8 else 0)


def band_envelopes(sig, sr, dtype=np.float64):
    """e[J][25] of one signal: sqrt(sum_k F[i][k] |S_j[k]|^2), in ``dtype`` from
    the windowed frame on."""
    W, hop, nfft, H = constants(sr)
    sig = np.asarray(sig, dtype=np.float64)
    J, _ = frame_counts(len(sig), sr)
    w = window(W)
    ctype = np.complex64 if dtype == np.float32 else np.complex128
    F = filter_table(sr).astype(dtype)
    frames = np.stack([sig[j * hop:j * hop + W] * w for j in range(J)]).astype(dtype)
    S = scipy.fft.fft(frames.astype(ctype), nfft, axis=1)[:, :H]
    assert S.dtype == ctype
    pw = (S.real * S.real + S.imag * S.imag).astype(dtype)
    e = np.sqrt(pw @ F.T)
    assert e.dtype == dtype
    return e


def envelope_samples(e):
    """E[M][25] in f64 from e[J][25]: the 8-tap low-pass, decimated by 4, the
    taps added in increasing order."""
    J = e.shape[0]
    M = (J - 8) // 4 + 1
    e = e.astype(np.float64)
    E = np.zeros((M, e.shape[1]))
    for d in range(8):
        E += G[d] * e[d:d + 4 * (M - 1) + 1:4]
    return E


def envelopes(x, y, sr, lag=0, clip=False, dtype=np.float64):
    """(Ex, Ey), [M][25] f64 each; None when J < 12 (M < 2)."""
    x = np.asarray(x, dtype=np.float64)
    J, M = frame_counts(len(x), sr)
    if M < 2:
        return None
    y = test_signal(y, len(x), lag, clip)
    return envelope_samples(band_envelopes(x, sr)), envelope_samples(band_envelopes(y, sr, dtype))


def band_sums(Ex, Ey):
    """The per-band sums of the header, [25] each: vx, sxx, cxy, vy, syy."""
    Ex = np.asarray(Ex, dtype=np.float64)
    Ey = np.asarray(Ey, dtype=np.float64)
    M = Ex.shape[0]
    mu = Ex.sum(axis=0) / M
    dx = Ex - mu[None, :]
    vx = (dx * dx).sum(axis=0)
    sxx = (Ex * Ex).sum(axis=0)
    cxy = (dx * Ey).sum(axis=0)
    sy = Ey.sum(axis=0)
    syy = (Ey * Ey).sum(axis=0)
    vy = np.maximum(syy - sy * sy / M, 0.0)
    return vx, sxx, cxy, vy, syy


def margins(Ex, Ey):
    """(smallest non-zero vx / sxx, smallest non-zero vy / syy, ok): ok when every
    ratio is exactly 0 with a zero denominator or at least MARGIN."""
    vx, sxx, _, vy, syy = band_sums(Ex, Ey)
    ok, least = True, []
    for v, s in ((vx, sxx), (vy, syy)):
        zero = s == 0.0
        ok = ok and bool(np.all(v[zero] == 0.0))
        ratio = v[~zero] / s[~zero]
        ok = ok and bool(np.all(ratio >= MARGIN))
        least.append(float(ratio.min()) if ratio.size else float("inf"))
    return least[0], least[1], ok


def transmission_index(Ex, Ey):
    """TI[25] of the header."""
    vx, sxx, cxy, vy, syy = band_sums(Ex, Ey)
    moves = (vx > DEAD * sxx) & (vy > DEAD * syy)
    with np.errstate(invalid="ignore", divide="ignore"):
        r2 = np.where(moves, np.minimum(cxy * cxy / (vx * vy), 1.0), 0.0)
    snr = 10.0 * np.log10(np.maximum(r2, TINY) / np.maximum(1.0 - r2, TINY))
    return (np.clip(snr, -15.0, 15.0) + 15.0) / 30.0


def score_from_envelopes(Ex, Ey, p=1.0):
    """(ncm, ncm_bif) from the envelope samples [M][25]."""
    Ex = np.asarray(Ex, dtype=np.float64)
    sxx = (Ex * Ex).sum(axis=0)
    if Ex.shape[0] < 2 or sxx.sum() == 0.0:
        return NAN, NAN
    ti = transmission_index(Ex, Ey)
    wb = sxx ** float(p)
    return float((A * ti).sum() / A.sum()), float((wb * ti).sum() / wb.sum())


def ncm(x, y, sr, lag=0, clip=False, dtype=np.float64, p=1.0, details=False):
    """(ncm, ncm_bif); with details=True also margins() of the envelopes (None
    when there are none)."""
    env = envelopes(x, y, sr, lag, clip, dtype)
    res = (NAN, NAN) if env is None else score_from_envelopes(env[0], env[1], p)
    return (res, None if env is None else margins(*env)) if details else res
