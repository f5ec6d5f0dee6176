"""numpy restatement of include/cse_segsnr.h: segmental SNR and frequency-weighted
segmental SNR (Loizou's comp_snr / comp_fwseg as pysepm's SNRseg / fwSNRseg
restate them, with the header's two stated differences: exactly-silent clean
frames are left out, and the spectra are divided by sum + EPS).

Every function takes dtype=: np.float64 is the specification; np.float32 runs
the test signal's side in f32 from the windowed frame on (scipy.fft on
complex64), with the frame sums and the mean over frames accumulated in f64 and
the clean side (s, ce, Wt) made in f64 and kept as f32, as the header's
precision paragraph says of the device.  That variant is the CPU stand-in for
the device's precision: the tolerance of tests/test_gpu_segsnr.py is derived
from its distance to f64 (tools/segsnr_tolerance.py).
"""

import numpy as np
import scipy.fft

EPS = 2.0 ** -52
NBANDS = 25
CENT = np.array([50.0, 120.0, 190.0, 260.0, 330.0, 400.0, 470.0, 540.0, 617.372, 703.378,
                 798.717, 904.128, 1020.38, 1148.30, 1288.72, 1442.54, 1610.70, 1794.16,
                 1993.93, 2211.08, 2446.71, 2701.97, 2978.04, 3276.17, 3597.63])
BAND = np.array([70.0, 70.0, 70.0, 70.0, 70.0, 70.0, 70.0, 77.3724, 86.0056, 95.3398, 105.411,
                 116.256, 127.914, 140.423, 153.823, 168.154, 183.457, 199.776, 217.153,
                 235.631, 255.255, 276.072, 298.126, 321.465, 346.136])
FLOOR = np.exp(-30.0 / (2.0 * 2.303))
LO, HI = -10.0, 35.0


def constants(sr):
    """(W, hop, NFFT, H) of a supported rate."""
    if sr not in (16000, 8000):
        raise NotImplementedError(f"segSNR: sample rate {sr} not supported (16000, 8000)")
    W = int(round(0.03 * sr))
    nfft = 1 << int(np.ceil(np.log2(2 * W)))
    return W, W // 4, nfft, nfft // 2


def window(W):
    """MATLAB hanning(W): strictly positive."""
    return 0.5 * (1.0 - np.cos(2.0 * np.pi * (np.arange(W) + 1.0) / (W + 1.0)))


def filter_table(sr):
    """F[25][H]: the critical-band filters, entries not above FLOOR zeroed."""
    _, _, _, H = constants(sr)
    f0 = np.floor(CENT / (sr / 2.0) * H)
    bw = BAND / (sr / 2.0) * H
    k = np.arange(H, dtype=np.float64)
    F = np.exp(-11.0 * ((k[None, :] - f0[:, None]) / bw[:, None]) ** 2
               + np.log(BAND[0]) - np.log(BAND)[:, None])
    F[~(F > FLOOR)] = 0.0
    return F


def test_signal(y, length, lag=0, clip=False):
    """The cell's test signal as cse_stoi_cells defines it: y[n - lag], zero
    outside [0, length), clipped to [-1, 1] when clip."""
    y = np.asarray(y, dtype=np.float64)[:length]
    out = np.zeros(length)
    n = np.arange(length)
    s = n - int(lag)
    ok = (s >= 0) & (s < len(y))
    out[ok] = y[s[ok]]
    return np.clip(out, -1.0, 1.0) if clip else out


def frame_values(x, y, sr, lag=0, clip=False, dtype=np.float64):
    """(segSNR value, fwSegSNR value) of every non-silent frame, [Ja] each;
    None when J < 1."""
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
    eps = dtype(EPS)
    ctype = np.complex64 if dtype == np.float32 else np.complex128
    seg, fw = [], []
    for j in range(J):
        xs = x[j * hop:j * hop + W]
        if not xs.any():  # silent: all W clean samples exactly 0 (from the f64 samples)
            continue
        xf = (xs * w).astype(dtype)
        yf = (y[j * hop:j * hop + W] * w).astype(dtype)
        # segSNR: the frame sums may accumulate in f64
        s = np.sum((xs * w) ** 2)  # clean side: f64
        d = xf - yf
        e = np.sum((d * d).astype(np.float64))
        v = 10.0 * np.log10(s / (e + EPS) + EPS)
        seg.append(min(max(v, LO), HI))
        # fwSegSNR
        # the clean side is made once per signal in f64 (cse_segsnr_prepare) and
        # kept as f32; the test side runs in `dtype` from the windowed frame on
        X = np.abs(scipy.fft.fft(xs * w, nfft)[:H])
        X = X / (np.sum(X) + EPS)
        ce64 = F64 @ X
        ce = ce64.astype(dtype)
        Wt = (ce64 ** 0.2).astype(dtype)
        Y = np.abs(scipy.fft.fft(yf.astype(ctype), nfft)[:H]).astype(dtype)
        Y = Y / dtype(np.sum(Y.astype(np.float64)) + EPS)
        pe = F @ Y
        err = np.maximum((ce - pe) ** 2, eps)
        pos = ce > 0
        snr = np.zeros(NBANDS, dtype=dtype)
        snr[pos] = dtype(10.0) * np.log10(ce[pos] ** 2 / err[pos])
        num = np.sum((Wt * snr).astype(np.float64))
        den = np.sum(Wt.astype(np.float64)) + EPS
        fw.append(min(max(num / den, LO), HI))
    return np.asarray(seg, dtype=np.float64), np.asarray(fw, dtype=np.float64)


def scores(x, y, sr, lag=0, clip=False, dtype=np.float64):
    """(segSNR, fwSegSNR) in dB; NaN for both when J < 1 or Ja = 0."""
    fv = frame_values(x, y, sr, lag, clip, dtype)
    if fv is None or len(fv[0]) == 0:
        return float("nan"), float("nan")
    return float(np.mean(fv[0])), float(np.mean(fv[1]))


def segsnr(x, y, sr, **kw):
    return scores(x, y, sr, **kw)[0]


def fwsegsnr(x, y, sr, **kw):
    return scores(x, y, sr, **kw)[1]
