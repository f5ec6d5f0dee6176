"""Extended STOI (ESTOI) in numpy — test helper, not collected.

The definition of include/cse_estoi.h on top of oracle.stoi_ref's functions:
pystoi 0.4.1's ``stoi(x, y, fs_sig, extended=True)`` (Jensen & Taal 2016) with
the one stated difference — no ``EPS * standard_normal`` jitter, divisors
``norm + EPS``.  Everything up to the band envelopes, and both special cases
(fewer than 30 frames -> 1e-5; no frame -> an exception, None from
calculate_estoi), are the plain path's.
"""

import numpy as np

from oracle import stoi_ref
from oracle.stoi_ref import EPS, FS, N_SEG


def rcn(a):
    """Row (over the 30 frames), then column (over the 15 bands) mean removal
    and normalisation of segments a: (J, 15, 30)."""
    a = a - np.mean(a, axis=2, keepdims=True)
    a = a / (np.linalg.norm(a, axis=2, keepdims=True) + EPS)
    a = a - np.mean(a, axis=1, keepdims=True)
    a = a / (np.linalg.norm(a, axis=1, keepdims=True) + EPS)
    return a


def estoi_from_envelopes(x_tob, y_tob):
    M = x_tob.shape[1]
    xs = np.array([x_tob[:, m - N_SEG:m] for m in range(N_SEG, M + 1)])
    ys = np.array([y_tob[:, m - N_SEG:m] for m in range(N_SEG, M + 1)])
    return float(np.sum(rcn(xs) * rcn(ys)) / (N_SEG * xs.shape[0]))


def frames(x, y, fs_sig):
    """(STFT of x, STFT of y) after resampling and silent-frame removal: the
    number of rows is M."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    if x.shape != y.shape:
        raise Exception(f"x and y should have the same length, found {x.shape} and {y.shape}")
    if fs_sig != FS:
        x = stoi_ref.resample_oct(x, FS, fs_sig)
        y = stoi_ref.resample_oct(y, FS, fs_sig)
    x, y = stoi_ref.remove_silent_frames(x, y)
    return stoi_ref.stft(x), stoi_ref.stft(y)


def estoi(x, y, fs_sig):
    xs, ys = frames(x, y, fs_sig)
    if xs.shape[0] < N_SEG:
        return 1e-5
    return estoi_from_envelopes(stoi_ref.band_envelopes(xs), stoi_ref.band_envelopes(ys))


def calculate_estoi(clean_reference, test_audio, sr):
    """calculate_stoi's wrapper: trim to the common length, None on failure."""
    try:
        n = min(len(clean_reference), len(test_audio))
        return estoi(clean_reference[:n], test_audio[:n], sr)
    except Exception:
        return None
