"""The inputs of tests/test_gpu_csii.py, shared with tools/csii_tolerance.py
(which measures the f32 restatement against the f64 one over exactly these).

Every case is (name, clean f64 [L], y f32 [L], sr, lag, clip).  The clips are
the synthetic pairs of classical_speech_enhancement_amd.synth, cut to the
lengths at which the kernel takes another path: no frame, one frame, 15 / 16 /
17 frames (around the eight waves of a workgroup and their second round), and a
few hundred.  A short synthetic clip can be one pause, so each length takes the
first pair whose cut holds speech in more than half of its frames.
"""

import numpy as np

from classical_speech_enhancement_amd.synth import make_pair

LENGTHS = {16000: (599, 600, 2280, 2400, 2520, 4000, 16000), 8000: (300, 2000, 16000)}
LAGS = (-7, 0, 13)


def speech_cut(L, sr, start=0):
    """(clean, noisy) of the first pair from ``start`` whose first L samples are
    mostly speech."""
    for i in range(start, start + 64):
        clean, noisy = make_pair(i, seconds=max(L / sr, 0.5), sr=sr)
        c = clean[:L]
        if np.count_nonzero(c) > L // 2:
            return c.copy(), noisy[:L].copy()
    raise AssertionError("no synthetic pair with speech at this length")


def length_cases():
    """One cell per length, rate and lag; the test signal is the noisy input
    scaled so that samples pass +-1 and the clip has something to do."""
    out = []
    for sr, lengths in LENGTHS.items():
        for L in lengths:
            clean, noisy = speech_cut(L, sr)
            y = (noisy * (1.2 / np.abs(noisy).max())).astype(np.float32)
            assert np.abs(y).max() > 1.0
            for lag in LAGS:
                out.append((f"{sr} Hz len {L} lag {lag}", clean, y, sr, lag, True))
    return out


def batch():
    """Three 4000-sample signals and five cells each through sig_of, unsorted;
    the cells lie in y in another order than their index, behind a 61-sample
    head: (clean [3, L] f64, y flat f32, y_offset, sig_of, lag)."""
    L = 4000
    pairs, start = [], 0
    for _ in range(3):
        c, n = speech_cut(L, 16000, start)
        pairs.append((c, n))
        start += 7
    clean = np.stack([c for c, _ in pairs])
    rng = np.random.default_rng(77)
    sig = np.array([2, 0, 1, 1, 0, 2, 2, 1, 0, 0, 1, 2, 0, 2, 1], dtype=np.int32)
    lag = np.array([LAGS[c % 3] for c in range(15)], dtype=np.int32)
    place = rng.permutation(15)
    y = np.zeros(61 + 15 * L, dtype=np.float32)
    off = np.zeros(15, dtype=np.int64)
    for c in range(15):
        c0, n0 = pairs[sig[c]]
        # noisy input with more or less of its noise: each cell scores differently
        g = 0.2 + 0.12 * c
        w = (c0 + g * (n0 - c0)) * 5.0
        off[c] = 61 + place[c] * L
        y[off[c]:off[c] + L] = w.astype(np.float32)
    return clean, y, off, sig, lag


def batch_cases():
    clean, y, off, sig, lag = batch()
    L = clean.shape[1]
    return [(f"batch cell {c}", clean[sig[c]], y[off[c]:off[c] + L], 16000, int(lag[c]), True)
            for c in range(len(sig))]


def pause_case():
    """1 s of a pair with exact-zero pauses (the synthetic pairs have them)."""
    clean, noisy = make_pair(1, seconds=1.0)
    assert np.count_nonzero(clean == 0.0) > 1000 and np.count_nonzero(clean) > 4000
    return ("pauses", clean, noisy.astype(np.float32), 16000, 0, False)


def sparse_levels_case():
    """White noise for 2400 samples, then 4800 exact zeros: the frames inside
    the noise and the two that hold three quarters and half of it are high, the
    one that holds a quarter is the only mid frame, and no frame is low."""
    rng = np.random.default_rng(5)
    clean = np.zeros(7200)
    clean[:2400] = 0.1 * rng.standard_normal(2400)
    y = (clean + 0.05 * rng.standard_normal(7200)).astype(np.float32)
    return ("one mid frame, no low frame", clean, y, 16000, 0, False)


def fixed_point_cases():
    """y = x and an all-zero y."""
    clean, _ = speech_cut(4000, 16000)
    return [("y = x", clean, clean.astype(np.float32), 16000, 0, False),
            ("zero y", clean, np.zeros(len(clean), dtype=np.float32), 16000, 0, False)]


def scale_case():
    """(clean, y): y is scored against 0.5 y."""
    clean, noisy = speech_cut(4000, 16000)
    return clean, noisy.astype(np.float32)


def direct_cases():
    """Every cell the GPU file compares with the restatement outside the sweep."""
    clean, y = scale_case()
    return (length_cases() + batch_cases() + [pause_case(), sparse_levels_case()]
            + fixed_point_cases()
            + [("scale 1", clean, y, 16000, 0, False),
               ("scale 0.5", clean, (0.5 * y).astype(np.float32), 16000, 0, False)])
