"""The inputs of tests/test_gpu_segsnr.py, built from an `enhance` callable so
that the GPU test (device plugins) and the CPU tolerance measurement
(tools/segsnr_tolerance.py, the oracle's plugins) walk the same cases.

A case is (name, clean f64 [L], y f32 [L], sr, lag, clip): one cell.
"""

import numpy as np

from classical_speech_enhancement_amd.synth import make_pair

OMLSA = dict(n_fft=512, hop_length=128, alpha=0.9, ksi_min=0.005, q=0.4, noise_mu=0.95,
             gain_floor=0.1, noise_percentile=10.0, noise_method="min_tracking")
SS = dict(alpha=1.5, beta=0.001, n_fft=512, hop_length=128, noise_percentile=10.0,
          noise_method="percentile")
N_CELLS = 37
N_SIG = 3
# pair ids whose 1-s / 0.5-s clips hold speech (a short synthetic clip can be one pause)
PAIRS_1S = (0, 1, 2)
PAIR_HALF = 3


def lags(L):
    """no shift; a few samples either way; more than a frame of zeros at the
    head; all but the last 100 samples shifted out."""
    return (0, 37, -37, 601, -(L - 100))


def clip_set(i, seconds, enhance):
    """clean (f64) and the test waveforms (f32) of pair i."""
    clean, noisy = make_pair(i, seconds=seconds)
    omlsa = enhance("omlsa", noisy, OMLSA)
    ss = enhance("ss", noisy, SS)
    loud = omlsa * (1.7 / np.max(np.abs(omlsa)))  # beyond [-1, 1]: the clip runs
    waves = [noisy, omlsa, ss, clean, loud]
    return clean, [np.asarray(w, dtype=np.float64).astype(np.float32) for w in waves]


def decimate(x):
    from scipy.signal import resample_poly
    return resample_poly(np.asarray(x, dtype=np.float64), 1, 2)


def launch(enhance, sr=16000):
    """The 37-cell launch: (clean [3, L] f64, y flat f32, y_offset, sig_of, lag).
    sig_of is mixed and unsorted, the cells lie in y in another order than
    their index and behind a 123-sample head, every waveform kind meets every
    lag."""
    sets = [clip_set(i, 1.0, enhance) for i in PAIRS_1S]
    if sr == 8000:
        sets = [(decimate(c), [decimate(w).astype(np.float32) for w in ws]) for c, ws in sets]
    clean = np.stack([c for c, _ in sets])
    L = clean.shape[1]
    lg = lags(L)
    sig = np.array([(7 * c + 1) % N_SIG for c in range(N_CELLS)], dtype=np.int32)
    kind = np.arange(N_CELLS) % 5
    lag = np.array([lg[(c // 5 + c) % 5] for c in range(N_CELLS)], dtype=np.int32)
    place = np.random.default_rng(5).permutation(N_CELLS)
    y = np.full(123 + N_CELLS * L, 0.25, dtype=np.float32)
    off = 123 + place.astype(np.int64) * L
    for c in range(N_CELLS):
        y[off[c]:off[c] + L] = sets[sig[c]][1][kind[c]]
    return clean, y, off, sig, lag


def launch_cases(enhance, sr=16000):
    clean, y, off, sig, lag = launch(enhance, sr)
    L = clean.shape[1]
    return [(f"{sr} cell {c}", clean[sig[c]], y[off[c]:off[c] + L], sr, int(lag[c]), True)
            for c in range(N_CELLS)]


def edge_cases(enhance):
    """len 600 (one frame), 599 (none), 8077 (a tail shorter than a hop)."""
    clean, waves = clip_set(PAIR_HALF, 0.5, enhance)
    full = np.concatenate([clean, clean[:77]])
    y = np.concatenate([waves[0], waves[1][:77]])
    start = int(np.flatnonzero(clean)[0]) + 200  # inside speech
    out = []
    for n in (600, 599):
        out.append((f"len {n}", clean[start:start + n].copy(), waves[0][start:start + n].copy(),
                    16000, 0, True))
    out.append(("len 8077", full, y, 16000, 0, True))
    return out


def silent_cases(enhance):
    """samples [3000, 5210) of the clean signal zeroed (edges off the hop
    grid): against clean itself and against noisy; an all-zero test signal."""
    clean, waves = clip_set(PAIR_HALF, 0.5, enhance)
    gap = clean.copy()
    gap[3000:5210] = 0.0
    return [("gap vs itself", gap, gap.astype(np.float32), 16000, 0, True),
            ("gap vs noisy", gap, waves[0], 16000, 0, True),
            ("zero test", clean, np.zeros(len(clean), np.float32), 16000, 0, True),
            ("zero test, gap", gap, np.zeros(len(clean), np.float32), 16000, 0, False)]


def zero_clean_batch(enhance):
    """(clean [3, L] with the middle signal all zero, y flat, off, sig): the
    zero signal's cells give NaN, the others are unaffected."""
    clean, waves = clip_set(PAIR_HALF, 0.5, enhance)
    L = len(clean)
    cl = np.stack([clean, np.zeros(L), clean[::-1].copy()])
    y = np.concatenate([waves[0], waves[1], waves[0], waves[2][::-1].copy()])
    return cl, y, np.arange(4, dtype=np.int64) * L, np.array([0, 1, 1, 2], dtype=np.int32)


GRID = {"spectralSubtractor": {"alpha": [1.0, 2.0], "beta": [0.01, 0.1], "n_fft": [512],
                               "hop_length": [128], "noise_percentile": [10.0],
                               "noise_method": ["percentile"]}}
GRID_PAIRS = (0, 1)


def python_layer_cases(enhance):
    """The cells the GPU file scores through metrics and search: the unclipped
    scalar and trimmed calls, the noisy baselines, and the 4-cell grid of the
    two 1-s pairs.  The grid cells stand at lag 0 here; on the device they are
    shifted by the alignment lag the engine finds, which only a GPU run
    knows."""
    from classical_speech_enhancement_amd.parameter_ranges import grid_cells
    clean, waves = clip_set(PAIR_HALF, 0.5, enhance)
    out = [("scalars", clean, waves[1], 16000, 0, False),
           ("trimmed", clean[:7000], waves[1][:7000], 16000, 0, False),
           ("quality noisy", clean, waves[0], 16000, 0, False)]
    for i in GRID_PAIRS:
        c, n = make_pair(i, seconds=1.0)
        out.append((f"baseline {i}", c, n.astype(np.float32), 16000, 0, False))
        for k, p in enumerate(grid_cells(GRID["spectralSubtractor"])):
            y = np.asarray(enhance("ss", n, p), dtype=np.float64).astype(np.float32)
            out.append((f"grid pair {i} cell {k}", c, y, 16000, 0, True))
    return out


def all_cases(enhance):
    """Every (clean, test) cell the GPU file scores, directly and through the
    Python layer (python_layer_cases says what stands in there)."""
    out = launch_cases(enhance, 16000) + launch_cases(enhance, 8000)
    out += python_layer_cases(enhance)
    out += edge_cases(enhance) + silent_cases(enhance)
    cl, y, off, sig = zero_clean_batch(enhance)
    L = cl.shape[1]
    out += [(f"zero-clean batch {c}", cl[sig[c]], y[off[c]:off[c] + L], 16000, 0, True)
            for c in range(4)]
    return out
