"""The measured tolerance of tests/test_gpu_wss.py (CPU only).

    python tools/wss_tolerance.py

Walks the inputs of the GPU file (tests/_segsnr_cases.py: the launches, the
edge and silent cases, and the Python layer's cells with the grid cells at lag
0; the enhanced waveforms made by the oracle's plugins in place of the
device's) and prints max |ref(f32) - ref(f64)| of tests/_wss_ref.py over the
scored cells, the worst cell, and for that cell its worst frame with the band
whose energy differs most.  The test tolerance is 8 times that figure (the
factor covers a different FFT factorisation and summation order from scipy's),
and may be no looser than 2e-2.
"""

import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import _segsnr_cases as cases  # noqa: E402
import _segsnr_ref as segref  # noqa: E402
import _wss_ref as ref  # noqa: E402
import oracle  # noqa: E402


def enhance(name, noisy, params):
    fn = oracle.advanced_mmse if name == "omlsa" else oracle.spectral_subtraction
    return fn(noisy, 16000, **params)


def worst_frame(clean, y, sr, lag, clip):
    """The kept frame whose f32 value is farthest from its f64 one, and the band
    of its test signal whose energy differs most between the two."""
    a = ref.frame_values(clean, y, sr, lag=lag, clip=clip)
    b = ref.frame_values(clean, y, sr, lag=lag, clip=clip, dtype=np.float32)
    k = int(np.argmax(np.abs(a - b)))
    W, hop, nfft, H = segref.constants(sr)
    x = np.asarray(clean, dtype=np.float64)
    yy = segref.test_signal(y, len(x), lag, clip)
    kept = [j for j in range(len(x) // hop - 4) if x[j * hop:j * hop + W].any()]
    f = yy[kept[k] * hop:kept[k] * hop + W] * segref.window(W)
    F = segref.filter_table(sr)
    e64 = ref.band_energies(f, F, nfft, H)
    e32 = ref.band_energies(f.astype(np.float32), F.astype(np.float32), nfft, H, np.float32)
    i = int(np.argmax(np.abs(e64 - e32)))
    return {"frame": kept[k], "value_f64": float(a[k]), "value_diff": float(abs(a[k] - b[k])),
            "band": i, "band_dB_f64": float(e64[i]), "band_dB_diff": float(abs(e64[i] - e32[i])),
            "frame_peak_dB": float(e64.max())}


def main():
    diffs, names, values = [], [], []
    worst_per_rate = {}
    keep = None
    for name, clean, y, sr, lag, clip in cases.all_cases(enhance):
        a = ref.wss(clean, y, sr, lag=lag, clip=clip)
        b = ref.wss(clean, y, sr, lag=lag, clip=clip, dtype=np.float32)
        if a != a:
            assert b != b, name
            continue
        d = abs(a - b)
        if not diffs or d > max(diffs):
            keep = (clean, y, sr, lag, clip)
        diffs.append(d)
        names.append(name)
        values.append(a)
        worst_per_rate[sr] = max(worst_per_rate.get(sr, 0.0), d)
    k = int(np.argmax(diffs))
    print(json.dumps({"cases": len(diffs), "wss_f32_vs_f64": diffs[k], "wss_case": names[k],
                      "wss_case_value": values[k], "worst_frame": worst_frame(*keep),
                      "worst_by_rate": {str(s): v for s, v in sorted(worst_per_rate.items())},
                      "median_diff": float(np.median(diffs)),
                      "score_min": float(np.min(values)), "score_median": float(np.median(values)),
                      "score_max": float(np.max(values)), "tol_wss": 8 * diffs[k]}))


if __name__ == "__main__":
    main()
