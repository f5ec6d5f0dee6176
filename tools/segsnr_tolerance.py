"""The measured tolerance of tests/test_gpu_segsnr.py (CPU only).

    python tools/segsnr_tolerance.py

Walks the inputs of the GPU file (tests/_segsnr_cases.py: the launches, the
edge and silent cases, and the Python layer's cells with the grid cells at lag
0; the enhanced waveforms made by the oracle's plugins in place of the
device's) and prints
max |ref(f32) - ref(f64)| of tests/_segsnr_ref.py for each score.  The test
tolerance is 8 times that figure (the factor covers a different FFT
factorisation and summation order from scipy's), and may be no looser than
1e-4 dB (segSNR) and 1e-3 dB (fwSegSNR).
"""

import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import _segsnr_cases as cases  # noqa: E402
import _segsnr_ref as ref  # noqa: E402
import oracle  # noqa: E402


def enhance(name, noisy, params):
    fn = oracle.advanced_mmse if name == "omlsa" else oracle.spectral_subtraction
    return fn(noisy, 16000, **params)


def main():
    worst = [0.0, 0.0]
    where = ["", ""]
    n = 0
    for name, clean, y, sr, lag, clip in cases.all_cases(enhance):
        a = ref.scores(clean, y, sr, lag=lag, clip=clip)
        b = ref.scores(clean, y, sr, lag=lag, clip=clip, dtype=np.float32)
        if a[0] != a[0]:
            assert b[0] != b[0] and b[1] != b[1], name
            continue
        n += 1
        for k in range(2):
            d = abs(a[k] - b[k])
            if d > worst[k]:
                worst[k], where[k] = d, name
    print(json.dumps({"cases": n, "segsnr_f32_vs_f64_dB": worst[0], "segsnr_case": where[0],
                      "fwsegsnr_f32_vs_f64_dB": worst[1], "fwsegsnr_case": where[1],
                      "tol_segsnr": 8 * worst[0], "tol_fwsegsnr": 8 * worst[1]}))


if __name__ == "__main__":
    main()
