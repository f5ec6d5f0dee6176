"""The measured tolerance of tests/test_gpu_lpc.py (CPU only).

    python tools/lpc_tolerance.py

Walks the inputs of the GPU file (tests/_lpc_cases.py: the launches, the speech
fixture, the edge, long, silent and zero cases, and the Python layer's cells
with the grid cells at lag 0; the enhanced waveforms made by the oracle's
plugins in place of the device's) and prints, per score, the worst

    |ref(device precision) - ref(f64)|

of tests/_lpc_ref.py, where the device precision is the one include/cse_lpc.h
states: fp64 throughout, a frame's two values stored as f32 before the n95
smallest are averaged in fp64.  Beside it: the worst |ref(f64) -
ref(longdouble)|, the specification's own rounding (how far another summation
order may move an fp64 result), and the all-f32 evaluation the header rules
out.  The test tolerance is 8 times the first figure and may be no looser than
1e-6 (LLR) and 1e-5 (CEP).
"""

import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import _lpc_cases as cases  # noqa: E402
import _lpc_ref as ref  # noqa: E402
import oracle  # noqa: E402

NAMES = ("llr", "cep")


def enhance(name, noisy, params):
    fn = oracle.advanced_mmse if name == "omlsa" else oracle.spectral_subtraction
    return fn(noisy, 16000, **params)


def main():
    kinds = ("device", "longdouble", "f32")
    worst = {k: [0.0, 0.0] for k in kinds}
    where = {k: ["", ""] for k in kinds}
    n = 0
    for name, clean, y, sr, lag, clip in cases.all_cases(enhance):
        a = ref.scores(clean, y, sr, lag=lag, clip=clip)
        got = {"device": ref.scores(clean, y, sr, lag=lag, clip=clip, store=np.float32),
               "longdouble": ref.scores(clean, y, sr, lag=lag, clip=clip, dtype=np.longdouble,
                                        exact=True),
               "f32": ref.scores(clean, y, sr, lag=lag, clip=clip, dtype=np.float32)}
        if a[0] != a[0]:
            assert all(b[0] != b[0] and b[1] != b[1] for b in got.values()), name
            continue
        n += 1
        for kind, b in got.items():
            for k in range(2):
                d = float(abs(np.longdouble(a[k]) - b[k]))
                if d > worst[kind][k] or d != d:
                    worst[kind][k], where[kind][k] = d, name
    out = {"cases": n}
    for k, s in enumerate(NAMES):
        out[f"{s}_device_vs_f64"] = worst["device"][k]
        out[f"{s}_device_case"] = where["device"][k]
        out[f"{s}_f64_vs_longdouble"] = worst["longdouble"][k]
        out[f"{s}_longdouble_case"] = where["longdouble"][k]
        out[f"{s}_f32_vs_f64"] = worst["f32"][k]
        out[f"tol_{s}"] = 8 * worst["device"][k]
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
