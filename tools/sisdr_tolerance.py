"""The measured tolerance of tests/test_gpu_sisdr.py (CPU only).

    python tools/sisdr_tolerance.py

include/cse_sisdr.h leaves the device one freedom, the order of the fp64 sums.
This walks the inputs of the GPU file (tests/_sisdr_cases.py: every length and
lag, the 37-cell launch, the clip, DC, no-interference and zero cases, the two
10-s plugin cells and the Python layer's cells with the grid cells at lag 0;
the enhanced waveforms made by the oracle's plugins in place of the device's),
evaluates the restatement (tests/_sisdr_ref.py) with each of its summation
orders (fsum, sequential, reversed, blocks of 64 then a tree, numpy pairwise)
and prints, per score, the largest spread in dB over the cases compared by
value.  The test tolerance is 8 times that spread (margin for a reduction shape
not tried here) and may be no looser than 1e-6 dB.  A case with a score that
is not finite is compared by class; the orders must agree on the class.
"""

import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import _sisdr_cases as cases  # noqa: E402
import _sisdr_ref as ref  # noqa: E402
import oracle  # noqa: E402


def enhance(name, noisy, params):
    fn = oracle.advanced_mmse if name == "omlsa" else oracle.spectral_subtraction
    return fn(noisy, 16000, **params)


def main():
    worst = [0.0, 0.0, 0.0]
    where = ["", "", ""]
    lo, hi = [np.inf] * 3, [-np.inf] * 3
    n_value = n_class = 0
    for case in cases.all_cases(enhance):
        base, by_value = cases.checked(case)
        got = np.array([cases.want(case, order) for order in ref.ORDERS])
        for k in range(3):
            if not by_value[k]:
                n_class += 1
                assert all(ref.same_class(g, base[k]) for g in got[:, k]), (case[0], got[:, k])
                continue
            n_value += 1
            lo[k], hi[k] = min(lo[k], base[k]), max(hi[k], base[k])
            spread = float(got[:, k].max() - got[:, k].min())
            if spread > worst[k] or spread != spread:
                worst[k], where[k] = spread, case[0]
    out = {"orders": list(ref.ORDERS), "scores_by_value": n_value, "scores_by_class": n_class}
    for k, s in enumerate(ref.NAMES):
        out[f"{s}_spread_db"] = worst[k]
        out[f"{s}_spread_case"] = where[k]
        out[f"{s}_range_db"] = [lo[k], hi[k]]
        out[f"tol_{s}"] = 8 * worst[k]
    out["tol"] = 8 * max(worst)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
