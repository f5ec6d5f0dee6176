"""Time of the device LLR / LPC cepstrum distance (cse_lpc_cells) on 10-s cells (GPU box).

    python tools/bench_lpc.py [--cells N --pairs P --reps R] [--out FILE]

The cells are tools/bench_stoi.py's: noisy versions of P synthetic 10-s clean
signals with random gains (some beyond [-1, 1]: the clip runs) and lags.  Each
figure is the median of R launches timed with HIP events after a warm-up
launch, the four kinds of launch alternating inside every repeat:

  both     cse_lpc_cells, both scores
  llr      cse_lpc_cells with a NULL cepstrum output (no cepstrum recursion)
  stoi     cse_stoi_cells on the same cells, in the same process
  copy     a device copy of the same waveform bytes: the traffic floor

Writes the JSON (default profiles/lpc_times.json) and prints it.
"""

import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from classical_speech_enhancement_amd.metrics import LpcPlan, StoiPlan  # noqa: E402
from classical_speech_enhancement_amd.synth import make_pair  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=4096)
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lpc_times.json"))
    a = ap.parse_args()
    pairs = [make_pair(100 + i, a.seconds) for i in range(a.pairs)]
    clean = torch.as_tensor(np.stack([c for c, _ in pairs])).cuda()
    L = clean.shape[1]
    rng = np.random.default_rng(0)
    noisy = torch.as_tensor(np.stack([n for _, n in pairs]).astype(np.float32)).cuda()
    sig = (np.arange(a.cells) % a.pairs).astype(np.int32)
    gains = torch.as_tensor(rng.uniform(0.3, 3.0, a.cells).astype(np.float32)).cuda()
    y = (noisy[torch.as_tensor(sig.astype(np.int64)).cuda()] * gains[:, None]).contiguous().view(-1)
    lag = rng.integers(-1600, 1601, a.cells).astype(np.int32)
    off_d = torch.as_tensor(np.arange(a.cells, dtype=np.int64) * L).cuda()
    sig_d, lag_d = torch.as_tensor(sig).cuda(), torch.as_tensor(lag).cuda()
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    dplan = LpcPlan(clean)
    e1.record()
    torch.cuda.synchronize()
    prep_ms = e0.elapsed_time(e1)
    splan = StoiPlan(clean)
    dst = torch.empty_like(y)
    kinds = {
        "both": lambda: dplan.score_async(y, off_d, sig_d, lag=lag_d, clip=True),
        "llr": lambda: dplan.score_async(y, off_d, sig_d, lag=lag_d, clip=True, which="llr"),
        "stoi": lambda: splan.score_async(y, off_d, sig_d, lag=lag_d, clip=True),
        "copy": lambda: dst.copy_(y),
    }
    outs = {k: fn() for k, fn in kinds.items()}  # warm-up (scratch allocation)
    torch.cuda.synchronize()
    times = {k: [] for k in kinds}
    for _ in range(a.reps):
        for k, fn in kinds.items():
            e0.record()
            outs[k] = fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1))
    q = outs["both"].cpu().numpy()
    assert np.isfinite(q).all() and np.isfinite(outs["stoi"].cpu().numpy()).all()
    assert (q[:, 0] >= 0).all() and (q[:, 0] <= 2).all() and (q[:, 1] <= 10).all()
    llr_alone = outs["llr"].cpu().numpy()
    assert np.array_equal(llr_alone[:, 0], q[:, 0]) and np.isnan(llr_alone[:, 1]).all()
    med = {k: float(np.median(v)) for k, v in times.items()}
    nbytes = int(y.numel()) * 4
    J = int(L // 120 - 4)
    line = {"what": "cse_lpc_cells", "device": torch.cuda.get_device_name(0), "cells": a.cells,
            "clip_s": a.seconds, "frames_per_cell": J, "reps": a.reps,
            "both_ms": med["both"], "llr_only_ms": med["llr"], "stoi_ms": med["stoi"],
            "copy_ms": med["copy"], "both_over_stoi": med["both"] / med["stoi"],
            "both_over_copy": med["both"] / med["copy"], "waveform_bytes": nbytes,
            "both_us_per_cell": 1e3 * med["both"] / a.cells,
            "stoi_us_per_cell": 1e3 * med["stoi"] / a.cells,
            "both_GBps_of_waveform": nbytes / med["both"] / 1e6,
            "prepare_ms": prep_ms, "cells_per_s": a.cells / (med["both"] / 1e3),
            "llr_mean": float(q[:, 0].mean()), "cep_mean": float(q[:, 1].mean()),
            "ms_all": {k: [round(t, 4) for t in v] for k, v in times.items()}}
    if a.out:
        with open(a.out, "w", encoding="utf-8") as f:
            json.dump(line, f, indent=1)
            f.write("\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
