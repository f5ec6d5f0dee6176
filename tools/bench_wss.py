"""Time of the device WSS (cse_wss_cells) on 10-s cells (GPU box).

    python tools/bench_wss.py [--cells N --pairs P --reps R] [--out FILE]

The cells are tools/bench_segsnr.py's: noisy versions of P synthetic 10-s clean
signals with random gains (some beyond [-1, 1]: the clip runs) and lags.  Each
figure is the median of R launches timed with HIP events after a warm-up
launch, the kinds of launch alternating inside every repeat:

  wss      cse_wss_cells
  both     cse_segsnr_cells, both scores, on the same cells in the same
           process: the kernel with the same transform and band sums per frame
  copy     a device copy of the same waveform bytes: the traffic floor

Writes the JSON (default profiles/wss_times.json) and prints it.
"""

import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from classical_speech_enhancement_amd.metrics import SegSnrPlan, WssPlan  # noqa: E402
from classical_speech_enhancement_amd.synth import make_pair  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=4096)
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "wss_times.json"))
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
    wplan = WssPlan(clean)
    e1.record()
    torch.cuda.synchronize()
    prep_ms = e0.elapsed_time(e1)
    qplan = SegSnrPlan(clean)
    dst = torch.empty_like(y)
    kinds = {
        "wss": lambda: wplan.score_async(y, off_d, sig_d, lag=lag_d, clip=True),
        "both": lambda: qplan.score_async(y, off_d, sig_d, lag=lag_d, clip=True),
        "copy": lambda: dst.copy_(y),
    }
    outs = {k: fn() for k, fn in kinds.items()}  # warm-up
    torch.cuda.synchronize()
    times = {k: [] for k in kinds}
    for _ in range(a.reps):
        for k, fn in kinds.items():
            e0.record()
            outs[k] = fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1))
    w = outs["wss"].cpu().numpy()
    assert np.isfinite(w).all() and (w >= 0).all()
    assert np.isfinite(outs["both"].cpu().numpy()).all()
    med = {k: float(np.median(v)) for k, v in times.items()}
    nbytes = int(y.numel()) * 4
    line = {"what": "cse_wss_cells", "device": torch.cuda.get_device_name(0), "cells": a.cells,
            "clip_s": a.seconds, "frames_per_cell": int(L // 120 - 4), "reps": a.reps,
            "wss_ms": med["wss"], "segsnr_both_ms": med["both"], "copy_ms": med["copy"],
            "wss_over_segsnr_both": med["wss"] / med["both"],
            "wss_over_copy": med["wss"] / med["copy"], "waveform_bytes": nbytes,
            "wss_GBps_of_waveform": nbytes / med["wss"] / 1e6,
            "prepare_ms": prep_ms, "cells_per_s": a.cells / (med["wss"] / 1e3),
            "wss_mean": float(w.mean()),
            "ms_all": {k: [round(t, 4) for t in v] for k, v in times.items()}}
    if a.out:
        with open(a.out, "w", encoding="utf-8") as f:
            json.dump(line, f, indent=1)
            f.write("\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
