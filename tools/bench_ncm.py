"""Time of the device NCM (cse_ncm_cells) on 10-s cells (GPU box).

    python tools/bench_ncm.py [--cells N --pairs P --reps R --sweep-pairs S] [--out FILE]

The cells are tools/bench_segsnr.py's: noisy versions of P synthetic 10-s clean
signals with random gains (some beyond [-1, 1]: the clip runs) and lags.  Each
figure is the median of R launches timed with HIP events after a warm-up
launch, the kinds of launch alternating inside every repeat, with the smallest
and the largest time beside it:

  ncm      cse_ncm_cells
  segsnr   cse_segsnr_cells, both scores, on the same cells in the same
           process: the same transform and band sums per frame
  csii     cse_csii_cells on the same cells: the other intelligibility measure
           on these frames
  stoi     cse_stoi_cells on the same cells: the sweep's default objective
  copy     a device copy of the same waveform bytes: the traffic floor

--sweep-pairs S (default 0: skipped) then times search.run_grid over S 10-s
pairs and the full grid, scored by STOI and by ncm (modulation=True) in turns,
wall clock around a device synchronisation, after one warm-up of each.

Writes the JSON (default profiles/ncm_times.json) and prints it.
"""

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from classical_speech_enhancement_amd import search  # noqa: E402
from classical_speech_enhancement_amd.metrics import (  # noqa: E402
    CsiiPlan, NcmPlan, SegSnrPlan, StoiPlan)
from classical_speech_enhancement_amd.synth import make_pair  # noqa: E402


def spread(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def time_sweep(n_pairs, seconds, reps):
    pairs = [make_pair(i, seconds) for i in range(n_pairs)]
    clean, noisy = [c for c, _ in pairs], [n for _, n in pairs]
    algorithms = list(search.ALGORITHM_GRIDS)
    specs = search.job_specs(n_pairs, algorithms, search.ALGORITHM_GRIDS)
    kinds = {"stoi": {}, "ncm": {"modulation": True}}
    times = {k: [] for k in kinds}
    tables = {}
    for rep in range(reps + 1):  # the first round warms up
        for k, kw in kinds.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tables[k], _ = search.run_grid(clean, noisy, specs, **kw)
            torch.cuda.synchronize()
            if rep:
                times[k].append((time.perf_counter() - t0) * 1e3)
    other = [c for c in range(search.NCOL) if c != 3]
    assert np.array_equal(tables["stoi"][:, other], tables["ncm"][:, other], equal_nan=True)
    col = tables["ncm"][:, 3]
    return {"pairs": n_pairs, "cells": len(specs), "reps": reps,
            "stoi_sweep_ms": spread(times["stoi"]), "ncm_sweep_ms": spread(times["ncm"]),
            "ncm_over_stoi_sweep": float(np.median(times["ncm"]) / np.median(times["stoi"])),
            "ncm_nan_cells": int(np.isnan(col).sum()), "ncm_mean": float(np.nanmean(col)),
            "ms_all": {k: [round(t, 2) for t in v] for k, v in times.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=4096)
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--sweep-pairs", type=int, default=0)
    ap.add_argument("--sweep-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ncm_times.json"))
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
    NcmPlan(clean)  # warm-up of the clean side
    torch.cuda.synchronize()
    e0.record()
    nplan = NcmPlan(clean)
    e1.record()
    torch.cuda.synchronize()
    prep_ms = e0.elapsed_time(e1)
    qplan, cplan, splan = SegSnrPlan(clean), CsiiPlan(clean), StoiPlan(clean)
    dst = torch.empty_like(y)
    kinds = {
        "ncm": lambda: nplan.score_async(y, off_d, sig_d, lag=lag_d, clip=True),
        "segsnr": lambda: qplan.score_async(y, off_d, sig_d, lag=lag_d, clip=True),
        "csii": lambda: cplan.score_async(y, off_d, sig_d, lag=lag_d, clip=True),
        "stoi": lambda: splan.score_async(y, off_d, sig_d, lag=lag_d, clip=True),
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
    w = outs["ncm"].cpu().numpy()
    assert np.isfinite(w).all() and (w >= 0).all() and (w <= 1).all()
    assert np.isfinite(outs["segsnr"].cpu().numpy()).all()
    assert np.isfinite(outs["stoi"].cpu().numpy()).all()
    med = {k: float(np.median(v)) for k, v in times.items()}
    nbytes = int(y.numel()) * 4
    line = {"what": "cse_ncm_cells", "device": torch.cuda.get_device_name(0), "cells": a.cells,
            "clip_s": a.seconds, "frames_per_cell": int(L // 120 - 4), "reps": a.reps,
            "ncm_ms": spread(times["ncm"]), "segsnr_both_ms": spread(times["segsnr"]),
            "csii_ms": spread(times["csii"]), "stoi_ms": spread(times["stoi"]),
            "copy_ms": spread(times["copy"]),
            "ncm_over_segsnr_both": med["ncm"] / med["segsnr"],
            "ncm_over_csii": med["ncm"] / med["csii"],
            "ncm_over_stoi": med["ncm"] / med["stoi"],
            "ncm_over_copy": med["ncm"] / med["copy"], "waveform_bytes": nbytes,
            "prepare_ms": prep_ms, "workspace_bytes": int(nplan.ws.numel()),
            "cells_per_s": a.cells / (med["ncm"] / 1e3),
            "ncm_mean": float(w[:, 0].mean()), "ncm_bif_mean": float(w[:, 1].mean()),
            "ms_all": {k: [round(t, 4) for t in v] for k, v in times.items()}}
    if a.sweep_pairs > 0:
        del outs, y, dst
        torch.cuda.empty_cache()
        line["sweep"] = time_sweep(a.sweep_pairs, a.seconds, a.sweep_reps)
    if a.out:
        with open(a.out, "w", encoding="utf-8") as f:
            json.dump(line, f, indent=1)
            f.write("\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
