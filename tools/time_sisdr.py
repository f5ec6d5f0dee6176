"""Time of the device SI-SDR / SI-SIR / SI-SAR (cse_sisdr_cells) on 10-s cells (GPU box).

    timeout 300 python tools/time_sisdr.py [--cells N --pairs P --reps R] [--out FILE]

The cells are tools/bench_lpc.py's: noisy versions of P synthetic 10-s clean
signals with random gains (some beyond [-1, 1]: the clip runs) and lags.  Each
figure is the median of R launches timed with HIP events after a warm-up
launch, the kinds of launch alternating inside every repeat, one process:

  all      cse_sisdr_cells, the three scores
  sisdr    cse_sisdr_cells, SI-SDR alone (the interference is not read)
  stoi     cse_stoi_cells on the same cells
  lpc      cse_lpc_cells on the same cells
  copy     a device copy of the same waveform bytes: the HBM rate this box
           sustains (bytes read plus bytes written over the time)

Beside the times: the bytes a cell's workgroup loads (y as f32, the clean and
interference samples as f64), the bytes that must come from HBM (every y sample
once; the signals once per launch), and the time each takes at the copy's rate.
Writes the JSON (default profiles/sisdr_times.json) and prints it.
"""

import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from classical_speech_enhancement_amd.metrics import LpcPlan, SiSdrPlan, StoiPlan  # noqa: E402
from classical_speech_enhancement_amd.synth import make_pair  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=4096)
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sisdr_times.json"))
    a = ap.parse_args()
    pairs = [make_pair(100 + i, a.seconds) for i in range(a.pairs)]
    clean = torch.as_tensor(np.stack([c for c, _ in pairs])).cuda()
    noisy64 = torch.as_tensor(np.stack([n for _, n in pairs])).cuda()
    L = clean.shape[1]
    rng = np.random.default_rng(0)
    noisy = noisy64.to(torch.float32)
    sig = (np.arange(a.cells) % a.pairs).astype(np.int32)
    gains = torch.as_tensor(rng.uniform(0.3, 3.0, a.cells).astype(np.float32)).cuda()
    y = (noisy[torch.as_tensor(sig.astype(np.int64)).cuda()] * gains[:, None]).contiguous().view(-1)
    lag = rng.integers(-1600, 1601, a.cells).astype(np.int32)
    off_d = torch.as_tensor(np.arange(a.cells, dtype=np.int64) * L).cuda()
    sig_d, lag_d = torch.as_tensor(sig).cuda(), torch.as_tensor(lag).cuda()
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    SiSdrPlan(clean, noisy64)  # the first launch of the prepare kernel is not timed
    torch.cuda.synchronize()
    e0.record()
    pplan = SiSdrPlan(clean, noisy64)
    e1.record()
    torch.cuda.synchronize()
    prep_ms = e0.elapsed_time(e1)
    splan, dplan = StoiPlan(clean), LpcPlan(clean)
    dst = torch.empty_like(y)
    kinds = {
        "all": lambda: pplan.score_async(y, off_d, sig_d, lag=lag_d, clip=True),
        "sisdr": lambda: pplan.score_async(y, off_d, sig_d, lag=lag_d, clip=True, which="sisdr"),
        "stoi": lambda: splan.score_async(y, off_d, sig_d, lag=lag_d, clip=True),
        "lpc": lambda: dplan.score_async(y, off_d, sig_d, lag=lag_d, clip=True),
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
    q = outs["all"].cpu().numpy()
    assert not np.isnan(q).any() and np.isfinite(outs["stoi"].cpu().numpy()).all()
    alone = outs["sisdr"].cpu().numpy()
    assert np.array_equal(alone[:, 0], q[:, 0]) and np.isnan(alone[:, 1:]).all()
    # the additive identity on what the device returned (+inf: a part that is exactly zero)
    lhs = 10 ** (-q[:, 0] / 10)
    rhs = 10 ** (-q[:, 1] / 10) + 10 ** (-q[:, 2] / 10)
    assert np.abs(lhs - rhs).max() <= 1e-9 * lhs.max()
    q = np.where(np.isfinite(q), q, np.nan)
    med = {k: float(np.median(v)) for k, v in times.items()}
    wave_bytes = int(y.numel()) * 4
    copy_rate = 2 * wave_bytes / (med["copy"] / 1e3)   # bytes per second, read + write
    loaded = {"all": 20 * L, "sisdr": 12 * L}          # per cell: y f32 + s (+ v) f64
    hbm = {k: wave_bytes + a.pairs * L * (16 if k == "all" else 8) for k in loaded}
    line = {"what": "cse_sisdr_cells", "device": torch.cuda.get_device_name(0), "cells": a.cells,
            "clip_s": a.seconds, "signals": a.pairs, "reps": a.reps,
            "all_ms": med["all"], "sisdr_only_ms": med["sisdr"], "stoi_ms": med["stoi"],
            "lpc_ms": med["lpc"], "copy_ms": med["copy"], "prepare_ms": prep_ms,
            "copy_GBps_read_plus_write": copy_rate / 1e9,
            "all_over_stoi": med["all"] / med["stoi"], "all_over_lpc": med["all"] / med["lpc"],
            "cells_per_s": a.cells / (med["all"] / 1e3),
            "sisdr_mean_db": float(np.nanmean(q[:, 0])), "sisir_mean_db": float(np.nanmean(q[:, 1])),
            "sisar_mean_db": float(np.nanmean(q[:, 2]))}
    for k in loaded:
        t_loaded = 1e3 * a.cells * loaded[k] / copy_rate
        t_hbm = 1e3 * hbm[k] / copy_rate
        line[f"{k}_bytes_loaded_per_cell"] = loaded[k]
        line[f"{k}_loaded_GBps"] = a.cells * loaded[k] / (med[k] / 1e3) / 1e9
        line[f"{k}_floor_ms_loaded_bytes_at_copy_rate"] = t_loaded
        line[f"{k}_over_loaded_floor"] = med[k] / t_loaded
        line[f"{k}_hbm_bytes"] = hbm[k]
        line[f"{k}_floor_ms_hbm_bytes_at_copy_rate"] = t_hbm
        line[f"{k}_over_hbm_floor"] = med[k] / t_hbm
    line["ms_all"] = {k: [round(t, 4) for t in v] for k, v in times.items()}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w", encoding="utf-8") as f:
            json.dump(line, f, indent=1)
            f.write("\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
