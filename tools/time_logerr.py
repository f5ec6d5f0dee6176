"""Time of the noise-PSD LogErr kernels (include/cse_logerr.h) at the bench's shape (GPU box).

    timeout 600 python tools/time_logerr.py [--pairs P --rows K --reps R --inner I] [--out FILE]

P synthetic 10-s pairs at n_fft 512 / hop 128 (P x 1,251 frames x 257 bins).
The estimates are the reference PSD times a random factor of +-9.5 dB per
element, K of them per signal.  Each figure is the median over R repeats of the
time of I back-to-back launches, timed with HIP events after a warm-up, divided
by I; the kinds of launch alternate inside every repeat, one process:

  reference   cse_logerr_reference on the P signals
  rows_1      cse_logerr_rows, one row per signal, totals only
  rows_1f     the same with the per-frame outputs
  rows_K      cse_logerr_rows, K rows per signal in one launch, totals only
  torch_1     the same score of one row per signal as torch operations
              (torch.where, log10, sums) on the same device
  torch_K     that formulation on K rows per signal
  copy        a device copy of R: the HBM rate this box sustains

Beside the times: the bytes each launch has to move once (R as f64, every N
as f32) and the time they take at the copy's rate.  The device's scores are
checked against torch's (1e-9 dB).  Writes the JSON (default
profiles/logerr_times.json) and prints it.
"""

import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from classical_speech_enhancement_amd import _lib  # noqa: E402
from classical_speech_enhancement_amd.engine import _ptr, _stream  # noqa: E402
from classical_speech_enhancement_amd.metrics import NoiseErrPlan  # noqa: E402
from classical_speech_enhancement_amd.synth import make_pair  # noqa: E402

FLOOR = 1e-12


def torch_score(R, N):
    """R [S, T, B] f64, N [K, S, T, B] f32 -> (over, under) [K, S] f64."""
    floor = torch.tensor(FLOOR, dtype=torch.float64, device=R.device)
    zero = torch.zeros((), dtype=torch.float64, device=R.device)
    Rf = torch.where(R < floor, floor, R)
    Nd = N.double()
    Nf = torch.where(Nd < floor, floor, Nd)
    d = 10.0 * torch.log10(Rf / Nf)
    o = torch.where(d > 0, zero, -d)
    u = torch.where(d < 0, zero, d)
    n = R.shape[1] * R.shape[2]
    return o.sum(-1).sum(-1) / n, u.sum(-1).sum(-1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=100)
    ap.add_argument("--rows", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "logerr_times.json"))
    a = ap.parse_args()
    lib = _lib.load()
    pairs = [make_pair(100 + i, a.seconds) for i in range(a.pairs)]
    clean = torch.as_tensor(np.stack([c for c, _ in pairs])).cuda()
    noisy = torch.as_tensor(np.stack([n for _, n in pairs])).cuda()
    plan = NoiseErrPlan(clean, noisy, 512, 128)
    S, T, B, K = plan.S, plan.T, plan.B, a.rows
    R = plan.R
    Pv = torch.empty_like(R).copy_(R)  # any positive power of the same shape
    gen = torch.Generator(device="cuda").manual_seed(0)
    fac = 10.0 ** (torch.rand((K, S, T, B), device="cuda", generator=gen) * 1.9 - 0.95)
    N = (R[None] * fac).float().contiguous()
    del fac
    dev = R.device
    sig1 = torch.arange(S, dtype=torch.int32, device=dev)
    sigK = sig1.repeat(K)
    off = torch.arange(K * S, dtype=torch.int64, device=dev) * (T * B)
    st = torch.full((K * S,), B, dtype=torch.int64, device=dev)
    scratch = torch.empty(max(int(lib.cse_logerr_scratch_bytes(K * S, T)), 1), dtype=torch.uint8,
                          device=dev)
    out = torch.empty((2, K * S), dtype=torch.float64, device=dev)
    fr = torch.empty((2, S, T), dtype=torch.float64, device=dev)
    Rout = torch.empty_like(R)
    dst = torch.empty_like(R)

    def rows(n, sig, frames):
        _lib.check(lib.cse_logerr_rows(
            _ptr(R), S, T, B, _ptr(N), _ptr(off), _ptr(st), _ptr(sig), n, ctypes.byref(plan.prm),
            _ptr(scratch), _ptr(out[0]), _ptr(out[1]), _ptr(fr[0]) if frames else None,
            _ptr(fr[1]) if frames else None, _stream()), "cse_logerr_rows")

    def reference():
        _lib.check(lib.cse_logerr_reference(_ptr(Pv), S, T, B, 0.9, _ptr(Rout), _stream()),
                   "cse_logerr_reference")

    kinds = {
        "reference": reference,
        "rows_1": lambda: rows(S, sig1, False),
        "rows_1f": lambda: rows(S, sig1, True),
        "rows_K": lambda: rows(K * S, sigK, False),
        "torch_1": lambda: torch_score(R, N[:1]),
        "torch_K": lambda: torch_score(R, N),
        "copy": lambda: dst.copy_(R),
    }
    # the device's scores against torch's, which is also the warm-up of every kind
    want = torch_score(R, N)
    rows(K * S, sigK, False)
    got = out.clone().view(2, K, S)
    torch.cuda.synchronize()
    worst = max(float((got[0] - want[0]).abs().max()), float((got[1] - want[1]).abs().max()))
    assert worst <= 1e-9, worst
    rows(S, sig1, False)
    one = out[:, :S].clone()
    assert torch.equal(one, got[:, 0])  # a row alone: the bits it has in the launch of K S rows
    del want
    for fn in kinds.values():
        fn()
    torch.cuda.synchronize()
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    times = {k: [] for k in kinds}
    for _ in range(a.reps):
        for k, fn in kinds.items():
            e0.record()
            for _ in range(a.inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / a.inner)
    med = {k: float(np.median(v)) for k, v in times.items()}
    r_bytes, n_bytes = S * T * B * 8, S * T * B * 4
    copy_rate = 2 * r_bytes / (med["copy"] / 1e3)  # bytes per second, read + write
    line = {"what": "cse_logerr_reference / cse_logerr_rows",
            "device": torch.cuda.get_device_name(0), "signals": S, "frames": T, "bins": B,
            "rows_per_signal": K, "reps": a.reps, "launches_per_timing": a.inner,
            "elements_per_estimate": S * T * B,
            "worst_difference_to_torch_db": worst,
            "copy_GBps_read_plus_write": copy_rate / 1e9}
    for k, v in med.items():
        line[f"{k}_ms"] = v
    line["rows_K_over_K_rows_1"] = med["rows_K"] / (K * med["rows_1"])
    line["rows_1_over_torch_1"] = med["rows_1"] / med["torch_1"]
    line["rows_K_over_torch_K"] = med["rows_K"] / med["torch_K"]
    for k, nbytes in (("reference", 2 * r_bytes), ("rows_1", r_bytes + n_bytes),
                      ("rows_K", r_bytes + K * n_bytes)):
        floor_ms = 1e3 * nbytes / copy_rate
        line[f"{k}_bytes"] = nbytes
        line[f"{k}_floor_ms_bytes_at_copy_rate"] = floor_ms
        line[f"{k}_over_floor"] = med[k] / floor_ms
    line["rows_1_elements_per_s"] = S * T * B / (med["rows_1"] / 1e3)
    line["rows_K_elements_per_s"] = K * S * T * B / (med["rows_K"] / 1e3)
    line["ms_all"] = {k: [round(t, 4) for t in v] for k, v in times.items()}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w", encoding="utf-8") as f:
            json.dump(line, f, indent=1)
            f.write("\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
