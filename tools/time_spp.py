"""Kernel time of cse_noise_spp at the sweep's shapes (100 signals of 10 s:
1,251 frames x 257 bins at n_fft 512 / hop 128, 626 x 513 at 1024 / 256), HIP
events, median of R runs after warm-up, in one process beside
  - cse_noise_mcra at the same shape and input,
  - cse_noise_median + cse_noise_min_tracking_med (one eps), the chain that
    yields min_tracking's raw rows,
  - a device-to-device copy with the same traffic (P read + N written = 12
    bytes per element: 6 bytes per element copied).
One signal of each shape is compared with the numpy restatement
(tests/_spp_ref.py): the number of unequal f32 values and the largest relative
difference in units of 2^-23.  Prints one JSON line; --out writes it.

    python tools/time_spp.py [--signals 100 --reps 25 --out profiles/spp_times.json]
    python tools/time_spp.py --spp-lib other.so   # A/B: cse_noise_spp from another build
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = ((1251, 257), (626, 513))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--signals", type=int, default=100)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--spp-lib", action="append", default=[])
    ap.add_argument("--out")
    a = ap.parse_args()
    import _spp_ref
    from classical_speech_enhancement_amd import _lib
    from classical_speech_enhancement_amd.engine import Engine, _ptr, _stream
    eng = Engine()
    lib = eng.lib
    S = a.signals

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), float(min(ms)), float(max(ms))

    variants = {"cse_noise_spp": lib.cse_noise_spp}
    for path in a.spp_lib:
        other = ctypes.CDLL(os.path.abspath(path))
        other.cse_noise_spp.restype = ctypes.c_int
        other.cse_noise_spp.argtypes = lib.cse_noise_spp.argtypes
        variants[os.path.basename(path)] = other.cse_noise_spp
    prm = _lib.SppParams()
    lib.cse_spp_default_params(ctypes.byref(prm))
    mprm = _lib.McraParams()
    lib.cse_mcra_default_params(ctypes.byref(mprm))
    out = {"signals": S, "reps": a.reps, "device": torch.cuda.get_device_name(0), "shapes": {}}
    for T, B in SHAPES:
        gen = torch.Generator(device="cuda").manual_seed(T)
        # exponential power with level changes up and down, so the guard fires
        P = -torch.log(torch.rand((S, T, B), dtype=torch.float64, device="cuda", generator=gen)
                       .clamp_min(1e-300))
        P[:, T // 3:T // 2] *= 100.0
        P[:, 3 * T // 4:] *= 30.0
        N = torch.empty((S, T, B), dtype=torch.float32, device="cuda")
        n = S * T * B
        row = {"bytes_read_written": n * 12}
        for name, fn in variants.items():
            def run(fn=fn):
                _lib.check(fn(_ptr(P), S, T, B, ctypes.byref(prm), 1e-10, _ptr(N), _stream()),
                           name)
            med, lo, hi = timed(run)
            st = {}
            ref = _spp_ref.spp(P[0].cpu().numpy(), 1e-10, stats=st)
            got = N[0].cpu().numpy()
            row[name] = {"ms": med, "min_ms": lo, "max_ms": hi,
                         "gb_per_s": n * 12 / med / 1e6,
                         "unequal_to_restatement": int((got != ref).sum()),
                         "compared": int(ref.size),
                         "max_rel_error_in_f32_steps":
                             float(np.max(np.abs(got.astype(np.float64) - ref) / ref) * 2.0 ** 23),
                         "clamped_share": st["clamped_share"], "capped": st["capped"],
                         "margin": st["margin"]}
        med_d = torch.empty((S, B), dtype=torch.float64, device="cuda")
        ws = torch.empty(int(lib.cse_noise_workspace_bytes(S, T, B)), dtype=torch.uint8,
                         device="cuda")

        def mcra():
            _lib.check(lib.cse_noise_mcra(_ptr(P), S, T, B, ctypes.byref(mprm), 1e-10, _ptr(N),
                                          _stream()), "mcra")

        def median():
            _lib.check(lib.cse_noise_median(_ptr(P), S, T, B, _ptr(med_d), _stream()), "median")

        def min_tracking():
            _lib.check(lib.cse_noise_min_tracking_med(_ptr(P), _ptr(med_d), S, T, B, 1e-10, _ptr(N),
                                                      0.0, None, _ptr(ws), _stream()), "min_tracking")

        def chain():
            median()
            min_tracking()
        src = torch.empty(n * 6, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        for name, fn in (("cse_noise_mcra", mcra), ("cse_noise_median", median),
                         ("cse_noise_min_tracking_med", min_tracking),
                         ("min_tracking_chain", chain),
                         ("copy_same_traffic", lambda: dst.copy_(src))):
            med, lo, hi = timed(fn)
            row[name] = {"ms": med, "min_ms": lo, "max_ms": hi}
        row["copy_same_traffic"]["gb_per_s"] = n * 12 / row["copy_same_traffic"]["ms"] / 1e6
        row["spp_share_of_copy_rate"] = row["copy_same_traffic"]["ms"] / row["cse_noise_spp"]["ms"]
        # the dependent chain: ns per frame of one wave (every wave runs all T frames)
        row["spp_ns_per_frame"] = row["cse_noise_spp"]["ms"] * 1e6 / T
        out["shapes"][f"{S}x{T}x{B}"] = row
        del P, N, src, dst, ws
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
