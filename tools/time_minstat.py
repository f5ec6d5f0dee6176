"""Kernel time of cse_noise_minstat (100 signals of 10 s: 1,251 frames x 257
bins at n_fft 512 / hop 128, 626 x 513 at 1024 / 256, 157 x 2049 at 4096 /
1024), HIP events after a warm-up, median of R runs, in one process and
alternating with cse_noise_mcra and cse_noise_spp at the same shape and input,
and with one signal instead of 100 (the serial chain of a single workgroup).
One signal of each shape is compared with the numpy restatement
(tests/_minstat_ref.py).  Prints one JSON line; --out writes it.

    python tools/time_minstat.py [--signals 100 --reps 7 --out profiles/minstat_times.json]
    python tools/time_minstat.py --minstat-lib other.so   # A/B: the entry point of another build
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

SHAPES = ((1251, 257), (626, 513), (157, 2049))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--signals", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--minstat-lib", action="append", default=[])
    ap.add_argument("--out")
    a = ap.parse_args()
    import _minstat_ref
    from classical_speech_enhancement_amd import _lib
    from classical_speech_enhancement_amd.engine import Engine, _ptr, _stream
    eng = Engine()
    lib = eng.lib
    S = a.signals
    prm = _lib.MinstatParams()
    lib.cse_minstat_default_params(ctypes.byref(prm))
    mprm = _lib.McraParams()
    lib.cse_mcra_default_params(ctypes.byref(mprm))
    sprm = _lib.SppParams()
    lib.cse_spp_default_params(ctypes.byref(sprm))
    others = {}
    for path in a.minstat_lib:
        other = ctypes.CDLL(os.path.abspath(path))
        other.cse_noise_minstat.restype = ctypes.c_int
        other.cse_noise_minstat.argtypes = lib.cse_noise_minstat.argtypes
        others[os.path.basename(path)] = other.cse_noise_minstat

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    out = {"signals": S, "reps": a.reps, "device": torch.cuda.get_device_name(0), "shapes": {}}
    for T, B in SHAPES:
        gen = torch.Generator(device="cuda").manual_seed(T)
        # exponential power with level changes up and down
        P = -torch.log(torch.rand((S, T, B), dtype=torch.float64, device="cuda", generator=gen)
                       .clamp_min(1e-300))
        P[:, T // 3:T // 2] *= 100.0
        P[:, 3 * T // 4:] *= 30.0
        N = torch.empty((S, T, B), dtype=torch.float32, device="cuda")

        def call(fn, p, n_sig, name):
            return lambda: _lib.check(fn(_ptr(P), n_sig, T, B, ctypes.byref(p), 1e-10, _ptr(N),
                                         _stream()), name)
        fns = {"cse_noise_minstat": call(lib.cse_noise_minstat, prm, S, "minstat"),
               "cse_noise_mcra": call(lib.cse_noise_mcra, mprm, S, "mcra"),
               "cse_noise_spp": call(lib.cse_noise_spp, sprm, S, "spp"),
               "cse_noise_minstat_one_signal": call(lib.cse_noise_minstat, prm, 1, "minstat")}
        for name, fn in others.items():
            def probe(fn=fn):  # a build without this shape's instantiation is left out
                return fn(_ptr(P), 1, T, B, ctypes.byref(prm), 1e-10, _ptr(N), _stream())
            if probe() == 0:
                fns[name] = call(fn, prm, S, name)
        torch.cuda.synchronize()
        for _ in range(3):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in fns}
        for _ in range(a.reps):  # alternating
            for k, fn in fns.items():
                ms[k].append(once(fn))
        row = {k: {"ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v))}
               for k, v in ms.items()}
        fns["cse_noise_minstat"]()
        got = N[0].cpu().numpy()
        st = {}
        ref = _minstat_ref.minstat(P[0].cpu().numpy(), 1e-10, stats=st)
        row["cse_noise_minstat"].update(
            unequal_to_restatement=int((got != ref).sum()), compared=int(ref.size),
            max_rel_error_in_f32_steps=float(np.max(np.abs(got.astype(np.float64) - ref) / ref)
                                             * 2.0 ** 23), **st)
        row["minstat_ns_per_frame"] = row["cse_noise_minstat"]["ms"] * 1e6 / T
        row["minstat_over_mcra"] = row["cse_noise_minstat"]["ms"] / row["cse_noise_mcra"]["ms"]
        row["minstat_over_spp"] = row["cse_noise_minstat"]["ms"] / row["cse_noise_spp"]["ms"]
        out["shapes"][f"{S}x{T}x{B}"] = row
        del P, N
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
