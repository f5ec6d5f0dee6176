"""Kernel time of cse_noise_imcra (100 signals of 10 s: 1,251 frames x 257 bins
at n_fft 512 / hop 128), HIP events after a warm-up, median of R runs, in one
process and alternating with cse_noise_mcra, cse_noise_spp and
cse_noise_minstat on the same P, all with default parameters, and with one
signal instead of 100 (five waves: the serial chain alone).  One signal is
compared with the numpy restatement (tests/_imcra_ref.py).  Prints one JSON
line; --out writes it.  --build prints the kernel's register, LDS and scratch
figures from a compile of csrc/cse_imcra.hip (needs hipcc, no GPU); --figures
takes that line from a file into the result, so that the timed run compiles
nothing.

    python tools/time_imcra.py --build > figures.json
    python tools/time_imcra.py --figures figures.json --out profiles/imcra_times.json
    python tools/time_imcra.py --imcra-lib other.so   # A/B: the entry point of another build
"""
import argparse
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

T, B = 1251, 257


def build_figures():
    """VGPR, AGPR, SGPR, scratch and static LDS of imcra_kernel, as the compiler
    reports them; the dynamic LDS is 2 U 64 doubles (8 KB at U = 8)."""
    src = os.path.join(ROOT, "classical_speech_enhancement_amd", "csrc", "cse_imcra.hip")
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize", "-fPIC",
           "-I" + os.path.join(ROOT, "include"), "-Rpass-analysis=kernel-resource-usage",
           "--cuda-device-only", "-c", src, "-o", os.devnull]
    text = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    text = text[text.index("imcra_kernel"):]
    grab = lambda key: int(re.search(re.escape(key) + r":\s*(\d+)", text).group(1))  # noqa: E731
    return {"vgprs": grab("VGPRs"), "agprs": grab("AGPRs"), "sgprs": grab("TotalSGPRs"),
            "scratch_bytes_per_lane": grab("ScratchSize [bytes/lane]"),
            "vgpr_spills": grab("VGPRs Spill"), "static_lds_bytes": grab("LDS Size [bytes/block]"),
            "dynamic_lds_bytes_at_defaults": 2 * 8 * 64 * 8,
            "waves_per_simd": grab("Occupancy [waves/SIMD]")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--signals", type=int, default=100)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--imcra-lib", action="append", default=[])
    ap.add_argument("--build", action="store_true")
    ap.add_argument("--figures")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.build:
        print(json.dumps(build_figures()))
        return
    import torch

    import _imcra_ref
    from classical_speech_enhancement_amd import _lib
    from classical_speech_enhancement_amd.engine import Engine, _ptr, _stream
    eng = Engine()
    lib = eng.lib
    S = a.signals
    prms = {}
    for name, cls in (("imcra", _lib.ImcraParams), ("mcra", _lib.McraParams),
                      ("spp", _lib.SppParams), ("minstat", _lib.MinstatParams)):
        prms[name] = cls()
        getattr(lib, f"cse_{name}_default_params")(ctypes.byref(prms[name]))
    others = {}
    for path in a.imcra_lib:
        other = ctypes.CDLL(os.path.abspath(path))
        other.cse_noise_imcra.restype = ctypes.c_int
        other.cse_noise_imcra.argtypes = lib.cse_noise_imcra.argtypes
        others[os.path.basename(path)] = other.cse_noise_imcra

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

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
    fns = {"cse_noise_imcra": call(lib.cse_noise_imcra, prms["imcra"], S, "imcra"),
           "cse_noise_mcra": call(lib.cse_noise_mcra, prms["mcra"], S, "mcra"),
           "cse_noise_spp": call(lib.cse_noise_spp, prms["spp"], S, "spp"),
           "cse_noise_minstat": call(lib.cse_noise_minstat, prms["minstat"], S, "minstat"),
           "cse_noise_imcra_one_signal": call(lib.cse_noise_imcra, prms["imcra"], 1, "imcra")}
    for name, fn in others.items():
        fns[name] = call(fn, prms["imcra"], S, name)
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
    fns["cse_noise_imcra"]()
    got = N[0].cpu().numpy()
    st = {}
    ref = _imcra_ref.imcra(P[0].cpu().numpy(), 1e-10, stats=st)
    row["cse_noise_imcra"].update(
        unequal_to_restatement=int((got != ref).sum()), compared=int(ref.size),
        max_rel_error_in_f32_steps=float(np.max(np.abs(got.astype(np.float64) - ref) / ref)
                                         * 2.0 ** 23), **st)
    one = row["cse_noise_imcra_one_signal"]["ms"]
    row["imcra_ns_per_frame"] = row["cse_noise_imcra"]["ms"] * 1e6 / T
    row["imcra_one_signal_ns_per_frame"] = one * 1e6 / T
    for k in ("mcra", "spp", "minstat"):
        row[f"imcra_over_{k}"] = row["cse_noise_imcra"]["ms"] / row[f"cse_noise_{k}"]["ms"]
    out = {"signals": S, "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "shape": f"{S}x{T}x{B}", "times": row}
    if a.figures:
        with open(a.figures) as f:
            out["build"] = json.load(f)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
