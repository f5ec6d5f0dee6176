"""Make tests/golden/plan_layout.npz — the tables and library calls of four plans.

Host side only: every plan is built with device="cpu" and a stand-in for the
library that records (entry point, arguments) and returns 0; only the *_bytes
size queries and cse_cells_per_group go to the real libcse.so (which loads
without a GPU).  Pointers are recorded as [buffer name, element offset] of the
plan buffer they fall in.  Per case and n_fft the file holds

  <case>/<n_fft>/packed, jobs        the uploaded tables (raw bytes)
  <case>/<n_fft>/order, split, idx, hop_jobs, sizes (SIZES order)
  <case>/<n_fft>/calls               JSON: prepare_stft, prepare_noise, enhance
                                     (and finalize where the case aligns)

The values pin the planning code to the commit the file was made at
(tests/test_plan_layout.py rebuilds every case and compares without a
tolerance), so regenerate it only from a commit whose tables are known good,
never to make that test pass:  python tests/golden/make_plan_layout.py
"""

import ctypes
import json
import os
import sys

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "plan_layout.npz")
REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
S = 2
SIZES = ("pool", "raw", "Ybuf", "g_out", "head")  # element counts, 0 if absent
# plan buffers a pointer argument may fall in (dicts: one buffer per hop)
BUFFERS = ("raw", "pool", "P", "Ptrue", "med", "ws", "Ybuf", "cells_d", "sse_d", "fin_d",
           "jobs_d", "g_out", "y_all", "head", "head_off", "sig_of", "xc_ws", "lag_d", "zero_d",
           "xst_d")


def cases():
    """name -> (L, specs, keyword arguments of Engine.plan)."""
    from classical_speech_enhancement_amd.parameter_ranges import grid_specs
    wiener = dict(alpha=0.98, gain_floor=0.05, n_fft=512, noise_percentile=20.0)
    mixed = [(k % S, "wiener", dict(wiener, hop_length=hop, noise_method=m))  # signals alternate
             for k, (hop, m) in enumerate((hop, m) for hop in (128, 64, 160, 32)
                                          for m in ("percentile", "min_tracking", "true_noise"))]
    mixed.append((1, "omlsa", dict(alpha=0.9, ksi_min=0.005, gain_floor=0.1, q=0.4, noise_mu=0.95,
                                   n_fft=400, hop_length=160, noise_percentile=10.0,
                                   noise_method="min_tracking")))
    short = [(s, "spectralSubtractor", dict(alpha=a, beta=0.05, n_fft=512, hop_length=128,
                                            noise_percentile=20.0, noise_method="percentile"))
             for s in range(S) for a in (1.0, 2.0, 3.0)]
    short += [(s, "omlsa", dict(alpha=0.9, ksi_min=0.005, gain_floor=0.1, q=0.4, noise_mu=mu,
                                n_fft=512, hop_length=128, noise_percentile=10.0,
                                noise_method="percentile"))
              for s in range(S) for mu in (0.92, 0.98)]
    return {
        "a": (8000, grid_specs(S), dict(align=True)),
        "b": (8000, grid_specs(S), dict(want_waveforms=True, want_gains=True)),
        "c": (4000, mixed, dict(want_waveforms=True, true_len=3000)),
        "d": (400, short, dict(want_waveforms=True, want_gains=True)),
    }


class Recorder:
    """Stands in for the loaded library: sizes from the real one, every other
    entry point is recorded and succeeds."""

    def __init__(self, real):
        self.real, self.calls, self.plan, self.inputs = real, [], None, {}

    def __getattr__(self, name):
        if name.endswith("_bytes") or name == "cse_cells_per_group":
            return getattr(self.real, name)

        def call(*args):
            self.calls.append([name] + [self.describe(a) for a in args])
            return 0
        return call

    def buffers(self):
        yield from self.inputs.items()
        for name in BUFFERS:
            b = getattr(self.plan, name, None)
            for hop, t in (b.items() if isinstance(b, dict) else [(None, b)]):
                if t is not None:
                    yield (name if hop is None else f"{name}[{hop}]"), t

    def describe(self, a):
        if a is None or isinstance(a, (int, float)):
            return a
        if isinstance(a, ctypes.c_void_p):
            if not a.value:
                return None
            for name, t in self.buffers():
                off = a.value - t.data_ptr()
                if 0 <= off < max(t.numel(), 1) * t.element_size():
                    assert off % t.element_size() == 0, (name, off)
                    return [name, off // t.element_size()]
            return ["temporary", 0]  # e.g. the true_len-trimmed copies of the inputs
        obj = a._obj  # ctypes.byref(struct)
        return {f: getattr(obj, f) for f, _ in obj._fields_}


def record(L, specs, kw):
    """{n_fft: {array name: value}} of one case, built by the package as it is."""
    import torch
    from classical_speech_enhancement_amd import _lib
    from classical_speech_enhancement_amd.engine import Engine

    class Stream:  # the stream argument of every launch: null
        cuda_stream = 0
    current, torch.cuda.current_stream = torch.cuda.current_stream, lambda *a, **k: Stream
    try:
        eng = Engine.__new__(Engine)  # no device
        eng.lib, eng.device = Recorder(_lib.load()), torch.device("cpu")
        noisy = torch.zeros((S, L), dtype=torch.float64)
        clean = torch.zeros((S, L), dtype=torch.float64)
        eng.lib.inputs = {"noisy": noisy, "clean": clean}
        mp = eng.plan(S, L, specs, **kw)
        out = {}
        for p in mp.plans:
            eng.lib.plan, eng.lib.calls = p, []
            p.prepare_stft(noisy, clean)
            p.prepare_noise(clean)
            p.enhance()
            if p.align:
                p.finalize()
            numel = {k: getattr(p, k, None) for k in SIZES}
            out[p.n_fft] = {
                "packed": p.cells_d.numpy().copy(), "jobs": p.jobs_d.numpy().copy(),
                "order": np.asarray(p.order, dtype=np.int64),
                "split": np.asarray(p.split, dtype=np.int64),
                "idx": np.asarray(p.idx, dtype=np.int64),
                "hop_jobs": np.array([(h,) + tuple(p.hop_jobs[h]) for h in p.hops], dtype=np.int64),
                "sizes": np.array([0 if numel[k] is None or (k == "head" and numel[k] is p.y_all)
                                   else numel[k].numel() for k in SIZES], dtype=np.int64),
                "calls": np.array(json.dumps(eng.lib.calls)),
            }
        return out
    finally:
        torch.cuda.current_stream = current


def main():
    sys.path.insert(0, REPO)
    flat = {}
    for name, (L, specs, kw) in cases().items():
        for n_fft, arrays in record(L, specs, kw).items():
            calls = json.loads(str(arrays["calls"]))
            print(name, n_fft, "cells", len(arrays["idx"]), "slots", len(arrays["order"]),
                  "split", arrays["split"].tolist(), "jobs", int(arrays["hop_jobs"][:, 2].sum()),
                  "sizes", arrays["sizes"].tolist(), "calls", [c[0] for c in calls])
            for k, v in arrays.items():
                flat[f"{name}/{n_fft}/{k}"] = v
    np.savez_compressed(OUT, **flat)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
