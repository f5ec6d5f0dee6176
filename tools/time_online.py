"""Time of the online enhancer's push (include/cse_online.h) on the GPU box.

    timeout 600 python tools/time_online.py [--reps R --inner I] [--out FILE]

n_fft 512 / hop 128, wiener + mcra and omlsa + spp, S = 1, 64 and 1,024
streams, pushes of k = 1 and k = 8 frames (and k = 64, for the per-frame
slope), at the ABI on device buffers that stay where they are: no host copy is
inside a timing.  After a prime and a warm-up push of 8 frames, per case:

  queued_ms   the median over R repeats of the time of I back-to-back pushes
              between two HIP events, divided by I: the rate of a caller who
              keeps the queue full
  synced_ms   the median over R x I pushes of the host clock around one push
              and a stream synchronise: what a caller who waits for every
              block sees

Per (algorithm, S) the two-point fit t(k) = launch_ms + k frame_ms through
k = 1 and k = 64 separates what a push costs once (the launch and the tables
every push rebuilds in LDS) from the dependent per-frame chain.  Beside them:
the hop's duration at 16 kHz (8 ms), which gives the real-time factor
S k hop_ms / queued_ms.  One JSON line per case (default
profiles/online_times.jsonl), printed too.
"""

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from classical_speech_enhancement_amd import _lib, online  # noqa: E402

N_FFT, HOP = 512, 128
CASES = {
    "wiener+mcra": ("wiener", dict(alpha=0.98, gain_floor=0.05, noise_method="mcra")),
    "omlsa+spp": ("omlsa", dict(alpha=0.92, ksi_min=0.005, gain_floor=0.1, q=0.4, noise_mu=0.95,
                                noise_method="spp")),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "online_times.jsonl"))
    a = ap.parse_args()
    lib = _lib.load()
    ref = ctypes.byref
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    hop_ms = 1e3 * HOP / 16000.0
    kmax = max(a.frames + [8])
    lines = []
    for name, (alg, params) in CASES.items():
        cfg = online.config(alg, dict(params, n_fft=N_FFT, hop_length=HOP))
        for S in a.streams:
            gen = torch.Generator(device="cuda").manual_seed(S)
            x = 0.1 * torch.randn((S * kmax * HOP,), dtype=torch.float64, device="cuda",
                                  generator=gen)
            y = torch.empty((S * kmax * HOP,), dtype=torch.float32, device="cuda")
            state = torch.empty(int(lib.cse_online_state_bytes(N_FFT, S)), dtype=torch.uint8,
                                device="cuda")
            h = _lib.OnlineHandle()
            c = online.abi_config(cfg)
            sp, xp, yp = (ctypes.c_void_p(t.data_ptr()) for t in (state, x, y))
            _lib.check(lib.cse_online_init(ref(h), ref(c), S, sp), "cse_online_init")
            _lib.check(lib.cse_online_prime(ref(h), xp, stream), "cse_online_prime")

            def push(k):
                _lib.check(lib.cse_online_push(ref(h), xp, k, yp, None, stream), "cse_online_push")

            push(8)  # spp's first push, and the code object's load
            for k in a.frames:
                push(k)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(y).all())
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            queued = {k: [] for k in a.frames}
            synced = {k: [] for k in a.frames}
            for _ in range(a.reps):  # the kinds alternate inside every repeat
                for k in a.frames:
                    e0.record()
                    for _ in range(a.inner):
                        push(k)
                    e1.record()
                    torch.cuda.synchronize()
                    queued[k].append(e0.elapsed_time(e1) / a.inner)
                    for _ in range(a.inner):
                        t0 = time.perf_counter()
                        push(k)
                        torch.cuda.current_stream().synchronize()
                        synced[k].append(1e3 * (time.perf_counter() - t0))
            q = {k: float(np.median(v)) for k, v in queued.items()}
            s = {k: float(np.median(v)) for k, v in synced.items()}
            k0, k1 = min(a.frames), max(a.frames)
            frame_ms = (q[k1] - q[k0]) / (k1 - k0) if k1 > k0 else float("nan")
            for k in a.frames:
                line = {"what": "cse_online_push", "device": torch.cuda.get_device_name(0),
                        "case": name, "n_fft": N_FFT, "hop": HOP, "streams": S, "frames_per_push": k,
                        "reps": a.reps, "pushes_per_timing": a.inner,
                        "queued_ms": q[k], "queued_ms_min": float(np.min(queued[k])),
                        "queued_ms_max": float(np.max(queued[k])), "synced_ms": s[k],
                        "fit_frame_ms": frame_ms, "fit_launch_ms": q[k0] - k0 * frame_ms,
                        "hop_ms": hop_ms, "audio_ms_per_push": S * k * hop_ms,
                        "real_time_factor_queued": S * k * hop_ms / q[k],
                        "real_time_factor_synced": S * k * hop_ms / s[k],
                        "stream_frames_per_s_queued": S * k / (q[k] / 1e3)}
                lines.append(line)
                print(json.dumps(line), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w", encoding="utf-8") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
