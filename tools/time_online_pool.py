"""Time of the pool's step (include/cse_online_pool.h) beside the lockstep push
(include/cse_online.h) on the GPU box, in one run.

    timeout 600 python tools/time_online_pool.py [--reps R --inner I] [--out FILE]

tools/time_online.py's set-up and protocol: n_fft 512 / hop 128, wiener + mcra
and omlsa + spp, S = 1, 64 and 1,024, k = 1 and k = 8 frames for every
stream, at the ABI on device buffers that stay where they are.  Per (case, S)
one pool of S open slots and one lockstep batch of S streams are primed and
warmed up; then, alternating inside every repeat, per k:

  queued_ms   the median over R repeats of the time of I back-to-back calls
              between two HIP events, divided by I
  synced_ms   the median over R x I calls of the host clock around one call
              and a stream synchronise

for cse_pool_step with the list [(slot, k) for every slot] and for
cse_online_push of k frames.  At S = 1,024 one ragged step (k drawn from
{1, 2, 4, 8} per slot, seeded) is timed the same way beside the lockstep push
at k = 8: the slowest item bounds a launch.  host_ms is the host clock around
the step call alone (checks, the list, its copy, the launch), and
list_copy_queued_ms the queued time of a host-to-device copy of the list's
size (24 bytes per slot, pageable memory) on its own.  One JSON line
per (case, S, k) with both times side by side (default
profiles/online_pool_times.jsonl), printed too.
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
KMAX = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--ragged-at", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "online_pool_times.jsonl"))
    a = ap.parse_args()
    lib = _lib.load()
    ref = ctypes.byref
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    sync = torch.cuda.current_stream().synchronize
    lines = []
    for name, (alg, params) in CASES.items():
        cfg = online.config(alg, dict(params, n_fft=N_FFT, hop_length=HOP))
        c = online.abi_config(cfg)
        for S in a.streams:
            gen = torch.Generator(device="cuda").manual_seed(S)
            x = 0.1 * torch.randn((S * KMAX * HOP,), dtype=torch.float64, device="cuda",
                                  generator=gen)
            y = torch.empty((S * KMAX * HOP,), dtype=torch.float32, device="cuda")
            xp, yp = ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(y.data_ptr())
            # the lockstep batch
            state = torch.empty(int(lib.cse_online_state_bytes(N_FFT, S)), dtype=torch.uint8,
                                device="cuda")
            h = _lib.OnlineHandle()
            _lib.check(lib.cse_online_init(ref(h), ref(c), S, ctypes.c_void_p(state.data_ptr())),
                       "cse_online_init")
            _lib.check(lib.cse_online_prime(ref(h), xp, stream), "cse_online_prime")
            # the pool: S slots, all open
            pstate = torch.empty(int(lib.cse_pool_state_bytes(N_FFT, S)), dtype=torch.uint8,
                                 device="cuda")
            pwork = torch.empty(int(lib.cse_pool_work_bytes(S)), dtype=torch.uint8, device="cuda")
            slots = (_lib.PoolSlot * S)()
            ph = _lib.PoolHandle()
            _lib.check(lib.cse_pool_init(ref(ph), ref(c), S, ctypes.c_void_p(pstate.data_ptr()),
                                         ctypes.c_void_p(pwork.data_ptr()),
                                         ctypes.cast(slots, ctypes.c_void_p)), "cse_pool_init")
            for s in range(S):
                head = ctypes.c_void_p(x.data_ptr() + 8 * s * (N_FFT - HOP))
                _lib.check(lib.cse_pool_open(ref(ph), s, None, head, stream), "cse_pool_open")

            def uniform(k):
                return (_lib.PoolItem * S)(*[_lib.PoolItem(s, k) for s in range(S)]), S * k

            lists = {k: uniform(k) for k in set(a.frames) | {KMAX}}
            kinds = [("uniform", k) for k in a.frames]
            if S == a.ragged_at:
                ks = np.random.default_rng(S).choice([1, 2, 4, 8], size=S)
                lists["ragged"] = ((_lib.PoolItem * S)(*[_lib.PoolItem(s, int(k))
                                                         for s, k in enumerate(ks)]), int(ks.sum()))
                kinds.append(("ragged", "ragged"))

            def push(k):
                _lib.check(lib.cse_online_push(ref(h), xp, k, yp, None, stream), "cse_online_push")

            def step(key):
                _lib.check(lib.cse_pool_step(ref(ph), lists[key][0], S, xp, yp, None, stream),
                           "cse_pool_step")

            push(KMAX)  # spp's first push and step, and the code objects' load
            step(KMAX)
            for _, key in kinds:
                step(key)
                push(KMAX if key == "ragged" else key)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(y).all())
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            times = {(who, key): {"queued": [], "synced": [], "host": []}
                     for who in ("pool", "lockstep") for _, key in kinds}
            for _ in range(a.reps):  # the kinds and the two paths alternate inside every repeat
                for _, key in kinds:
                    k_push = KMAX if key == "ragged" else key
                    for who, call, arg in (("pool", step, key), ("lockstep", push, k_push)):
                        t = times[who, key]
                        e0.record()
                        for _ in range(a.inner):
                            call(arg)
                        e1.record()
                        torch.cuda.synchronize()
                        t["queued"].append(e0.elapsed_time(e1) / a.inner)
                        for _ in range(a.inner):
                            t0 = time.perf_counter()
                            call(arg)
                            t1 = time.perf_counter()
                            sync()
                            t["synced"].append(1e3 * (time.perf_counter() - t0))
                            t["host"].append(1e3 * (t1 - t0))
            # the work list's copy alone: 24 bytes per item from pageable host memory
            rec = torch.zeros(24 * S, dtype=torch.uint8)
            copies = []
            for _ in range(a.reps):
                e0.record()
                for _ in range(a.inner):
                    pwork[:24 * S].copy_(rec, non_blocking=True)
                e1.record()
                torch.cuda.synchronize()
                copies.append(e0.elapsed_time(e1) / a.inner)
            for kind, key in kinds:
                p, q = times["pool", key], times["lockstep", key]
                line = {"what": "cse_pool_step beside cse_online_push",
                        "device": torch.cuda.get_device_name(0), "case": name, "n_fft": N_FFT,
                        "hop": HOP, "slots": S, "kind": kind,
                        "frames_per_slot": key if kind == "uniform" else [1, 2, 4, 8],
                        "frames_per_step": lists[key][1],
                        "lockstep_frames_per_push": KMAX if kind == "ragged" else key,
                        "reps": a.reps, "calls_per_timing": a.inner,
                        "list_copy_queued_ms": float(np.median(copies))}
                for who, t in (("pool", p), ("lockstep", q)):
                    line.update({f"{who}_queued_ms": float(np.median(t["queued"])),
                                 f"{who}_queued_ms_min": float(np.min(t["queued"])),
                                 f"{who}_queued_ms_max": float(np.max(t["queued"])),
                                 f"{who}_synced_ms": float(np.median(t["synced"])),
                                 f"{who}_host_ms": float(np.median(t["host"]))})
                lines.append(line)
                print(json.dumps(line), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w", encoding="utf-8") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
