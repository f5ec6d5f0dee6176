"""The online enhancer on the device (include/cse_online.h): chunking is
invisible bit for bit, the output is the offline plugins' on the same clip to
the parity bound, the tracked rows are cse_noise_<method>'s, streams of a batch
are independent, and the ABI refuses what the header says it refuses before
any launch.  Clips are one second."""

import ctypes
import functools

import numpy as np
import pytest
import torch

import _online_ref
from _online_cases import ALG_PARAMS, TRACKER_PARAMS, chunkings, clip, params_for, run
from classical_speech_enhancement_amd import _lib, online, plugins
from conftest import rel_l2, rel_max

pytestmark = pytest.mark.gpu

LENGTH = 16000 + 37
MARGIN = 1e-9   # cse_spp.h's |pm - ph_max|; for mcra |S - delta Smin| / S
PLUGINS = {"spectralSubtractor": plugins.spectral_subtraction, "wiener": plugins.wiener_filter,
           "mmse": plugins.mmse, "omlsa": plugins.advanced_mmse}


def enhancer(alg, params, S=1):
    return online.OnlineEnhancer(alg, params, n_streams=S, want_noise=True)


@functools.lru_cache(maxsize=None)
def clips_with_margin(alg, method, n_fft, hop, S):
    """S clips whose fp64 restatement keeps the tracker's discontinuity at
    least MARGIN away (the next seed where one does not), and that margin."""
    params = params_for(alg, method, n_fft, hop)
    cfg = online.config(alg, params)
    out, seed = [], 0
    while len(out) < S:
        assert seed < 16
        core = _online_ref.RefCore(cfg, 1)
        run(online.OnlineEnhancer(alg, params, want_noise=True, core=core), clip(LENGTH, seed), [])
        margin = core.margins()[0]
        print(f"{alg} {method} {n_fft}/{hop} seed {seed}: margin {margin:.3e}")
        if margin >= MARGIN:
            out.append((seed, margin))
        seed += 1
    return tuple(out)


def offline(alg, method, n_fft, hop, x):
    fn = PLUGINS[alg]
    return fn(x, 16000, n_fft=n_fft, hop_length=hop, noise_percentile=20.0, noise_method=method,
              **ALG_PARAMS[alg], **{method: TRACKER_PARAMS[method]})


# ------------------------------------------------------------ 1. chunking
def test_chunking_is_invisible_bit_for_bit():
    params = params_for("wiener", "mcra", 512, 128)  # window_frames = 8
    x = clip(LENGTH)
    base_y, base_n = run(enhancer("wiener", params), x, [])
    assert base_y.shape == x.shape and base_y.dtype == np.float32
    assert base_n.shape == (1 + LENGTH // 128, 257)
    assert np.isfinite(base_y).all() and np.abs(base_y).max() > 1e-3
    for name, cuts in chunkings(LENGTH, 128).items():
        y, rows = run(enhancer("wiener", params), x, cuts)
        assert y.tobytes() == base_y.tobytes(), name
        assert rows.tobytes() == base_n.tobytes(), name


def test_chunking_spp_first_push_carries_init_frames():
    params = params_for("omlsa", "spp", 512, 128)
    x = clip(LENGTH)
    base_y, base_n = run(enhancer("omlsa", params), x, [])
    for name in ("one hop", "977 samples"):
        y, rows = run(enhancer("omlsa", params), x, chunkings(LENGTH, 128)[name])
        assert y.tobytes() == base_y.tobytes(), name
        assert rows.tobytes() == base_n.tobytes(), name


# ----------------------------------------------- 2. and 3. against offline
CASES = [(alg, m, 512, 128, 1) for alg in ALG_PARAMS for m in ("mcra", "spp")] + [
    ("wiener", "mcra", 128, 32, 3), ("omlsa", "spp", 512, 256, 1), ("mmse", "mcra", 1024, 128, 1),
    ("spectralSubtractor", "mcra", 2048, 512, 2)]


@pytest.mark.parametrize("alg,method,n_fft,hop,S", CASES)
def test_output_is_the_offline_plugins(alg, method, n_fft, hop, S):
    picked = clips_with_margin(alg, method, n_fft, hop, S)
    assert all(m >= MARGIN for _, m in picked)
    x = np.stack([clip(LENGTH, seed) for seed, _ in picked])
    params = params_for(alg, method, n_fft, hop)
    assert online.config(alg, params).mu == (0.9 if alg == "mmse" else
                                             0.95 if alg == "omlsa" else 0.0)
    y, rows = run(enhancer(alg, params, S), x if S > 1 else x[0], list(range(977, LENGTH, 977)))
    y, rows = y.reshape(S, -1), rows.reshape(S, -1, n_fft // 2 + 1)
    eng = plugins.engine()
    for s in range(S):
        want = offline(alg, method, n_fft, hop, x[s])
        l2, mx = rel_l2(y[s], want), rel_max(y[s], want)
        print(f"{alg} {method} {n_fft}/{hop} stream {s}: rel-L2 {l2:.3e} rel-max {mx:.3e}")
        assert l2 <= 1e-5 and mx <= 1e-5
        # the rows: Engine.noise_estimate of the same clip, equal or adjacent f32 values
        _, P = eng.stft(torch.as_tensor(x[s]).cuda().view(1, -1), n_fft, hop, want_y=False)
        N = eng.noise_estimate(method, P, eps=online.config(alg, params).eps,
                               **TRACKER_PARAMS[method])[0].cpu().numpy().astype(np.float64)
        d = np.abs(rows[s].astype(np.float64) - N)
        print(f"   rows: max |d| / N {np.max(d / N):.3e}, differing {np.mean(d > 0):.2%}")
        assert rows[s].shape == N.shape and np.all(d <= 2.0 ** -23 * N)


# ------------------------------------------------------------ 4. batching
def test_a_stream_of_a_batch_equals_the_stream_alone():
    params = params_for("mmse", "spp", 512, 128)
    x = np.stack([clip(LENGTH, seed) for seed in range(3)])
    cuts = [700, 5000]
    y, rows = run(enhancer("mmse", params, 3), x, cuts)
    assert y.shape == x.shape
    for s in range(3):
        ys, rs = run(enhancer("mmse", params), x[s], cuts)
        assert ys.tobytes() == y[s].tobytes() and rs.tobytes() == rows[s].tobytes(), s
    assert y[0].tobytes() != y[1].tobytes()


# --------------------------------------------------------------- 5. reset
def test_reset_gives_the_same_output_again():
    params = params_for("omlsa", "mcra", 512, 128)
    x = clip(LENGTH)
    e = enhancer("omlsa", params)
    first = run(e, x, [3000])
    with pytest.raises(RuntimeError, match="push after finish"):
        e.push(x[:10])
    e.reset()
    e.push(clip(LENGTH, 1)[:4000])  # abandoned mid-stream
    e.reset()
    again = run(e, x, [8000])
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()


# ------------------------------------------------------- 6. ABI refusals
def test_abi_refusals_come_before_any_launch():
    lib = _lib.load()
    params = params_for("wiener", "spp", 512, 128)
    cfg = online.abi_config(online.config("wiener", params))
    h = _lib.OnlineHandle()
    ptr, ref = ctypes.c_void_p(256), ctypes.byref  # never dereferenced: refused first
    err = lambda: lib.cse_last_error().decode()  # noqa: E731

    def refused(rc, word):
        assert rc == -1 and word in err(), (rc, err())

    assert lib.cse_online_state_bytes(512, 3) == 3 * lib.cse_online_state_bytes(512, 1) > 0
    assert lib.cse_online_state_bytes(512, 0) == 0
    for n_fft in (64, 4096, 400, 0):
        assert lib.cse_online_state_bytes(n_fft, 1) == -1
    assert lib.cse_online_state_bytes(512, -1) == -1
    refused(lib.cse_online_init(None, ref(cfg), 1, ptr), "NULL handle")
    refused(lib.cse_online_init(ref(h), None, 1, ptr), "NULL handle or configuration")
    refused(lib.cse_online_init(ref(h), ref(cfg), 1, None), "NULL state")
    refused(lib.cse_online_init(ref(h), ref(cfg), -1, ptr), "n_streams=-1")
    for field, value, word in (("n_fft", 400, "n_fft=400"), ("n_fft", 4096, "n_fft=4096"),
                               ("n_fft", 64, "n_fft=64"), ("hop", 160, "hop=160"),
                               ("hop", 512, "hop=512"), ("algo", 4, "algo=4"),
                               ("noise_method", 5, "coupled bins"),
                               ("noise_method", 6, "coupled bins"),
                               ("noise_method", 0, "whole clip"), ("noise_method", 1, "whole clip"),
                               ("noise_method", 2, "whole clip"), ("noise_method", 9, "unknown"),
                               ("eps", 0.0, "eps=0")):
        bad = online.abi_config(online.config("wiener", params))
        setattr(bad, field, value)
        refused(lib.cse_online_init(ref(h), ref(bad), 1, ptr), word)
    bad = online.abi_config(online.config("wiener", params))
    bad.spp.ph_max = 1.5
    refused(lib.cse_online_init(ref(h), ref(bad), 1, ptr), "cse_online_init: prior_h1")
    # a live handle: pushes in the wrong state, bad arguments, spp's short first push
    state = torch.zeros(int(lib.cse_online_state_bytes(512, 1)), dtype=torch.uint8, device="cuda")
    sp = ctypes.c_void_p(state.data_ptr())
    assert lib.cse_online_init(ref(h), ref(cfg), 1, sp) == 0, err()
    x = torch.zeros(6 * 128, dtype=torch.float64, device="cuda")
    y = torch.full((6 * 128,), 7.0, dtype=torch.float32, device="cuda")
    xp, yp = ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(y.data_ptr())
    refused(lib.cse_online_push(ref(h), xp, 1, yp, None, None), "not primed")
    refused(lib.cse_online_finish(ref(h), yp, None), "not primed")
    refused(lib.cse_online_prime(ref(h), None, None), "NULL handle or x_head")
    assert lib.cse_online_prime(ref(h), xp, None) == 0, err()
    refused(lib.cse_online_push(None, xp, 1, yp, None, None), "NULL handle")
    refused(lib.cse_online_push(ref(h), None, 1, yp, None, None), "NULL handle, x or y")
    refused(lib.cse_online_push(ref(h), xp, 1, None, None, None), "NULL handle, x or y")
    refused(lib.cse_online_push(ref(h), xp, -1, yp, None, None), "k=-1")
    refused(lib.cse_online_push(ref(h), xp, 5, yp, None, None), "k=5 < init_frames=6")
    assert lib.cse_online_push(ref(h), xp, 0, yp, None, None) == 0 and h.frames == 0
    torch.cuda.synchronize()
    assert float(y.min()) == 7.0  # nothing ran
    assert lib.cse_online_push(ref(h), xp, 6, yp, None, None) == 0, err()
    assert h.frames == 6
    assert lib.cse_online_push(ref(h), xp, 1, yp, None, None) == 0, err()  # later pushes: any k
    torch.cuda.synchronize()
    assert float(y.abs().max()) == 0.0  # silence in, silence out
    refused(lib.cse_online_finish(ref(h), None, None), "NULL handle or y_tail")
    assert lib.cse_online_finish(ref(h), yp, None) == 0, err()
    refused(lib.cse_online_push(ref(h), xp, 1, yp, None, None), "finished")
    # no streams: everything is accepted and nothing is launched
    h0 = _lib.OnlineHandle()
    assert lib.cse_online_init(ref(h0), ref(cfg), 0, None) == 0, err()
    assert lib.cse_online_prime(ref(h0), xp, None) == 0
    assert lib.cse_online_push(ref(h0), xp, 6, yp, None, None) == 0
    assert lib.cse_online_finish(ref(h0), yp, None) == 0
    torch.cuda.synchronize()
