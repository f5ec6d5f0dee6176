"""The online enhancer without a device (include/cse_online.h): the stateful
restatement (tests/_online_ref.py) against the whole-clip restatements and the
offline composition, and OnlineEnhancer's buffering, padding, trimming and
refusals over that restatement as its core."""

import numpy as np
import pytest

import _mcra_ref
import _online_ref
import _spp_ref
import oracle
from classical_speech_enhancement_amd import online
from _online_cases import ALG_PARAMS, chunkings, clip, params_for, run
from conftest import rel_max
from oracle import gain_ref

SHAPES = [(128, 32), (512, 128), (512, 256), (1024, 128)]
LENGTHS = [2085, 16037]


def run_online(alg, params, x, cuts, n_streams=1, want_noise=False):
    """x [n] or [S][n] through OnlineEnhancer over the restatement, cut at the
    sample positions ``cuts``; returns the concatenated output (and rows)."""
    cfg = online.config(alg, params)
    e = online.OnlineEnhancer(alg, params, n_streams=n_streams, want_noise=True,
                              core=_online_ref.RefCore(cfg, n_streams))
    y, rows = run(e, x, cuts)
    return (y, rows) if want_noise else y


def tracker_kw(cfg):
    from classical_speech_enhancement_amd import trackers
    return dict(zip(trackers.TRACKERS[cfg.method].defaults, cfg.values))


def offline(alg, params, x):
    """oracle.stft -> tracker restatement -> smooth_noise where the algorithm
    applies it -> the oracle gain loop -> oracle.istft(length=len)."""
    cfg = online.config(alg, params)
    Y = oracle.stft(x, cfg.n_fft, cfg.hop)
    P = np.abs(Y) ** 2
    track = _mcra_ref.mcra if cfg.method == "mcra" else _spp_ref.spp
    N = track(P.T, eps=cfg.eps, **tracker_kw(cfg)).T.astype(np.float64)
    code = _online_ref.CODES[cfg.algo]
    p = cfg.param
    if code in ("MMSE", "OMLSA"):
        N = gain_ref.smooth_noise(N, cfg.mu)
    if code == "SS":
        S = gain_ref.ss_spectrum(Y, P, np.maximum(N, cfg.eps), p[0], p[1])
    elif code == "WIENER":
        S = Y * gain_ref.wiener_gains(P, np.maximum(N, cfg.eps), p[0], p[1], cfg.eps)
    elif code == "MMSE":
        S = Y * gain_ref.mmse_gains(P, N, p[0], p[1], p[2], p[3], cfg.eps)
    else:
        S = Y * gain_ref.omlsa_gains(P, np.maximum(N, cfg.eps), p[0], p[1], p[3], p[2], cfg.eps,
                                     p[4])
    return oracle.istft(S, hop_length=cfg.hop, win_length=cfg.n_fft, length=len(x))


# ---------------------------------------------------------------- trackers
@pytest.mark.parametrize("method", ["mcra", "spp"])
@pytest.mark.parametrize("n_fft,hop", [(128, 32), (512, 128)])
def test_stateful_trackers_equal_the_whole_clip_restatements(method, n_fft, hop):
    x = clip(16037)
    params = params_for("wiener", method, n_fft, hop)
    cfg = online.config("wiener", params)
    P = (np.abs(oracle.stft(x, n_fft, hop)) ** 2).T
    track = _mcra_ref.mcra if method == "mcra" else _spp_ref.spp
    want = track(P, eps=cfg.eps, **tracker_kw(cfg))
    step = _online_ref.make_tracker(cfg)
    if method == "spp":
        step.start(P[:cfg.first_frames])
    got = np.stack([np.maximum(step.step(p), cfg.eps).astype(np.float32) for p in P])
    assert got.tobytes() == want.tobytes()
    # and through the wrapper: the rows every push returns, one hop at a time
    _, rows = run_online("wiener", params, x, chunkings(len(x), hop)["one hop"], want_noise=True)
    assert rows.shape == want.shape and rows.tobytes() == want.tobytes()


# ---------------------------------------------------------------- waveform
@pytest.mark.parametrize("method", ["mcra", "spp"])
@pytest.mark.parametrize("alg", list(ALG_PARAMS))
@pytest.mark.parametrize("n_fft,hop", SHAPES)
def test_restatement_equals_the_offline_composition(alg, method, n_fft, hop):
    for length in LENGTHS:
        x = clip(length)
        params = params_for(alg, method, n_fft, hop)
        want = offline(alg, params, x)
        got = run_online(alg, params, x, list(range(977, length, 977)))
        assert got.shape == want.shape
        err = rel_max(got, want)
        print(f"{alg} {method} {n_fft}/{hop} len {length}: rel-max {err:.3e}")
        assert err <= 1e-12


# ---------------------------------------------------------------- chunking
@pytest.mark.parametrize("alg,method,n_fft,hop", [("wiener", "mcra", 512, 128),
                                                  ("omlsa", "spp", 128, 32),
                                                  ("mmse", "mcra", 512, 256)])
def test_chunking_is_invisible(alg, method, n_fft, hop):
    x = clip(2085 if n_fft == 128 else 16037)
    params = params_for(alg, method, n_fft, hop)
    base_y, base_n = run_online(alg, params, x, [], want_noise=True)
    assert len(base_y) == len(x)
    for name, cuts in chunkings(len(x), hop).items():
        y, rows = run_online(alg, params, x, cuts, want_noise=True)
        assert y.tobytes() == base_y.tobytes(), name
        assert rows.tobytes() == base_n.tobytes(), name


# ------------------------------------------- length invariant and refusals
@pytest.mark.parametrize("length", [257, 258, 300, 383, 384, 385, 511, 512, 513, 1000])
def test_output_length_equals_input_length(length):
    params = params_for("wiener", "mcra", 512, 128)
    x = clip(16037)[:length]
    pieces = []
    e = online.OnlineEnhancer("wiener", params, core=_online_ref.RefCore(
        online.config("wiener", params), 1))
    for a in range(0, length, 100):
        pieces.append(e.push(x[a:a + 100]))
        assert pieces[-1].ndim == 1
    assert e.push(x[:0]).shape == (0,)
    pieces.append(e.finish())
    assert sum(len(p) for p in pieces) == length
    if length // 128 + 1 >= 5:  # the documented limit: offline is the simple estimate below
        assert rel_max(np.concatenate(pieces), offline("wiener", params, x)) <= 1e-12


def test_streams_in_lockstep_and_shapes():
    params = params_for("wiener", "spp", 128, 32)
    x = np.stack([clip(2085, s) for s in range(3)])
    y, rows = run_online("wiener", params, x, [500, 501, 1500], n_streams=3, want_noise=True)
    assert y.shape == x.shape and rows.shape == (3, 1 + 2085 // 32, 65)
    for s in range(3):
        assert y[s].tobytes() == run_online("wiener", params, x[s], []).tobytes()
    e = online.OnlineEnhancer("wiener", params, n_streams=3,
                              core=_online_ref.RefCore(online.config("wiener", params), 3))
    with pytest.raises(ValueError, match="1-D block"):
        e.push(x[0])
    with pytest.raises(ValueError, match="shape"):
        e.push(x[:2])


def test_latency_is_the_look_ahead():
    """Output o appears with the push that brings input o + latency, not before."""
    params = params_for("wiener", "mcra", 128, 32)
    cfg = online.config("wiener", params)
    e = online.OnlineEnhancer("wiener", params, core=_online_ref.RefCore(cfg, 1))
    assert e.latency == 127
    x = clip(2085)
    got = 0
    for n in range(600):
        got += len(e.push(x[n:n + 1]))
        # with inputs [0, n] in, every o with o + latency <= n is out, and no o beyond n - (n_fft - hop)
        assert max(n + 1 - e.latency, 0) <= got <= max(n + 1 - (128 - 32), 0)


def test_refusals():
    ok = params_for("wiener", "mcra", 512, 128)
    for method, word in (("minstat", "coupled bins"), ("imcra", "coupled bins"),
                         ("percentile", "whole clip"), ("min_tracking", "whole clip"),
                         ("true_noise", "whole clip"), ("nonsense", "Unbekannte Methode")):
        with pytest.raises(ValueError, match=word):
            online.config("wiener", dict(ok, noise_method=method))
    for n_fft, hop in ((64, 16), (4096, 1024), (400, 100), (512, 160), (512, 512), (512, 32)):
        with pytest.raises(ValueError, match="n_fft|hop_length"):
            online.config("wiener", dict(ok, n_fft=n_fft, hop_length=hop))
    with pytest.raises(TypeError, match="mcra takes no parameter 'alpha_x'"):
        online.config("wiener", dict(ok, mcra_alpha_x=0.5))
    with pytest.raises(ValueError, match="alpha_d"):
        online.config("wiener", dict(ok, mcra_alpha_d=1.5))
    with pytest.raises(ValueError, match="noise_mu"):
        online.config("omlsa", dict(alpha=0.9, ksi_min=0.01, gain_floor=0.1, q=0.4, n_fft=512,
                                    hop_length=128, noise_method="mcra"))
    with pytest.raises(ValueError, match="unknown algorithm"):
        online.config("nonsense", ok)
    cfg = online.config("wiener", ok)
    with pytest.raises(ValueError, match="n_streams"):
        online.OnlineEnhancer("wiener", ok, n_streams=0, core=_online_ref.RefCore(cfg, 0))
    e = online.OnlineEnhancer("wiener", ok, core=_online_ref.RefCore(cfg, 1))
    e.push(clip(2085)[:256])
    with pytest.raises(ValueError, match="at least 257 samples"):
        e.finish()  # the reflect padding needs n_fft/2 + 1 samples
    assert len(e.push(clip(2085)[256:])) + len(e.finish()) == 2085
    with pytest.raises(RuntimeError, match="push after finish"):
        e.push(clip(2085)[:10])
    e.reset()
    assert len(e.push(clip(2085))) + len(e.finish()) == 2085
    # spp holds back init_frames frames: a clip with fewer cannot be finished
    sp = params_for("wiener", "spp", 512, 128)
    e = online.OnlineEnhancer("wiener", sp, core=_online_ref.RefCore(online.config("wiener", sp), 1))
    e.push(clip(2085)[:600])  # 5 frames < init_frames = 6
    with pytest.raises(ValueError, match="init_frames=6"):
        e.finish()


def test_config_carries_the_cell_parameters():
    cfg = online.config("advanced_mmse", params_for("omlsa", "spp", 1024, 128))
    assert cfg.algorithm == "omlsa" and cfg.algo == 3 and cfg.eps == 1e-10 and cfg.mu == 0.95
    assert cfg.param[:5] == (0.92, 0.005, 0.1, 0.4, 80.0) and cfg.first_frames == 6
    assert online.config("mmse", dict(alpha=0.9, ksi_min=0.01, gain_min=0.1, n_fft=512,
                                      hop_length=128, noise_method="mcra")).mu == 0.98
    c = online.abi_config(cfg)
    assert (c.n_fft, c.hop, c.algo, c.noise_method) == (1024, 128, 3, 4)
    assert c.spp.init_frames == 6 and c.spp.alpha_pow == 0.75 and c.mcra.window_frames == 125
