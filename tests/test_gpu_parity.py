"""HIP path vs the oracle / golden vectors (needs an MI355X: -m gpu).

Tolerance (north-star): enhanced waveforms match the fp64
reference path within rel-L2 <= 1e-5 AND max|diff| <= 1e-5 * max|ref|.
Element-wise relative error is not used (it diverges at near-zero samples).
"""

import numpy as np
import pytest

import oracle
from classical_speech_enhancement_amd.synth import make_pair
from conftest import load_golden, rel_l2, rel_max

pytestmark = pytest.mark.gpu

TOL = 1e-5
CELLS = {
    "ss": dict(alpha=2.0, beta=0.005),
    "wiener": dict(alpha=0.95, gain_floor=0.05),
    "mmse": dict(alpha=0.98, ksi_min=0.01, gain_min=0.05, gain_max=1.0),
    "omlsa": dict(alpha=0.9, ksi_min=0.005, gain_floor=0.1, noise_mu=0.95, q=0.4),
}


@pytest.fixture(scope="module")
def P():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from classical_speech_enhancement_amd import plugins
    return plugins


ORACLE = {"ss": oracle.spectral_subtraction, "wiener": oracle.wiener_filter,
          "mmse": oracle.mmse, "omlsa": oracle.advanced_mmse}


def _fn(P, alg):
    return {"ss": P.spectral_subtraction, "wiener": P.wiener_filter, "mmse": P.mmse,
            "omlsa": P.advanced_mmse}[alg]


def test_plugins_match_reference_golden(P):
    g = load_golden("algorithms_0p75s.npz")
    noisy, clean = g["noisy"], g["clean"].astype(np.float64)
    worst = 0.0
    for key in g.files:
        if not key.startswith("y|"):
            continue
        alg, method, n_fft, hop, pct = key.split("|")[1:]
        kw = dict(CELLS[alg], n_fft=int(n_fft), hop_length=int(hop),
                  noise_percentile=float(pct), noise_method=method)
        if method == "true_noise":
            kw["clean_audio"] = clean
        y = _fn(P, alg)(noisy, 16000, **kw)
        e2, em = rel_l2(y, g[key]), rel_max(y, g[key])
        worst = max(worst, e2, em)
        assert e2 <= TOL and em <= TOL, (key, e2, em)
    print("worst relative error", worst)


def test_noise_estimates_match_reference_golden(P):
    g = load_golden("algorithms_0p75s.npz")
    noisy, clean = g["noisy"], g["clean"].astype(np.float64)
    for key in g.files:
        if not key.startswith("N|"):
            continue
        method, n_fft, hop, pct, eps = key.split("|")[1:]
        N = P.noise_estimation(noisy, 16000, method=method, n_fft=int(n_fft),
                               hop_length=int(hop), percentile=float(pct),
                               clean_audio=clean, eps=float(eps))
        assert N.shape == g[key].shape, key
        # fp32 storage of an fp64 estimate: relative 1e-6 elementwise
        np.testing.assert_allclose(N, g[key], rtol=1e-6, atol=0, err_msg=key)


def test_short_hops_match_reference_golden(P):
    """cse_enhance_cells_short_hop (n_fft 512 at hop 32 / 64, 1024 at 64)
    through the plugins against the reference's outputs (float32-stored, 6e-8),
    incl. T = 4 (static fallback) and T = 10 clips at hop 32."""
    g = load_golden("short_hops_0p5s.npz")
    noisy, clean = g["noisy"], g["clean"].astype(np.float64)
    n = 0
    for key in g.files:
        if key.startswith("y|"):
            alg, method, n_fft, hop = key.split("|")[1:]
            kw = dict(CELLS[alg], n_fft=int(n_fft), hop_length=int(hop), noise_percentile=10.0,
                      noise_method=method)
            if method == "true_noise":
                kw["clean_audio"] = clean
            y = _fn(P, alg)(noisy, 16000, **kw)
        elif key.startswith("t|"):
            m, alg = key.split("|")[1:]
            y = _fn(P, alg)(g[f"noisy|{m}"], 16000, **dict(CELLS[alg], n_fft=512, hop_length=32,
                                                             noise_percentile=20.0,
                                                             noise_method="min_tracking"))
        else:
            continue
        ref = g[key].astype(np.float64)
        assert y.shape == ref.shape, key
        assert rel_l2(y, ref) <= TOL and rel_max(y, ref) <= TOL, (key, rel_l2(y, ref))
        n += 1
    assert n == 44


def test_short_and_sweep_hops_in_one_plan(P):
    """One plan mixing sweep-hop, short-hop and generic-shape cells (three
    launches over one packed table) equals the cells run one plan each (the
    same cell code; a misplaced output pointer would show as a gross error);
    gain matrices at a short hop and unsupported shapes raise."""
    import torch
    from classical_speech_enhancement_amd.engine import Engine
    clean, noisy = make_pair(5, seconds=0.5)
    eng = Engine()
    x = torch.as_tensor(np.stack([noisy, noisy[::-1].copy()])).cuda()
    c = torch.as_tensor(np.stack([clean, clean[::-1].copy()])).cuda()
    specs = []
    for s in (0, 1):
        for alg, kw in (("wiener", CELLS["wiener"]), ("omlsa", CELLS["omlsa"]),
                        ("ss", CELLS["ss"]), ("mmse", CELLS["mmse"])):
            for n_fft, hop in ((512, 128), (512, 32), (1024, 64), (1024, 256), (512, 64),
                               (512, 160), (1024, 512)):
                specs.append((s, alg, dict(kw, n_fft=n_fft, hop_length=hop, noise_percentile=10.0,
                                           noise_method="min_tracking")))
    together = eng.run(x, specs, clean=c, want_waveforms=True)
    yt = together["y"].cpu().numpy()
    for i, sp in enumerate(specs):
        alone = eng.run(x, [sp], clean=c, want_waveforms=True)
        ya = alone["y"][0].cpu().numpy()
        assert rel_max(yt[i], ya) <= 1e-6, sp
        assert abs(together["sse"][i] - alone["sse"][0]) <= 1e-9 * alone["sse"][0], sp
        assert together["finite"][i] and alone["finite"][0], sp
    with pytest.raises(ValueError, match="gain matrices"):
        eng.run(x, specs[1:2], clean=c, want_gains=True)
    with pytest.raises(ValueError, match="engine supports"):
        eng.run(x, [(0, "wiener", dict(CELLS["wiener"], n_fft=1024, hop_length=2048,
                                       noise_percentile=10.0, noise_method="percentile"))])
    with pytest.raises(ValueError, match="engine supports"):
        eng.run(x, [(0, "wiener", dict(CELLS["wiener"], n_fft=401, hop_length=160,
                                       noise_percentile=10.0, noise_method="percentile"))])


@pytest.mark.parametrize("n_fft,hop", [(512, 32), (512, 64), (1024, 64)])
def test_short_hops_10s_vs_oracle(P, n_fft, hop):
    """10-s signals (5001 frames at hop 32) at the short hops, every algorithm,
    against the fp64 oracle at the north-star tolerance."""
    clean, noisy = make_pair(3, seconds=10.0)
    for alg, method in (("ss", "true_noise"), ("wiener", "percentile"),
                        ("mmse", "min_tracking"), ("omlsa", "min_tracking")):
        kw = dict(CELLS[alg], n_fft=n_fft, hop_length=hop, noise_percentile=10.0,
                  noise_method=method)
        if method == "true_noise":
            kw["clean_audio"] = clean
        y = _fn(P, alg)(noisy, 16000, **kw)
        ref = ORACLE[alg](noisy, 16000, **kw)
        assert rel_l2(y, ref) <= TOL and rel_max(y, ref) <= TOL, (alg, rel_l2(y, ref))


def test_generic_shapes_match_reference_golden(P):
    """cse_enhance_cells_generic (any even n_fft in [64, 4096], any hop up to
    n_fft; here 128/32, 256/64, 512/160, 512/512, 1024/512, 2048/512 and the
    direct-DFT shapes 400/160, 320/80) through the plugins against the
    reference's outputs (float32-stored)."""
    g = load_golden("generic_shapes_0p5s.npz")
    noisy, clean = g["noisy"], g["clean"].astype(np.float64)
    n = 0
    for key in g.files:
        if not key.startswith("y|"):
            continue
        alg, method, n_fft, hop = key.split("|")[1:]
        kw = dict(CELLS[alg], n_fft=int(n_fft), hop_length=int(hop), noise_percentile=10.0,
                  noise_method=method)
        if method == "true_noise":
            kw["clean_audio"] = clean
        y = _fn(P, alg)(noisy, 16000, **kw)
        ref = g[key].astype(np.float64)
        assert y.shape == ref.shape, key
        assert rel_l2(y, ref) <= TOL and rel_max(y, ref) <= TOL, (key, rel_l2(y, ref))
        n += 1
    assert n == 108


@pytest.mark.parametrize("n_fft,hop", [(256, 80), (512, 160), (2048, 512), (400, 160), (4096, 1024)])
def test_generic_shapes_10s_vs_oracle(P, n_fft, hop):
    """10-s signals at generic shapes, every algorithm, against the oracle."""
    clean, noisy = make_pair(4, seconds=10.0)
    for alg, method in (("ss", "true_noise"), ("wiener", "percentile"),
                        ("mmse", "min_tracking"), ("omlsa", "min_tracking")):
        kw = dict(CELLS[alg], n_fft=n_fft, hop_length=hop, noise_percentile=10.0,
                  noise_method=method)
        if method == "true_noise":
            kw["clean_audio"] = clean
        y = _fn(P, alg)(noisy, 16000, **kw)
        ref = ORACLE[alg](noisy, 16000, **kw)
        assert rel_l2(y, ref) <= TOL and rel_max(y, ref) <= TOL, (alg, rel_l2(y, ref))


HOP1_SLICE = slice(4000, 5600)  # a voiced stretch of make_pair(4, 1.0) and make_pair(8, 2.0)


@pytest.mark.parametrize("n_fft,hop,seconds", [(64, 16, 1.0), (64, 64, 1.0), (66, 22, 1.0),
                                               (4000, 1000, 2.0), (4094, 2047, 2.0),
                                               (64, 1, None), (130, 1, None)])
def test_generic_edge_shapes_vs_oracle(P, n_fft, hop, seconds):
    """The shapes no other test runs through the layers above the STFT: n_fft
    64 (stft_kernel<64>, B = 33), hop = n_fft, the direct DFT at 66 and above
    2048 (B = 2001 and 2048: the 9-bins-per-thread noise finish), and hop 1;
    every algorithm against the fp64 oracle at the north-star tolerance, on
    short clips so the oracle stays quick.  The hop-1 clips are 1600 samples
    from inside a 1-s pair: its first 1600 samples are silent, so the slice
    must hold speech (asserted).  No case is ill-conditioned in the oracle
    itself (test_tiny_lengths' check, asserted, never skipped on)."""
    clean, noisy = make_pair(4, seconds=seconds or 1.0)
    if seconds is None:
        clean, noisy = clean[HOP1_SLICE].copy(), noisy[HOP1_SLICE].copy()
        assert len(clean) == 1600 and np.sqrt(np.mean(clean ** 2)) > 0.01
    for alg, method in (("ss", "true_noise"), ("wiener", "percentile"),
                        ("mmse", "min_tracking"), ("omlsa", "min_tracking")):
        kw = dict(CELLS[alg], n_fft=n_fft, hop_length=hop, noise_percentile=10.0,
                  noise_method=method)
        if method == "true_noise":
            kw["clean_audio"] = clean
        ref = ORACLE[alg](noisy, 16000, **kw)
        cond = rel_l2(ORACLE[alg](noisy * (1 + 1e-9), 16000, **kw), ref)
        print(f"{n_fft}/{hop} {alg}: oracle conditioning {cond:.2e}")
        assert cond <= 1e-6, (alg, cond)
        y = _fn(P, alg)(noisy, 16000, **kw)
        assert y.shape == ref.shape and np.all(np.isfinite(y))
        assert rel_l2(y, ref) <= TOL and rel_max(y, ref) <= TOL, (alg, rel_l2(y, ref))


@pytest.mark.parametrize("n_fft,hop", [(400, 160), (2048, 512), (256, 64), (4096, 1024),
                                       (64, 16), (4000, 1000), (4094, 2047), (64, 1)])
def test_noise_estimation_generic_shapes(P, n_fft, hop):
    """plugins.noise_estimation at STFT shapes beyond the grid's (the generic
    STFT: radix 2 or, at 400, 4000 and 4094, the direct DFT; B = 33, 2001 and
    2048 bins in the noise kernels) against the oracle's estimators; fp32
    storage of fp64 estimates, rtol 1e-6.  At hop 1 the clip is 1600 voiced
    samples of the pair (1601 frames): the whole pair would be 32001 frames,
    past the 16384 the estimators sort."""
    clean, noisy = make_pair(8, seconds=2.0)
    if hop == 1:
        clean, noisy = clean[HOP1_SLICE].copy(), noisy[HOP1_SLICE].copy()
        assert np.sqrt(np.mean(clean ** 2)) > 0.01
    for method in ("percentile", "min_tracking", "true_noise"):
        kw = dict(method=method, n_fft=n_fft, hop_length=hop, percentile=15.0,
                  clean_audio=clean, eps=1e-10)
        N = P.noise_estimation(noisy, 16000, **kw)
        ref = oracle.noise_estimation(noisy, 16000, **kw)
        assert N.shape == ref.shape, (method, N.shape, ref.shape)
        np.testing.assert_allclose(N, ref, rtol=1e-6, atol=0, err_msg=method)


def test_generic_gains_and_sse_match_oracle():
    """The generic kernel's gain matrices against the oracle's gain loops, and
    its SNR error sums against the oracle's (clean-scored, lag 0)."""
    import torch
    from classical_speech_enhancement_amd.engine import Engine
    from oracle import gain_ref
    clean, noisy = make_pair(6, seconds=1.0)
    eng = Engine()
    x = torch.as_tensor(noisy).cuda().view(1, -1)
    c = torch.as_tensor(clean).cuda().view(1, -1)
    specs = [(0, "wiener", dict(CELLS["wiener"], n_fft=256, hop_length=64,
                                 noise_percentile=20.0, noise_method="min_tracking")),
             (0, "mmse", dict(CELLS["mmse"], n_fft=512, hop_length=160, noise_percentile=10.0,
                               noise_method="percentile")),
             (0, "omlsa", dict(CELLS["omlsa"], n_fft=2048, hop_length=512,
                                noise_percentile=10.0, noise_method="min_tracking")),
             # the direct-DFT branch (n_fft not a power of two) and the smallest n_fft
             (0, "mmse", dict(CELLS["mmse"], n_fft=400, hop_length=160, noise_percentile=10.0,
                               noise_method="min_tracking")),
             (0, "wiener", dict(CELLS["wiener"], n_fft=400, hop_length=160,
                                 noise_percentile=20.0, noise_method="percentile")),
             (0, "omlsa", dict(CELLS["omlsa"], n_fft=64, hop_length=16, noise_percentile=10.0,
                                noise_method="min_tracking")),
             (0, "mmse", dict(CELLS["mmse"], n_fft=64, hop_length=16, noise_percentile=10.0,
                               noise_method="percentile"))]
    res = eng.run(x, specs, clean=c, want_gains=True)
    for i, ((sig, alg, p), G) in enumerate(zip(specs, res["G"])):
        Y, Pw, N = gain_ref.analyse(noisy, 16000, p["n_fft"], p["hop_length"],
                                    p["noise_percentile"], p["noise_method"], None,
                                    {"wiener": 1e-10, "mmse": 1e-12, "omlsa": 1e-10}[alg])
        if alg == "wiener":
            ref = gain_ref.wiener_gains(Pw, np.maximum(N, 1e-10), p["alpha"], p["gain_floor"])
        elif alg == "mmse":
            if N.ndim == 2 and N.shape[1] > 1:  # a per-frame estimate is smoothed (mmse.py:48-54)
                N = gain_ref.smooth_noise(N, 0.98)
            ref = gain_ref.mmse_gains(Pw, N, p["alpha"], p["ksi_min"], p["gain_min"], p["gain_max"])
        else:
            Ns = gain_ref.smooth_noise(np.maximum(N, 1e-10), p["noise_mu"])
            ref = gain_ref.omlsa_gains(Pw, Ns, p["alpha"], p["ksi_min"], p["q"], p["gain_floor"])
        Gd = G.double().cpu().numpy().T
        assert Gd.shape == ref.shape, (alg, p["n_fft"], Gd.shape, ref.shape)
        assert rel_l2(Gd, ref) < 1e-5, (alg, p["n_fft"], rel_l2(Gd, ref))
        y = ORACLE[alg](noisy, 16000, **p)
        sse_ref = float(np.sum((clean - np.clip(y, -1, 1)) ** 2))
        assert abs(res["sse"][i] - sse_ref) <= 1e-5 * sse_ref, (alg, res["sse"][i], sse_ref)
        assert res["finite"][i]


def test_config1_ss_true_noise_10s(P):
    g = load_golden("config1_ss_true_noise_10s.npz")
    clean, noisy = make_pair(0, seconds=10.0)
    y = P.spectral_subtraction(noisy, 16000, alpha=1.5, beta=0.001, n_fft=512, hop_length=128,
                               noise_percentile=10.0, noise_method="true_noise",
                               clean_audio=clean)
    assert rel_l2(y, g["y"]) <= TOL and rel_max(y, g["y"]) <= TOL


def test_short_clip_edge_cases(P):
    g = load_golden("short_clips.npz")
    for tag in ("t3", "t20"):
        noisy = g[f"noisy|{tag}"]
        for alg in CELLS:
            for method in ("percentile", "min_tracking"):
                y = _fn(P, alg)(noisy, 16000, **dict(CELLS[alg], n_fft=512, hop_length=128,
                                                     noise_percentile=20.0, noise_method=method))
                ref = g[f"y|{tag}|{alg}|{method}"]
                assert rel_l2(y, ref) <= TOL and rel_max(y, ref) <= TOL, (tag, alg, method)


def test_tiny_lengths(P):
    """1..700-sample inputs (repeated reflect padding, single frame) against the
    reference fixture; the empty input raises ValueError."""
    g = load_golden("tiny_clips.npz")
    for key in g.files:
        kind, rest = key.split("|", 1)
        if kind not in ("y", "err"):
            continue
        n, alg, method, n_fft, hop = rest.split("|")
        noisy = g[f"noisy|{n}"]
        kw = dict(CELLS[alg], n_fft=int(n_fft), hop_length=int(hop), noise_percentile=20.0,
                  noise_method=method)
        if kind == "err":
            with pytest.raises(ValueError):
                _fn(P, alg)(noisy, 16000, **kw)
            continue
        y = _fn(P, alg)(noisy, 16000, **kw)
        ref = g[key]
        assert len(y) == len(ref)
        assert np.all(np.isfinite(y)), key
        # SS on 1-2 samples is ill-conditioned in the reference itself: its
        # output is set by the phase of FFT rounding noise in the (exactly
        # zero) bins above bin 1, because beta*N dominates there.  A 1e-9
        # relative input perturbation moves the fp64 oracle by 40-70 %, so
        # only finiteness and length are checked for such cases.
        cond = rel_l2(ORACLE[alg](noisy * (1 + 1e-9), 16000, **kw), ref)
        if cond > 1e-6:
            continue
        if np.max(np.abs(ref)) == 0:
            assert np.max(np.abs(y)) == 0, key
            continue
        assert rel_l2(y, ref) <= TOL and rel_max(y, ref) <= TOL, (key, rel_l2(y, ref))


def test_unknown_method_and_missing_clean_raise(P):
    _, noisy = make_pair(1, seconds=0.5)
    with pytest.raises(ValueError, match="Unbekannte Methode"):
        P.wiener_filter(noisy, 16000, 512, 128, 0.95, 0.05, 10.0, "bogus")
    with pytest.raises(ValueError, match="TrueNoiseEstimator"):
        P.wiener_filter(noisy, 16000, 512, 128, 0.95, 0.05, 10.0, "true_noise")
    # an odd n_fft: the reference's istft infers n_fft - 1 from the bins and
    # rejects the longer window (librosa ParameterError); the mirror raises too
    with pytest.raises(ValueError, match="even n_fft"):
        P.wiener_filter(noisy, 16000, 511, 128, 0.95, 0.05, 10.0, "percentile")
    # even, but outside [64, 4096]: refused for its size (the host-side twin:
    # test_engine_host.test_route_refusals_name_their_reason)
    for n_fft in (8192, 62):
        with pytest.raises(ValueError, match=r"n_fft in \[64, 4096\]"):
            P.mmse(noisy, 16000, 0.98, 0.01, 0.05, 1.0, n_fft, 16, 10.0, "percentile")
    for hop in (0, 513):
        with pytest.raises(ValueError, match=r"hop in \[1, n_fft\]"):
            P.wiener_filter(noisy, 16000, 512, hop, 0.95, 0.05, 10.0, "percentile")


def test_gain_matrices_match_oracle_gains():
    """The recursion alone: device G vs oracle gain loops on the same P, N."""
    import torch
    from classical_speech_enhancement_amd.engine import Engine
    from oracle import gain_ref
    clean, noisy = make_pair(2, seconds=1.0)
    eng = Engine()
    x = torch.as_tensor(noisy).cuda().view(1, -1)
    specs = [(0, "wiener", dict(CELLS["wiener"], n_fft=512, hop_length=128,
                                 noise_percentile=20.0, noise_method="min_tracking")),
             (0, "mmse", dict(CELLS["mmse"], n_fft=512, hop_length=256, noise_percentile=10.0,
                               noise_method="percentile")),
             (0, "omlsa", dict(CELLS["omlsa"], n_fft=1024, hop_length=256,
                                noise_percentile=10.0, noise_method="min_tracking"))]
    res = eng.run(x, specs, want_gains=True)
    for (sig, alg, p), G in zip(specs, res["G"]):
        Y, Pw, N = gain_ref.analyse(noisy, 16000, p["n_fft"], p["hop_length"],
                                    p["noise_percentile"], p["noise_method"], None,
                                    {"wiener": 1e-10, "mmse": 1e-12, "omlsa": 1e-10}[alg])
        if alg == "wiener":
            ref = gain_ref.wiener_gains(Pw, np.maximum(N, 1e-10), p["alpha"], p["gain_floor"])
        elif alg == "mmse":
            ref = gain_ref.mmse_gains(Pw, N, p["alpha"], p["ksi_min"], p["gain_min"], p["gain_max"])
        else:
            Ns = gain_ref.smooth_noise(np.maximum(N, 1e-10), p["noise_mu"])
            ref = gain_ref.omlsa_gains(Pw, Ns, p["alpha"], p["ksi_min"], p["q"], p["gain_floor"])
        Gd = G.double().cpu().numpy().T
        assert rel_l2(Gd, ref) < 1e-5, (alg, rel_l2(Gd, ref))
        assert np.max(np.abs(Gd - ref)) < 1e-4, alg


def test_bin_m2_by_one_wave_matches_the_per_lane_form():
    """The sweep kernels evaluate bin M/2 of every cell in one wave per frame
    (cse_enhance.hip WG::M2C, r06); the gain-writing kernels (want_gains) keep
    the per-lane form.  Same cells through both: waveforms and SNR sums agree
    to rounding (the same arithmetic on the same row values; printed whether
    bit for bit), every algorithm, both n_fft, every frame parity, lag 0."""
    import torch
    from classical_speech_enhancement_amd.engine import Engine
    clean, noisy = make_pair(6, seconds=1.3)
    eng = Engine()
    x = torch.as_tensor(noisy).cuda().view(1, -1)
    c = torch.as_tensor(clean).cuda().view(1, -1)
    specs = []
    for n_fft, hop in ((512, 128), (512, 256), (1024, 256), (1024, 128)):
        for alg in ("ss", "wiener", "mmse", "omlsa"):
            name = {"ss": "spectralSubtractor"}.get(alg, alg)
            specs.append((0, name, dict(CELLS[alg], n_fft=n_fft, hop_length=hop, noise_percentile=20.0,
                                        noise_method="min_tracking")))
    a = eng.run(x, specs, clean=c, want_waveforms=True)
    b = eng.run(x, specs, clean=c, want_waveforms=True, want_gains=True)
    ya, yb = a["y"].double().cpu().numpy(), b["y"].double().cpu().numpy()
    same = [bool(np.array_equal(ya[j], yb[j])) for j in range(len(specs))]
    print("bit-identical waveforms:", sum(same), "of", len(specs))
    for j, (_, alg, p) in enumerate(specs):
        scale = np.max(np.abs(yb[j]))
        assert np.max(np.abs(ya[j] - yb[j])) <= 1e-6 * scale, (alg, p["n_fft"], p["hop_length"])
        assert abs(a["sse"][j] - b["sse"][j]) <= 1e-6 * b["sse"][j], (alg, p["n_fft"])
    assert a["finite"].all() and b["finite"].all()


@pytest.mark.parametrize("v_max", [5.0, 20.0, 80.0, 150.0])
def test_omlsa_v_max_against_oracle(P, v_max):
    """OMLSA's v_max (advanced_mmse.py signature default 80, not swept by the
    grid) below the LSA clamp, between it and 80, and beyond fp32's e^v range
    (the kernel caps it at 80, where p = 1 in fp32 already): enhanced waveform
    vs the fp64 oracle."""
    _, noisy = make_pair(3, seconds=1.5)
    for n_fft, hop in ((512, 128), (1024, 256)):
        kw = dict(CELLS["omlsa"], n_fft=n_fft, hop_length=hop, noise_percentile=20.0,
                  noise_method="min_tracking", v_max=v_max)
        y = P.advanced_mmse(noisy, 16000, **kw)
        ref = oracle.advanced_mmse(noisy, 16000, **kw)
        assert np.all(np.isfinite(y))
        assert rel_l2(y, ref) <= TOL and rel_max(y, ref) <= TOL, (n_fft, rel_l2(y, ref))


def test_grid_snr_table_matches_reference(P):
    """Full HEAD grid on a 0.5-s pair: per-cell SNR of the clipped waveform."""
    import torch
    from classical_speech_enhancement_amd.engine import Engine, snr_db
    g = load_golden("grid_snr_0p5s.npz")
    clean, noisy = g["clean"], g["noisy"]
    eng = Engine()
    x = torch.as_tensor(noisy).cuda().view(1, -1)
    c = torch.as_tensor(clean).cuda().view(1, -1)
    ps = float(np.sum(clean ** 2))
    for short, name in (("ss", "spectralSubtractor"), ("mmse", "mmse"), ("wiener", "wiener"),
                        ("omlsa", "omlsa")):
        cells = oracle.grid_cells(oracle.GRIDS[name])
        res = eng.run(x, [(0, name, p) for p in cells], clean=c)
        assert res["finite"].all()
        snr = snr_db(res["sse"], ps)
        np.testing.assert_allclose(snr, g[f"snr_lag0|{short}"], rtol=0, atol=2e-4,
                                   err_msg=name)


def test_grid_snr_aligned_matches_reference(P):
    """finalize_enhanced on the device: the reference's own per-cell SNR after
    cross-correlation alignment (speech_enhancement_comparison.py:92-106), full
    HEAD grid on a 0.5-s pair — 852 of the 1920 MMSE cells have a non-zero lag."""
    import torch
    from classical_speech_enhancement_amd.engine import Engine, snr_db
    g = load_golden("grid_snr_0p5s.npz")
    clean, noisy = g["clean"], g["noisy"]
    eng = Engine()
    x = torch.as_tensor(noisy).cuda().view(1, -1)
    c = torch.as_tensor(clean).cuda().view(1, -1)
    ps = float(np.sum(clean ** 2))
    moved = 0
    for short, name in (("ss", "spectralSubtractor"), ("mmse", "mmse"), ("wiener", "wiener"),
                        ("omlsa", "omlsa")):
        cells = oracle.grid_cells(oracle.GRIDS[name])
        res = eng.run(x, [(0, name, p) for p in cells], clean=c, align=True)
        assert res["finite"].all()
        assert (res["xcorr_status"] == 0).all()
        moved += int(np.sum(res["lag"] != 0))
        snr = snr_db(res["sse"], ps)
        np.testing.assert_allclose(snr, g[f"snr|{short}"], rtol=0, atol=2e-4, err_msg=name)
    assert moved >= 800


def test_alignment_lags_10s_vs_oracle(P):
    """10-s pair: device lags and aligned SNR of sampled MMSE / SS cells against
    the oracle's align_lag / finalize on its own fp64 outputs (n = 32000
    correlated samples, 7 FFT blocks of 4,992)."""
    import torch
    from classical_speech_enhancement_amd.engine import Engine, snr_db
    clean, noisy = make_pair(5, seconds=10.0)
    eng = Engine()
    x = torch.as_tensor(noisy).cuda().view(1, -1)
    c = torch.as_tensor(clean).cuda().view(1, -1)
    rng = np.random.default_rng(1)
    cells = []
    for name in ("mmse", "spectralSubtractor"):
        grid = [p for p in oracle.grid_cells(oracle.GRIDS[name]) if p["n_fft"] == 512]
        cells += [(name, grid[i]) for i in rng.choice(len(grid), 6, replace=False)]
    res = eng.run(x, [(0, a, p) for a, p in cells], clean=c, align=True)
    ps = float(np.sum(clean ** 2))
    for j, (name, p) in enumerate(cells):
        y = oracle.ALGORITHMS[name](noisy, 16000, **p)
        lag = oracle.align_lag(clean, y, 16000)
        assert res["lag"][j] == (lag or 0), (name, p, res["lag"][j], lag)
        e = oracle.finalize_enhanced(y, clean, 16000)
        ref = oracle.calculate_snr(clean, e)
        assert abs(snr_db(res["sse"][j:j + 1], ps)[0] - ref) < 2e-4, (name, p)


@pytest.mark.parametrize("case", ["zero", "dc", "dc_noise", "tone", "shift40"])
def test_alignment_flat_and_periodic_heads(P, case):
    """Heads whose correlation with the clean head is flat (more than 64 lags
    within the fp32 margin of the maximum: every one re-evaluated in fp64, XG
    lags per pass) or periodic, against the oracle's align_lag
    (speech_enhancement_comparison.py:38-69; np.argmax takes the first of
    equal values):
      zero      all-zero head: every c(l) is 0 -> lag -max_lag (early out);
      dc        a constant head: sig0 = 0 exactly, c(l) = 0 -> lag -max_lag,
                though the fp32 FFT of the raw head sees 0.25 (all 3,201 lags
                inside its margin); the centred pass sees 0 -> early out;
      dc_noise  0.5 + 1e-4 noise: all 3,201 lags within the raw pass's
                margin, a handful within the centred pass's, whose fp64
                re-evaluation picks the true maximum;
      tone      a 37-sample-period sinusoid: periodic peaks;
      shift40   the clean signal delayed by 40 samples (f32): lag -40.
    Correctness only: the per-call time of these heads is measured by
    tools/time_alignment.py (HIP events around the cse_xcorr_lag launch,
    profiles/r06_alignment_heads.json), not asserted here."""
    from classical_speech_enhancement_amd import _lib
    from classical_speech_enhancement_amd.engine import Engine
    from classical_speech_enhancement_amd.prepare import alignment_lag_status
    clean, _ = make_pair(3, 3.0)
    n = len(clean)
    rng = np.random.default_rng(5)
    head = {
        "zero": np.zeros(n),
        "dc": np.full(n, 0.25),
        "dc_noise": 0.5 + 1e-4 * rng.standard_normal(n),
        "tone": 0.3 * np.sin(2 * np.pi * np.arange(n) / 37.0),
        "shift40": np.roll(clean, 40),
    }[case].astype(np.float32).astype(np.float64)
    eng = Engine()
    ref = oracle.align_lag(clean, head, 16000)
    lag, status = alignment_lag_status(clean, head, 16000, eng)
    print(f"{case}: lag {lag} (oracle {ref}), status {status}")
    assert lag == ref, (case, lag, ref)
    if case in ("zero", "dc", "dc_noise"):
        assert status == _lib.XCORR_FLAT and lag == (-1600 if case != "dc_noise" else lag)
    if case == "shift40":
        assert lag == -40 and status == _lib.XCORR_OK


@pytest.mark.parametrize("length", [4993, 7999, 9985])
def test_alignment_odd_and_block_edge_lengths(P, length):
    """Correlated heads of odd length and of one sample past a 4992-sample
    block boundary (4993, 9985): the last block's final sample must be read,
    the samples past n must not (lags and aligned SNR vs the oracle)."""
    import torch
    from classical_speech_enhancement_amd.engine import Engine, snr_db
    clean, noisy = make_pair(11, seconds=0.7)
    clean, noisy = clean[:length].copy(), noisy[:length].copy()
    eng = Engine()
    x = torch.as_tensor(noisy).cuda().view(1, -1)
    c = torch.as_tensor(clean).cuda().view(1, -1)
    rng = np.random.default_rng(length)
    grid = [p for p in oracle.grid_cells(oracle.GRIDS["mmse"]) if p["n_fft"] == 512]
    cells = [grid[i] for i in rng.choice(len(grid), 8, replace=False)]
    res = eng.run(x, [(0, "mmse", p) for p in cells], clean=c, align=True)
    assert (res["xcorr_status"] == 0).all()
    ps = float(np.sum(clean ** 2))
    for j, p in enumerate(cells):
        y = oracle.ALGORITHMS["mmse"](noisy, 16000, **p)
        lag = oracle.align_lag(clean, y, 16000)
        assert res["lag"][j] == (lag or 0), (p, res["lag"][j], lag)
        ref = oracle.calculate_snr(clean, oracle.finalize_enhanced(y, clean, 16000))
        assert abs(snr_db(res["sse"][j:j + 1], ps)[0] - ref) < 2e-4, p


@pytest.mark.parametrize("n_fft", [512, 1024])
@pytest.mark.parametrize("alg", ["spectralSubtractor", "wiener", "mmse", "omlsa"])
def test_full_size_grid_properties(alg, n_fft):
    """10-s pair, one algorithm's half of the full grid (one n_fft): finite,
    deterministic, duplicate cells (min_tracking ignores noise_percentile)
    bit-identical, sampled cells within tolerance of the oracle."""
    import torch
    from classical_speech_enhancement_amd.engine import Engine
    clean, noisy = make_pair(4, seconds=10.0)
    eng = Engine()
    x = torch.as_tensor(noisy).cuda().view(1, -1)
    c = torch.as_tensor(clean).cuda().view(1, -1)
    cells = [p for p in oracle.grid_cells(oracle.GRIDS[alg]) if p["n_fft"] == n_fft]
    specs = [(0, alg, p) for p in cells]
    r1 = eng.run(x, specs, clean=c)
    r2 = eng.run(x, specs, clean=c)
    assert r1["finite"].all()
    assert np.array_equal(r1["sse"], r2["sse"])
    key = lambda p: tuple((k, v) for k, v in sorted(p.items()) if k != "noise_percentile")
    first, dup = {}, 0
    for i, p in enumerate(cells):
        if p["noise_method"] in ("min_tracking", "true_noise"):
            k = key(p)
            if k in first:
                assert r1["sse"][i] == r1["sse"][first[k]]
                dup += 1
            else:
                first[k] = i
    assert dup > 0
    rng = np.random.default_rng(0)
    pick = rng.choice(len(specs), 2, replace=False)
    res = eng.run(x, [specs[i] for i in pick], clean=c, want_waveforms=True)
    for j, i in enumerate(pick):
        kw = dict(cells[i])
        if kw["noise_method"] == "true_noise":
            kw["clean_audio"] = clean
        ref = oracle.ALGORITHMS[alg](noisy, 16000, **kw)
        y = res["y"][j].double().cpu().numpy()
        assert rel_l2(y, ref) <= TOL and rel_max(y, ref) <= TOL, (alg, cells[i])
        sse_ref = np.sum((clean - np.clip(ref, -1, 1)) ** 2)
        assert abs(res["sse"][j] - sse_ref) <= 1e-4 * sse_ref


def test_presentation_wavs_loose(P):
    """Real speech (the reference's committed WAVs): ≈1e-2 rel-L2, limited by the
    resampler stand-in and PCM16 — a loose end-to-end pin of the librosa parts."""
    g = load_golden("presentation_wavs.npz")
    for stem, var, fn in (("p257_090", "pesq", P.spectral_subtraction),
                          ("p257_090", "stoi", P.spectral_subtraction),
                          ("p257_135", "pesq", P.wiener_filter)):
        clean = g[f"clean|{stem}"].astype(np.float64)
        noisy = g[f"noisy|{stem}"].astype(np.float64)
        kw = {k.split("|")[-1]: g[k].item() for k in g.files
              if k.startswith(f"param|{stem}|{var}|")}
        if kw["noise_method"] == "true_noise":
            kw["clean_audio"] = clean
        y = fn(noisy, 16000, **kw)
        e = oracle.finalize_enhanced(y, clean, 16000)
        exp = g[f"expected|{stem}|{var}"].astype(np.float64) / 32768.0
        m = min(len(e), len(exp))
        assert rel_l2(e[:m], exp[:m]) < 1.5e-2, (stem, var)


def test_search_run_grid_on_device(P):
    """The rewritten sweep on the GPU: per-cell SNR table vs the oracle at lag 0,
    pairs of two lengths batched separately, and the selected cells' oracle
    scores within float noise of the oracle's own winners."""
    from classical_speech_enhancement_amd import search
    from _grid_worker import SMALL_GRIDS, oracle_compute
    pairs = [make_pair(i, s) for i, s in enumerate((1.2, 1.2, 1.5))]
    clean = [c for c, _ in pairs]
    noisy = [x for _, x in pairs]
    specs = search.job_specs(len(pairs), grids=SMALL_GRIDS)
    table, best = search.run_grid(clean, noisy, specs)
    ref = oracle_compute(clean, noisy, specs, np.arange(len(specs)))
    assert np.array_equal(table[:, 2], ref[:, 2])
    np.testing.assert_allclose(table[:, 1], ref[:, 1], rtol=0, atol=2e-4)
    # STOI of the device outputs (fp32 gains: outputs within 1e-6 of the
    # oracle's) against the oracle's STOI of its own outputs
    assert (ref[:, 3] > 0.3).mean() > 0.5  # most cells hold >= 30 STOI frames
    np.testing.assert_allclose(table[:, 3], ref[:, 3], rtol=0, atol=2e-6)
    for objective, col, tol in (("snr", 1, 1e-3), ("stoi", 3, 4e-6)):
        got = best if objective == "snr" else search.select_best(specs, table, "stoi")
        ref_best = search.select_best(specs, ref, objective)
        for k, (cid, score) in got.items():
            rcid, rscore = ref_best[k]
            assert cid >= 0 and rcid >= 0
            assert ref[cid, col] >= rscore - tol, (objective, k, cid, rcid)


def test_long_signal_beyond_8192_frames(P):
    """A 90-s clip: T = 11251 frames at hop 128 (the LDS sort holds up to
    16384), percentile and min-tracking estimators and two algorithms against
    the oracle; past 16384 frames the engine refuses with an error."""
    clean, noisy = make_pair(9, seconds=90.0)
    for alg, method in (("omlsa", "percentile"), ("wiener", "min_tracking")):
        kw = dict(CELLS[alg], n_fft=512, hop_length=128, noise_percentile=10.0,
                  noise_method=method)
        y = _fn(P, alg)(noisy, 16000, **kw)
        ref = ORACLE[alg](noisy, 16000, **kw)
        assert rel_l2(y, ref) <= TOL and rel_max(y, ref) <= TOL, (alg, method, rel_l2(y, ref))
    from classical_speech_enhancement_amd._lib import CseError
    long = np.tile(noisy, 3)  # 270 s: 33751 frames
    with pytest.raises(CseError):
        P.advanced_mmse(long, 16000, **dict(CELLS["omlsa"], n_fft=512, hop_length=128,
                                            noise_percentile=10.0, noise_method="percentile"))


def test_noise_params_and_short_clean_match_reference_golden(P):
    """Estimator constructor parameters through plugins.noise_estimation, and a
    clean reference shorter than the noisy signal (TrueNoise trim + frame
    edge-pad, noise_estimation.py:128-153) through noise_estimation and every
    algorithm plugin, against the reference's outputs."""
    from test_oracle_golden import _noise_param_cases
    g = load_golden("noise_params.npz")
    xs = {"n": g["noisy"], "s": g["short_noisy"]}
    for i, (method, kw) in enumerate(_noise_param_cases()):
        for tag, x in xs.items():
            for n_fft, hop in ((512, 128), (1024, 256)):
                N = P.noise_estimation(x, 16000, method=method, n_fft=n_fft, hop_length=hop,
                                       **kw)
                ref = g[f"N|{i}|{tag}|{n_fft}|{hop}"]
                assert N.shape == ref.shape, (i, tag)
                np.testing.assert_allclose(N, ref, rtol=1e-6, atol=0, err_msg=f"{i}|{tag}")
    clean, noisy = g["clean"], g["noisy"]
    n = 0
    for key in g.files:
        if key.startswith("Ntrue|"):
            m, n_fft, hop = map(int, key.split("|")[1:])
            N = P.noise_estimation(noisy, 16000, method="true_noise", n_fft=n_fft,
                                   hop_length=hop, clean_audio=clean[:m], eps=1e-12)
            assert N.shape == g[key].shape
            np.testing.assert_allclose(N, g[key], rtol=1e-6, atol=0, err_msg=key)
        elif key.startswith("y|"):
            m, alg, n_fft, hop = key.split("|")[1:]
            y = _fn(P, alg)(noisy, 16000, **dict(CELLS[alg], n_fft=int(n_fft),
                                                 hop_length=int(hop), noise_percentile=10.0,
                                                 noise_method="true_noise",
                                                 clean_audio=clean[:int(m)]))
            assert rel_l2(y, g[key]) <= TOL and rel_max(y, g[key]) <= TOL, key
            n += 1
    assert n == 24


@pytest.mark.parametrize("T_sec", [1.0, 20.0])
def test_percentile_pairs_equal_single_estimates(P, T_sec):
    """cse_noise_percentile_med2 (two percentiles sharing one eps: the frame
    energies once, then each percentile's selection and statistic) against
    cse_noise_percentile_med at the same eps, bit for bit: both outputs of a
    pair, and the odd estimate of a group (N_b = NULL), at T = 126 and 2,501
    (the wave-sort and LDS-sort statistic paths: T <= 2048 and above), plus the oracle's
    PercentileNoiseEstimator (noise_estimation.py:20-56) to 1e-6."""
    import torch
    from classical_speech_enhancement_amd import _lib
    from classical_speech_enhancement_amd.engine import Engine, _ptr, _stream
    eng = Engine()
    lib = eng.lib
    clean, noisy = make_pair(2, T_sec)
    x = torch.as_tensor(np.stack([noisy, clean])).cuda()
    _, Pw = eng.stft(x, 512, 128, want_y=False)
    S, T, B = Pw.shape
    med = torch.empty((S, B), dtype=torch.float64, device="cuda")
    ws = torch.empty(int(lib.cse_noise_workspace_bytes(S, T, B)), dtype=torch.uint8, device="cuda")
    st = _stream()
    _lib.check(lib.cse_noise_median(_ptr(Pw), S, T, B, _ptr(med), st), "median")
    for eps in (1e-10, 1e-12):
        one = {}
        for pct in (10.0, 20.0):
            o = torch.empty((S, B), dtype=torch.float32, device="cuda")
            _lib.check(lib.cse_noise_percentile_med(_ptr(Pw), _ptr(med), S, T, B, pct, eps, _ptr(o),
                                                    _ptr(ws), st), "med")
            one[pct] = o.cpu().numpy()
        a = torch.empty((S, B), dtype=torch.float32, device="cuda")
        b = torch.empty((S, B), dtype=torch.float32, device="cuda")
        _lib.check(lib.cse_noise_percentile_med2(_ptr(Pw), _ptr(med), S, T, B, 10.0, 20.0, eps,
                                                 _ptr(a), _ptr(b), _ptr(ws), st), "med2")
        assert np.array_equal(a.cpu().numpy(), one[10.0]) and np.array_equal(b.cpu().numpy(), one[20.0])
        c = torch.full((S, B), -1.0, dtype=torch.float32, device="cuda")
        _lib.check(lib.cse_noise_percentile_med2(_ptr(Pw), _ptr(med), S, T, B, 20.0, 0.0, eps,
                                                 _ptr(c), None, _ptr(ws), st), "med2 odd")
        assert np.array_equal(c.cpu().numpy(), one[20.0])
        for s in range(S):
            Pc = Pw[s].cpu().numpy().T  # (B, T) as the reference's estimator takes it
            for pct in (10.0, 20.0):
                ref = oracle.percentile_noise(Pc, eps=eps, percentile=pct)
                assert rel_l2(one[pct][s], np.ravel(ref)) < 1e-6, (T_sec, eps, s, pct)


@pytest.mark.parametrize("T", [65, 94, 100, 626, 1251, 2048])
def test_noise_median_exact(T):
    """cse_noise_median (the selection kernel for 65 <= T <= 2048) equals
    numpy's median over frames bit for bit (noise_estimation.py:34/:101-102
    np.median): random powers over 40 binades, columns of ties, all-equal and
    all-zero columns, odd and even T."""
    import torch
    from classical_speech_enhancement_amd import _lib
    from classical_speech_enhancement_amd.engine import Engine, _ptr, _stream
    lib = Engine().lib
    rng = np.random.default_rng(T)
    S, B = 3, 257
    P = 10.0 ** rng.uniform(-12, 3, size=(S, T, B))
    P[0, :, 1] = 0.5                                     # all equal
    P[0, :, 2] = 0.0                                     # all zero
    P[1, :, 3] = rng.integers(0, 4, T) * 0.25            # heavy ties
    P[1, :, 4] = np.where(rng.random(T) < 0.6, 1e-10, P[1, :, 4])  # a floor shared by most frames
    P[2, :, 5] = np.arange(T)[::-1] * 1e-3               # monotone
    Pd = torch.as_tensor(P).cuda()
    med = torch.empty((S, B), dtype=torch.float64, device="cuda")
    _lib.check(lib.cse_noise_median(_ptr(Pd), S, T, B, _ptr(med), _stream()), "median")
    ref = np.median(P, axis=1)
    got = med.cpu().numpy()
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:5]


@pytest.mark.parametrize("n_fft,sec", [(512, 0.75), (1024, 0.75), (512, 10.0), (1024, 10.0)])
def test_noise_median_exact_on_stft(n_fft, sec):
    """The same on STFT powers of speech-like pairs (the engine's own P: ties
    from the reflect padding, columns spanning a few binades, the pad lanes of a
    short column sharing the keys' prefix), T = 94 and 1,251 frames."""
    import torch
    from classical_speech_enhancement_amd import _lib
    from classical_speech_enhancement_amd.engine import Engine, _ptr, _stream
    eng = Engine()
    clean, noisy = make_pair(6, sec)
    x = torch.as_tensor(np.stack([noisy, clean, noisy - clean])).cuda()
    _, Pw = eng.stft(x, n_fft, 128, want_y=False)
    S, T, B = Pw.shape
    med = torch.empty((S, B), dtype=torch.float64, device="cuda")
    _lib.check(eng.lib.cse_noise_median(_ptr(Pw), S, T, B, _ptr(med), _stream()), "median")
    ref = np.median(Pw.cpu().numpy(), axis=1)
    got = med.cpu().numpy()
    assert np.array_equal(got, ref), (T, B, np.argwhere(got != ref)[:5])


@pytest.mark.parametrize("T_sec", [1.0, 20.0])
def test_percentile_quad_equals_single_estimates(P, T_sec):
    """cse_noise_percentile_quad (two percentiles x two eps in four launches)
    against four cse_noise_percentile_med calls, bit for bit, with one output
    left NULL in a second call (T = 126 and 2,501 frames: the wave order
    statistics; the LDS path is the k > 2048 fallback)."""
    import torch
    from classical_speech_enhancement_amd import _lib
    from classical_speech_enhancement_amd.engine import Engine, _ptr, _stream
    eng = Engine()
    lib = eng.lib
    clean, noisy = make_pair(3, T_sec)
    x = torch.as_tensor(np.stack([noisy, clean, 0.5 * noisy])).cuda()
    _, Pw = eng.stft(x, 512, 128, want_y=False)
    S, T, B = Pw.shape
    med = torch.empty((S, B), dtype=torch.float64, device="cuda")
    ws = torch.empty(int(lib.cse_noise_workspace_bytes(S, T, B)), dtype=torch.uint8, device="cuda")
    st = _stream()
    _lib.check(lib.cse_noise_median(_ptr(Pw), S, T, B, _ptr(med), st), "median")
    one = {}
    for pct in (10.0, 20.0):
        for eps in (1e-10, 1e-12):
            o = torch.empty((S, B), dtype=torch.float32, device="cuda")
            _lib.check(lib.cse_noise_percentile_med(_ptr(Pw), _ptr(med), S, T, B, pct, eps, _ptr(o),
                                                    _ptr(ws), st), "med")
            one[(pct, eps)] = o.cpu().numpy()
    outs = {k: torch.full((S, B), -1.0, dtype=torch.float32, device="cuda") for k in one}
    _lib.check(lib.cse_noise_percentile_quad(
        _ptr(Pw), _ptr(med), S, T, B, 10.0, 20.0, 1e-10, 1e-12, _ptr(outs[(10.0, 1e-10)]),
        _ptr(outs[(10.0, 1e-12)]), _ptr(outs[(20.0, 1e-10)]), _ptr(outs[(20.0, 1e-12)]), _ptr(ws),
        st), "quad")
    for k, o in outs.items():
        assert np.array_equal(o.cpu().numpy(), one[k]), (T_sec, k)
    skip = torch.full((S, B), -1.0, dtype=torch.float32, device="cuda")
    _lib.check(lib.cse_noise_percentile_quad(
        _ptr(Pw), _ptr(med), S, T, B, 10.0, 20.0, 1e-10, 1e-12, None, None, _ptr(skip), None,
        _ptr(ws), st), "quad, one output")
    assert np.array_equal(skip.cpu().numpy(), one[(20.0, 1e-10)])


@pytest.mark.parametrize("B", [257, 513])
def test_noise_finish_jobs_bit_exact(P, B):
    """cse_noise_finish (the batched noise-row post-processing the engine runs
    after the estimators) against its numpy restatement, bit for bit: the
    smoothing s_t = mu s_{t-1} + (1 - mu) n_t in fp64 in numpy's order
    (mmse.py:48-54, advanced_mmse.py:60-66), the fix_length zero pad of a static
    row (spectral_subtractor.py:40-41, advanced_mmse.py:54-55: n_t = 0 for t >= 1)
    and the in-loop floor 1/max(N, eps) in fp32 (wiener_filter.py:58, mmse.py:71,
    advanced_mmse.py:87).  Frame counts around the kernel's 16-frame load blocks
    (1, 2, 16, 17, 33, 1,251)."""
    import torch
    from classical_speech_enhancement_amd import _lib
    from classical_speech_enhancement_amd.engine import Engine, _ptr, _stream
    eng = Engine()
    lib = eng.lib
    rng = np.random.default_rng(7)
    S = 3
    # (src_frames, out_frames, mu, inv_eps)
    cases = []
    for T in (1, 2, 16, 17, 33, 1251):
        cases += [(T, T, 0.98, 1e-10), (T, T, 0.0, 0.0), (T, T, 0.92, 0.0),
                  (1, T, 0.95, 1e-10), (1, T, 0.0, 0.0)]
    cases += [(1, 1, 0.0, 1e-12), (1, 1, 0.5, 0.0)]
    srcs, src_off, o = [], [], 0
    for (sf, _, _, _) in cases:
        a = rng.lognormal(-12.0, 3.0, size=(S, sf, B)).astype(np.float32)
        a[:, :, ::37] = 0.0  # below any eps: the floor decides
        srcs.append(a)
        src_off.append(o)
        o += a.size
    src = np.concatenate([a.ravel() for a in srcs])
    jt = np.zeros(len(cases), dtype=_lib.NOISE_JOB_DTYPE)
    dst_off, d = [], 0
    for j, (sf, of, mu, ie) in enumerate(cases):
        dst_off.append(d)
        jt[j] = (src_off[j], d, sf, of, mu, ie)
        d += S * of * B
    src_d = torch.as_tensor(src).cuda()
    dst_d = torch.full((d,), np.nan, dtype=torch.float32, device="cuda")
    jobs_d = torch.from_numpy(jt.view(np.uint8).copy()).cuda()
    _lib.check(lib.cse_noise_finish(_ptr(jobs_d), len(cases), S, B, _ptr(src_d), _ptr(dst_d),
                                    _stream()), "cse_noise_finish")
    out = dst_d.cpu().numpy()
    for j, (sf, of, mu, ie) in enumerate(cases):
        n = np.zeros((S, of, B))
        n[:, :min(sf, of)] = srcs[j][:, :min(sf, of)].astype(np.float64)
        ref = np.empty((S, of, B))
        s = n[:, 0].copy()
        ref[:, 0] = s
        for t in range(1, of):
            s = mu * s + (1.0 - mu) * n[:, t]
            ref[:, t] = s
        r32 = ref.astype(np.float32)
        if ie > 0.0:
            r32 = np.float32(1.0) / np.maximum(r32, np.float32(ie))
        got = out[dst_off[j]:dst_off[j] + S * of * B].reshape(S, of, B)
        assert np.array_equal(got, r32), (cases[j], np.abs(got - r32).max())
