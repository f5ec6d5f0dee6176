"""Device extended STOI (cse_estoi_prepare / cse_estoi_cells) against the numpy
restatement of include/cse_estoi.h (tests/_estoi_ref.py); needs a GPU.

Tolerance: |ESTOI_dev - ESTOI_ref| <= 1e-8, the project's STOI tolerance and
1/100 of the selection tolerance on STOI (1e-6,
speech_enhancement_comparison.py:183).  The device computes in fp64; the test
signals enter as the f32 the enhance kernel writes, and the restatement sees
the same f32 values.  pystoi's jittered form differs from the restatement by at
most 6.5e-14 on the synthetic pairs and 1.6e-11 on the 1e-6-scaled one (CPU).
Worst |device - restatement| observed on an MI355X over every case of this
file: 2.6e-13 (the 1-s synthetic pair; the 16-kHz and 22.05-kHz batches and
the grid cells 1e-14 to 2e-13, the 1e-6-scaled signal 2.8e-14, the 10-kHz
tile-edge, fragmented-silence and clean-against-itself cases 0 to 1e-16).
Each case prints its difference (pytest -s).
"""

import numpy as np
import pytest

import _estoi_ref
from oracle import stoi_ref

pytestmark = pytest.mark.gpu
TOL = 1e-8
WORST = {"diff": 0.0}


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from classical_speech_enhancement_amd import metrics
    return metrics


def _f32(x):
    return np.asarray(x).astype(np.float32).astype(np.float64)


def _close(got, ref, what):
    d = abs(got - ref)
    WORST["diff"] = max(WORST["diff"], d)
    print(f"estoi {what}: device {got!r} ref {ref!r} diff {d:.3e} (worst so far "
          f"{WORST['diff']:.3e})")
    assert d <= TOL, (what, got, ref)


@pytest.mark.parametrize("seconds", [1.0, 3.7])
def test_synthetic_pairs(dev, seconds):
    from classical_speech_enhancement_amd.synth import make_pair
    clean, noisy = make_pair(int(seconds * 10), seconds=seconds)
    got = dev.calculate_stoi(clean, noisy, 16000, extended=True)
    _close(got, _estoi_ref.calculate_estoi(clean, _f32(noisy), 16000), f"{seconds} s")
    # the default still scores plain STOI
    plain = dev.calculate_stoi(clean, noisy, 16000)
    assert abs(plain - stoi_ref.calculate_stoi(clean, _f32(noisy), 16000)) <= TOL
    assert abs(plain - got) > 1e-3


def test_short_and_no_frame(dev):
    from classical_speech_enhancement_amd.synth import make_pair
    clean, noisy = make_pair(4, seconds=0.4)
    assert _estoi_ref.estoi(clean, noisy, 16000) == 1e-5
    assert dev.calculate_stoi(clean, noisy, 16000, extended=True) == 1e-5
    assert dev.calculate_stoi(clean[:300], noisy[:300], 16000, extended=True) is None


def _stationary(n, seed):
    """Noise plus tones at 10 kHz: no frame is 40 dB below the loudest."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 10000.0
    clean = (0.1 * rng.standard_normal(n) + 0.2 * np.sin(2 * np.pi * 440.0 * t)
             + 0.1 * np.sin(2 * np.pi * 1730.0 * t + 1.0))
    return clean, clean + 0.15 * rng.standard_normal(n)


@pytest.mark.parametrize("M", [29, 30, 93, 94, 158])
def test_tile_edges_at_10_khz(dev, M):
    """J = M - 29 segments: none (1e-5), 1, 64 (one full tile), 65 (a full tile
    and a one-segment tile), 129 (three tiles)."""
    clean, test = _stationary(256 + 128 * M, M)
    test = _f32(test)
    assert _estoi_ref.frames(clean, test, 10000)[0].shape[0] == M
    got = dev.calculate_stoi(clean, test, 10000, extended=True)
    ref = _estoi_ref.estoi(clean, test, 10000)
    if M < 30:
        assert got == ref == 1e-5
    else:
        _close(got, ref, f"10 kHz M={M}")


def test_degenerate_test_signals(dev):
    from classical_speech_enhancement_amd.synth import make_pair
    clean, noisy = make_pair(77, seconds=2.0)
    assert dev.calculate_stoi(clean, np.zeros_like(clean), 16000, extended=True) == 0.0
    assert _estoi_ref.estoi(clean, np.zeros_like(clean), 16000) == 0.0
    for what, t in (("1e-6 x noisy", 1e-6 * noisy), ("clean", clean)):
        got = dev.calculate_stoi(clean, t, 16000, extended=True)
        _close(got, _estoi_ref.calculate_estoi(clean, _f32(t), 16000), what)


def test_fragmented_silence(dev):
    """The signal of test_gpu_stoi.test_fragmented_silence (3.7 s of it):
    frames dropped all along, so the kept frames are far from contiguous."""
    rng = np.random.default_rng(21)
    n = 59200
    t = np.arange(n)
    burst = ((t % 1120) < 480).astype(np.float64)
    clean = rng.standard_normal(n) * (burst + 1e-4)
    for k, test in enumerate((clean + 0.1 * rng.standard_normal(n), 0.5 * clean)):
        got = dev.calculate_stoi(clean, test, 16000, extended=True)
        _close(got, _estoi_ref.calculate_estoi(clean, _f32(test), 16000), f"fragmented {k}")


def _batch(dev, sr, L, clean, noisy, n_cells, max_lag, seed, extended=True):
    """n_cells outputs against two clean signals, each with its own gain (some
    beyond [-1, 1]: the clip runs) and lag; (plan, device scores, test signals)."""
    import torch
    from classical_speech_enhancement_amd.results import shift_and_fit
    rng = np.random.default_rng(seed)
    outs, sig, lags = [], [], []
    for c in range(n_cells):
        s = c % 2
        outs.append((noisy[s] * rng.uniform(0.5, 6.0)).astype(np.float32))
        sig.append(s)
        lags.append(int(rng.integers(-max_lag, max_lag + 1)) if c % 3 else 0)
    plan = dev.StoiPlan(torch.as_tensor(clean).cuda(), sr, extended=extended)
    yflat = torch.as_tensor(np.concatenate(outs)).cuda()
    got = plan.score(yflat, np.arange(n_cells) * L, sig, lag=lags, clip=True)
    tests = [shift_and_fit(outs[c].astype(np.float64), lags[c], L) for c in range(n_cells)]
    return plan, got, tests, sig, (yflat, lags)


def test_batched_cells_lag_and_clip(dev):
    from classical_speech_enhancement_amd.synth import make_pair
    L = 24000
    pairs = [make_pair(40 + i, seconds=L / 16000) for i in range(2)]
    clean = np.stack([c for c, _ in pairs])
    plan, got, tests, sig, (yflat, lags) = _batch(dev, 16000, L, clean, [n for _, n in pairs],
                                                  12, 1600, 9)
    for c in range(12):
        _close(got[c], _estoi_ref.estoi(clean[sig[c]], tests[c], 16000), f"batch cell {c}")
    # the extended workspace starts with the plain one: cse_stoi_cells on it
    # (the plan's plain branch) still returns plain STOI
    plan.extended = False
    plain = plan.score(yflat, np.arange(12) * L, sig, lag=lags, clip=True)
    for c in range(12):
        assert abs(plain[c] - stoi_ref.stoi(clean[sig[c]], tests[c], 16000)) <= TOL, c


def test_other_rate_batched_cells(dev):
    from scipy.signal import resample_poly
    from classical_speech_enhancement_amd.synth import make_pair
    sr, L = 22050, 33075
    g = np.gcd(sr, 16000)
    pairs = [make_pair(50 + i, seconds=1.5) for i in range(2)]
    at = [[resample_poly(x, sr // g, 16000 // g)[:L] for x in p] for p in pairs]
    clean = np.stack([c for c, _ in at])
    _, got, tests, sig, _ = _batch(dev, sr, L, clean, [n for _, n in at], 8, 2205, 13)
    for c in range(8):
        _close(got[c], _estoi_ref.estoi(clean[sig[c]], tests[c], sr), f"22.05 kHz cell {c}")


GRID = {"spectralSubtractor": {"alpha": [1.0, 2.0], "beta": [0.01, 0.1], "n_fft": [512],
                               "hop_length": [128], "noise_percentile": [10.0],
                               "noise_method": ["percentile", "min_tracking"]}}


def _cell_estoi(clean, noisy, params, lag):
    """ESTOI of one grid cell's plugin output, finalised like the sweep does."""
    from classical_speech_enhancement_amd import plugins
    from classical_speech_enhancement_amd.results import shift_and_fit
    y = plugins.spectral_subtraction(noisy, 16000, **params)
    return _estoi_ref.estoi(clean, shift_and_fit(y, int(lag), len(clean)), 16000)


def test_optimize_parameters_extended(dev):
    from classical_speech_enhancement_amd import search
    from classical_speech_enhancement_amd.synth import make_pair
    clean, noisy = make_pair(3, seconds=1.0)
    res = search.optimize_parameters(clean, noisy, 16000, "spectralSubtractor",
                                     GRID["spectralSubtractor"], extended=True)
    assert res["extended"] is True
    table = res["table"]
    specs = search.job_specs(1, ["spectralSubtractor"], GRID)
    assert table.shape == (8, search.NCOL) and (table[:, 2] == 1).all()
    for cid in range(8):
        _close(table[cid, 3], _cell_estoi(clean, noisy, specs[cid][2], table[cid, 4]),
               f"grid cell {cid}")
    _close(res["baseline"]["stoi"], _estoi_ref.estoi(clean, _f32(noisy), 16000), "baseline")
    sid = res["stoi"]["cell"]
    assert res["stoi"]["score"] == table[sid, 3]
    assert sid == search.select_best(specs, table, "stoi")[(0, "spectralSubtractor")][0]
    assert res["improvements"]["stoi"] == res["stoi"]["score"] - res["baseline"]["stoi"]
    # the default scores plain STOI and carries no flag
    plain = search.optimize_parameters(clean, noisy, 16000, "spectralSubtractor",
                                       GRID["spectralSubtractor"])
    assert "extended" not in plain
    assert np.abs(plain["table"][:, 3] - table[:, 3]).min() > 1e-3
    assert np.array_equal(plain["table"][:, [0, 1, 2, 4, 5]], table[:, [0, 1, 2, 4, 5]])


def test_run_sweep_extended(dev, tmp_path):
    import os
    from classical_speech_enhancement_amd import search
    from classical_speech_enhancement_amd.synth import make_pair
    clean, noisy = make_pair(5, seconds=1.0)
    rows = search.run_sweep([clean], [noisy], ["p05"], str(tmp_path), grids=GRID, extended=True)
    assert len(rows) == 1 and rows[0]["stoi_extended"] is True
    r = rows[0]
    specs = search.job_specs(1, ["spectralSubtractor"], GRID)
    table, _ = search.run_grid([clean], [noisy], specs, extended=True)
    sid, score = search.select_best(specs, table, "stoi")[(0, "spectralSubtractor")]
    assert r["stoi_stoiopt"] == score and r["best_params_stoi"] == specs[sid][2]
    _close(r["stoi_stoiopt"], _cell_estoi(clean, noisy, specs[sid][2], table[sid, 4]),
           "sweep winner")
    _close(r["stoi_noisy"], _estoi_ref.estoi(clean, _f32(noisy), 16000), "sweep baseline")
    for tag in ("stoi", "snr"):
        assert os.path.exists(os.path.join(
            tmp_path, "results_spectralSubtractor", f"p05_spectralSubtractor_optimized_{tag}.wav"))
    plain = search.run_sweep([clean], [noisy], ["p05"], str(tmp_path / "plain"), grids=GRID)
    assert "stoi_extended" not in plain[0]
    assert abs(plain[0]["stoi_stoiopt"] - r["stoi_stoiopt"]) > 1e-3
