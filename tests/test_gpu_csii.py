"""Device CSII / I3 (cse_csii_prepare / cse_csii_cells) against the fp64 numpy
restatement of include/cse_csii.h (tests/_csii_ref.py); needs a GPU.  The
comparison is always against the restatement, never against the device.

Tolerance, measured, not guessed: the cell kernel works in fp32 from the
windowed frame on, so the yardstick is the restatement run in f32
(dtype=np.float32: scipy's complex64 FFT, f32 sums of Pxy and Pyy, f32 band sums
and logarithms) against itself in f64.  tools/csii_tolerance.py walks the inputs
of this file (tests/_csii_cases.py, and the sweep test's cells with the grid
cells at lag 0 and the oracle's plugins in place of the device's) and finds

    max |ref(f32) - ref(f64)| = 6.23e-8

over the four outputs of 61 cells (CSII_high of the 8-kHz 16000-sample clip;
I3: 4.3e-8).  The test tolerance is 8 times that figure, 4.98e-7 absolute (the
factor covers a different FFT factorisation and summation order from scipy's),
inside the cap of 1e-5, ten times the STOI objective's selection step.  Every
input classifies its frames with a relative margin of at least 1e-9 (asserted;
the smallest is 4.2e-3), so device and restatement put every frame in the same
level.  Each case prints its difference (pytest -s).
"""

import numpy as np
import pytest

import _csii_cases as cases
import _csii_ref as ref
import _segsnr_cases as segcases

pytestmark = pytest.mark.gpu
F32_VS_F64 = 6.23e-8   # tools/csii_tolerance.py
TOL = 8 * F32_VS_F64
assert TOL <= 1e-5
MARGIN = 1e-9
WORST = [0.0]
ALG = "spectralSubtractor"
NAMES = ("csii_high", "csii_mid", "csii_low", "i3")


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from classical_speech_enhancement_amd import metrics
    return metrics


def _close(got, want, what):
    """got, want: four values each."""
    for k in range(4):
        g, w = float(got[k]), float(want[k])
        if w != w:
            assert g != g, (what, NAMES[k], g)
            continue
        d = abs(g - w)
        WORST[0] = max(WORST[0], d)
        print(f"csii {what} {NAMES[k]}: device {g!r} ref {w!r} diff {d:.3e} "
              f"(tol {TOL:.2e}, worst so far {WORST[0]:.3e})")
        assert d <= TOL, (what, NAMES[k], g, w)


def _want(clean, y, sr, lag=0, clip=False):
    res, n_l, margin = ref.csii(clean, y, sr, lag=lag, clip=clip, details=True)
    assert margin >= MARGIN
    return res, n_l


def _plan(dev, clean, sr=16000):
    import torch
    clean = np.asarray(clean, dtype=np.float64)
    return dev.CsiiPlan(torch.as_tensor(clean.reshape(-1, clean.shape[-1])).cuda(), sr)


def _cuda(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _one(dev, clean, y, sr, lag, clip):
    return _plan(dev, clean, sr).score(_cuda(y), [0], [0], lag=[lag], clip=clip)[0]


@pytest.mark.parametrize("sr", [16000, 8000])
def test_lengths_and_lags(dev, sr):
    """No frame, one frame, 15 / 16 / 17 frames around the eight waves and their
    second round, and longer clips; lags either way; the clip at work."""
    seen = set()
    for name, clean, y, rate, lag, clip in cases.length_cases():
        if rate != sr:
            continue
        assert clip and np.abs(y).max() > 1.0
        want, n_l = _want(clean, y, sr, lag, clip)
        got = _one(dev, clean, y, sr, lag, clip)
        hop = 120 if sr == 16000 else 60
        J = len(clean) // hop - 4
        seen.add(J)
        if J < 1:
            assert all(v != v for v in want) and np.isnan(got).all()
        else:
            assert n_l.sum() >= 1
            _close(got, want, name)
    assert seen >= ({0, 1, 15, 16, 17} if sr == 16000 else {1})


def test_three_signals_five_cells_each(dev):
    clean, y, off, sig, lag = cases.batch()
    L = clean.shape[1]
    assert sorted(np.bincount(sig).tolist()) == [5, 5, 5] and (np.diff(sig) < 0).any()
    assert off.min() == 61 and (np.diff(off) < 0).any() and np.abs(y).max() > 1.0
    plan = _plan(dev, clean)
    got = plan.score(_cuda(y), off, sig, lag=lag, clip=True)
    assert got.shape == (15, 4) and got.dtype == np.float64
    full = 0
    for c in range(15):
        want, n_l = _want(clean[sig[c]], y[off[c]:off[c] + L], 16000, int(lag[c]), True)
        full += all(w == w for w in want)
        _close(got[c], want, f"batch cell {c} sig {sig[c]} lag {lag[c]}")
    assert full >= 10  # most cells have all three levels and an I3
    # the same call twice: the same bits
    again = plan.score(_cuda(y), off, sig, lag=lag, clip=True)
    assert np.array_equal(got.view(np.int64), again.view(np.int64))
    # one column on request, device indices and a caller's buffer
    import torch
    out = torch.empty(15, dtype=torch.float64, device="cuda")
    res = plan.score_async(_cuda(y), torch.as_tensor(off).cuda(), torch.as_tensor(sig).cuda(),
                           lag=torch.as_tensor(lag).cuda(), clip=True, out=out, which="i3")
    assert res is out
    assert np.array_equal(out.cpu().numpy(), got[:, 3], equal_nan=True)
    with pytest.raises(ValueError):
        plan.score(_cuda(y), off, sig, which="stoi")
    with pytest.raises(ValueError):
        plan.score(_cuda(y), off, sig[:-1])
    assert plan.score(_cuda(y), [], []).shape == (0, 4)
    # a cell scored with only its own signal in the batch: the same bits
    alone = _plan(dev, clean[sig[0]]).score(_cuda(y), off[:1], [0], lag=lag[:1], clip=True)
    assert np.array_equal(alone[0].view(np.int64), got[0].view(np.int64))


def test_pauses_and_sparse_levels(dev):
    name, clean, y, sr, lag, clip = cases.pause_case()
    want, n_l = _want(clean, y, sr, lag, clip)
    assert (n_l >= 1).all() and n_l.sum() < len(clean) // 120 - 4
    _close(_one(dev, clean, y, sr, lag, clip), want, name)
    name, clean, y, sr, lag, clip = cases.sparse_levels_case()
    want, n_l = _want(clean, y, sr, lag, clip)
    assert n_l[1] == 1 and n_l[2] == 0
    got = _one(dev, clean, y, sr, lag, clip)
    assert got[1] == 1.0 and np.isnan(got[2]) and np.isnan(got[3])
    _close(got, want, name)


def test_fixed_points_and_scale(dev):
    (n1, clean, y1, sr, _, _), (n0, _, y0, _, _, _) = cases.fixed_point_cases()
    want, n_l = _want(clean, y1, sr)
    assert (n_l >= 1).all() and want[:3] == (1.0, 1.0, 1.0)
    got = _one(dev, clean, y1, sr, 0, False)
    _close(got, want, n1)
    assert round(float(got[3]), 5) == 0.99977
    want, _ = _want(clean, y0, sr)
    assert want[:3] == (0.0, 0.0, 0.0)
    got = _one(dev, clean, y0, sr, 0, False)
    assert got[:3].tolist() == [0.0, 0.0, 0.0]
    _close(got, want, n0)
    clean, y = cases.scale_case()
    want, _ = _want(clean, y, 16000)
    a = _one(dev, clean, y, 16000, 0, False)
    b = _one(dev, clean, (0.5 * y).astype(np.float32), 16000, 0, False)
    _close(a, want, "scale 1")
    _close(b, want, "scale 0.5")
    _close(b, a, "0.5 y against y")


def test_zero_clean_in_a_batch(dev):
    clean, y, off, sig, lag = cases.batch()
    cl = clean.copy()
    cl[1] = 0.0
    got = _plan(dev, cl).score(_cuda(y), off, sig, lag=lag, clip=True)
    ref_got = _plan(dev, clean).score(_cuda(y), off, sig, lag=lag, clip=True)
    for c in range(15):
        if sig[c] == 1:
            assert np.isnan(got[c]).all()
        else:
            assert np.array_equal(got[c].view(np.int64), ref_got[c].view(np.int64))


def test_einval_paths(dev):
    import torch
    clean, y = cases.scale_case()
    plan = _plan(dev, clean)
    lib = plan.lib
    yd = _cuda(y)
    off = torch.zeros(1, dtype=torch.int64, device="cuda")
    sig = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = torch.empty(4, dtype=torch.float64, device="cuda")
    L = len(clean)
    ok = [yd.data_ptr(), off.data_ptr(), None, sig.data_ptr(), 1, 1, L, 16000, 1,
          plan.ws.data_ptr(), None, out.data_ptr(), None]
    assert lib.cse_csii_cells(*ok) == 0
    torch.cuda.synchronize()
    _close(out.cpu().numpy(), _want(clean, y, 16000, 0, True)[0], "raw call")
    for k, bad in ((0, None), (1, None), (3, None), (9, None), (11, None), (4, -1), (5, 0),
                   (5, -2), (6, 0), (7, 44100)):
        args = list(ok)
        args[k] = bad
        assert lib.cse_csii_cells(*args) == -1, k
        assert b"cse_csii_cells" in lib.cse_last_error()
    none = list(ok)
    none[4] = 0
    assert lib.cse_csii_cells(*none) == 0  # n_cells == 0 launches nothing
    assert lib.cse_csii_prepare(clean.ctypes.data, 1, L, 22050, plan.ws.data_ptr(), None) == -1
    assert lib.cse_csii_prepare(None, 1, L, 16000, plan.ws.data_ptr(), None) == -1
    assert lib.cse_csii_prepare(plan.clean.data_ptr(), -1, L, 16000, plan.ws.data_ptr(), None) == -1
    with pytest.raises(NotImplementedError):
        _plan(dev, clean, 22050)


def test_scalars(dev):
    name, clean, y, sr, lag, clip = cases.pause_case()
    want, _ = _want(clean, y, sr)
    _close(dev.csii(clean, y, 16000), want, "scalar")
    i3 = dev.calculate_csii(clean, y[:9000], 16000)
    w2, _ = _want(clean[:9000], y[:9000], 16000)
    assert abs(i3 - w2[3]) <= TOL
    assert dev.calculate_csii(clean[:300], y[:300], 16000) is None
    with pytest.raises(NotImplementedError):
        dev.csii(clean, y, 22050)
    enh = (0.5 * (y + clean)).astype(np.float32)
    q = dev.evaluate_audio_quality(clean, y, enh, 16000, coherence=True)
    we, _ = _want(clean, enh, 16000)
    _close([q[f"{n}_enhanced"] for n in NAMES], we, "evaluate_audio_quality")
    _close([q[f"{n}_noisy"] for n in NAMES], want, "evaluate_audio_quality, noisy")
    assert q["i3_improvement"] == q["i3_enhanced"] - q["i3_noisy"] and q["i3_improvement"] > 0
    plain = dev.evaluate_audio_quality(clean, y, enh, 16000)
    assert not any("csii" in k or "i3" in k for k in plain)
    assert all(plain[k] == q[k] for k in plain)


# --------------------------------------------------------------------- search
def _cell_wave(clean, noisy, params, lag):
    """One grid cell's plugin output, finalised like the sweep does."""
    from classical_speech_enhancement_amd import plugins
    from classical_speech_enhancement_amd.results import shift_and_fit
    y = plugins.spectral_subtraction(noisy, 16000, **params).astype(np.float32)
    return shift_and_fit(y.astype(np.float64), int(lag), len(clean))


_GRID_RUN = {}


def _grid_run():
    """The 4-cell grid on the two 1-s pairs, with and without the switch, once."""
    if not _GRID_RUN:
        from classical_speech_enhancement_amd import search
        from classical_speech_enhancement_amd.synth import make_pair
        pairs = [make_pair(i, seconds=1.0) for i in segcases.GRID_PAIRS]
        clean, noisy = [c for c, _ in pairs], [n for _, n in pairs]
        specs = search.job_specs(2, [ALG], segcases.GRID)
        plain, pbest = search.run_grid(clean, noisy, specs)
        table, best = search.run_grid(clean, noisy, specs, coherence=True)
        _GRID_RUN.update(clean=clean, noisy=noisy, specs=specs, plain=plain, pbest=pbest,
                         table=table, best=best)
    return _GRID_RUN


def test_run_grid_coherence(dev):
    from classical_speech_enhancement_amd import search
    g = _grid_run()
    specs, plain, table = g["specs"], g["plain"], g["table"]
    assert len(specs) == 8
    assert plain.shape == table.shape == (8, search.NCOL)
    # the plain table is what it was, and only column 3 differs
    other = [c for c in range(search.NCOL) if c != 3]
    assert np.array_equal(table[:, other], plain[:, other], equal_nan=True)
    assert not np.array_equal(table[:, 3], plain[:, 3])
    assert g["best"] == g["pbest"]  # the SNR winners
    for pair in range(2):
        ids = [c for c in range(8) if specs[c][0] == pair]
        waves = np.stack([_cell_wave(g["clean"][pair], g["noisy"][pair], specs[c][2],
                                     table[c, 4]) for c in ids]).astype(np.float32)
        L = waves.shape[1]
        # column 3 is CsiiPlan's I3 on the finalised waveforms
        got = _plan(dev, g["clean"][pair]).score(_cuda(waves.reshape(-1)),
                                                 np.arange(len(ids)) * L,
                                                 np.zeros(len(ids), dtype=np.int32), clip=True)
        for k, c in enumerate(ids):
            assert abs(table[c, 3] - got[k, 3]) <= TOL, (c, table[c, 3], got[k, 3])
            want, _ = _want(g["clean"][pair], waves[k], 16000, 0, True)
            assert want[3] == want[3]
            d = abs(table[c, 3] - want[3])
            print(f"csii grid cell {c}: device {table[c, 3]!r} ref {want[3]!r} diff {d:.3e}")
            assert d <= TOL
    direct = search.engine_compute(g["clean"], g["noisy"], specs, np.arange(8), stoi="coherence")
    assert np.array_equal(direct, table, equal_nan=True)
    with pytest.raises(ValueError):
        search.run_grid(g["clean"], g["noisy"], specs, extended=True, coherence=True)


def test_run_sweep_coherence(dev, tmp_path):
    import os
    from classical_speech_enhancement_amd import search
    g = _grid_run()
    clean, noisy = g["clean"][1], g["noisy"][1]
    rows = search.run_sweep([clean], [noisy], ["p01"], str(tmp_path), grids=segcases.GRID,
                            coherence=True)
    r = rows[0]
    assert r["stoi_coherence"] is True and "stoi_extended" not in r
    specs = search.job_specs(1, [ALG], segcases.GRID)
    table, _ = search.run_grid([clean], [noisy], specs, coherence=True)
    sid, sscore = search.select_best(specs, table, "stoi")[(0, ALG)]
    assert r["stoi_stoiopt"] == sscore and r["best_params_stoi"] == specs[sid][2]
    want, _ = _want(clean, noisy.astype(np.float32), 16000)
    assert abs(r["stoi_noisy"] - want[3]) <= TOL
    assert os.path.exists(os.path.join(tmp_path, f"results_{ALG}",
                                       f"p01_{ALG}_optimized_stoi.wav"))
    plain = search.run_sweep([clean], [noisy], ["p01"], str(tmp_path / "plain"),
                             grids=segcases.GRID)
    assert "stoi_coherence" not in plain[0] and set(plain[0]) | {"stoi_coherence"} == set(r)
    assert plain[0]["stoi_noisy"] != r["stoi_noisy"]
    res = search.optimize_parameters(clean, noisy, 16000, ALG, segcases.GRID[ALG], coherence=True)
    assert res["coherence"] is True and "extended" not in res
    assert res["stoi"]["score"] == sscore and res["stoi"]["cell"] == sid
    assert abs(res["baseline"]["stoi"] - want[3]) <= TOL
