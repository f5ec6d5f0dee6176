"""WSS on the host: the restatement of include/cse_wss.h (tests/_wss_ref.py), the
composite measures, the library's argument checks and the search plumbing of
the "wss" objective.  No GPU."""

import os

import numpy as np
import pytest

import _segsnr_ref as segref
import _wss_ref as ref
from classical_speech_enhancement_amd import _lib, metrics, results, search
from classical_speech_enhancement_amd.synth import make_pair

ALG = "spectralSubtractor"
GRID = {ALG: {"alpha": [1.0, 2.0], "beta": [0.01, 0.1], "n_fft": [512], "hop_length": [128],
              "noise_percentile": [10.0], "noise_method": ["percentile"]}}


# ------------------------------------------------------------------ peak rule
def test_peak_of_a_strictly_rising_spectrum():
    E = np.arange(25.0) * 1.5 - 40.0
    assert np.array_equal(ref.nearest_peak(E), np.full(24, E[23]))


@pytest.mark.parametrize("E", [-np.arange(25.0) * 0.7, np.full(25, -12.5)])
def test_peak_of_a_falling_or_flat_spectrum(E):
    assert np.array_equal(ref.nearest_peak(E), np.full(24, E[0]))


@pytest.mark.parametrize("m", [1, 7, 23, 24])
def test_peak_of_a_single_maximum(m):
    E = -np.abs(np.arange(25.0) - m) * 2.0
    P = ref.nearest_peak(E)
    assert np.array_equal(P[:m], np.full(m, E[m - 1]))        # the quirk: one below the maximum
    assert np.array_equal(P[m:], np.full(24 - m, E[m]))


def test_peak_with_a_plateau():
    # rises to a plateau over bands 5..8, falls to a flat floor at bands 14 and
    # 15, rises again from band 15
    E = np.concatenate([np.arange(6.0), np.full(3, 5.0), 5.0 - np.arange(1.0, 7.0),
                        np.arange(10.0) - 1.0])
    assert len(E) == 25 and E[5] == E[8] == 5.0 and E[14] == E[15] == -1.0
    P = ref.nearest_peak(E)
    assert np.array_equal(P[:5], np.full(5, E[4]))    # rising run 0..4: the band before its end
    # the flat steps are not rising: the leftward search runs over them, and
    # over the fall, to the plateau's first band
    assert np.array_equal(P[5:15], np.full(10, E[5]))
    assert np.array_equal(P[15:], np.full(9, E[23]))


def test_peak_rule_agrees_with_the_matlab_loops():
    rng = np.random.default_rng(11)
    for _ in range(1000):
        E = rng.integers(-6, 7, 25).astype(np.float64)   # many ties
        assert np.array_equal(ref.nearest_peak(E), ref.nearest_peak_matlab(E))
    E = rng.normal(size=25).astype(np.float32)
    assert ref.nearest_peak(E).dtype == np.float32
    assert np.array_equal(ref.nearest_peak(E), ref.nearest_peak_matlab(E))


def test_weights_are_at_most_one():
    rng = np.random.default_rng(12)
    for dtype in (np.float64, np.float32):
        E = (rng.normal(size=25) * 20.0).astype(dtype)
        W = ref.weights(E)
        assert W.dtype == dtype and (W > 0).all() and (W <= 1).all()
        assert W[np.argmax(E[:-1])] <= 1.0


# ----------------------------------------------------------- score properties
def _pair(i=0, seconds=0.5):
    clean, noisy = make_pair(i, seconds=seconds)
    return clean, noisy


def test_identical_signals_score_zero():
    clean, _ = _pair()
    assert ref.wss(clean, clean, 16000) == 0.0
    assert ref.wss(segref_decimate(clean), segref_decimate(clean), 8000) == 0.0


def segref_decimate(x):
    from scipy.signal import resample_poly
    return resample_poly(np.asarray(x, dtype=np.float64), 1, 2)


def test_gain_invariance_above_the_floor():
    clean, noisy = _pair()
    # the synthetic clean signal's pauses are exact zeros and its upper bands
    # fall below the floor: a dither keeps every band of every frame above it
    clean = clean + 1e-3 * np.random.default_rng(3).normal(size=len(clean))
    # no band of any kept frame reaches the 1e-10 floor, scaled or not
    W, hop, nfft, H = segref.constants(16000)
    F, w = segref.filter_table(16000), segref.window(W)
    for sig, g in ((clean, 1.0), (noisy, 0.25), (clean, 0.5), (noisy, 0.5)):
        for j in range(len(sig) // hop - 4):
            if clean[j * hop:j * hop + W].any():
                S = np.abs(np.fft.fft(g * sig[j * hop:j * hop + W] * w, nfft)[:H]) ** 2
                assert (F @ S).min() > 1e-10
    base = ref.wss(clean, noisy, 16000)
    assert base > 1.0
    assert abs(ref.wss(clean, 0.25 * noisy, 16000) - base) <= 1e-9
    assert abs(ref.wss(0.5 * clean, 0.5 * noisy, 16000) - base) <= 1e-9


def test_n95():
    assert ref.n95(30) == 29 and ref.n95(10) == 10 and ref.n95(1) == 1 and ref.n95(20) == 19
    clean, noisy = _pair()
    fv = ref.frame_values(clean, noisy, 16000)
    k = ref.n95(len(fv))
    assert k < len(fv)
    assert ref.wss(clean, noisy, 16000) == float(np.mean(np.sort(fv)[:k]))
    assert ref.wss(clean, noisy, 16000) < float(np.mean(fv))   # the trimming does something


def test_no_frame_and_zero_clean_give_nan():
    clean, noisy = _pair()
    start = int(np.flatnonzero(clean)[0]) + 200
    assert np.isnan(ref.wss(clean[start:start + 599], noisy[start:start + 599], 16000))
    assert np.isfinite(ref.wss(clean[start:start + 600], noisy[start:start + 600], 16000))
    assert np.isnan(ref.wss(np.zeros(8000), noisy, 16000))
    assert np.isnan(ref.wss(np.zeros(8000), noisy, 16000, dtype=np.float32))


def test_silent_frames_are_left_out():
    clean, noisy = _pair()
    gap = clean.copy()
    gap[3000:5210] = 0.0
    W, hop, _, _ = segref.constants(16000)
    J = len(gap) // hop - 4
    silent = [j for j in range(J) if not gap[j * hop:j * hop + W].any()]
    assert len(silent) >= 10
    fv = ref.frame_values(gap, noisy, 16000)
    assert len(fv) == J - len(silent)
    # the kept frames have the values they have without the rule
    full = ref.frame_values(np.where(gap == 0.0, 1e-300, gap), noisy, 16000)
    keep = np.array([j not in silent for j in range(J)])
    assert np.allclose(full[keep], fv, rtol=1e-12, atol=0)


def test_zero_test_frame_is_finite():
    clean, _ = _pair()
    for dtype in (np.float64, np.float32):
        fv = ref.frame_values(clean, np.zeros(len(clean)), 16000, dtype=dtype)
        assert np.isfinite(fv).all() and (fv > 0).all()


def test_lag_and_clip_define_the_test_signal():
    clean, noisy = _pair()
    shifted = np.concatenate([np.zeros(37), noisy[:-37]])
    assert ref.wss(clean, noisy, 16000, lag=37) == ref.wss(clean, shifted, 16000)
    loud = noisy * (3.0 / np.abs(noisy).max())   # beyond [-1, 1]: the clip runs
    assert ref.wss(clean, loud, 16000, clip=True) == ref.wss(clean, np.clip(loud, -1, 1), 16000)
    assert ref.wss(clean, loud, 16000, clip=True) != ref.wss(clean, loud, 16000)


def test_f32_variant_is_close_to_f64():
    clean, noisy = _pair()
    a = ref.wss(clean, noisy, 16000)
    b = ref.wss(clean, noisy, 16000, dtype=np.float32)
    assert a != b and abs(a - b) < 1e-3


def test_unsupported_rate():
    with pytest.raises(NotImplementedError):
        ref.wss(np.ones(4000), np.ones(4000), 44100)


# ------------------------------------------------------------------ composite
def test_composite_formulas():
    csig, cbak, covl = metrics.composite(2.0, 0.5, 40.0, 3.0)
    assert csig == pytest.approx(3.093 - 0.5145 + 1.206 - 0.36, abs=1e-12)      # 3.4245
    assert cbak == pytest.approx(1.634 + 0.956 - 0.28 + 0.189, abs=1e-12)       # 2.499
    assert covl == pytest.approx(1.594 + 1.61 - 0.256 - 0.28, abs=1e-12)        # 2.668
    assert csig == pytest.approx(3.4245, abs=1e-12) and cbak == pytest.approx(2.499, abs=1e-12)
    assert covl == pytest.approx(2.668, abs=1e-12)


def test_composite_clamps():
    assert metrics.composite(4.5, 0.0, 0.0, 35.0) == (5.0, 5.0, 5.0)
    assert metrics.composite(-0.5, 2.0, 150.0, -10.0) == (1.0, 1.0, 1.0)


def test_composite_nan_propagates():
    nan = float("nan")
    csig, cbak, covl = metrics.composite(2.0, nan, 40.0, 3.0)
    assert np.isnan(csig) and np.isnan(covl) and cbak == pytest.approx(2.499, abs=1e-12)
    csig, cbak, covl = metrics.composite(2.0, 0.5, 40.0, nan)
    assert np.isnan(cbak) and not np.isnan(csig) and not np.isnan(covl)
    assert all(np.isnan(v) for v in metrics.composite(nan, 0.5, 40.0, 3.0))
    assert all(np.isnan(v) for v in metrics.composite(2.0, 0.5, nan, 3.0))


def test_composite_broadcasts():
    pesq = np.array([[1.5], [2.5]])
    wss = np.array([20.0, 40.0, 60.0])
    csig, cbak, covl = metrics.composite(pesq, 0.5, wss, 3.0)
    assert csig.shape == cbak.shape == covl.shape == (2, 3)
    for i in range(2):
        for j in range(3):
            one = metrics.composite(pesq[i, 0], 0.5, wss[j], 3.0)
            assert (csig[i, j], cbak[i, j], covl[i, j]) == one
    assert "silent" in metrics.composite.__doc__ and "composite.m" in metrics.composite.__doc__


# ---------------------------------------------------------------------- _lib
def test_lib_exports():
    assert _lib.EXPORTS_WSS == ("cse_wss_workspace_bytes", "cse_wss_prepare",
                                "cse_wss_scratch_bytes", "cse_wss_cells")
    assert not set(_lib.EXPORTS_WSS) & set(_lib.EXPORTS)
    header = open(os.path.join(os.path.dirname(_lib.HERE), "include", "cse_wss.h")).read()
    for name in _lib.EXPORTS_WSS:
        assert name + "(" in header


def test_library_exports_the_entry_points():
    lib = _lib.load()  # build() comes before the tests: a missing library is an error
    for name in _lib.EXPORTS_WSS:
        assert hasattr(lib, name)
    # the size functions need no device
    assert lib.cse_wss_workspace_bytes(2, 16000, 16000) > 2 * (16000 // 120 - 4) * 49 * 4
    assert lib.cse_wss_workspace_bytes(2, 16000, 8000) > 0
    assert lib.cse_wss_workspace_bytes(2, 16000, 44100) == -1
    assert lib.cse_wss_workspace_bytes(-1, 16000, 16000) == -1
    assert lib.cse_wss_workspace_bytes(1, -1, 16000) == -1
    assert lib.cse_wss_scratch_bytes(1, 16000, 44100) == -1
    assert lib.cse_wss_scratch_bytes(-1, 16000, 16000) == -1
    # scratch is 0 while J <= 1536: 1540 * 120 samples are 1536 frames
    assert lib.cse_wss_scratch_bytes(4096, 160000, 16000) == 0
    assert lib.cse_wss_scratch_bytes(7, 1540 * 120, 16000) == 0
    assert lib.cse_wss_scratch_bytes(7, 1541 * 120, 16000) >= 7 * 1537 * 4
    assert lib.cse_wss_scratch_bytes(7, 1540 * 60, 8000) == 0
    assert lib.cse_wss_scratch_bytes(7, 1541 * 60, 8000) >= 7 * 1537 * 4
    # argument checks come before any device work
    assert lib.cse_wss_cells(None, None, None, None, 1, 1, 16000, 16000, 1, None, None, None,
                             None) < 0
    assert b"cse_wss_cells" in lib.cse_last_error()
    assert lib.cse_wss_prepare(None, 1, 16000, 16000, None, None) < 0
    assert b"cse_wss_prepare" in lib.cse_last_error()
    assert lib.cse_wss_prepare(None, 1, 16000, 11025, None, None) < 0
    assert b"11025" in lib.cse_last_error()


def test_the_new_unit_is_built_with_the_common_flags():
    import __graft_entry__ as entry
    assert "cse_wss.hip" in entry.SOURCES and "cse_wss.hip" not in entry.OWN_FLAGS


def test_kernel_src_sha_is_the_parents():
    import bench
    assert bench.kernel_src_sha() == "0294b26e5cf891db"


# ------------------------------------------------------------ search plumbing
def test_table_width():
    assert search.NCOL == 6 and search.WSS_COLUMNS == {"wss": search.NCOL + 7}
    assert search.table_width() == 6
    assert search.table_width(quality=True) == 8
    assert search.table_width(distortion=True) == search.table_width(True, True) == 10
    assert search.table_width(separation=True) == search.table_width(True, True, True) == 13
    assert search.table_width(wss=True) == search.NCOL + 8
    assert search.table_width(True, True, True, True) == search.NCOL + 8
    assert search.TOLERANCE["wss"] == 1e-2


def _table(scores):
    t = np.full((len(scores), search.NCOL + 8), np.nan)
    t[:, :search.NCOL] = 0.0
    t[:, 2] = 1
    t[:, 3] = 0.5
    t[:, search.WSS_COLUMNS["wss"]] = scores
    return t


def test_select_best_wss_minimises():
    specs = search.job_specs(1, [ALG], GRID)
    # a tie inside 1e-2 keeps the earlier cell; a gain beyond it moves on
    t = _table([50.0, 49.995, 60.0, 50.0])
    assert search.select_best(specs, t, "wss")[(0, ALG)] == (0, 50.0)
    t = _table([50.0, 49.995, 49.985, 49.98])
    assert search.select_best(specs, t, "wss")[(0, ALG)] == (2, 49.985)
    assert search.select_best(list(specs), t, "wss")[(0, ALG)] == (2, 49.985)
    # a non-finite cell and a NaN score are skipped
    t = _table([1.0, np.nan, 30.0, 40.0])
    t[0, 2] = 0
    assert search.select_best(specs, t, "wss")[(0, ALG)] == (2, 30.0)
    assert search.select_best(list(specs), t, "wss")[(0, ALG)] == (2, 30.0)
    # nothing scored: no winner
    t = _table([np.nan] * 4)
    assert search.select_best(specs, t, "wss")[(0, ALG)] == (-1, None)
    # the old objectives read the same columns of the wider table
    t = _table([3.0, 2.0, 1.0, 4.0])
    t[:, 1] = [1.0, 2.0, 3.0, 2.5]
    assert search.select_best(specs, t, "snr")[(0, ALG)] == (2, 3.0)
    assert search.select_best(specs, t, "wss")[(0, ALG)] == (2, 1.0)


def test_select_best_wss_needs_its_column():
    specs = search.job_specs(1, [ALG], GRID)
    t = _table([3.0, 2.0, 1.0, 4.0])
    for width in (search.NCOL, search.NCOL + 2, search.NCOL + 4, search.NCOL + 7):
        with pytest.raises(ValueError, match=r"wss=True table of 14 columns, this one has "
                                             + str(width)):
            search.select_best(specs, t[:, :width], "wss")


def test_run_grid_passes_the_flag_and_checks_the_width():
    clean, noisy = make_pair(0, seconds=0.25)
    specs = search.job_specs(1, [ALG], GRID)

    def compute(clean, noisy, specs, ids, width=search.NCOL + 8):
        v = np.full((len(ids), width), np.nan)
        v[:, :search.NCOL] = 0.0
        v[:, 2] = 1
        v[:, 1] = [1.0, 4.0, 2.0, 3.0]
        if width > search.WSS_COLUMNS["wss"]:
            v[:, search.WSS_COLUMNS["wss"]] = [30.0, 20.0, 10.0, 40.0]
        return v
    table, best = search.run_grid([clean], [noisy], specs, compute=compute, wss=True)
    assert table.shape == (4, search.NCOL + 8) and best[(0, ALG)] == (1, 4.0)
    assert search.select_best(specs, table, "wss")[(0, ALG)] == (2, 10.0)
    _, best = search.run_grid([clean], [noisy], specs, compute=compute, wss=True, objective="wss")
    assert best[(0, ALG)] == (2, 10.0)
    with pytest.raises(ValueError, match=r"wss=True\)"):
        search.run_grid([clean], [noisy], specs, wss=True,
                        compute=lambda *a: compute(*a, width=search.NCOL + 7))
    # without the flag the message is what it was
    with pytest.raises(ValueError, match=r"expected 6 columns \(quality=False\)$"):
        search.run_grid([clean], [noisy], specs, compute=compute)


# -------------------------------------------------------------------- results
def test_result_row_wss_keys(tmp_path):
    old = set(results.ROW_KEYS) | {"snr_snropt", "best_params_snr"}
    row = results.result_row("p", ALG, 16000, 1.0, 2.0, {"alpha": 1.0}, wss_noisy=80.0,
                             wss_best=42.0, wss_params={"alpha": 2.0}, snr_wssopt=4.0)
    assert set(row) == old | set(results.WSS_KEYS)
    assert row["best_params_wss"] == {"alpha": 2.0} and row["wss_best"] == 42.0
    other = dict(row, wss_best=44.0, stem="q")
    means = results.write_summary([row, other], [ALG], str(tmp_path))[ALG]
    assert means["wss_best_mean"] == 43.0 and means["wss_noisy_mean"] == 80.0
    assert means["snr_wssopt_mean"] == 4.0
    # all or none: a part of the keywords would leave a half-filled row
    with pytest.raises(TypeError, match="go together"):
        results.result_row("p", ALG, 16000, 1.0, 2.0, {}, wss_best=1.0)
    with pytest.raises(TypeError, match="snr_wssopt"):
        results.result_row("p", ALG, 16000, 1.0, 2.0, {}, wss_noisy=80.0, wss_best=42.0,
                           wss_params={})
    plain = results.result_row("p", ALG, 16000, 1.0, 2.0, {"alpha": 1.0})
    assert set(plain) == old
    assert "wss_best_mean" not in results.write_summary([plain], [ALG], str(tmp_path / "b"))[ALG]
