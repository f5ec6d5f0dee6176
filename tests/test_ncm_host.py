"""Host-side checks of the NCM feature (include/cse_ncm.h): the numpy
restatement's fixed points and rules, the bindings, and the sweep's modulation
switch.  No GPU."""

import inspect
import os

import numpy as np
import pytest

import _ncm_cases as cases
import _ncm_ref as ref
from classical_speech_enhancement_amd import _lib, metrics, scores, search
from classical_speech_enhancement_amd.synth import make_pair

ALG = "spectralSubtractor"
GRID = {ALG: {"alpha": [1.0, 2.0], "beta": [0.01, 0.1], "n_fft": [512], "hop_length": [128],
              "noise_percentile": [10.0], "noise_method": ["percentile"]}}


@pytest.fixture(scope="module")
def clip3():
    return make_pair(0, seconds=3.0)


def _ramp(M, slope):
    """[M][25] hand-made envelopes: 1 + slope * m in every band."""
    return np.tile((1.0 + slope * np.arange(M))[:, None], (1, 25))


# ---------------------------------------------------------------- restatement
def test_identical_signals_score_one(clip3):
    clean, _ = clip3
    for dtype in (np.float64, np.float32):
        assert ref.ncm(clean, clean, 16000, dtype=dtype) == (1.0, 1.0)


def test_zero_test_signal_scores_zero(clip3):
    clean, _ = clip3
    for dtype in (np.float64, np.float32):
        assert ref.ncm(clean, np.zeros(len(clean)), 16000, dtype=dtype) == (0.0, 0.0)


def test_scale_invariance(clip3):
    clean, noisy = clip3
    a = ref.ncm(clean, noisy, 16000)
    assert ref.ncm(clean, 0.5 * noisy, 16000) == pytest.approx(a, rel=0, abs=1e-12)
    assert ref.ncm(clean, 3.7 * noisy, 16000) == pytest.approx(a, rel=0, abs=1e-12)
    assert all(0.0 < v < 1.0 for v in a)


def test_ncm_falls_with_the_noise():
    """The pair's own noise scaled by 0.1, 0.3, 1, 3 and 10, pairs 0 to 3 at 1 s
    and 3 s.  ncm falls strictly from 0.3 on for every pair and over all five
    gains for pairs 0 and 1.  Pairs 2 and 3 have bands the clean signal barely
    reaches, whose index follows the noise's chance correlation; between 0.1 and
    0.3, where every other band is saturated, that moves ncm by less than 1e-3
    either way (pair 3, 1 s: 0.7693, 0.7702; pair 2, 3 s: 0.7621, 0.7621)."""
    for seconds in (1.0, 3.0):
        for i in range(4):
            clean, ys = cases.noise_ladder(i, seconds)
            v = [ref.ncm(clean, y, 16000)[0] for y in ys]
            assert all(a > b for a, b in zip(v[1:], v[2:])), (i, seconds, v)
            if i < 2:
                assert v[0] > v[1], (i, seconds, v)
            else:
                assert v[0] > v[1] - 1e-3, (i, seconds, v)
            assert v[0] > v[2] and v[0] - v[4] > 0.5, (i, seconds, v)


def test_lag_and_clip_define_the_test_signal(clip3):
    clean, noisy = clip3
    shifted = np.concatenate([np.zeros(13), noisy[:-13]])
    assert ref.ncm(clean, noisy, 16000, lag=13) == ref.ncm(clean, shifted, 16000)
    loud = noisy * (3.0 / np.abs(noisy).max())
    assert ref.ncm(clean, loud, 16000, clip=True) == ref.ncm(clean, np.clip(loud, -1, 1), 16000)
    assert ref.ncm(clean, loud, 16000, clip=True) != ref.ncm(clean, loud, 16000)


def test_dead_band_rules():
    rng = np.random.default_rng(3)
    Ex = 1.0 + rng.random((9, 25))
    Ey = 1.0 + rng.random((9, 25))
    base = ref.transmission_index(Ex, Ey)
    assert ((base >= 0.0) & (base <= 1.0)).all() and base.std() > 0.0
    # a constant clean band, a constant test band and an all-zero test band carry
    # no modulation: TI = 0 there, the other bands keep their value to the bit
    x2, y2 = Ex.copy(), Ey.copy()
    x2[:, 3] = 0.7
    y2[:, 5] = 0.4
    y2[:, 8] = 0.0
    ti = ref.transmission_index(x2, y2)
    assert ti[3] == 0.0 and ti[5] == 0.0 and ti[8] == 0.0
    keep = [i for i in range(25) if i not in (3, 5, 8)]
    assert np.array_equal(ti[keep], base[keep])
    # an envelope that moves by less than f32 rounding is dead, one that moves
    # by 2^-15 of its level (v / s of about 2^-30) is not
    still = 1.0 + 2.0 ** -22 * rng.random(9)
    moving = 1.0 + 2.0 ** -13 * rng.random(9)
    y3 = Ey.copy()
    y3[:, 0], y3[:, 1] = still, moving
    x3 = Ex.copy()
    x3[:, 1] = moving
    ti = ref.transmission_index(x3, y3)
    assert ti[0] == 0.0 and ti[1] == 1.0
    # the weights: a dead band counts with TI = 0 in both scores
    a, b = ref.score_from_envelopes(x2, y2)
    assert a == pytest.approx((ref.A * ti_of(x2, y2)).sum() / ref.A.sum(), abs=1e-15)
    sxx = (x2 * x2).sum(axis=0)
    assert b == pytest.approx((sxx * ti_of(x2, y2)).sum() / sxx.sum(), abs=1e-15)


def ti_of(Ex, Ey):
    return ref.transmission_index(Ex, Ey)


def test_zero_clean_rule():
    Ey = _ramp(5, 0.1)
    assert all(v != v for v in ref.score_from_envelopes(np.zeros((5, 25)), Ey))
    # one live band is enough for a score; the zero bands are dead
    Ex = np.zeros((5, 25))
    Ex[:, 7] = 1.0 + 0.2 * np.arange(5)
    a, b = ref.score_from_envelopes(Ex, Ey)
    assert a == pytest.approx(ref.A[7] / ref.A.sum(), abs=1e-15) and b == 1.0
    assert all(v != v for v in ref.ncm(np.zeros(4447), np.ones(4447), 16000))


def test_two_samples_correlate_fully():
    rng = np.random.default_rng(8)
    Ex, Ey = 1.0 + rng.random((2, 25)), 1.0 + rng.random((2, 25))
    assert ref.score_from_envelopes(Ex, Ey) == (1.0, 1.0)


def test_bif_power_zero_is_the_plain_mean(clip3):
    clean, noisy = clip3
    Ex, Ey = ref.envelopes(clean, noisy, 16000)
    ti = ref.transmission_index(Ex, Ey)
    a0, b0 = ref.score_from_envelopes(Ex, Ey, 0.0)
    a1, b1 = ref.score_from_envelopes(Ex, Ey, 1.0)
    assert b0 == pytest.approx(ti.mean(), abs=1e-15) and a0 == a1 and b0 != b1
    # a zero band still counts with weight 0^0 = 1
    Ex2 = Ex.copy()
    Ex2[:, 0] = 0.0
    t2 = ref.transmission_index(Ex2, Ey)
    assert t2[0] == 0.0
    assert ref.score_from_envelopes(Ex2, Ey, 0.0)[1] == pytest.approx(t2.mean(), abs=1e-15)


def test_eleven_frames_give_nan_and_twelve_do_not():
    for sr, hop in ((16000, 120), (8000, 60)):
        clean, noisy = cases.speech_cut(16 * hop + cases.TAIL, sr)
        n11, n12 = 15 * hop, 16 * hop
        assert ref.frame_counts(n12 - 1, sr) == (11, 1) and ref.frame_counts(n12, sr) == (12, 2)
        assert all(v != v for v in ref.ncm(clean[:n12 - 1], noisy[:n12 - 1], sr))
        assert all(v != v for v in ref.ncm(clean[:n11], noisy[:n11], sr))
        assert all(v == v for v in ref.ncm(clean[:n12], noisy[:n12], sr))
    assert ref.frame_counts(479, 16000) == (0, 0) and ref.frame_counts(8 * 120 + 480, 16000) == (8, 1)


def test_f32_variant_is_close_to_f64(clip3):
    clean, noisy = clip3
    a = ref.ncm(clean, noisy, 16000)
    b = ref.ncm(clean, noisy, 16000, dtype=np.float32)
    assert a != b and max(abs(p - q) for p, q in zip(a, b)) < 1e-6


def test_every_gpu_input_keeps_its_margin():
    scored = 0
    for name, clean, y, sr, lag, clip in cases.direct_cases():
        res, m = ref.ncm(clean, y, sr, lag=lag, clip=clip, details=True)
        if m is None:
            assert all(v != v for v in res), name
            continue
        assert m[2], (name, m)
        scored += 1
    assert scored > 50


def test_unsupported_rate():
    with pytest.raises(NotImplementedError):
        ref.ncm(np.ones(4000), np.ones(4000), 44100)


# ------------------------------------------------------------------- bindings
def test_lib_exports():
    assert _lib.EXPORTS_NCM == ("cse_ncm_workspace_bytes", "cse_ncm_prepare",
                                "cse_ncm_scratch_bytes", "cse_ncm_cells")
    assert not set(_lib.EXPORTS_NCM) & set(_lib.EXPORTS)
    header = open(os.path.join(os.path.dirname(_lib.HERE), "include", "cse_ncm.h")).read()
    for name in _lib.EXPORTS_NCM:
        assert name + "(" in header
    assert "double bif_power, double* ncm," in header
    # what NcmPlan calls is what the list and the header hold
    for part in ("workspace_bytes", "prepare", "scratch_bytes", "cells"):
        assert f"{metrics.NcmPlan._PREFIX}_{part}" in _lib.EXPORTS_NCM
    assert metrics.NcmPlan._WHICH == ("ncm", "ncm_bif")
    assert issubclass(metrics.NcmPlan, metrics.SegSnrPlan)


def test_library_exports_the_entry_points():
    import ctypes
    lib = _lib.load()  # build() comes before the tests: a missing library is an error
    for name in _lib.EXPORTS_NCM:
        assert hasattr(lib, name)
    assert lib.cse_ncm_cells.argtypes[11] is ctypes.c_double
    # the size functions need no device: e[J][25] and dx[M][25] as f64 and a few rows
    J = 160000 // 120 - 4
    M = (J - 8) // 4 + 1
    n = lib.cse_ncm_workspace_bytes(1, 160000, 16000)
    assert (J + M) * 25 * 8 <= n < (J + M) * 25 * 8 + (1 << 12)
    assert lib.cse_ncm_workspace_bytes(2, 16000, 8000) > 0
    assert lib.cse_ncm_workspace_bytes(0, 16000, 16000) >= 0
    assert lib.cse_ncm_workspace_bytes(1, 100, 16000) >= 0       # no frame
    assert lib.cse_ncm_workspace_bytes(2, 16000, 44100) == -1
    assert lib.cse_ncm_workspace_bytes(-1, 16000, 16000) == -1
    assert lib.cse_ncm_workspace_bytes(2, -1, 16000) == -1
    assert lib.cse_ncm_scratch_bytes(100, 16000, 16000) == 0
    assert lib.cse_ncm_scratch_bytes(100, 16000, 22050) == -1
    assert lib.cse_ncm_scratch_bytes(-1, 16000, 16000) == -1


def test_argument_checks_come_before_device_work():
    """NULL pointers, negative counts, len < 1, an unsupported rate and a
    negative or non-finite exponent are refused on the host: no device is needed
    to be told so."""
    lib = _lib.load()
    p = 4096  # any non-NULL value: a refused call never reads it
    assert lib.cse_ncm_prepare(None, 1, 4000, 16000, p, None) == -1
    assert lib.cse_ncm_prepare(p, 1, 4000, 16000, None, None) == -1
    assert lib.cse_ncm_prepare(p, 0, 4000, 16000, p, None) == -1
    assert lib.cse_ncm_prepare(p, 1, 0, 16000, p, None) == -1
    assert lib.cse_ncm_prepare(p, 1, 4000, 11025, p, None) == -1
    assert b"11025" in lib.cse_last_error()
    ok = (p, p, None, p, 1, 1, 4000, 16000, 1, p, None, 1.0, p, None)
    for k, bad in ((0, None), (1, None), (3, None), (9, None), (12, None), (4, -1), (5, 0),
                   (6, 0), (7, 48000), (11, -0.5), (11, float("nan")), (11, float("inf"))):
        args = list(ok)
        args[k] = bad
        assert lib.cse_ncm_cells(*args) == -1, k
        assert b"cse_ncm_cells" in lib.cse_last_error()
    assert b"bif_power" in lib.cse_last_error()
    # no cells: nothing is launched, and nothing of the device is touched
    none = list(ok)
    none[4] = 0
    assert lib.cse_ncm_cells(*none) == 0


def test_plan_refuses_a_bad_exponent_before_the_device():
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="bif_power"):
            metrics.NcmPlan(None, bif_power=bad)
        with pytest.raises(ValueError, match="bif_power"):
            metrics.ncm(np.ones(4000), np.ones(4000), 16000, bif_power=bad)


def test_the_new_unit_is_built_with_the_common_flags():
    import __graft_entry__ as entry
    assert "cse_ncm.hip" in entry.SOURCES and "cse_ncm.hip" not in entry.OWN_FLAGS


def test_the_pinned_registries_are_the_parents():
    import bench
    assert bench.kernel_src_sha() == "0294b26e5cf891db"
    assert tuple(scores.FAMILIES) == ("quality", "distortion", "separation", "wss")
    assert "ncm" not in _lib.CELL_SCORES and len(_lib.CELL_SCORES) == 3
    assert search.TOLERANCE["stoi"] == 1e-6
    assert not any("ncm" in k for k in search.TOLERANCE)


# ------------------------------------------------------------ search plumbing
def test_plain_signatures_keep_their_defaults():
    for fn in (search.run_grid, search.optimize_parameters, search.run_sweep,
               metrics.evaluate_audio_quality):
        prm = inspect.signature(fn).parameters
        assert prm["modulation"].default is False
        for other in ("extended", "coherence", "quality", "distortion", "separation"):
            if other in prm:
                assert prm[other].default is False
    assert inspect.signature(search.engine_compute).parameters["stoi"].default is True
    prm = inspect.signature(metrics.NcmPlan.score_async).parameters
    assert prm["which"].default == "both" and prm["bif_power"].default is None
    assert inspect.signature(metrics.NcmPlan.__init__).parameters["bif_power"].default == 1.0
    assert inspect.signature(metrics.ncm).parameters["bif_power"].default == 1.0


@pytest.mark.parametrize("pair", [("extended", "coherence"), ("extended", "modulation"),
                                  ("coherence", "modulation")])
def test_the_three_switches_exclude_each_other(tmp_path, pair):
    clean, noisy = make_pair(0, seconds=0.25)
    specs = search.job_specs(1, [ALG], GRID)
    kw = {pair[0]: True, pair[1]: True}
    msg = f"{pair[0]} and {pair[1]} both fill the STOI column"

    def compute(clean, noisy, specs, ids):
        raise AssertionError("refused before any cell is computed")
    with pytest.raises(ValueError, match=msg):
        search.run_grid([clean], [noisy], specs, compute=compute, **kw)
    with pytest.raises(ValueError, match=msg):
        search.optimize_parameters(clean, noisy, 16000, ALG, GRID[ALG], compute=compute, **kw)
    with pytest.raises(ValueError, match=msg):
        search.run_sweep([clean], [noisy], ["p"], str(tmp_path), grids=GRID, **kw)


def test_engine_compute_stoi_values():
    clean, noisy = make_pair(0, seconds=0.25)
    specs = search.job_specs(1, [ALG], GRID)
    with pytest.raises(ValueError, match=r"^stoi='ncm': True, False or 'extended'.*'modulation'"):
        search.engine_compute([clean], [noisy], specs, np.arange(4), engine=object(), stoi="ncm")


def test_run_grid_passes_the_switch_to_a_callers_compute_untouched():
    clean, noisy = make_pair(0, seconds=0.25)
    specs = search.job_specs(1, [ALG], GRID)
    seen = []

    def compute(clean, noisy, specs, ids):
        seen.append(len(ids))
        v = np.zeros((len(ids), search.NCOL))
        v[:, 2] = 1.0
        v[:, 3] = [0.5, float("nan"), 0.7, 0.6]
        return v
    table, best = search.run_grid([clean], [noisy], specs, compute=compute, modulation=True)
    assert seen == [4] and table.shape == (4, search.NCOL)
    assert search.select_best(specs, table, "stoi")[(0, ALG)] == (2, 0.7)
