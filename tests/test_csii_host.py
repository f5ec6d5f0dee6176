"""Host-side checks of the CSII / I3 feature (include/cse_csii.h): the numpy
restatement's fixed points, the bindings, and the sweep's coherence switch.
No GPU."""

import inspect
import math
import os

import numpy as np
import pytest

import _csii_cases as cases
import _csii_ref as ref
from classical_speech_enhancement_amd import _lib, metrics, scores, search
from classical_speech_enhancement_amd.synth import make_pair

ALG = "spectralSubtractor"
GRID = {ALG: {"alpha": [1.0, 2.0], "beta": [0.01, 0.1], "n_fft": [512], "hop_length": [128],
              "noise_percentile": [10.0], "noise_method": ["percentile"]}}
I3_ONE = 1.0 / (1.0 + math.exp(-(-3.47 + 1.84 + 9.99)))
I3_ZERO = 1.0 / (1.0 + math.exp(3.47))


@pytest.fixture(scope="module")
def clip3():
    """A 3-s synthetic clip with frames in all three levels."""
    clean, noisy = make_pair(0, seconds=3.0)
    _, n_l, _ = ref.levels(clean, 16000)
    assert (n_l > 1).all()
    return clean, noisy


# ---------------------------------------------------------------- restatement
def test_identical_signals_score_one(clip3):
    clean, _ = clip3
    for dtype in (np.float64, np.float32):
        high, mid, low, i3 = ref.csii(clean, clean, 16000, dtype=dtype)
        assert high == mid == low == 1.0
        assert i3 == pytest.approx(I3_ONE, abs=1e-15) and round(i3, 5) == 0.99977


def test_zero_test_signal_scores_zero(clip3):
    clean, _ = clip3
    for dtype in (np.float64, np.float32):
        high, mid, low, i3 = ref.csii(clean, np.zeros(len(clean)), 16000, dtype=dtype)
        assert high == mid == low == 0.0
        assert i3 == pytest.approx(I3_ZERO, abs=1e-15)


def test_scale_invariance(clip3):
    clean, noisy = clip3
    a = ref.csii(clean, noisy, 16000)
    assert ref.csii(clean, 0.5 * noisy, 16000) == a      # a power of two: to the bit
    b = ref.csii(clean, 3.7 * noisy, 16000)
    assert np.allclose(a, b, rtol=0, atol=1e-12)
    assert 0.0 < a[3] < 1.0 and all(0.0 <= v <= 1.0 for v in a)


def test_nan_rules():
    # no frame
    clean, noisy = cases.speech_cut(599, 16000)
    assert all(v != v for v in ref.csii(clean, noisy, 16000))
    assert ref.levels(clean, 16000)[1].sum() == 0
    # an all-zero clean signal: every frame is in no level
    res, n_l, margin = ref.csii(np.zeros(4000), np.ones(4000), 16000, details=True)
    assert all(v != v for v in res) and n_l.sum() == 0 and margin == float("inf")
    # one frame: its level alone, MSC = 1, score 1; no I3
    clean, noisy = cases.speech_cut(600, 16000)
    res, n_l, _ = ref.csii(clean, noisy, 16000, details=True)
    assert sorted(n_l.tolist()) == [0, 0, 1]
    for L in range(3):
        assert res[L] == 1.0 if n_l[L] else res[L] != res[L]
    assert res[3] != res[3]


def test_a_level_with_one_frame_and_one_with_none():
    name, clean, y, sr, lag, clip = cases.sparse_levels_case()
    res, n_l, margin = ref.csii(clean, y, sr, details=True)
    assert n_l[1] == 1 and n_l[2] == 0 and n_l[0] > 1 and margin >= 1e-9
    assert 0.0 < res[0] < 1.0 and res[1] == 1.0 and res[2] != res[2] and res[3] != res[3]


def test_exact_zero_pauses_are_in_no_level():
    name, clean, y, sr, lag, clip = cases.pause_case()
    code, n_l, _ = ref.levels(clean, sr)
    silent = [j for j in range(len(code)) if not clean[j * 120:j * 120 + 480].any()]
    assert silent and all(code[j] == 3 for j in silent)
    assert n_l.sum() < len(code)


def test_lag_and_clip_define_the_test_signal(clip3):
    clean, noisy = clip3
    shifted = np.concatenate([np.zeros(13), noisy[:-13]])
    assert ref.csii(clean, noisy, 16000, lag=13) == ref.csii(clean, shifted, 16000)
    loud = noisy * (3.0 / np.abs(noisy).max())
    assert ref.csii(clean, loud, 16000, clip=True) == ref.csii(clean, np.clip(loud, -1, 1), 16000)
    assert ref.csii(clean, loud, 16000, clip=True) != ref.csii(clean, loud, 16000)


def test_i3_falls_with_the_noise(clip3):
    clean, _ = clip3
    noise = np.random.default_rng(21).standard_normal(len(clean))
    p_s, p_n = np.mean(clean ** 2), np.mean(noise ** 2)
    i3 = []
    for snr in (20.0, 5.0, -5.0):
        y = clean + noise * np.sqrt(p_s / (p_n * 10 ** (snr / 10.0)))
        i3.append(ref.csii(clean, y, 16000)[3])
    assert I3_ONE > i3[0] > i3[1] > i3[2] > I3_ZERO
    assert i3[0] - i3[2] > 0.2


def test_f32_variant_is_close_to_f64(clip3):
    clean, noisy = clip3
    a = ref.csii(clean, noisy, 16000)
    b = ref.csii(clean, noisy, 16000, dtype=np.float32)
    assert a != b and max(abs(p - q) for p, q in zip(a, b)) < 1e-6


def test_every_gpu_input_keeps_its_level_margin():
    for name, clean, y, sr, lag, clip in cases.direct_cases():
        assert ref.levels(clean, sr)[2] >= 1e-9, name


def test_unsupported_rate():
    with pytest.raises(NotImplementedError):
        ref.csii(np.ones(4000), np.ones(4000), 44100)


# ------------------------------------------------------------------- bindings
def test_lib_exports():
    assert _lib.EXPORTS_CSII == ("cse_csii_workspace_bytes", "cse_csii_prepare",
                                 "cse_csii_scratch_bytes", "cse_csii_cells")
    assert not set(_lib.EXPORTS_CSII) & set(_lib.EXPORTS)
    header = open(os.path.join(os.path.dirname(_lib.HERE), "include", "cse_csii.h")).read()
    for name in _lib.EXPORTS_CSII:
        assert name + "(" in header
    # what CsiiPlan calls is what the list and the header hold
    for part in ("workspace_bytes", "prepare", "scratch_bytes", "cells"):
        assert f"{metrics.CsiiPlan._PREFIX}_{part}" in _lib.EXPORTS_CSII
    assert metrics.CsiiPlan._WHICH == ("csii_high", "csii_mid", "csii_low", "i3")


def test_library_exports_the_entry_points():
    lib = _lib.load()  # build() comes before the tests: a missing library is an error
    for name in _lib.EXPORTS_CSII:
        assert hasattr(lib, name)
    # the size functions need no device
    J = 160000 // 120 - 4
    n = lib.cse_csii_workspace_bytes(1, 160000, 16000)
    assert J * 512 * 8 < n < J * 512 * 8 + (1 << 16)          # the spectra: 5.4 MB for 10 s
    assert lib.cse_csii_workspace_bytes(2, 16000, 8000) > 0
    assert lib.cse_csii_workspace_bytes(0, 16000, 16000) >= 0
    assert lib.cse_csii_workspace_bytes(2, 16000, 44100) == -1
    assert lib.cse_csii_workspace_bytes(-1, 16000, 16000) == -1
    assert lib.cse_csii_workspace_bytes(2, -1, 16000) == -1
    assert lib.cse_csii_scratch_bytes(100, 16000, 16000) == 0
    assert lib.cse_csii_scratch_bytes(100, 16000, 22050) == -1
    assert lib.cse_csii_scratch_bytes(-1, 16000, 16000) == -1


def test_argument_checks_come_before_device_work():
    """NULL pointers, negative counts, len < 1 and an unsupported rate are
    refused on the host: no device is needed to be told so."""
    lib = _lib.load()
    p = 4096  # any non-NULL value: a refused call never reads it
    assert lib.cse_csii_prepare(None, 1, 4000, 16000, p, None) == -1
    assert lib.cse_csii_prepare(p, 1, 4000, 16000, None, None) == -1
    assert lib.cse_csii_prepare(p, 0, 4000, 16000, p, None) == -1
    assert lib.cse_csii_prepare(p, 1, 0, 16000, p, None) == -1
    assert lib.cse_csii_prepare(p, 1, 4000, 11025, p, None) == -1
    assert b"11025" in lib.cse_last_error()
    ok = (p, p, None, p, 1, 1, 4000, 16000, 1, p, None, p, None)
    for k, bad in ((0, None), (1, None), (3, None), (9, None), (11, None), (4, -1), (5, 0),
                   (6, 0), (7, 48000)):
        args = list(ok)
        args[k] = bad
        assert lib.cse_csii_cells(*args) == -1, k
    assert b"cse_csii_cells" in lib.cse_last_error()


def test_the_new_unit_is_built_with_the_common_flags():
    import __graft_entry__ as entry
    assert "cse_csii.hip" in entry.SOURCES and "cse_csii.hip" not in entry.OWN_FLAGS


def test_the_pinned_registries_are_the_parents():
    import bench
    assert bench.kernel_src_sha() == "0294b26e5cf891db"
    assert tuple(scores.FAMILIES) == ("quality", "distortion", "separation", "wss")
    assert "csii" not in _lib.CELL_SCORES
    assert search.TOLERANCE["stoi"] == 1e-6
    assert not any("csii" in k or "i3" in k for k in search.TOLERANCE)


# ------------------------------------------------------------ search plumbing
def test_plain_signatures_keep_their_defaults():
    for fn in (search.run_grid, search.optimize_parameters, search.run_sweep,
               metrics.evaluate_audio_quality):
        prm = inspect.signature(fn).parameters
        assert prm["coherence"].default is False
        for other in ("extended", "quality", "distortion", "separation"):
            if other in prm:
                assert prm[other].default is False
    assert inspect.signature(search.engine_compute).parameters["stoi"].default is True
    assert inspect.signature(metrics.CsiiPlan.score_async).parameters["which"].default == "all"


def test_extended_and_coherence_exclude_each_other(tmp_path):
    clean, noisy = make_pair(0, seconds=0.25)
    specs = search.job_specs(1, [ALG], GRID)

    def compute(clean, noisy, specs, ids):
        raise AssertionError("refused before any cell is computed")
    with pytest.raises(ValueError, match="extended and coherence"):
        search.run_grid([clean], [noisy], specs, compute=compute, extended=True, coherence=True)
    with pytest.raises(ValueError, match="extended and coherence"):
        search.optimize_parameters(clean, noisy, 16000, ALG, GRID[ALG], compute=compute,
                                   extended=True, coherence=True)
    with pytest.raises(ValueError, match="extended and coherence"):
        search.run_sweep([clean], [noisy], ["p"], str(tmp_path), grids=GRID, extended=True,
                         coherence=True)


def test_engine_compute_stoi_values():
    clean, noisy = make_pair(0, seconds=0.25)
    specs = search.job_specs(1, [ALG], GRID)
    with pytest.raises(ValueError, match=r"^stoi='i3': True, False or 'extended'"):
        search.engine_compute([clean], [noisy], specs, np.arange(4), engine=object(), stoi="i3")


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
    table, best = search.run_grid([clean], [noisy], specs, compute=compute, coherence=True)
    assert seen == [4] and table.shape == (4, search.NCOL)


def test_select_best_skips_nan_in_the_intelligibility_column():
    specs = search.job_specs(1, [ALG], GRID)
    nan = float("nan")

    def table(col):
        t = np.zeros((4, search.NCOL))
        t[:, 2] = 1.0
        t[:, 3] = col
        return t
    # a NaN I3 (no mid or low frame) is skipped; ties within 1e-6 keep the earlier cell
    assert search.select_best(specs, table([nan, 0.5, nan, 0.5000005]), "stoi")[(0, ALG)] == (1, 0.5)
    assert search.select_best(specs, table([nan, 0.5, nan, 0.50001]), "stoi")[(0, ALG)] == \
        (3, 0.50001)
    assert search.select_best(specs, table([0.9, nan, nan, nan]), "stoi")[(0, ALG)] == (0, 0.9)
    win, score = search.select_best(specs, table([nan] * 4), "stoi")[(0, ALG)]
    assert win == -1
