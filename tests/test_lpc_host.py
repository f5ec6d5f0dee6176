"""LLR / LPC cepstrum distance without a GPU: the numpy restatement of
include/cse_lpc.h (tests/_lpc_ref.py) against checks that do not share its
code, the header's constants, the built library's exports and argument errors,
and the search / results / metrics plumbing of the distortion columns (an
oracle-style compute function stands in for the device)."""

import os

import numpy as np
import pytest

import _lpc_cases as cases
import _lpc_ref as ref
from _grid_worker import oracle_compute, pairs
from classical_speech_enhancement_amd import _lib, metrics, results, search

GRID = cases.GRID
ALG = "spectralSubtractor"
HEADER = os.path.join(os.path.dirname(_lib.HERE), "include", "cse_lpc.h")


def oracle_enhance(name, noisy, params):
    import oracle
    fn = oracle.advanced_mmse if name == "omlsa" else oracle.spectral_subtraction
    return fn(noisy, 16000, **params)


def _frames(sr, n=40, seed=0):
    """Windowed frames of a well-conditioned signal: an AR(2) resonance plus white noise."""
    W, hop, P = ref.constants(sr)
    rng = np.random.default_rng(seed)
    e = rng.standard_normal(n * hop + W + 200)
    s = np.zeros_like(e)
    for i in range(2, len(e)):
        s[i] = 1.3 * s[i - 1] - 0.8 * s[i - 2] + e[i]
    s = s[200:] + 0.1 * rng.standard_normal(len(e) - 200)
    idx = np.arange(n)[:, None] * hop + np.arange(W)[None, :]
    return s[idx] * ref.window(W), P


# ---------------------------------------------------------------- restatement
@pytest.mark.parametrize("sr", [16000, 8000])
def test_levinson_solves_the_normal_equations(sr):
    from scipy.linalg import solve_toeplitz
    f, P = _frames(sr)
    R = ref.autocorr(f, P)
    # the autocorrelation against its definition, one lag at a time
    assert R[3, 5] == pytest.approx(sum(f[3, i] * f[3, i + 5] for i in range(f.shape[1] - 5)),
                                    rel=1e-12)
    A = ref.levinson(R)
    assert (A[:, 0] == 1).all()
    for j in range(len(R)):
        a = solve_toeplitz(R[j, :-1], -R[j, 1:])
        assert np.allclose(A[j, 1:], a, rtol=0, atol=1e-9 * np.abs(a).max())


def test_levinson_guard_stops_and_leaves_zeros():
    P = 16
    R = np.zeros((3, P + 1))
    R[1, 0] = 1.0          # white: every k is 0
    R[2] = 1.0             # a constant: k_1 = -1, |k_1| < 1 is false
    A = ref.levinson(R)
    assert np.array_equal(A[0], np.eye(P + 1)[0])   # E_0 > 0 is false
    assert np.array_equal(A[1], np.eye(P + 1)[0])
    assert np.array_equal(A[2], np.eye(P + 1)[0])
    assert np.isfinite(A).all()


@pytest.mark.parametrize("sr", [16000, 8000])
def test_llr_is_not_negative_before_the_clamp(sr):
    """A_x minimises a T(R_x) a^T over monic a: every other predictor gives a larger form."""
    fx, P = _frames(sr, seed=1)
    fy, _ = _frames(sr, seed=2)
    Rx = ref.autocorr(fx, P)
    Ax, Ay = ref.levinson(Rx), ref.levinson(ref.autocorr(fy, P))
    ratio = ref.toeplitz_form(Rx, Ay) / ref.toeplitz_form(Rx, Ax)
    assert (ratio >= 1 - 1e-12).all() and (ratio > 1.001).any()


def test_a_signal_against_itself_scores_zero():
    clean, noisy = cases.perturbed_pair(0, 1.0)
    assert ref.scores(clean, clean, 16000) == (0.0, 0.0)
    assert ref.scores(clean[::2], clean[::2], 8000) == (0.0, 0.0)
    a = ref.scores(clean, noisy, 16000)
    assert 0.05 < a[0] < 1.9 and 0.5 < a[1] < 9.5


def test_scores_do_not_depend_on_the_level_of_y():
    clean, noisy = cases.perturbed_pair(1, 1.0)
    a = ref.scores(clean, noisy, 16000)
    b = ref.scores(clean, 0.3 * noisy, 16000)
    assert a != (0.0, 0.0)
    assert abs(a[0] - b[0]) < 1e-10 and abs(a[1] - b[1]) < 1e-10


def test_cepstrum_recursion_against_the_log_spectrum():
    """c_n of a minimum-phase A(z) is the n-th coefficient of -log A(z): an
    N-point inverse FFT of -log|A| gives (c_n + aliases) / 2.  With every root
    inside radius rho, |c_n| <= P rho^n / n, so the aliases of c_1..c_P are
    bounded by 2 P rho^(N - P) / ((N - P) (1 - rho^N))."""
    rng = np.random.default_rng(3)
    P, N, rho = 16, 256, 0.9
    ang = rng.uniform(0.1, 3.0, P // 2)
    rad = rng.uniform(0.5, rho, P // 2)
    roots = np.concatenate([rad * np.exp(1j * ang), rad * np.exp(-1j * ang)])
    A = np.real(np.poly(roots))[None, :]
    c = ref.cepstrum(A)[0]
    direct = np.array([np.real(np.sum(roots ** n)) / n for n in range(1, P + 1)])
    assert np.allclose(c[1:], direct, rtol=0, atol=1e-12)
    spec = np.fft.fft(A[0], N)
    cc = 2 * np.real(np.fft.ifft(-np.log(np.abs(spec))))[1:P + 1]
    bound = 2 * P * rho ** (N - P) / ((N - P) * (1 - rho ** N))
    assert 1e-13 < bound < 1e-10
    assert np.abs(cc - c[1:]).max() <= bound + 1e-13


def test_n95_table():
    assert [ref.n95(j) for j in (1, 10, 11, 20, 30, 1329)] == [1, 10, 10, 19, 29, 1263]
    v = np.arange(30, dtype=np.float64)
    assert ref.trimmed_mean(v) == np.arange(29).sum() / 29   # half-even rounding would keep 28


def test_edge_lengths_have_the_frames_they_are_named_for():
    got = {}
    for name, clean, y, sr, lag, clip in cases.edge_cases(oracle_enhance):
        fv = ref.frame_values(clean, y, sr, lag=lag, clip=clip)
        got[len(clean)] = None if fv is None else len(fv[0])
    assert got == {600: 1, 599: None, 1680: 10, 1800: 11, 4080: 30}
    assert np.isnan(ref.scores(np.ones(599), np.ones(599), 16000)).all()
    assert np.isnan(ref.scores(np.zeros(8000), np.ones(8000), 16000)).all()
    for name, clean, y, sr, lag, clip in cases.long_cases(oracle_enhance):
        assert sr == 8000 and len(clean) // 60 - 4 in (1536, 1537)


def test_zero_test_signal_is_finite_and_the_gap_leaves_frames_out():
    for name, clean, y, sr, lag, clip in cases.silent_cases(oracle_enhance):
        a = ref.scores(clean, y, sr, lag=lag, clip=clip)
        assert np.isfinite(a).all() and 0 <= a[0] <= 2 and 0 <= a[1] <= 10, name
        fv = ref.frame_values(clean, y, sr, lag=lag, clip=clip)
        if "gap" in name:
            assert len(fv[0]) < len(clean) // 120 - 4
    for name, clean, y, sr, lag, clip in cases.raw_cases(oracle_enhance)[:5]:
        a = ref.scores(clean, y, sr, lag=lag, clip=clip)
        assert np.isfinite(a).all() and 0 <= a[0] <= 2 and 0 <= a[1] <= 10, name


def test_launch_noisy_cells_are_not_saturated():
    """The parity test must not run on clamped values: the noisy-kind cells of
    the launch that are not shifted out of the clip (lags 0, 37, -37) score
    strictly inside the ranges."""
    for sr in (16000, 8000):
        clean, y, off, sig, lag, kind = cases.launch(oracle_enhance, sr)
        L = clean.shape[1]
        seen = 0
        for c in range(cases.N_CELLS):
            if kind[c] != 0 or abs(int(lag[c])) > 37:
                continue
            a = ref.scores(clean[sig[c]], y[off[c]:off[c] + L], sr, lag=int(lag[c]), clip=True)
            assert 0.05 < a[0] < 1.9 and 0.5 < a[1] < 9.5, (sr, c, a)
            seen += 1
        assert seen >= 4
    clean, tests = cases.speech()
    a = ref.scores(clean, tests["noisy"], 16000, clip=True)
    assert 0.05 < a[0] < 1.9 and 0.5 < a[1] < 9.5


def test_device_precision_stand_in_is_inside_the_caps():
    clean, noisy = cases.perturbed_pair(0, 1.0)
    y = noisy.astype(np.float32)
    a = ref.scores(clean, y, 16000)
    b = ref.scores(clean, y, 16000, store=np.float32)
    assert a != b
    assert abs(a[0] - b[0]) <= 1e-6 / 8 and abs(a[1] - b[1]) <= 1e-5 / 8


# --------------------------------------------------------------------- header
def test_header_constants():
    text = open(HEADER).read()
    assert ref.constants(16000) == (480, 120, 16) and ref.constants(8000) == (240, 60, 10)
    assert "W = round(0.03 sr) (480, 240); hop = W / 4" in text
    assert "Order P = 16 at 16 kHz,\n * 10 at 8 kHz" in text
    assert "n95 = (19 Ja + 10) div 20" in text and "clamped to [0, 2]" in text
    assert "min(10, (10 / ln 10) sqrt(2 sum_{n=1}^{P} (c_x[n] - c_y[n])^2))" in text
    assert (ref.LLR_MAX, ref.CEP_MAX) == (2.0, 10.0)
    with pytest.raises(NotImplementedError):
        ref.constants(22050)


# ----------------------------------------------------------------------- _lib
def test_lib_exports_and_abi():
    assert _lib.EXPORTS_LPC == ("cse_lpc_workspace_bytes", "cse_lpc_prepare",
                                "cse_lpc_scratch_bytes", "cse_lpc_cells")
    assert _lib.ABI_VERSION == 5
    assert not set(_lib.EXPORTS_LPC) & (set(_lib.EXPORTS) | set(_lib.EXPORTS_SEGSNR))
    header = open(HEADER).read()
    for name in _lib.EXPORTS_LPC:
        assert name + "(" in header
    import __graft_entry__ as entry
    assert "cse_lpc.hip" in entry.SOURCES and "cse_lpc.hip" not in entry.OWN_FLAGS


def test_library_exports_the_entry_points():
    lib = _lib.load()  # build() comes before the tests: a missing library is an error
    for name in _lib.EXPORTS_LPC:
        assert hasattr(lib, name)
    assert lib.cse_version() == 5
    # the size functions need no device: per frame 2 P + 3 doubles
    assert lib.cse_lpc_workspace_bytes(2, 16000, 16000) >= 2 * 129 * 35 * 8
    assert lib.cse_lpc_workspace_bytes(2, 16000, 8000) >= 2 * 262 * 23 * 8
    assert lib.cse_lpc_workspace_bytes(2, 16000, 22050) == -1
    assert lib.cse_lpc_workspace_bytes(-1, 16000, 16000) == -1
    # the selection stays in LDS up to 1536 frames, then two f32 per frame and cell
    assert lib.cse_lpc_scratch_bytes(4096, 160000, 16000) == 0
    assert lib.cse_lpc_scratch_bytes(7, 60 * 1540, 8000) == 0
    per = lib.cse_lpc_scratch_bytes(1, 60 * 1541, 8000)
    assert 2 * 1537 * 4 <= per <= 2 * 1600 * 4
    assert lib.cse_lpc_scratch_bytes(7, 60 * 1541, 8000) == 7 * per
    assert lib.cse_lpc_scratch_bytes(1, 16000, 44100) == -1
    assert lib.cse_lpc_scratch_bytes(-1, 16000, 16000) == -1
    # argument checks come before any device work
    assert lib.cse_lpc_cells(None, None, None, None, 1, 1, 16000, 16000, 1, None, None, None,
                             None, None) < 0
    assert b"cse_lpc_cells" in lib.cse_last_error()
    assert lib.cse_lpc_prepare(None, 1, 16000, 11025, None, None) < 0
    assert b"11025" in lib.cse_last_error()
    assert lib.cse_lpc_prepare(None, 1, 0, 16000, None, None) < 0


def test_plan_chunks_by_the_reported_scratch():
    class Lib:
        def __init__(self, per):
            self.per = per

        def cse_lpc_scratch_bytes(self, n, L, sr):
            return n * self.per

    plan = object.__new__(metrics.LpcPlan)
    plan.L, plan.sr = 60 * 1541, 8000
    for per, want in ((0, metrics.SEGSNR_MAX_CELLS), (12800, (1 << 30) // 12800), (3 << 30, 1)):
        plan.lib = Lib(per)
        assert plan.cells_per_launch() == want
        assert want * per <= max(metrics.SEGSNR_SCRATCH_BYTES, per)
    assert metrics.LpcPlan._WHICH == ("llr", "cep")
    assert metrics.SegSnrPlan._WHICH == ("segsnr", "fwsegsnr")


# ------------------------------------------------------------ search plumbing
def test_columns_and_tolerances():
    assert search.NCOL == 6 and search.QUALITY_COLUMNS == {"segsnr": 6, "fwsegsnr": 7}
    assert search.DISTORTION_COLUMNS == {"llr": 8, "cep": 9}
    assert search.TOLERANCE["llr"] == 1e-4 and search.TOLERANCE["cep"] == 1e-3
    assert search.TOLERANCE["fwsegsnr"] == 1e-3 and search.TOLERANCE["stoi"] == 1e-6
    assert [search.table_width(q, d) for q in (False, True) for d in (False, True)] == [6, 10, 8, 10]


def _table(scores, col):
    t = np.zeros((len(scores), 10))
    t[:, 2] = 1
    t[:, col] = scores
    return t


def _min_scan(sc, ok, tol):
    """A cell replaces the incumbent when value < incumbent - tol, from +inf."""
    incumbent, win = np.inf, -1
    for k in range(len(sc)):
        if ok[k] and sc[k] < incumbent - tol:
            incumbent, win = float(sc[k]), k
    return win, (incumbent if win >= 0 else None)


@pytest.mark.parametrize("objective", ["llr", "cep"])
def test_select_best_minimises(objective):
    specs = search.job_specs(1, [ALG], GRID)
    col = search.DISTORTION_COLUMNS[objective]
    tol = search.TOLERANCE[objective]
    for form in (specs, list(specs)):
        # a tie inside tol keeps the earlier cell; a gain beyond it moves on
        t = _table([1.0, 1.0 - 0.9 * tol, 1.5, 1.0], col)
        assert search.select_best(form, t, objective)[(0, ALG)] == (0, 1.0)
        t = _table([1.0, 1.0 - 0.9 * tol, 1.0 - 1.1 * tol, 1.0 - 1.5 * tol], col)
        assert search.select_best(form, t, objective)[(0, ALG)] == (2, 1.0 - 1.1 * tol)
        # a non-finite cell and a NaN score are skipped; the value comes back itself
        t = _table([0.1, np.nan, 0.7, 0.9], col)
        t[0, 2] = 0
        assert search.select_best(form, t, objective)[(0, ALG)] == (2, 0.7)
        # zero is a score like any other, and nothing scored gives (-1, None)
        assert search.select_best(form, _table([0.5, 0.0, 0.0, 0.2], col), objective)[(0, ALG)] \
            == (1, 0.0)
        assert search.select_best(form, _table([np.nan] * 4, col), objective)[(0, ALG)] == (-1, None)
        with pytest.raises(ValueError, match="distortion=True"):
            search.select_best(form, t[:, :8], objective)
        # the old objectives read the same columns of the wider table
        t[:, 3] = [0.1, 0.9, 0.2, 0.3]
        assert search.select_best(form, t, "stoi")[(0, ALG)][0] == 1
    with pytest.raises(ValueError, match="pesq is absent"):
        search.select_best(specs, t, "pesq")
    with pytest.raises(ValueError, match="quality=True"):
        search.select_best(specs, t[:, :6], "fwsegsnr")


@pytest.mark.parametrize("objective", ["llr", "cep"])
@pytest.mark.parametrize("tol", [-0.1, 0.0, 0.05])
def test_select_best_against_a_plain_loop_over_several_groups(objective, tol):
    grids = dict(GRID, wiener={"alpha": [0.9, 0.98], "gain_floor": [0.05, 0.1], "n_fft": [512],
                               "hop_length": [128], "noise_percentile": [20.0],
                               "noise_method": ["percentile"]})
    specs = search.job_specs(2, list(grids), grids)
    assert len(specs) == 16
    col = search.DISTORTION_COLUMNS[objective]
    t = np.zeros((16, 10))
    t[:, 2] = 1
    t[:, col] = [1.5, 1.4, 1.6, 1.3, 0.9, 0.8, 0.7, 0.72, 0.5, 0.54, 0.48, 0.4, 2.0, 1.96, 2.0, 0.0]
    t[5, 2] = 0
    t[10, col] = np.nan
    want = {}
    for g, key in enumerate([(0, ALG), (0, "wiener"), (1, ALG), (1, "wiener")]):
        rows = np.arange(4 * g, 4 * g + 4)
        ok = (t[rows, 2] != 0) & ~np.isnan(t[rows, col])
        win, score = _min_scan(t[rows, col], ok, tol)
        want[key] = (-1, None) if win < 0 else (int(rows[win]), score)
    assert want[(0, ALG)] == (3, 1.3) and want[(1, "wiener")] == (15, 0.0)
    assert dict(search.select_best(specs, t, objective, tol=tol)) == want
    assert dict(search.select_best(list(specs), t, objective, tol=tol)) == want


def distortion_compute(quality):
    """oracle_compute plus the distortion columns (and, with quality, the
    quality columns) from the restatements, of the finalised output rounded to
    f32 like the device's waveforms."""
    import _segsnr_ref
    import oracle

    def compute(clean, noisy, specs, ids):
        base = oracle_compute(clean, noisy, specs, ids)
        out = np.full((len(ids), 10), np.nan)
        out[:, :6] = base
        for j, cid in enumerate(ids):
            pair, alg, p = specs[cid]
            if not base[j, 2]:
                continue
            c = np.asarray(clean[pair], np.float64)
            y = oracle.ALGORITHMS[alg](noisy[pair], 16000, **p)
            e32 = oracle.finalize_enhanced(np.asarray(y, np.float32).astype(np.float64), c, 16000)
            if quality:
                out[j, 6:8] = _segsnr_ref.scores(c, e32, 16000)
            out[j, 8:] = ref.scores(c, e32, 16000)
        return out
    return compute


def _perturbed(n, seconds):
    ps = [cases.perturbed_pair(i, seconds) for i in range(n)]
    return [c for c, _ in ps], [x for _, x in ps]


def test_run_grid_column_layout_with_and_without_quality():
    clean, noisy = _perturbed(2, 0.5)
    specs = search.job_specs(2, [ALG], GRID)
    both, best = search.run_grid(clean, noisy, specs, compute=distortion_compute(True),
                                 quality=True, distortion=True, objective="llr")
    only, best_only = search.run_grid(clean, noisy, specs, compute=distortion_compute(False),
                                      distortion=True, objective="llr")
    assert both.shape == only.shape == (8, 10)
    assert np.isnan(only[:, 6:8]).all() and np.isfinite(both[:, 6:8]).all()
    assert np.array_equal(both[:, 8:], only[:, 8:]) and np.isfinite(both[:, 8:]).all()
    assert np.array_equal(both[:, :6], only[:, :6], equal_nan=True)
    assert best == best_only == search.select_best(specs, both, "llr")
    for (pair, alg), (cid, score) in best.items():
        rows = np.arange(4 * pair, 4 * pair + 4)
        assert score == both[cid, 8] and cid in rows
        assert score <= both[rows, 8].min() + search.TOLERANCE["llr"]
    # the quality objectives still read columns 6 and 7 of the wider table
    assert search.select_best(specs, both, "fwsegsnr") == search.select_best(specs, both[:, :8],
                                                                           "fwsegsnr")
    # a compute function of another width is refused
    with pytest.raises(ValueError, match="10 columns"):
        search.run_grid(clean, noisy, specs, compute=oracle_compute, distortion=True)
    with pytest.raises(ValueError, match="8 columns"):
        search.run_grid(clean, noisy, specs, compute=distortion_compute(True), quality=True)
    # and the default still returns the plain table
    plain, _ = search.run_grid(clean, noisy, specs, compute=oracle_compute)
    assert plain.shape == (8, 6) and np.array_equal(plain, both[:, :6], equal_nan=True)
    # gather_records moves the wider rows as they are
    order = np.array([3, 0, 4, 1, 2, 7, 6, 5])
    local = np.concatenate([order[:, None].astype(np.float64), both[order]], axis=1)
    assert np.array_equal(search.gather_records(local, 8), both, equal_nan=True)


def test_optimize_parameters_distortion_entries():
    clean, noisy = _perturbed(1, 0.5)
    base = ref.scores(clean[0], noisy[0], 16000)
    res = search.optimize_parameters(clean[0], noisy[0], 16000, ALG, GRID[ALG],
                                     compute=distortion_compute(False),
                                     stoi_fn=lambda c, n, sr: 0.5, distortion=True,
                                     distortion_fn=lambda c, n, sr: base)
    specs = search.job_specs(1, [ALG], GRID)
    table = res["table"]
    assert table.shape == (4, 10)
    for k, name in enumerate(("llr", "cep")):
        cid, score = search.select_best(specs, table, name)[(0, ALG)]
        assert res[name] == {"score": score, "params": dict(specs[cid][2]), "cell": cid,
                             "snr": float(table[cid, 1])}
        assert res["baseline"][name] == base[k]
        assert res["improvements"][name] == base[k] - score   # lower is better
    assert "segsnr" not in res and "fwsegsnr" not in res
    plain = search.optimize_parameters(clean[0], noisy[0], 16000, ALG, GRID[ALG],
                                       compute=oracle_compute, stoi_fn=lambda c, n, sr: 0.5)
    assert "llr" not in plain and "cep" not in plain and plain["table"].shape == (4, 6)
    assert set(plain["baseline"]) == {"snr", "stoi"}


# -------------------------------------------------------- results and metrics
OLD_KEYS = set(results.ROW_KEYS) | {"snr_snropt", "best_params_snr"}
D_ARGS = dict(llr_noisy=1.2, cep_noisy=6.0, llr_best=0.4, llr_params={"alpha": 2.0}, snr_llropt=4.0)
Q_ARGS = dict(segsnr_noisy=-1.0, fwsegsnr_noisy=3.0, fwsegsnr_best=7.5,
              fwsegsnr_params={"alpha": 2.0}, snr_fwsegopt=4.0)


def test_result_row_distortion_keys(tmp_path):
    assert results.DISTORTION_ARGS == ("llr_noisy", "cep_noisy", "llr_best", "llr_params",
                                       "snr_llropt")
    assert results.DISTORTION_KEYS == ("llr_noisy", "cep_noisy", "llr_best", "best_params_llr",
                                       "snr_llropt")
    assert results.QUALITY_KEYS == ("segsnr_noisy", "fwsegsnr_noisy", "fwsegsnr_best",
                                    "best_params_fwsegsnr", "snr_fwsegopt")
    plain = results.result_row("p", ALG, 16000, 1.0, 2.0, {"alpha": 1.0}, stoi_noisy=0.5)
    assert set(plain) == OLD_KEYS
    row = results.result_row("p", ALG, 16000, 1.0, 2.0, {"alpha": 1.0}, **D_ARGS)
    assert set(row) == OLD_KEYS | set(results.DISTORTION_KEYS)
    assert row["best_params_llr"] == {"alpha": 2.0} and row["llr_best"] == 0.4
    assert set(results.result_row("p", ALG, 16000, 1.0, 2.0, {}, **Q_ARGS)) \
        == OLD_KEYS | set(results.QUALITY_KEYS)
    assert set(results.result_row("p", ALG, 16000, 1.0, 2.0, {}, **Q_ARGS, **D_ARGS)) \
        == OLD_KEYS | set(results.QUALITY_KEYS) | set(results.DISTORTION_KEYS)
    other = dict(row, llr_best=0.6, stem="q")
    means = results.write_summary([row, other], [ALG], str(tmp_path))[ALG]
    assert means["llr_best_mean"] == 0.5 and means["llr_noisy_mean"] == 1.2
    assert means["cep_noisy_mean"] == 6.0 and means["snr_llropt_mean"] == 4.0
    assert "fwsegsnr_best_mean" not in means
    plain_means = results.write_summary([plain], [ALG], str(tmp_path / "plain"))[ALG]
    assert set(plain_means) == {"count"} | {k for k, _ in results.SUMMARY_KEYS}
    with pytest.raises(TypeError):
        results.result_row("p", ALG, 16000, 1.0, 2.0, {}, wss_best=1.0)


def test_evaluate_audio_quality_keys(monkeypatch):
    """Default and quality=True keys as before; distortion=True adds llr_* and
    cep_* with improvement = noisy - enhanced (the device calls stubbed)."""
    fake = {"noisy": 1.0, "enh": 0.25}

    def score(clean, test, sr, **kw):
        return fake[test]
    for name in ("calculate_stoi", "calculate_segsnr", "calculate_fwsegsnr", "calculate_llr",
                 "calculate_cep"):
        monkeypatch.setattr(metrics, name, score)
    monkeypatch.setattr(metrics, "calculate_snr", lambda c, e: 3.0)
    plain = metrics.evaluate_audio_quality("c", "noisy", "enh", 16000)
    assert set(plain) == {"stoi_noisy", "stoi_enhanced", "stoi_improvement", "snr_enhanced"}
    q = metrics.evaluate_audio_quality("c", "noisy", "enh", 16000, quality=True)
    assert set(q) == set(plain) | {f"{k}_{s}" for k in ("segsnr", "fwsegsnr")
                                   for s in ("noisy", "enhanced", "improvement")}
    d = metrics.evaluate_audio_quality("c", "noisy", "enh", 16000, distortion=True)
    assert set(d) == set(plain) | {f"{k}_{s}" for k in ("llr", "cep")
                                   for s in ("noisy", "enhanced", "improvement")}
    assert d["llr_improvement"] == 0.75 and d["cep_improvement"] == 0.75
    assert d["stoi_improvement"] == -0.75
