"""SI-SDR / SI-SIR / SI-SAR without a GPU: the numpy restatement of
include/cse_sisdr.h (tests/_sisdr_ref.py) against hand-computed values and the
properties the header states, the cap on the shared inputs
(tests/_sisdr_cases.py), the built library's exports and argument errors, and
the search / results / metrics plumbing of the separation columns."""

import math

import numpy as np
import pytest

import _sisdr_cases as cases
import _sisdr_ref as ref
from _grid_worker import oracle_compute
from classical_speech_enhancement_amd import _lib, metrics, results, search

GRID = cases.GRID
ALG = "spectralSubtractor"
INF, NAN = math.inf, math.nan
SEP = search.SEPARATION_COLUMNS


def _f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32)


def _cells(n=6, L=3000, seed=0):
    """Constructed cells: y = g s + b v + artifacts with known parts."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        s = rng.standard_normal(L) * 0.2
        v = rng.standard_normal(L) * 0.1
        y = (0.5 + 0.1 * k) * s + (0.05 + 0.2 * k) * v + 0.03 * (k + 1) * rng.standard_normal(L)
        out.append((s, s + v, _f32(y)))
    return out


# ---------------------------------------------------------------- restatement
def test_hand_computed_values():
    s = np.array([1.0, 2.0, 3.0])
    z = s + np.array([1.0, -1.0, 0.5])
    # y = g s: the residual is exactly zero, so every ratio is x / 0 = +inf
    assert ref.scores(s, _f32(2 * s), z, zero_mean=False) == (INF, INF, INF)
    assert ref.scores(s, _f32(2 * s), None, zero_mean=False)[0] == INF
    # y = 0 s: a = 0, et = 0, 0 / 0
    assert all(x != x for x in ref.scores(s, np.zeros(3, np.float32), z, zero_mean=False))
    # y orthogonal to s: et = 0, log10(0) = -inf; the residual is y, partly along v
    y = _f32([3.0, 0.0, -1.0])
    assert float(np.dot(y, s)) == 0.0
    sdr, sir, sar = ref.scores(s, y, z, zero_mean=False)
    assert (sdr, sir, sar) == (-INF, -INF, -INF)
    # numbers small enough to follow by hand: s = (1, 0), v = (0, 2), y = (2, 1)
    # a = 2, et = 4, r2 = 5 - 4 = 1, rv = 2, ei = 4 / 4 = 1, ea = 0
    sdr, sir, sar = ref.scores([1.0, 0.0], _f32([2.0, 1.0]), [1.0, 2.0], zero_mean=False)
    assert sdr == pytest.approx(10 * math.log10(4.0), abs=1e-13) and sir == sdr and sar == INF
    # ss == 0 gives NaN whatever y is
    assert all(x != x for x in ref.scores(np.zeros(3), y, z, zero_mean=False))


def test_noisy_input_scores_sisdr_equal_to_sisir():
    """y = s + v with s orthogonal to v: all of the residual is interference."""
    s = np.array([1.0, -1.0, 2.0, 0.0])
    v = np.array([1.0, 1.0, 0.0, 3.0])
    assert float(np.dot(s, v)) == 0.0
    sdr, sir, sar = ref.scores(s, _f32(s + v), s + v, zero_mean=False)
    assert sdr == sir == pytest.approx(10 * math.log10(6.0 / 11.0), abs=1e-13) and sar == INF
    # in general a = 1 + sv / ss and the residual is v - (sv / ss) s: not all along v
    for s, z, _ in _cells(3):
        sdr, sir, sar = ref.scores(s, _f32(z), z)
        assert sir >= sdr and math.isfinite(sar)


def test_additive_identity():
    for s, z, y in _cells():
        for zm in (True, False):
            sdr, sir, sar = ref.scores(s, y, z, zero_mean=zm)
            assert all(math.isfinite(x) for x in (sdr, sir, sar))
            lhs = 10 ** (-sdr / 10)
            rhs = 10 ** (-sir / 10) + 10 ** (-sar / 10)
            assert abs(lhs - rhs) <= 1e-12 * lhs


def test_no_interference_left():
    """y = g s + artifacts orthogonal to v: sisir = +inf and sisar = sisdr."""
    s = np.array([1.0, 2.0, 0.0, 0.0])
    v = np.array([0.0, 0.0, 1.0, 0.0])
    y = _f32([2.0, 4.0, 0.0, 0.5])
    sdr, sir, sar = ref.scores(s, y, s + v, zero_mean=False)
    assert sir == INF and sar == sdr == pytest.approx(10 * math.log10(20.0 / 0.25), abs=1e-13)
    # noisy == clean: vv == 0 takes the guard, not 0 / 0
    sdr2, sir2, sar2 = ref.scores(s, y, s.copy(), zero_mean=False)
    assert (sdr2, sir2, sar2) == (sdr, INF, sdr)


def test_zero_mean_equals_explicit_mean_removal():
    """The centred sums against the same signals with their means removed first
    (the widened f32 test signal, the clean signal and the interference, in
    f64).  Means of 0.02-0.03 under signals of 0.1-0.2 cancel two of the centred
    form's sixteen digits: 1e-10 dB leaves three orders of margin."""
    for s, z, y in _cells(4, seed=3):
        s, z = s + 0.02, z + 0.051
        y = _f32(y.astype(np.float64) + 0.017)
        a = ref.scores(s, y, z, zero_mean=True)
        t = y.astype(np.float64)
        sc, vc, tc = s - s.mean(), (z - s) - (z - s).mean(), t - t.mean()
        b = ref.finish(math.fsum(tc * sc), math.fsum(tc * vc), math.fsum(tc * tc),
                       math.fsum(sc * sc), math.fsum(vc * vc), math.fsum(sc * vc))
        assert np.allclose(a, b, rtol=0, atol=1e-10)
        raw = ref.scores(s, y, z, zero_mean=False)
        assert abs(raw[0] - a[0]) > 1e-3   # the offsets do matter


def test_scale_invariance():
    """si_sdr(s, c y) for c = 0.25 and 3, to 1e-10 dB.  y is kept on a grid of
    2^-12 so that c y is exact in f32, the type of a test signal: the scores
    then differ by the rounding of the sums alone."""
    for s, z, y in _cells(4, seed=5):
        y = _f32(np.round(y.astype(np.float64) * 4096) / 4096)
        for zm in (True, False):
            base = ref.scores(s, y, z, zero_mean=zm)
            assert all(math.isfinite(x) for x in base)
            for c in (0.25, 3.0):
                cy = _f32(c * y.astype(np.float64))
                assert np.array_equal(cy.astype(np.float64), c * y.astype(np.float64))
                got = ref.scores(s, cy, z, zero_mean=zm)
                assert np.allclose(got, base, rtol=0, atol=1e-10)


def test_lag_and_clip_define_the_test_signal():
    y = _f32([0.5, -2.0, 3.0, 0.25])
    assert np.array_equal(ref.test_signal(y, 4, 0, True), [0.5, -1.0, 1.0, 0.25])
    assert np.array_equal(ref.test_signal(y, 4, 1, False), [0.0, 0.5, -2.0, 3.0])
    assert np.array_equal(ref.test_signal(y, 4, -3, False), [0.25, 0.0, 0.0, 0.0])
    assert not ref.test_signal(y, 4, 4, False).any() and not ref.test_signal(y, 4, -9, True).any()


def test_summation_orders_agree():
    x = np.random.default_rng(1).standard_normal(1000)
    exact = ref.total(x, "fsum")
    for order in ref.ORDERS:
        assert abs(ref.total(x, order) - exact) < 1e-12
    assert ref.total(np.zeros(0), "blocks") == 0.0


def test_shared_inputs_respect_the_cap():
    """Every finite score of every shared case lies inside [-30, 60] dB, the
    non-finite ones are the classes the cases mean to produce, and the lengths,
    lags and structure the issue asks for are there."""
    got = {c[0]: cases.checked(c) for c in cases.host_cases()}
    assert len(got) == len(cases.host_cases())       # the names are unique
    for L in cases.LENGTHS:
        for lag in (0, 1, -1, 3, -3, L - 1, -(L - 1), L, -L, L + 5):
            assert f"len {L} lag {lag}" in got
        for lag in (L, -L, L + 5):                    # all of y shifted out
            assert all(x != x for x in got[f"len {L} lag {lag}"][0])
        if L >= 255:
            assert all(got[f"len {L} lag {lag}"][1] == [True] * 3 for lag in (0, 1, -3, L - 1))
    assert got["len 1 lag 0"][0] == (INF, INF, INF)
    assert got["noisy == clean"][0][1] == INF
    assert got["noisy == clean"][0][0] == got["noisy == clean"][0][2]
    assert all(x != x for x in got["clean == 0"][0] + got["y == 0"][0])
    assert got["clip on"][0] != got["clip off"][0]
    assert abs(got["dc, zero_mean"][0][0] - got["dc, raw"][0][0]) > 1e-3
    clean, noisy, y, off, sig, lag, kind = cases.launch()
    assert clean.shape == (3, 4097) and len(off) == 37
    assert sorted(set(sig.tolist())) == [0, 1, 2] and (np.diff(sig) < 0).any()
    assert off.min() == 123 and (off % 2 == 1).any() and (np.diff(off) < 0).any()
    gaps = np.diff(np.sort(off))
    assert (gaps > clean.shape[1]).all()              # non-contiguous cells
    assert np.abs(y).max() > 1.0 and len(set(lag.tolist())) >= 5
    assert all(got[f"launch cell {c}"][1] == [True] * 3 for c in range(37))


# ------------------------------------------------------------------- the ABI
def test_library_exports_and_argument_errors():
    lib = _lib.load()  # build() comes before the tests: a missing library is an error
    for name in _lib.EXPORTS_SISDR:
        assert hasattr(lib, name)
    assert lib.cse_version() == 5
    # the size functions need no device: v as f64 only with interference
    with_v = lib.cse_sisdr_workspace_bytes(4, 160000, 1)
    without = lib.cse_sisdr_workspace_bytes(4, 160000, 0)
    assert with_v >= without + 4 * 160000 * 8 and 4 * 5 * 8 <= without < 4096
    assert lib.cse_sisdr_workspace_bytes(0, 1, 1) >= 0
    assert lib.cse_sisdr_workspace_bytes(-1, 16000, 1) == -1
    assert lib.cse_sisdr_workspace_bytes(1, -1, 0) == -1
    assert lib.cse_sisdr_scratch_bytes(4096, 160000) == 0
    assert lib.cse_sisdr_scratch_bytes(-1, 160000) == -1
    assert lib.cse_sisdr_scratch_bytes(1, -5) == -1
    # argument checks come before any device work (no device here)
    one = 8  # any non-NULL address: the checks below never reach the device
    assert lib.cse_sisdr_cells(None, None, None, None, 1, 1, 16000, 1, None, None, None, None,
                               None, None, None) < 0
    assert b"cse_sisdr_cells" in lib.cse_last_error()
    assert lib.cse_sisdr_cells(one, one, None, one, 1, 1, 0, 1, one, one, None, one, None, None,
                               None) < 0                       # len < 1
    assert b"len=0" in lib.cse_last_error()
    assert lib.cse_sisdr_cells(one, one, None, one, -1, 1, 16, 1, one, one, None, one, None, None,
                               None) < 0                       # negative count
    assert lib.cse_sisdr_cells(one, one, None, one, 1, 1, 16, 1, one, one, None, None, None, None,
                               None) < 0                       # no output
    assert lib.cse_sisdr_cells(one, one, None, one, 1, 1, 16, 1, one, one, None, one, one, None,
                               None) < 0                       # sisir without sisar
    assert b"both or neither" in lib.cse_last_error()
    # nothing to do: no launch, no error
    assert lib.cse_sisdr_cells(one, one, None, one, 0, 1, 16, 1, one, one, None, one, None, None,
                               None) == 0
    assert lib.cse_sisdr_cells(one, one, None, one, 5, 0, 16, 1, one, one, None, one, None, None,
                               None) == 0
    assert lib.cse_sisdr_prepare(None, None, 1, 16, 1, None, None) < 0
    assert b"cse_sisdr_prepare" in lib.cse_last_error()
    assert lib.cse_sisdr_prepare(one, None, 1, 0, 1, one, None) < 0
    assert lib.cse_sisdr_prepare(one, None, -2, 16, 1, one, None) < 0
    assert lib.cse_sisdr_prepare(one, None, 0, 16, 1, one, None) == 0   # no signal: nothing runs


# ------------------------------------------------------------ search plumbing
def test_columns_widths_and_tolerances():
    assert search.NCOL == 6 and SEP == {"sisdr": 10, "sisir": 11, "sisar": 12}
    assert [search.table_width(q, d, s) for s in (False, True) for q in (False, True)
            for d in (False, True)] == [6, 10, 8, 10, 13, 13, 13, 13]
    # defaults unchanged
    assert search.table_width() == 6 and search.table_width(True) == 8
    assert search.table_width(False, True) == 10 and search.table_width(quality=True) == 8
    assert search.QUALITY_COLUMNS == {"segsnr": 6, "fwsegsnr": 7}
    assert search.DISTORTION_COLUMNS == {"llr": 8, "cep": 9}
    assert search.RECORD_FIELDS == ("cell_id", "sse", "snr", "finite", "stoi", "lag", "xstatus")
    for name in SEP:
        assert search.TOLERANCE[name] == 1e-3 and search.SCAN_START[name] == -math.inf
    assert search.TOLERANCE["stoi"] == 1e-6 and search.TOLERANCE["llr"] == 1e-4


def _table(scores, col):
    t = np.zeros((len(scores), search.NCOL + 7))
    t[:, 2] = 1
    t[:, col] = scores
    return t


@pytest.mark.parametrize("objective", ["sisdr", "sisir", "sisar"])
def test_select_best_maximises_and_skips_what_is_not_finite(objective):
    specs = search.job_specs(1, [ALG], GRID)
    col, tol = SEP[objective], search.TOLERANCE[objective]
    for form in (specs, list(specs)):
        # negative dB values are scores like any other; a tie inside tol keeps the earlier cell
        t = _table([-12.0, -12.0 + 0.9 * tol, -20.0, -12.0], col)
        assert search.select_best(form, t, objective)[(0, ALG)] == (0, -12.0)
        t = _table([3.0, 3.0 + 0.9 * tol, 3.0 + 1.1 * tol, 3.0 + 1.5 * tol], col)
        assert search.select_best(form, t, objective)[(0, ALG)] == (2, 3.0 + 1.1 * tol)
        # a NaN and a +inf are skipped like "llr" skips a NaN; so is -inf, and a cell that is not finite
        t = _table([9.0, NAN, INF, 7.5], col)
        t[0, 2] = 0
        assert search.select_best(form, t, objective)[(0, ALG)] == (3, 7.5)
        t = _table([-INF, 2.0, INF, NAN], col)
        assert search.select_best(form, t, objective)[(0, ALG)] == (1, 2.0)
        assert search.select_best(form, _table([NAN, INF, -INF, INF], col), objective)[(0, ALG)] \
            == (-1, None)
        with pytest.raises(ValueError, match="separation=True"):
            search.select_best(form, t[:, :10], objective)
        # the other objectives read their columns of the wider table as before
        t[:, 3] = [0.1, 0.9, 0.2, 0.3]
        t[:, 8] = [1.0, 0.4, 0.2, 0.3]
        assert search.select_best(form, t, "stoi")[(0, ALG)][0] == 1
        assert search.select_best(form, t, "llr")[(0, ALG)] == (2, 0.2)
    with pytest.raises(ValueError, match="pesq is absent"):
        search.select_best(specs, t, "pesq")


def separation_compute(quality=False, distortion=False):
    """oracle_compute plus the separation columns from the restatement, of the
    finalised output rounded to f32 like the device's waveforms."""
    import oracle

    def compute(clean, noisy, specs, ids):
        base = oracle_compute(clean, noisy, specs, ids)
        out = np.full((len(ids), 13), np.nan)
        out[:, :6] = base
        for j, cid in enumerate(ids):
            pair, alg, p = specs[cid]
            if not base[j, 2]:
                continue
            c = np.asarray(clean[pair], np.float64)
            y = oracle.ALGORITHMS[alg](noisy[pair], 16000, **p)
            e32 = oracle.finalize_enhanced(np.asarray(y, np.float32).astype(np.float64), c, 16000)
            out[j, 10:] = ref.scores(c, e32.astype(np.float32), noisy[pair])
            if quality:
                out[j, 6:8] = (1.0 + j, 2.0 + j)
            if distortion:
                out[j, 8:10] = (0.5, 5.0)
        return out
    return compute


def _pairs(n, seconds=0.5):
    from classical_speech_enhancement_amd.synth import make_pair
    ps = [make_pair(i, seconds) for i in range(n)]
    return [c for c, _ in ps], [x for _, x in ps]


def test_run_grid_column_layout():
    clean, noisy = _pairs(2)
    specs = search.job_specs(2, [ALG], GRID)
    only, best = search.run_grid(clean, noisy, specs, compute=separation_compute(),
                                 separation=True, objective="sisdr")
    every, _ = search.run_grid(clean, noisy, specs, compute=separation_compute(True, True),
                               quality=True, distortion=True, separation=True)
    assert only.shape == every.shape == (8, 13)
    assert np.isnan(only[:, 6:10]).all() and np.isfinite(every[:, 6:10]).all()
    assert np.array_equal(only[:, 10:], every[:, 10:]) and np.isfinite(only[:, 10:]).all()
    assert np.array_equal(only[:, :6], every[:, :6], equal_nan=True)
    assert best == search.select_best(specs, only, "sisdr")
    for (pair, alg), (cid, score) in best.items():
        rows = np.arange(4 * pair, 4 * pair + 4)
        assert score == only[cid, 10] and cid in rows
        assert score >= only[rows, 10].max() - search.TOLERANCE["sisdr"]
    # a compute function of another width is refused
    with pytest.raises(ValueError, match="13 columns"):
        search.run_grid(clean, noisy, specs, compute=oracle_compute, separation=True)
    # the default still returns the plain table, equal to the first columns
    plain, _ = search.run_grid(clean, noisy, specs, compute=oracle_compute)
    assert plain.shape == (8, 6) and np.array_equal(plain, only[:, :6], equal_nan=True)
    # gather_records moves the wider rows as they are
    order = np.array([3, 0, 4, 1, 2, 7, 6, 5])
    local = np.concatenate([order[:, None].astype(np.float64), only[order]], axis=1)
    assert np.array_equal(search.gather_records(local, 8), only, equal_nan=True)


def test_optimize_parameters_separation_entries():
    clean, noisy = _pairs(1)
    base = ref.scores(clean[0], noisy[0].astype(np.float32))[0]
    res = search.optimize_parameters(clean[0], noisy[0], 16000, ALG, GRID[ALG],
                                     compute=separation_compute(), stoi_fn=lambda c, n, sr: 0.5,
                                     separation=True, separation_fn=lambda c, n, sr: base)
    specs = search.job_specs(1, [ALG], GRID)
    table = res["table"]
    assert table.shape == (4, 13)
    for name in SEP:
        cid, score = search.select_best(specs, table, name)[(0, ALG)]
        want = {"score": score, "params": dict(specs[cid][2]), "cell": cid,
                "snr": float(table[cid, 1])}
        want.update({k: float(table[cid, c]) for k, c in SEP.items() if k != name})
        assert res[name] == want and score == table[cid, SEP[name]]
    assert res["baseline"]["sisdr"] == base
    assert res["improvements"]["sisdr"] == res["sisdr"]["score"] - base
    assert "sisir" not in res["baseline"] and "sisar" not in res["improvements"]
    plain = search.optimize_parameters(clean[0], noisy[0], 16000, ALG, GRID[ALG],
                                       compute=oracle_compute, stoi_fn=lambda c, n, sr: 0.5)
    assert not set(SEP) & set(plain) and plain["table"].shape == (4, 6)
    assert set(plain["baseline"]) == {"snr", "stoi"}


# -------------------------------------------------------- results and metrics
OLD_KEYS = set(results.ROW_KEYS) | {"snr_snropt", "best_params_snr"}
P_ARGS = dict(sisdr_noisy=4.0, sisdr_best=9.5, sisir_sisdropt=15.0, sisar_sisdropt=11.0,
              sisdr_params={"alpha": 2.0}, snr_sisdropt=8.0)
D_ARGS = dict(llr_noisy=1.2, cep_noisy=6.0, llr_best=0.4, llr_params={"alpha": 2.0}, snr_llropt=4.0)


def test_result_row_separation_keys(tmp_path):
    assert results.SEPARATION_KEYS == ("sisdr_noisy", "sisdr_best", "sisir_sisdropt",
                                       "sisar_sisdropt", "best_params_sisdr", "snr_sisdropt")
    assert "sisar_noisy" not in results.SEPARATION_KEYS
    # the existing key tuples are what they were
    assert results.DISTORTION_KEYS == ("llr_noisy", "cep_noisy", "llr_best", "best_params_llr",
                                       "snr_llropt")
    assert results.QUALITY_KEYS == ("segsnr_noisy", "fwsegsnr_noisy", "fwsegsnr_best",
                                    "best_params_fwsegsnr", "snr_fwsegopt")
    assert len(results.ROW_KEYS) == 18 and len(results.SUMMARY_KEYS) == 10
    plain = results.result_row("p", ALG, 16000, 1.0, 2.0, {"alpha": 1.0}, stoi_noisy=0.5)
    assert set(plain) == OLD_KEYS
    row = results.result_row("p", ALG, 16000, 1.0, 2.0, {"alpha": 1.0}, **P_ARGS)
    assert set(row) == OLD_KEYS | set(results.SEPARATION_KEYS)
    assert row["best_params_sisdr"] == {"alpha": 2.0} and row["sisdr_best"] == 9.5
    assert row["sisir_sisdropt"] == 15.0 and row["sisar_sisdropt"] == 11.0
    assert set(results.result_row("p", ALG, 16000, 1.0, 2.0, {}, **D_ARGS, **P_ARGS)) \
        == OLD_KEYS | set(results.DISTORTION_KEYS) | set(results.SEPARATION_KEYS)
    other = dict(row, sisdr_best=10.5, stem="q", sisar_sisdropt=None)
    means = results.write_summary([row, other], [ALG], str(tmp_path))[ALG]
    assert means["sisdr_best_mean"] == 10.0 and means["sisdr_noisy_mean"] == 4.0
    assert means["sisir_sisdropt_mean"] == 15.0 and means["sisar_sisdropt_mean"] == 11.0
    assert means["snr_sisdropt_mean"] == 8.0 and "llr_best_mean" not in means
    plain_means = results.write_summary([plain], [ALG], str(tmp_path / "plain"))[ALG]
    assert set(plain_means) == {"count"} | {k for k, _ in results.SUMMARY_KEYS}
    with pytest.raises(TypeError):
        results.result_row("p", ALG, 16000, 1.0, 2.0, {}, sisar_noisy=1.0)


def test_evaluate_audio_quality_keys(monkeypatch):
    """Default keys as before; separation=True adds the five separation keys
    (the device calls stubbed)."""
    def fake_si_sdr(x, y, noisy=None, zero_mean=True):
        assert len(x) == len(y) == 5
        return 4.0 if noisy is None else (9.0, 14.0, 10.5)
    monkeypatch.setattr(metrics, "calculate_stoi", lambda c, t, sr, **kw: 0.5)
    monkeypatch.setattr(metrics, "calculate_snr", lambda c, e: 3.0)
    monkeypatch.setattr(metrics, "si_sdr", fake_si_sdr)
    c, z, e = np.zeros(7), np.zeros(5), np.zeros(6)   # trimmed to the common length
    plain = metrics.evaluate_audio_quality(c, z, e, 16000)
    assert set(plain) == {"stoi_noisy", "stoi_enhanced", "stoi_improvement", "snr_enhanced"}
    p = metrics.evaluate_audio_quality(c, z, e, 16000, separation=True)
    assert set(p) == set(plain) | {"sisdr_noisy", "sisdr_enhanced", "sisdr_improvement",
                                   "sisir_enhanced", "sisar_enhanced"}
    assert p["sisdr_improvement"] == 5.0 and p["sisir_enhanced"] == 14.0
    assert all(plain[k] == p[k] for k in plain)
    assert metrics.SiSdrPlan._WHICH == ("sisdr", "sisir", "sisar")
