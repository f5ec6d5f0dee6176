"""segSNR / fwSegSNR without a GPU: the numpy restatement of
include/cse_segsnr.h (tests/_segsnr_ref.py) against the properties the header
states, the filter table, and the search / results plumbing of the quality
columns (an oracle-style compute function stands in for the device)."""

import os
import socket

import numpy as np
import pytest

import _segsnr_ref as ref
from _grid_worker import oracle_compute, pairs
from classical_speech_enhancement_amd import _lib, results, search
from classical_speech_enhancement_amd.synth import make_pair

GRID = {"spectralSubtractor": {"alpha": [1.0, 2.0], "beta": [0.01, 0.1], "n_fft": [512],
                               "hop_length": [128], "noise_percentile": [10.0],
                               "noise_method": ["percentile"]}}
ALG = "spectralSubtractor"


# ---------------------------------------------------------------- restatement
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_clean_against_clean_is_35(dtype):
    clean, _ = make_pair(0, seconds=1.0)
    assert ref.scores(clean, clean, 16000, dtype=dtype) == (35.0, 35.0)
    # an exactly-zero stretch whose edges are off the hop grid
    gap = clean.copy()
    gap[3001:5207] = 0.0
    assert 3001 % 120 and 5207 % 120
    fv = ref.frame_values(gap, gap, 16000, dtype=dtype)
    assert 0 < len(fv[0]) < len(gap) // 120 - 4  # frames were left out
    assert ref.scores(gap, gap, 16000, dtype=dtype) == (35.0, 35.0)
    # 8 kHz
    assert ref.scores(clean[::2], clean[::2], 8000, dtype=dtype) == (35.0, 35.0)


def test_silent_frame_count_of_the_10_s_pair():
    clean, noisy = make_pair(0, seconds=10.0)
    J = len(clean) // 120 - 4
    silent = sum(not clean[j * 120:j * 120 + 480].any() for j in range(J))
    assert (J, silent) == (1329, 502)


def test_frame_count_edges():
    clean, noisy = make_pair(0, seconds=0.5)
    start = int(np.flatnonzero(clean)[0]) + 200
    for sr, hop in ((16000, 120), (8000, 60)):
        x, y = clean[start:start + 5 * hop], noisy[start:start + 5 * hop]
        assert np.isnan(ref.scores(x[:-1], y[:-1], sr)).all()
        fv = ref.frame_values(x, y, sr)
        assert len(fv[0]) == len(fv[1]) == 1
        assert np.isfinite(ref.scores(x, y, sr)).all()
    # a tail shorter than a hop is ignored
    assert ref.scores(clean[:8040], noisy[:8040], 16000) == ref.scores(clean[:8077], noisy[:8077], 16000)


def test_zero_signals():
    clean, noisy = make_pair(0, seconds=0.5)
    assert np.isnan(ref.scores(np.zeros(8000), noisy, 16000)).all()
    for dtype in (np.float64, np.float32):
        z = ref.scores(clean, np.zeros(8000), 16000, dtype=dtype)
        assert np.isfinite(z).all() and abs(z[0]) <= 1e-3 and abs(z[1]) <= 1e-3


@pytest.mark.parametrize("lag", [37, -37, 601, -7900])
def test_lag_is_the_explicit_shift(lag):
    clean, noisy = make_pair(0, seconds=0.5)
    n = len(noisy)
    shifted = np.zeros(n)
    if lag >= 0:
        shifted[lag:] = noisy[:n - lag]
    else:
        shifted[:n + lag] = noisy[-lag:]
    assert ref.scores(clean, noisy, 16000, lag=lag) == ref.scores(clean, shifted, 16000)
    assert ref.scores(clean, noisy, 16000, lag=lag) != ref.scores(clean, noisy, 16000)


def test_clip_matters_beyond_one():
    clean, noisy = make_pair(0, seconds=0.5)
    loud = noisy * (1.7 / np.abs(noisy).max())
    a = ref.scores(clean, loud, 16000, clip=True)
    assert a == ref.scores(clean, np.clip(loud, -1, 1), 16000)
    assert a != ref.scores(clean, loud, 16000)
    assert ref.scores(clean, noisy, 16000, clip=True) == ref.scores(clean, noisy, 16000)


def test_unsupported_rate():
    with pytest.raises(NotImplementedError):
        ref.scores(np.ones(4000), np.ones(4000), 22050)


def test_f32_variant_is_close_to_f64():
    """The stand-in for the device's precision stays inside the caps the GPU
    tolerance may not exceed (1e-4 / 8 and 1e-3 / 8 dB) on a noisy pair."""
    clean, noisy = make_pair(0, seconds=1.0)
    a = ref.scores(clean, noisy.astype(np.float32), 16000)
    b = ref.scores(clean, noisy.astype(np.float32), 16000, dtype=np.float32)
    assert a != b
    assert abs(a[0] - b[0]) <= 1e-4 / 8 and abs(a[1] - b[1]) <= 1e-3 / 8


# --------------------------------------------------------------- filter table
@pytest.mark.parametrize("sr,H", [(16000, 512), (8000, 256)])
def test_filter_table(sr, H):
    F = ref.filter_table(sr)
    assert F.shape == (25, H)
    nz = F > 0
    for i in range(25):
        k = np.flatnonzero(nz[i])
        assert len(k) and np.array_equal(k, np.arange(k[0], k[-1] + 1)), i
        assert F[i].max() == pytest.approx(ref.BAND[0] / ref.BAND[i], rel=1e-12)
    # H / (sr / 2) is the same at both rates: one pinned table
    assert int(nz.sum()) == 357
    assert nz.sum(axis=1).tolist() == [7] * 8 + [9, 9, 11, 11, 13, 13, 15, 15, 17, 19, 19, 21,
                                                  23, 25, 25, 27, 29]
    assert int(np.flatnonzero(nz.any(axis=0))[-1]) == 244


# ------------------------------------------------------------ search plumbing
def test_columns_keep_their_values():
    assert search.NCOL == 6
    assert search.QUALITY_COLUMNS == {"segsnr": 6, "fwsegsnr": 7}
    assert search.TOLERANCE["segsnr"] == search.TOLERANCE["fwsegsnr"] == 1e-3
    assert len(search.RECORD_FIELDS) == 7 and search.TABLE_COLUMN["xstatus"] == 5


def _table(scores, col):
    t = np.zeros((len(scores), 8))
    t[:, 2] = 1
    t[:, 3] = 0.5
    t[:, col] = scores
    return t


@pytest.mark.parametrize("objective", ["segsnr", "fwsegsnr"])
def test_select_best_quality_objectives(objective):
    specs = search.job_specs(1, [ALG], GRID)
    col = search.QUALITY_COLUMNS[objective]
    # a tie inside 1e-3 keeps the earlier cell; a gain beyond it moves on
    t = _table([5.0, 5.0009, 4.0, 5.0], col)
    assert search.select_best(specs, t, objective)[(0, ALG)] == (0, 5.0)
    t = _table([5.0, 5.0009, 5.0011, 5.0015], col)
    assert search.select_best(specs, t, objective)[(0, ALG)] == (2, 5.0011)
    # a non-finite cell and a NaN score are skipped
    t = _table([9.0, np.nan, 3.0, 2.0], col)
    t[0, 2] = 0
    assert search.select_best(specs, t, objective)[(0, ALG)] == (2, 3.0)
    # dB scores below the reference's starting incumbent of -1 are still selected
    neg = _table([-7.0, -6.9995, -5.0, np.nan], col)
    assert search.select_best(specs, neg, objective)[(0, ALG)] == (2, -5.0)
    assert search.select_best(list(specs), neg, objective)[(0, ALG)] == (2, -5.0)
    # while the old objectives keep the reference's start
    low = neg.copy()
    low[:, 1] = -7.0
    assert search.select_best(specs, low, "snr")[(0, ALG)] == (-1, None)
    # the list form of the specs takes the same path
    assert search.select_best(list(specs), t, objective)[(0, ALG)] == (2, 3.0)
    with pytest.raises(ValueError, match="quality=True"):
        search.select_best(specs, t[:, :6], objective)
    # the old objectives read the same columns of the wider table
    assert search.select_best(specs, t, "stoi")[(0, ALG)][0] == 1


def _jump_scan(sc, ok, tol, start):
    """The reference's loop, cell by cell (speech_enhancement_comparison.py:183-216)."""
    incumbent, win = start, -1
    for k in range(len(sc)):
        if ok[k] and sc[k] > incumbent + tol:
            incumbent, win = float(sc[k]), k
    return win, (incumbent if win >= 0 else None)


@pytest.mark.parametrize("objective", ["snr", "stoi", "segsnr", "fwsegsnr"])
@pytest.mark.parametrize("tol", [-0.1, 0.0, 0.05])
def test_select_best_any_tolerance_over_several_groups(objective, tol):
    """Two pairs x two algorithms: every group starts its own scan, with both
    forms of the specs and on both sides of tol = 0 (two code paths)."""
    grids = dict(GRID, wiener={"alpha": [0.9, 0.98], "gain_floor": [0.05, 0.1], "n_fft": [512],
                               "hop_length": [128], "noise_percentile": [20.0],
                               "noise_method": ["percentile"]})
    specs = search.job_specs(2, list(grids), grids)
    assert len(specs) == 16
    col = {**search.TABLE_COLUMN, **search.QUALITY_COLUMNS}[objective]
    t = np.zeros((16, 8))
    t[:, 2] = 1
    t[:, col] = [3, 4, 2, 5, 1, 2, 3, 2.5, 0.5, 0.45, 0.52, 0.6, -3, -2.95, -4, -2]
    t[5, 2] = 0
    t[10, col] = np.nan
    start = -np.inf if objective in search.QUALITY_COLUMNS else -1.0
    want = {}
    for g, key in enumerate([(0, ALG), (0, "wiener"), (1, ALG), (1, "wiener")]):
        rows = np.arange(4 * g, 4 * g + 4)
        ok = (t[rows, 2] != 0) & ~np.isnan(t[rows, col])
        win, score = _jump_scan(t[rows, col], ok, tol, start)
        want[key] = (-1, None) if win < 0 else (int(rows[win]), score)
    assert want[(0, ALG)] == (3, 5.0)
    assert want[(1, "wiener")][0] == (-1 if start == -1.0 else 15)
    assert dict(search.select_best(specs, t, objective, tol=tol)) == want
    assert dict(search.select_best(list(specs), t, objective, tol=tol)) == want


def test_unknown_objective_still_raises_key_error():
    specs = search.job_specs(1, [ALG], GRID)
    with pytest.raises(KeyError):
        search.select_best(specs, np.zeros((4, 8)), "loudness")
    with pytest.raises(ValueError):
        search.select_best(specs, np.zeros((4, 8)), "pesq")


def test_cells_per_launch_comes_from_the_byte_budget():
    """SegSnrPlan's chunking against a library that reports scratch: the cells
    per launch are the budget over the per-cell figure, never a fixed count."""
    from classical_speech_enhancement_amd import metrics

    class Lib:
        def __init__(self, per):
            self.per = per

        def cse_segsnr_scratch_bytes(self, n, L, sr):
            return n * self.per

    plan = object.__new__(metrics.SegSnrPlan)
    plan.L, plan.sr = 160000, 16000
    for per, want in ((0, metrics.SEGSNR_MAX_CELLS), (1 << 20, 1024), (3 << 30, 1),
                      (1, metrics.SEGSNR_MAX_CELLS)):
        plan.lib = Lib(per)
        assert plan.cells_per_launch() == want
        assert want * per <= max(metrics.SEGSNR_SCRATCH_BYTES, per)


def test_gather_records_takes_its_width_from_the_records():
    rng = np.random.default_rng(0)
    for width in (7, 9):
        vals = rng.standard_normal((5, width - 1))
        order = np.array([3, 0, 4, 1, 2])
        local = np.concatenate([order[:, None].astype(np.float64), vals], axis=1)
        table = search.gather_records(local, 5)
        assert table.shape == (5, width - 1)
        assert np.array_equal(table[order], vals)
    with pytest.raises(ValueError):
        search.gather_records(np.zeros((2, 5)), 2)


def quality_compute(clean, noisy, specs, ids):
    """oracle_compute plus the two quality columns from the restatement, of the
    finalised output rounded to f32 like the device's waveforms."""
    import oracle
    base = oracle_compute(clean, noisy, specs, ids)
    out = np.full((len(ids), 8), np.nan)
    out[:, :6] = base
    for j, cid in enumerate(ids):
        pair, alg, p = specs[cid]
        if not base[j, 2]:
            continue
        c = np.asarray(clean[pair], np.float64)
        y = oracle.ALGORITHMS[alg](noisy[pair], 16000, **p)
        e32 = oracle.finalize_enhanced(np.asarray(y, np.float32).astype(np.float64), c, 16000)
        out[j, 6:] = ref.scores(c, e32, 16000)
    return out


def test_run_grid_quality_single_process():
    clean, noisy = pairs(2, 0.5)
    specs = search.job_specs(2, [ALG], GRID)
    table, best = search.run_grid(clean, noisy, specs, compute=quality_compute, quality=True,
                                  objective="fwsegsnr")
    assert table.shape == (8, 8)
    full = quality_compute(clean, noisy, specs, np.arange(8))
    assert np.array_equal(table, full, equal_nan=True)
    assert best == search.select_best(specs, full, "fwsegsnr")
    assert all(v[0] >= 0 for v in best.values())
    # a compute function of the plain width is refused when quality is asked for
    with pytest.raises(ValueError, match="8 columns"):
        search.run_grid(clean, noisy, specs, compute=oracle_compute, quality=True)
    # and the default still returns the plain table
    plain, _ = search.run_grid(clean, noisy, specs, compute=oracle_compute)
    assert np.array_equal(plain, full[:, :6], equal_nan=True)


def quality_rank_main(rank, world, port, outdir):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        clean, noisy = pairs(2, 0.5)
        specs = search.job_specs(2, [ALG], GRID)
        table, best = search.run_grid(clean, noisy, specs, compute=quality_compute, quality=True,
                                      objective="fwsegsnr")
        np.savez(os.path.join(outdir, f"rank{rank}.npz"), table=table,
                 win=np.array([v[0] for v in best.values()]))
    finally:
        dist.destroy_process_group()


def test_run_grid_quality_gloo_world_2(tmp_path):
    import torch.multiprocessing as tmp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    tmp.spawn(quality_rank_main, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    clean, noisy = pairs(2, 0.5)
    specs = search.job_specs(2, [ALG], GRID)
    full = quality_compute(clean, noisy, specs, np.arange(8))
    win = [v[0] for v in search.select_best(specs, full, "fwsegsnr").values()]
    for r in range(2):
        d = np.load(tmp_path / f"rank{r}.npz")
        assert d["table"].shape == (8, 8)
        assert np.array_equal(d["table"], full, equal_nan=True)
        assert d["win"].tolist() == win


def test_optimize_parameters_quality_entries():
    clean, noisy = pairs(1, 0.5)
    base = ref.scores(clean[0], noisy[0], 16000)
    res = search.optimize_parameters(clean[0], noisy[0], 16000, ALG, GRID[ALG],
                                     compute=quality_compute, stoi_fn=lambda c, n, sr: 0.5,
                                     quality=True, quality_fn=lambda c, n, sr: base)
    specs = search.job_specs(1, [ALG], GRID)
    table = res["table"]
    assert table.shape == (4, 8)
    for k, name in enumerate(("segsnr", "fwsegsnr")):
        cid, score = search.select_best(specs, table, name)[(0, ALG)]
        assert res[name] == {"score": score, "params": dict(specs[cid][2]), "cell": cid,
                             "snr": float(table[cid, 1])}
        assert res["baseline"][name] == base[k]
        assert res["improvements"][name] == score - base[k]
    plain = search.optimize_parameters(clean[0], noisy[0], 16000, ALG, GRID[ALG],
                                       compute=oracle_compute, stoi_fn=lambda c, n, sr: 0.5)
    assert "segsnr" not in plain and "fwsegsnr" not in plain
    assert set(plain["baseline"]) == {"snr", "stoi"}


# ----------------------------------------------------------------------- _lib
def test_lib_exports_and_abi():
    assert _lib.EXPORTS_SEGSNR == ("cse_segsnr_workspace_bytes", "cse_segsnr_prepare",
                                   "cse_segsnr_scratch_bytes", "cse_segsnr_cells")
    assert _lib.ABI_VERSION == 5
    assert not set(_lib.EXPORTS_SEGSNR) & set(_lib.EXPORTS)
    header = open(os.path.join(os.path.dirname(_lib.HERE), "include", "cse_segsnr.h")).read()
    for name in _lib.EXPORTS_SEGSNR:
        assert name + "(" in header


def test_library_exports_the_entry_points():
    lib = _lib.load()  # build() comes before the tests: a missing library is an error
    for name in _lib.EXPORTS_SEGSNR:
        assert hasattr(lib, name)
    # the size functions need no device
    assert lib.cse_segsnr_workspace_bytes(2, 16000, 16000) > 2 * 16000 * 4
    assert lib.cse_segsnr_workspace_bytes(2, 16000, 8000) > 0
    assert lib.cse_segsnr_workspace_bytes(2, 16000, 22050) == -1
    assert lib.cse_segsnr_workspace_bytes(-1, 16000, 16000) == -1
    assert lib.cse_segsnr_scratch_bytes(4096, 160000, 16000) == 0
    assert lib.cse_segsnr_scratch_bytes(1, 16000, 44100) == -1
    # argument checks come before any device work
    assert lib.cse_segsnr_cells(None, None, None, None, 1, 1, 16000, 16000, 1, None, None, None,
                                None, None) < 0
    assert b"cse_segsnr_cells" in lib.cse_last_error()
    assert lib.cse_segsnr_prepare(None, 1, 16000, 11025, None, None) < 0
    assert b"11025" in lib.cse_last_error()


def test_kernel_src_sha_is_the_parents():
    """The enhance kernels, cse_common.hpp, cse_special.hpp and cse.h are
    untouched: the committed PMC profiles keep matching this build."""
    import bench
    assert bench.kernel_src_sha() == "0294b26e5cf891db"


# -------------------------------------------------------------------- results
OLD_KEYS = set(results.ROW_KEYS) | {"snr_snropt", "best_params_snr"}


def test_result_row_default_keys_are_unchanged(tmp_path):
    row = results.result_row("p", ALG, 16000, 1.0, 2.0, {"alpha": 1.0}, stoi_noisy=0.5,
                             stoi_best=0.6, stoi_params={"alpha": 2.0}, snr_stoiopt=1.5)
    assert set(row) == OLD_KEYS
    means = results.write_summary([row], [ALG], str(tmp_path))
    assert set(means[ALG]) == {"count"} | {k for k, _ in results.SUMMARY_KEYS}


def test_result_row_quality_keys(tmp_path):
    row = results.result_row("p", ALG, 16000, 1.0, 2.0, {"alpha": 1.0}, segsnr_noisy=-1.0,
                             fwsegsnr_noisy=3.0, fwsegsnr_best=7.5,
                             fwsegsnr_params={"alpha": 2.0}, snr_fwsegopt=4.0)
    assert set(row) == OLD_KEYS | set(results.QUALITY_KEYS)
    assert row["best_params_fwsegsnr"] == {"alpha": 2.0} and row["fwsegsnr_best"] == 7.5
    other = dict(row, fwsegsnr_best=8.5, stem="q")
    means = results.write_summary([row, other], [ALG], str(tmp_path))[ALG]
    assert means["fwsegsnr_best_mean"] == 8.0 and means["segsnr_noisy_mean"] == -1.0
    assert means["snr_fwsegopt_mean"] == 4.0 and means["fwsegsnr_noisy_mean"] == 3.0
    with pytest.raises(TypeError):
        results.result_row("p", ALG, 16000, 1.0, 2.0, {}, pesq_best=1.0)
