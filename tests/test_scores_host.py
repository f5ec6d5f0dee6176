"""The score-family registry (classical_speech_enhancement_amd/scores.py), the
parts that need no GPU: what search.py and results.py derive from the records
equals what was written out per family before (the literals below are this
file's own), every record agrees with metrics, _lib and its header, and the
loops over the records (select_best, table_width, result_row, summary_means) do
for every family what the per-family code did."""

import ast
import inspect
import itertools
import math
import os
import re

import numpy as np
import pytest

from classical_speech_enhancement_amd import _lib, results, scores, search
from classical_speech_enhancement_amd.scores import FAMILIES

INCLUDE = os.path.join(os.path.dirname(__file__), "..", "include")
FLAGS = ("quality", "distortion", "separation", "wss")
NCOL = 6
# objective -> (column, sign, tolerance, skips +-inf, flag, width of its family's table)
OBJECTIVES = {
    "segsnr": (6, +1, 1e-3, False, "quality", 8), "fwsegsnr": (7, +1, 1e-3, False, "quality", 8),
    "llr": (8, -1, 1e-4, False, "distortion", 10), "cep": (9, -1, 1e-3, False, "distortion", 10),
    "sisdr": (10, +1, 1e-3, True, "separation", 13),
    "sisir": (11, +1, 1e-3, True, "separation", 13),
    "sisar": (12, +1, 1e-3, True, "separation", 13),
    "wss": (13, -1, 1e-2, False, "wss", 14)}
ARGS = {
    "quality": ("segsnr_noisy", "fwsegsnr_noisy", "fwsegsnr_best", "fwsegsnr_params",
                "snr_fwsegopt"),
    "distortion": ("llr_noisy", "cep_noisy", "llr_best", "llr_params", "snr_llropt"),
    "separation": ("sisdr_noisy", "sisdr_best", "sisir_sisdropt", "sisar_sisdropt",
                   "sisdr_params", "snr_sisdropt"),
    "wss": ("wss_noisy", "wss_best", "wss_params", "snr_wssopt")}
KEYS = {
    "quality": ("segsnr_noisy", "fwsegsnr_noisy", "fwsegsnr_best", "best_params_fwsegsnr",
                "snr_fwsegopt"),
    "distortion": ("llr_noisy", "cep_noisy", "llr_best", "best_params_llr", "snr_llropt"),
    "separation": ("sisdr_noisy", "sisdr_best", "sisir_sisdropt", "sisar_sisdropt",
                   "best_params_sisdr", "snr_sisdropt"),
    "wss": ("wss_noisy", "wss_best", "best_params_wss", "snr_wssopt")}
SUMMARY = {
    "quality": (("segsnr_noisy_mean", "segsnr_noisy"), ("fwsegsnr_noisy_mean", "fwsegsnr_noisy"),
                ("fwsegsnr_best_mean", "fwsegsnr_best"), ("snr_fwsegopt_mean", "snr_fwsegopt")),
    "distortion": (("llr_noisy_mean", "llr_noisy"), ("cep_noisy_mean", "cep_noisy"),
                   ("llr_best_mean", "llr_best"), ("snr_llropt_mean", "snr_llropt")),
    "separation": (("sisdr_noisy_mean", "sisdr_noisy"), ("sisdr_best_mean", "sisdr_best"),
                   ("sisir_sisdropt_mean", "sisir_sisdropt"),
                   ("sisar_sisdropt_mean", "sisar_sisdropt"),
                   ("snr_sisdropt_mean", "snr_sisdropt")),
    "wss": (("wss_noisy_mean", "wss_noisy"), ("wss_best_mean", "wss_best"),
            ("snr_wssopt_mean", "snr_wssopt"))}
MARKER = {"quality": "fwsegsnr_best", "distortion": "llr_best", "separation": "sisdr_best",
          "wss": "wss_best"}
# flag -> (plan class, the cse_<prefix>_ of its entry points and the name of its header)
PLANS = {"quality": ("SegSnrPlan", "segsnr"), "distortion": ("LpcPlan", "lpc"),
         "separation": ("SiSdrPlan", "sisdr"), "wss": ("WssPlan", "wss")}
VALUES = {"quality": dict(segsnr_noisy=-1.0, fwsegsnr_noisy=3.0, fwsegsnr_best=7.5,
                          fwsegsnr_params={"alpha": 2.0}, snr_fwsegopt=5.0),
          "distortion": dict(llr_noisy=1.2, cep_noisy=6.0, llr_best=0.4,
                             llr_params={"alpha": 2.0}, snr_llropt=4.0),
          "separation": dict(sisdr_noisy=4.0, sisdr_best=9.5, sisir_sisdropt=15.0,
                             sisar_sisdropt=11.0, sisdr_params={"beta": 0.1}, snr_sisdropt=8.0),
          "wss": dict(wss_noisy=40.0, wss_best=22.0, wss_params={"alpha": 1.0}, snr_wssopt=3.0)}
ALG = "spectralSubtractor"
SUBSETS = [s for r in range(5) for s in itertools.combinations(FLAGS, r)]


# ------------------------------------------------------------------ registry
def test_registry_order_and_module_is_host_only():
    assert tuple(FAMILIES) == FLAGS
    assert [f.flag for f in FAMILIES.values()] == list(FLAGS)
    assert tuple(scores.OBJECTIVES) == tuple(OBJECTIVES)
    tree = ast.parse(open(scores.__file__).read())
    names = {a.name.split(".")[0] for n in ast.walk(tree) if isinstance(n, ast.Import)
             for a in n.names}
    names |= {n.module or "" for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)}
    assert names <= {"collections", "typing"}


def test_legacy_constants_keep_their_values():
    assert search.NCOL == scores.NCOL == NCOL
    assert search.QUALITY_COLUMNS == {"segsnr": 6, "fwsegsnr": 7}
    assert search.DISTORTION_COLUMNS == {"llr": 8, "cep": 9}
    assert search.SEPARATION_COLUMNS == {"sisdr": 10, "sisir": 11, "sisar": 12}
    assert search.WSS_COLUMNS == {"wss": 13}
    assert list(search.SEPARATION_COLUMNS) == ["sisdr", "sisir", "sisar"]
    assert search.SCAN_START == dict.fromkeys(OBJECTIVES, -math.inf)
    assert search.TOLERANCE == {
        "stoi": 1e-6, "pesq": 1e-3, "balance": 1e-5, "snr": 1e-5, "segsnr": 1e-3,
        "fwsegsnr": 1e-3, "llr": 1e-4, "cep": 1e-3, "sisdr": 1e-3, "sisir": 1e-3, "sisar": 1e-3,
        "logerr": 1e-3, "wss": 1e-2}
    for flag in FLAGS:
        up = flag.upper()
        assert getattr(results, up + "_ARGS") == ARGS[flag]
        assert getattr(results, up + "_KEYS") == KEYS[flag]
        assert getattr(results, up + "_SUMMARY_KEYS") == SUMMARY[flag]
    entries = ("workspace_bytes", "prepare", "scratch_bytes", "cells")
    assert _lib.EXPORTS_SEGSNR == tuple(f"cse_segsnr_{e}" for e in entries)
    assert _lib.EXPORTS_LPC == tuple(f"cse_lpc_{e}" for e in entries)
    assert _lib.EXPORTS_WSS == tuple(f"cse_wss_{e}" for e in entries)


@pytest.mark.parametrize("flags", list(itertools.product([False, True], repeat=4)))
def test_table_width(flags):
    quality, distortion, separation, wss = flags
    want = NCOL + (8 if wss else 7 if separation else 4 if distortion else 2 if quality else 0)
    assert search.table_width(*flags) == want
    assert search.table_width(**dict(zip(FLAGS, flags))) == want
    assert search.table_width() == NCOL


@pytest.mark.parametrize("flag", FLAGS)
def test_record_matches_metrics_lib_and_header(flag):
    from classical_speech_enhancement_amd import metrics
    f = FAMILIES[flag]
    plan, prefix = PLANS[flag]
    assert f.plan == plan
    assert f.names == tuple(n for n, v in OBJECTIVES.items() if v[4] == flag)
    assert (f.first, scores.width(f)) == (OBJECTIVES[f.names[0]][0], OBJECTIVES[f.names[0]][5])
    assert f.tolerance == {n: OBJECTIVES[n][2] for n in f.names}
    assert f.lead in f.names and set(f.baselines) <= set(f.names)
    assert f.plan_takes_noisy == (flag == "separation") and f.all_or_none == (flag == "wss")
    cls = getattr(metrics, plan)
    assert cls._WHICH == f.names
    # every entry point the plan calls is exported and declared in its header:
    # the ones its own source names, and SegSnrPlan's _fn(...) under its prefix
    src = inspect.getsource(cls)
    used = set(re.findall(r"cse_%s_\w+" % prefix, src))
    if issubclass(cls, metrics.SegSnrPlan):
        assert cls._PREFIX == "cse_" + prefix
        used |= {f"cse_{prefix}_{e}"
                 for e in re.findall(r'_fn\("(\w+)"\)', inspect.getsource(metrics.SegSnrPlan))}
        assert len(used) == 4
    exports = getattr(_lib, "EXPORTS_" + prefix.upper())
    header = open(os.path.join(INCLUDE, f"cse_{prefix}.h")).read()
    assert used and used <= set(exports)
    for name in used:
        assert re.search(r"\b%s\s*\(" % name, header), name
    # evaluate_audio_quality and optimize_parameters find calculate_<name> by name
    for name in f.names if not f.plan_takes_noisy else f.baselines:
        assert callable(getattr(metrics, "calculate_" + name))


# --------------------------------------------------------------- select_best
GRID = {ALG: dict(alpha=[1.0, 2.0, 3.0], beta=[0.01, 0.1], n_fft=[512, 1024], hop_length=[128],
                  noise_percentile=[10.0], noise_method=["percentile"]),
        "wiener": dict(alpha=[0.9, 0.98], gain_floor=[0.1, 0.2, 0.3], n_fft=[512],
                       hop_length=[128], noise_percentile=[10.0, 20.0],
                       noise_method=["percentile"])}


def _specs():
    return search.job_specs(3, [ALG, "wiener"], GRID)


def _table(n, width=NCOL + 8):
    """Seeded scores on a coarse lattice (ties and near ties inside every
    tolerance), cells that are not finite, and NaN, +inf and -inf sprinkled
    over the score columns."""
    rng = np.random.default_rng(20)
    t = np.round(rng.normal(size=(n, width)) * 3, 1)
    t[1::4, 3:] = t[0::4, 3:][:len(t[1::4])] + 5e-5  # inside every tolerance
    t[:, 2] = rng.random(n) > 0.15
    for v in (np.nan, np.inf, -np.inf):
        t[rng.integers(0, n, n // 5), rng.integers(3, width, n // 5)] = v
    return t


def _scan(specs, table, objective, tol):
    """The sequential best-so-far rule, one (pair, algorithm) group at a time."""
    col, sign, dflt, finite_only, _, _ = OBJECTIVES[objective]
    tol = dflt if tol is None else tol
    best = {}
    for cid, (pair, alg, _) in enumerate(specs):
        best.setdefault((pair, alg), [-math.inf if sign > 0 else math.inf, -1])
        v = float(table[cid, col])
        if table[cid, 2] == 0 or v != v or (finite_only and not math.isfinite(v)):
            continue
        inc = best[(pair, alg)]
        if (v > inc[0] + tol) if sign > 0 else (v < inc[0] - tol):
            inc[:] = [v, cid]
    return {k: (win, inc if win >= 0 else None) for k, (inc, win) in best.items()}


@pytest.mark.parametrize("tol", [None, 0.25, -0.25])
@pytest.mark.parametrize("objective", list(OBJECTIVES))
def test_select_best_is_the_per_group_scan(objective, tol):
    specs = _specs()
    table = _table(len(specs))
    assert table.shape == (72, 14)
    for kind in (specs, [tuple(s) for s in specs]):
        got = search.select_best(kind, table, objective, tol)
        want = _scan(specs, table, objective, tol)
        assert list(got) == list(want) == [(p, a) for p in range(3) for a in (ALG, "wiener")]
        assert dict(got) == want
    assert any(win >= 0 for win, _ in want.values())


def test_select_best_skips_and_tolerance_have_something_to_do():
    """The seeded table makes every rule matter somewhere: the winners change
    when the skip of +-inf or the tolerance is left out."""
    specs = _specs()
    table = _table(len(specs))
    cols = table[:, NCOL:]
    assert np.isnan(cols).any() and (cols == np.inf).any() and (cols == -np.inf).any()
    assert (table[:, 2] == 0).any()
    assert any(dict(search.select_best(specs, table, o, 0.0)) != dict(search.select_best(specs, table, o))
               for o in OBJECTIVES)
    sep = [o for o, v in OBJECTIVES.items() if v[3]]
    assert any(np.isinf(table[table[:, 2] != 0][:, OBJECTIVES[o][0]]).any() for o in sep)


@pytest.mark.parametrize("objective", list(OBJECTIVES))
def test_select_best_names_the_table_it_needs(objective):
    col, _, _, _, flag, need = OBJECTIVES[objective]
    specs = _specs()
    for width in (NCOL, NCOL + 2, NCOL + 4, NCOL + 7, NCOL + 8):
        table = _table(len(specs), width)
        if width > col:
            search.select_best(specs, table, objective)
            continue
        msg = (f"objective '{objective}' needs a {flag}=True table of {need} columns, "
               f"this one has {width}")
        for kind in (specs, list(specs)):
            with pytest.raises(ValueError, match="^" + re.escape(msg) + "$"):
                search.select_best(kind, table, objective)
    with pytest.raises(ValueError, match="not scored on the device"):
        search.select_best(specs, _table(len(specs)), "pesq")


# ---------------------------------------------------------------- result_row
def _row(**kw):
    return results.result_row("p", ALG, 16000, 1.0, 2.0, {"alpha": 1.0}, **kw)


@pytest.mark.parametrize("subset", SUBSETS, ids=lambda s: "+".join(s) or "none")
def test_result_row_for_every_subset(subset):
    kw = {k: v for flag in subset for k, v in VALUES[flag].items()}
    row = _row(**kw)
    plain = _row()
    assert list(row) == list(plain) + [k for flag in FLAGS if flag in subset for k in KEYS[flag]]
    assert all(row[k] == plain[k] for k in plain)
    for flag in subset:
        for arg, key in zip(ARGS[flag], KEYS[flag]):
            assert row[key] == VALUES[flag][arg], key
        params = next(a for a in ARGS[flag] if a.endswith("_params"))
        assert row["best_params_" + params[:-7]] is not VALUES[flag][params]  # a copy
    with pytest.raises(TypeError, match=r"^result_row: unexpected keywords \['abc', 'zzz'\]$"):
        _row(zzz=1, abc=2, **kw)


def test_result_row_partial_groups():
    """A part of the WSS keywords raises; a part of another group's fills None
    (and {} for the parameters), as it always did."""
    for drop in ARGS["wss"]:
        kw = {k: v for k, v in VALUES["wss"].items() if k != drop}
        with pytest.raises(TypeError, match=r"^result_row: the WSS keywords go together, "
                                            r"missing \['%s'\]$" % drop):
            _row(**kw)
        with pytest.raises(TypeError, match="the WSS keywords go together"):
            _row(**kw, **VALUES["quality"])
    with pytest.raises(TypeError, match=r"missing \['snr_wssopt', 'wss_noisy', 'wss_params'\]$"):
        _row(wss_best=1.0)
    for flag in ("quality", "distortion", "separation"):
        for drop in ARGS[flag]:
            row = _row(**{k: v for k, v in VALUES[flag].items() if k != drop})
            for arg, key in zip(ARGS[flag], KEYS[flag]):
                want = VALUES[flag][arg] if arg != drop else {} if arg.endswith("_params") else None
                assert row[key] == want, (drop, key)
        lone = _row(**{ARGS[flag][0]: 1.5})
        assert [lone[k] for k in KEYS[flag]] == [1.5] + [
            {} if k.startswith("best_params_") else None for k in KEYS[flag][1:]]


# -------------------------------------------------------------- summary_means
@pytest.mark.parametrize("subset", SUBSETS, ids=lambda s: "+".join(s) or "none")
def test_summary_means_follow_the_marker_key(subset):
    kw = {k: v for flag in subset for k, v in VALUES[flag].items()}
    rows = [_row(**kw), _row()]
    means = results.summary_means(rows, [ALG, "wiener"])
    base = [k for k, _ in results.SUMMARY_KEYS]
    assert list(means[ALG]) == ["count"] + base + [
        k for flag in FLAGS if flag in subset for k, _ in SUMMARY[flag]]
    assert list(means["wiener"]) == ["count"] + base and means["wiener"]["count"] == 0
    for flag in subset:
        for key, field in SUMMARY[flag]:
            assert means[ALG][key] == VALUES[flag][field]  # the row without the keys is skipped
    # the marker alone decides: a row that has only it gets the whole group
    for flag in FLAGS:
        got = results.summary_means([dict(_row(), **{MARKER[flag]: 2.0})], [ALG])[ALG]
        assert [k for k in got if k not in base and k != "count"] == [k for k, _ in SUMMARY[flag]]
        assert got[MARKER[flag] + "_mean"] == 2.0
        other = dict(_row(), **{KEYS[flag][0]: 2.0}) if KEYS[flag][0] != MARKER[flag] else _row()
        assert list(results.summary_means([other], [ALG])[ALG]) == ["count"] + base
