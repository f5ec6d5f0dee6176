"""Grid-search driver: the data-parallel rewrite of the reference's sweep.

The reference walks pairs -> algorithms -> parameter combinations one cell at
a time (speech_enhancement_comparison.py:149-226 inside optimize_parameters,
called per algorithm from run_algorithm_on_pair :278-294 and main :440-455).
Here the whole (pair x algorithm x grid cell) set is one job:

  job_specs      the reference's enumeration order; a cell's index in this
                 list is its cell_id (grid order inside each (pair, algorithm))
  work_items     cells grouped by what they share on the device:
                 (pair, n_fft, hop, algorithm) -> one STFT, one set of noise
                 rows; cost = cells x frames x bins x algorithm weight
  assign_shards  contiguous runs of cell ids of equal modelled cost per rank
                 (SURVEY §8(e)'s cost model): whole pairs per rank, so each
                 pair's STFT and noise PSDs run on one rank (two at a cut)
  run_grid       each rank computes its cells (Engine on its GPU), then ONE
                 all_gather of fixed-size 56-B records (RECORD_FIELDS: cell_id,
                 sse, snr, finite, stoi, lag, xstatus; a 6-column table)
                 (RCCL over xGMI for backend "nccl", gloo in CPU tests)
  select_best    rank 0's sequential best-so-far scan in grid order
                 (speech_enhancement_comparison.py:183-216) — NOT an argmax:
                 a later cell replaces the incumbent only if it beats it by
                 more than tol, so ties within tol keep the earlier cell

Scores: the reference scores cells by STOI, PESQ and their balance
(evaluation_metrics.py:30-36, 104-115).  The device path computes STOI
(cse_stoi_cells, pystoi 0.4.1 restated) and the SNR of the clipped output
(evaluation_metrics.py:39-58).  PESQ's C extension is not in this image, so
the PESQ and balance objectives are not scored; STOI and SNR each get the
reference's sequential selection (the reference itself skips a cell whose
PESQ is None, speech_enhancement_comparison.py:180-181 — that rule is dropped, or nothing would be selected).
Each cell is scored like finalize_enhanced (:92-106): its output is aligned
to the clean reference by the cross-correlation lag (on the device,
cse_xcorr_lag), length-matched, checked for finiteness and clipped, then
calculate_snr and calculate_stoi.

extended=True (run_grid, optimize_parameters, run_sweep; stoi="extended" in
engine_compute) scores extended STOI in place of STOI (cse_estoi_cells,
include/cse_estoi.h): the STOI column and every stoi field then hold ESTOI, and
the selection and its tolerance are the STOI objective's.

coherence=True (run_grid, optimize_parameters, run_sweep; stoi="coherence" in
engine_compute) scores I3, the fit of the three-level coherence speech
intelligibility index (cse_csii_cells, include/cse_csii.h; Kates & Arehart
2005), in place of STOI in exactly the same way: the STOI column and every stoi
field then hold I3, and the selection and its tolerance are the STOI
objective's.  A clip with no mid-level or no low-level frame has no I3: its
cells hold NaN in the column and the scan skips them, like any cell without a
score.  extended and coherence exclude each other.

modulation=True (run_grid, optimize_parameters, run_sweep; stoi="modulation" in
engine_compute) scores ncm, the normalized covariance measure with the fixed
articulation-index weights (cse_ncm_cells, include/cse_ncm.h), in place of STOI
in exactly the same way: the STOI column and every stoi field then hold ncm,
and the selection and its tolerance are the STOI objective's.  A clip of fewer
than 12 30-ms frames has no ncm (NaN, skipped).  modulation excludes extended
and coherence: the three switches fill one column.

quality=True (engine_compute, run_grid, optimize_parameters, run_sweep) adds the
quality objective the reference takes from PESQ: segmental SNR and
frequency-weighted segmental SNR (cse_segsnr_cells, include/cse_segsnr.h;
Hu & Loizou 2008) of the same finalised waveforms, as two more table columns
(QUALITY_COLUMNS) with objectives "segsnr" and "fwsegsnr".  The default leaves
every table, record and result as it was.

distortion=True (the same four functions) adds the two LPC envelope measures
of include/cse_lpc.h, the log-likelihood ratio and the cepstrum distance
(cse_lpc_cells; Hu & Loizou 2008's best predictor of signal distortion), as
columns 8 and 9 (DISTORTION_COLUMNS) of a table that then always has NCOL + 4
columns: columns 6 and 7 are the quality columns, NaN unless quality=True is
given too.  "llr" and "cep" are objectives that are minimised.

separation=True (the same four functions) adds the scale-invariant SDR of
include/cse_sisdr.h and its two parts, SI-SIR (what is left of the noise) and
SI-SAR (what the algorithm added), from cse_sisdr_cells with the pair's own
noisy - clean as the interference: columns 10 to 12 (SEPARATION_COLUMNS) of a
table that then always has NCOL + 7 columns, the quality and distortion columns
NaN unless asked for too.  "sisdr", "sisir" and "sisar" are maximised; a value
that is not finite (NaN, +inf, -inf) is skipped.

wss=True (engine_compute, run_grid, run_sweep) adds the weighted spectral slope
distance of include/cse_wss.h (cse_wss_cells), the one ingredient of Hu &
Loizou's composite measures besides PESQ that the other columns do not hold:
column NCOL + 7 (WSS_COLUMNS) of a table that then always has NCOL + 8 columns,
the earlier optional columns NaN unless asked for too.  "wss" is minimised.

These four keywords are the records of scores.FAMILIES, in table order; the
tables, the selection, the sweep's per-family work and the result rows loop
over the records, and the per-family constants below (QUALITY_COLUMNS, ...) are
derived from them.  The public signatures keep one keyword per family and pass
the requested records, or the dict of flags, down.  STOI is no family: it owns
column 3 of every table and the extended, coherence and modulation switches.

score_noise_estimators and sweep_tracker judge noise-PSD estimates themselves,
with no enhancement algorithm on top: the logarithmic estimation error of
include/cse_logerr.h (cse_logerr_rows) against the smoothed power of the pair's
own noisy - clean, split into over- and under-estimation.  sweep_tracker
enumerates one tracker's parameter sets in grid_cells' order and applies the
sequential best-so-far rule to the mean over pairs, minimised.
"""

import math
import os
from collections import OrderedDict

import numpy as np

from . import scores
from .parameter_ranges import ALGORITHM_GRIDS, grid_cells
from .scores import FAMILIES, OBJECTIVES
from .trackers import TRACKERS

# per-bin cost weights (measured kernel time per frame, OMLSA ~ 3x SS)
ALGO_WEIGHT = {"spectralSubtractor": 1.0, "wiener": 1.1, "mmse": 2.0, "omlsa": 3.0}
# tolerance of the best-so-far update per objective (speech_enhancement_comparison.py:183,194,205)
# and the optional families' (scores.FAMILIES)
TOLERANCE = {"stoi": 1e-6, "pesq": 1e-3, "balance": 1e-5, "snr": 1e-5,
             # logerr (dB, sweep_tracker's objectives): the step of the other dB objectives
             "logerr": 1e-3,
             **{name: tol for f in FAMILIES.values() for name, tol in f.tolerance.items()}}

# one float64 row per cell.  lag: finalize_enhanced's alignment lag (0 when
# not aligned); xstatus: cse_xcorr_lag's status (engine: XCORR_OK, XCORR_FLAT =
# the exact many-candidate path ran, XCORR_NONFINITE; 0 when not aligned)
RECORD_FIELDS = ("cell_id", "sse", "snr", "finite", "stoi", "lag", "xstatus")
TABLE_COLUMN = {"sse": 0, "snr": 1, "finite": 2, "stoi": 3, "lag": 4,
                "xstatus": 5}  # table = records without cell_id
NCOL = len(RECORD_FIELDS) - 1
assert NCOL == scores.NCOL
# The optional families' columns follow the NCOL ones in registry order: a
# table is as wide as its last requested family needs, the earlier families'
# columns NaN unless asked for too.  quality: NCOL + 2 columns; distortion:
# NCOL + 4, minimised (select_best scans the negated column); separation: NCOL +
# 7, unbounded dB values of which select_best skips what is not finite; wss:
# NCOL + 8, minimised.
QUALITY_COLUMNS, DISTORTION_COLUMNS, SEPARATION_COLUMNS, WSS_COLUMNS = (
    scores.columns(f) for f in FAMILIES.values())
# where select_best's scan starts: the reference's -1 (speech_enhancement_comparison.py:126-141)
# unless the objective's values go below it (the families' dB scores and distances)
SCAN_START = {name: -math.inf for name in OBJECTIVES}


def table_width(quality=False, distortion=False, separation=False, wss=False):
    """Columns of a table: NCOL, + 2 with quality, + 4 with distortion (with or
    without quality), + 7 with separation, + 8 with wss (whatever else is asked
    for)."""
    return _width(scores.requested(quality=quality, distortion=distortion, separation=separation,
                                   wss=wss))


def _width(fams):
    return scores.width(fams[-1]) if fams else NCOL
# bound on the cell waveforms held at once for STOI scoring (f32 bytes): 48 GiB
# of the 288 GB HBM, i.e. 10 full 10-s pairs (7,308 computed cells x 640 KB each)
# per batch, two batches in flight.  100-pair sweep (late r04, call_r04s.sh in profiles/r04_commands.md):
# 16 GiB 1.48-1.49 s, 32 GiB 1.31-1.32 s, 48 GiB 1.256-1.258 s, 64 GiB
# 1.253-1.295 s; 96 GiB ran out of memory
STOI_WAVE_BYTES = 48 << 30
# share of the device memory free when a sweep starts that the two STOI
# batches in flight may take together (a smaller GPU, or plans cached by the
# caller, shrink the batches below STOI_WAVE_BYTES instead of running out)
STOI_FREE_SHARE = 0.6


def stoi_wave_bytes():
    """Bytes of cell waveforms per STOI batch: STOI_WAVE_BYTES, capped at half
    of STOI_FREE_SHARE of the device memory free now (two batches in flight)."""
    import torch
    free, _ = torch.cuda.mem_get_info()
    # blocks torch's caching allocator holds but no tensor uses are free to this
    # process too (mem_get_info counts them as taken)
    free += torch.cuda.memory_reserved() - torch.cuda.memory_allocated()
    return int(min(STOI_WAVE_BYTES, STOI_FREE_SHARE * free / 2))


class JobSpecs(list):
    """job_specs' result: the list of (pair, algorithm, params) tuples, plus
    numpy columns so the sweep's per-cell bookkeeping (grouping, duplicate
    cells, plan keys, selection) runs without per-cell Python loops:
      pair [n], alg [n] (index into .algorithms), cell [n] (index into
      .cells[alg], the algorithm's grid in reference order).
    Every pair shares the same params dict per grid cell (read-only)."""

    def __init__(self, n_pairs, algorithms, cells):
        algorithms = list(algorithms)
        super().__init__((pair, alg, p) for pair in range(n_pairs) for alg in algorithms
                         for p in cells[alg])
        self.algorithms = algorithms
        self.cells = cells
        per = [len(cells[a]) for a in algorithms]
        self.per_pair = int(sum(per))
        a_col = np.concatenate([np.full(n, k, dtype=np.int64) for k, n in enumerate(per)] or
                               [np.zeros(0, np.int64)])
        c_col = np.concatenate([np.arange(n, dtype=np.int64) for n in per] or [np.zeros(0, np.int64)])
        self.pair = np.repeat(np.arange(n_pairs, dtype=np.int64), self.per_pair)
        self.alg = np.tile(a_col, n_pairs)
        self.cell = np.tile(c_col, n_pairs)
        self._rep = {}

    def grid_rep(self, alg_index, length):
        """For each cell of one algorithm's grid, the first grid cell the engine
        computes identically for signals of this length: same n_fft, hop and
        algorithm parameters and the same noise PSD (engine.noise_key — e.g.
        min_tracking, true_noise and the trackers ignore noise_percentile).  The
        noise key decides, not the method's name: a method whose key leaves
        noise_percentile out is deduplicated without being named here."""
        key = (alg_index, int(length))
        if key not in self._rep:
            from .engine import ALGOS, DEFAULTS, n_frames, noise_key
            alg = self.algorithms[alg_index]
            names = ALGOS[alg][2]
            dflt = DEFAULTS.get(alg, {})
            first, rep = {}, []
            for c, p in enumerate(self.cells[alg]):
                hop = int(p["hop_length"])
                k = (int(p["n_fft"]), hop, tuple(float(p[n] if n in p else dflt[n]) for n in names),
                     noise_key(alg, p, n_frames(length, hop)))
                rep.append(first.setdefault(k, c))
            self._rep[key] = np.asarray(rep, dtype=np.int64)
        return self._rep[key]

    def nfft(self, ids):
        """n_fft of each of ``ids``."""
        if not hasattr(self, "_nfft"):
            self._nfft = [np.array([int(p["n_fft"]) for p in self.cells[a]], dtype=np.int64)
                          for a in self.algorithms]
        ids = np.asarray(ids, dtype=np.int64)
        out = np.empty(len(ids), dtype=np.int64)
        for a, col in enumerate(self._nfft):
            sel = self.alg[ids] == a
            out[sel] = col[self.cell[ids[sel]]]
        return out

    def representative(self, ids, lengths):
        """Global index of the cell computed in place of each of ``ids`` (the
        first identical cell of the same pair and algorithm)."""
        ids = np.asarray(ids, dtype=np.int64)
        lens = np.asarray(lengths, dtype=np.int64)
        present = np.zeros(len(lens), dtype=bool)
        present[self.pair[ids]] = True
        uL = np.unique(lens[present])
        if len(uL) <= 1:  # one clip length (the sweep's case): one table lookup per cell
            if len(uL) == 0:
                return ids.copy()
            L = int(uL[0])
            delta = np.concatenate([self.grid_rep(a, L) - np.arange(len(self.cells[alg]))
                                    for a, alg in enumerate(self.algorithms)])
            off = np.concatenate([[0], np.cumsum([len(self.cells[a]) for a in self.algorithms])[:-1]])
            return ids + delta[off[self.alg[ids]] + self.cell[ids]]
        out = ids.copy()
        for a in range(len(self.algorithms)):
            for L in {int(lengths[q]) for q in np.unique(self.pair[ids[self.alg[ids] == a]])}:
                sel = (self.alg[ids] == a) & (np.asarray(lengths)[self.pair[ids]] == L)
                c = self.cell[ids[sel]]
                out[sel] = ids[sel] - c + self.grid_rep(a, L)[c]
        return out


def job_specs(n_pairs, algorithms=None, grids=None, n_fft=None):
    """(pair, algorithm, params) for every pair x algorithm x grid cell, in the
    reference's order (pairs outermost, registry order of algorithms, grid
    order with the last key fastest), as a JobSpecs list.  One params dict per
    grid cell is shared by every pair (read-only): the engine recognises equal
    batch structures by params identity."""
    grids = grids or ALGORITHM_GRIDS
    algorithms = list(algorithms or grids)
    cells = {alg: [p for p in grid_cells(grids[alg]) if n_fft is None or p["n_fft"] == n_fft]
             for alg in algorithms}
    return JobSpecs(n_pairs, algorithms, cells)


def frames(length, hop):
    return 1 + int(length) // int(hop)


def work_items(specs, lengths):
    """Group cell ids by (pair, n_fft, hop, algorithm).  Returns a list of
    (cost, [cell ids]) (ids ascending within an item)."""
    if isinstance(specs, JobSpecs):
        # per grid cell: n_fft, hop; the group key is a mixed-radix integer
        nf = np.concatenate([[int(p["n_fft"]) for p in specs.cells[a]] for a in specs.algorithms])
        hp = np.concatenate([[int(p["hop_length"]) for p in specs.cells[a]] for a in specs.algorithms])
        off = np.concatenate([[0], np.cumsum([len(specs.cells[a]) for a in specs.algorithms])[:-1]])
        g = off[specs.alg] + specs.cell
        key = ((specs.pair * 4096 + nf[g]) * 4096 + hp[g]) * 64 + specs.alg
        uk, inv = np.unique(key, return_inverse=True)
        order = np.argsort(inv, kind="stable")
        bounds = np.searchsorted(inv[order], np.arange(len(uk) + 1))
        lengths = np.asarray(lengths)
        items = []
        for u in range(len(uk)):
            ids = order[bounds[u]:bounds[u + 1]]
            c0 = int(ids[0])
            alg = specs.algorithms[int(specs.alg[c0])]
            per_cell = (frames(lengths[specs.pair[c0]], hp[g[c0]]) * (int(nf[g[c0]]) // 2 + 1)
                        * ALGO_WEIGHT.get(alg, 1.0))
            items.append((per_cell * len(ids), ids.tolist()))
        return items
    groups = OrderedDict()
    for cid, (pair, alg, p) in enumerate(specs):
        key = (pair, int(p["n_fft"]), int(p["hop_length"]), alg)
        groups.setdefault(key, []).append(cid)
    items = []
    for (pair, n_fft, hop, alg), ids in groups.items():
        per_cell = frames(lengths[pair], hop) * (n_fft // 2 + 1) * ALGO_WEIGHT.get(alg, 1.0)
        items.append((per_cell * len(ids), ids))
    return items


def cell_costs(specs, lengths):
    """Modelled cost of every cell: frames x bins x algorithm weight."""
    lengths = np.asarray(lengths, dtype=np.int64)
    if isinstance(specs, JobSpecs):
        nf = np.concatenate([[int(p["n_fft"]) for p in specs.cells[a]] for a in specs.algorithms])
        hp = np.concatenate([[int(p["hop_length"]) for p in specs.cells[a]] for a in specs.algorithms])
        wt = np.concatenate([[ALGO_WEIGHT.get(a, 1.0)] * len(specs.cells[a])
                             for a in specs.algorithms])
        n_pairs = len(specs) // max(specs.per_pair, 1)
        if n_pairs and len(lengths) >= n_pairs and (lengths[:n_pairs] == lengths[0]).all():
            # one clip length: every pair's block of cells costs the same
            return np.tile((1 + int(lengths[0]) // hp) * (nf // 2 + 1) * wt, n_pairs)
        off = np.concatenate([[0], np.cumsum([len(specs.cells[a]) for a in specs.algorithms])[:-1]])
        g = off[specs.alg] + specs.cell
        return (1 + lengths[specs.pair] // hp[g]) * (nf[g] // 2 + 1) * wt[g]
    return np.array([frames(lengths[pair], p["hop_length"]) * (int(p["n_fft"]) // 2 + 1)
                     * ALGO_WEIGHT.get(alg, 1.0) for (pair, alg, p) in specs], dtype=np.float64)


def assign_shards(specs, lengths, world):
    """Rank of every cell and each rank's modelled load: the job cut into
    ``world`` contiguous runs of cell ids of equal modelled cost (a cell goes to
    the run its cost midpoint falls in).

    Cell ids run pairs -> algorithms -> grid (job_specs), so a rank holds whole
    pairs plus at most a part of one pair at each end of its run: the per-pair
    analysis (STFT and noise PSDs of each (n_fft, hop)) runs on at most
    ceil(pairs / world) + 1 pairs per rank, and every rank gets the same mix of
    algorithms and hops, so an error in the cost model (ALGO_WEIGHT) shifts
    every rank alike.  (A greedy LPT over (pair, n_fft, hop, algorithm) items,
    r01-r02, spread each pair's items over many ranks: at world 8 on the
    100-pair job every rank ran the analysis of 25 pairs instead of 13.)"""
    cost = cell_costs(specs, lengths).astype(np.float64)
    n = len(cost)
    rank_of = np.zeros(n, dtype=np.int64)
    if world > 1 and n:
        total = float(cost.sum())
        mid = np.cumsum(cost) - 0.5 * cost
        rank_of = np.minimum((mid * world / total).astype(np.int64), world - 1)
    load = np.bincount(rank_of, weights=cost, minlength=world).tolist() if n else [0.0] * world
    return rank_of, load


def _unique_inverse(x):
    """np.unique(x, return_inverse=True) for non-negative integer ids, in O(n)
    with a mark array instead of a sort (the sweep's 974,400 representatives)."""
    x = np.asarray(x, dtype=np.int64)
    if len(x) == 0:
        return x.copy(), np.zeros(0, dtype=np.int64)
    mark = np.zeros(int(x.max()) + 1, dtype=bool)
    mark[x] = True
    rank = np.cumsum(mark) - 1
    return np.flatnonzero(mark), rank[x]


def engine_compute(clean, noisy, specs, ids, engine=None, align=True, stoi=True, quality=False,
                   distortion=False, separation=False, wss=False):
    """Device compute of the cells ``ids``: per-cell (sse, snr, finite, stoi,
    lag, xstatus), scored after finalize_enhanced's alignment (align=False: at
    lag 0, lag and xstatus 0).  stoi=False leaves the STOI column NaN (no
    waveforms are kept); stoi="extended" fills it with extended STOI,
    stoi="coherence" with the CSII's I3 (include/cse_csii.h; NaN for a clip
    without mid-level or low-level frames), stoi="modulation" with the
    normalized covariance measure ncm (include/cse_ncm.h; NaN for a clip of
    fewer than 12 frames).
    quality=True appends segsnr and fwsegsnr (QUALITY_COLUMNS; NaN where the
    cell is not finite), scored on the side stream from the same waveforms,
    with or without STOI.  distortion=True makes the rows NCOL + 4 wide and
    fills llr and cep (DISTORTION_COLUMNS) the same way; the quality columns
    are then there too, NaN unless quality=True.  separation=True makes the rows
    NCOL + 7 wide and fills sisdr, sisir and sisar (SEPARATION_COLUMNS), the
    interference being the pair's noisy - clean; the quality and distortion
    columns are NaN unless asked for.  wss=True makes the rows NCOL + 8 wide and
    fills wss (WSS_COLUMNS) the same way, the earlier optional columns NaN unless
    asked for.

    clean/noisy: lists of 1-D float arrays (host) indexed by pair.  Pairs are
    batched by length (the engine's signal batches are rectangular), and, when
    STOI is scored, in groups whose cell waveforms fit stoi_wave_bytes().  With
    job_specs' JobSpecs, cells the engine computes identically (a quarter of
    the HEAD grid: min_tracking ignores noise_percentile) are computed once
    and their rows copied, and batches of the same structure reuse one device
    plan (Engine.run(reuse=...)).

    Device memory: an engine made here is dropped with its cached plans on
    return.  A caller's engine keeps its plan_cache_size; the STOI path holds
    two plans while it runs (double-buffered waveforms: 2 x stoi_wave_bytes(),
    96 GiB peak on an idle 288-GB device, plus each plan's analysis buffers)
    and trims the cache back to
    the caller's size on return."""
    from .engine import Engine
    if not (isinstance(stoi, bool) or stoi in ("extended", "coherence", "modulation")):
        raise ValueError(f"stoi={stoi!r}: True, False or 'extended' (or 'coherence' or "
                         "'modulation')")
    own = engine is None
    eng = engine or Engine()
    size0 = eng.plan_cache_size
    try:
        return _engine_compute(eng, clean, noisy, specs, ids, align, stoi, scores.requested(
            quality=quality, distortion=distortion, separation=separation, wss=wss))
    finally:
        if own:
            eng._plan_cache.clear()
        else:
            eng.plan_cache_size = size0
            while len(eng._plan_cache) > max(size0, 1):
                eng._plan_cache.popitem(last=False)


class _I3Column:
    """metrics.CsiiPlan behind the one-column score_async the sweep calls: I3."""

    def __init__(self, clean):
        from . import metrics
        self.plan = metrics.CsiiPlan(clean)

    def score_async(self, y, y_offset, sig_of, lag=None, clip=True):
        return self.plan.score_async(y, y_offset, sig_of, lag=lag, clip=clip, which="i3")


class _NcmColumn:
    """metrics.NcmPlan behind the one-column score_async the sweep calls: ncm."""

    def __init__(self, clean):
        from . import metrics
        self.plan = metrics.NcmPlan(clean)

    def score_async(self, y, y_offset, sig_of, lag=None, clip=True):
        return self.plan.score_async(y, y_offset, sig_of, lag=lag, clip=clip, which="ncm")


def _stoi_plan(kind, clean):
    """The plan that fills the STOI column for engine_compute's stoi=kind."""
    from . import metrics
    if kind == "coherence":
        return _I3Column(clean)
    if kind == "modulation":
        return _NcmColumn(clean)
    return metrics.StoiPlan(clean, extended=(kind == "extended"))


def _stoi_switch(extended, coherence, modulation=False):
    """engine_compute's stoi= of the three switches, which exclude each other."""
    on = [name for name, flag in (("extended", extended), ("coherence", coherence),
                                  ("modulation", modulation)) if flag]
    if len(on) > 1:
        raise ValueError(f"{on[0]} and {on[1]} both fill the STOI column: choose one")
    return on[0] if on else True


def _engine_compute(eng, clean, noisy, specs, ids, align, stoi, fams=()):
    """engine_compute's work; fams: the requested families' records (scores.requested)."""
    import torch
    from . import metrics
    from .engine import snr_db, spec_fingerprint, structure_digest
    # the cell waveforms are scored on the side stream
    keep = bool(stoi) or bool(fams)
    ids = np.asarray(ids, dtype=np.int64)
    lengths = [len(x) for x in noisy]
    js_specs = isinstance(specs, JobSpecs)
    if js_specs:
        comp, back = _unique_inverse(specs.representative(ids, lengths))
        pair_of = specs.pair[comp]
    else:
        comp, back = ids, np.arange(len(ids))
        pair_of = np.fromiter((specs[c][0] for c in comp), dtype=np.int64, count=len(comp))
    vals = np.full((len(comp), _width(fams)), np.nan)
    by_len = OrderedDict()
    upairs, first = np.unique(pair_of, return_index=True)
    for pair in upairs[np.argsort(first, kind="stable")].tolist():  # first-appearance order
        by_len.setdefault(lengths[pair], []).append(pair)
    # STOI runs on the engine's side stream: the STOI of one n_fft's cells
    # overlaps the next n_fft's enhance and alignment on the main stream
    # (tools/overlap_probe.py: 20.4 -> 17.6 ms for one launch of each).
    # ready[key]: event after the last STOI that read the waveforms of the
    # plan with that reuse key (a reusing run overwrites them in place).
    main = torch.cuda.current_stream() if keep else None
    side = eng.side_stream() if keep else None
    inflight, ready = [], {}
    if keep:  # consecutive batches alternate between two plans (waveform buffers)
        eng.plan_cache_size = max(eng.plan_cache_size, 2)
    nbatch = 0

    def collect(item):
        rows_, fin_, outs_, ev_, _refs = item
        ev_.synchronize()
        fin_ = np.asarray(fin_, dtype=bool)[:, None]
        for first, out_ in outs_:
            v = out_.cpu().numpy()
            v = v[:, None] if v.ndim == 1 else v  # [n]: one column
            vals[rows_, first:first + v.shape[1]] = np.where(fin_, v, np.nan)

    sorted_pairs = len(pair_of) < 2 or bool((pair_of[1:] >= pair_of[:-1]).all())
    for L, pairs_l in by_len.items():
        if sorted_pairs:  # JobSpecs ids: each pair's cells are one run of comp
            pa = np.asarray(pairs_l, dtype=np.int64)
            lo, hi = np.searchsorted(pair_of, pa, "left"), np.searchsorted(pair_of, pa, "right")
            rows = {p: np.arange(a, b) for p, a, b in zip(pairs_l, lo.tolist(), hi.tolist())}
        else:
            rows = {p: np.flatnonzero(pair_of == p) for p in pairs_l}
        batches, cur, n_cur = [], [], 0
        cap = stoi_wave_bytes() if keep else 0
        for pair in pairs_l:
            n = len(rows[pair])
            if keep and cur and (n_cur + n) * L * 4 > cap:
                batches.append(cur)
                cur, n_cur = [], 0
            cur.append(pair)
            n_cur += n
        batches.append(cur)
        for pairs in batches:
            js = np.concatenate([rows[p] for p in pairs])
            slot_of = np.full(int(max(pairs)) + 1, -1, dtype=np.int64)
            slot_of[pairs] = np.arange(len(pairs))
            sig = slot_of[pair_of[js]]  # the batch slot of each cell's pair
            nz = torch.as_tensor(np.stack([np.asarray(noisy[p], np.float64) for p in pairs])).cuda()
            cl = torch.as_tensor(np.stack([np.asarray(clean[p], np.float64) for p in pairs])).cuda()
            cpow = np.array([float(np.dot(np.asarray(clean[p], np.float64),
                                          np.asarray(clean[p], np.float64))) for p in pairs])
            # (first column, plan) in launch order: STOI, which is no family (it
            # owns column 3), then the requested families in registry order
            plans = [(TABLE_COLUMN["stoi"], _stoi_plan(stoi, cl))] if stoi else []
            for f in fams:
                cls = getattr(metrics, f.plan)
                plans.append((f.first, cls(cl, nz) if f.plan_takes_noisy else cls(cl)))
            state = {}

            def on_plan(p, sse, fin, lag, js=js, sig=sig, L=L, plans=plans, state=state):
                """one n_fft's cells are final: queue their scores on the side stream"""
                idx = np.asarray(p.idx, dtype=np.int64)
                lg = lag if lag is not None else np.zeros(len(idx), dtype=np.int64)
                # uploads on the main stream (a pageable copy would wait for the
                # side stream's queue), then the side stream takes over
                off_d = torch.as_tensor(idx * L).cuda()
                sig_d = torch.as_tensor(sig[idx].astype(np.int32)).cuda()
                lag_d = torch.as_tensor(np.asarray(lg, dtype=np.int32)).cuda()
                y = p.y_all.view(-1)  # the run's waveform buffer (every n_fft's rows)
                side.wait_stream(main)
                with torch.cuda.stream(side):
                    outs = [(first, plan.score_async(y, off_d, sig_d, lag=lag_d, clip=True))
                            for first, plan in plans]
                    ev = torch.cuda.Event()
                    ev.record(side)
                state["ev"] = ev
                # the last entry keeps what the queued kernels read alive until collect
                inflight.append((js[idx], fin, outs, ev, (y, off_d, sig_d, lag_d, plans)))
                while len(inflight) > 2:  # bound the STOI scratch held in flight
                    collect(inflight.pop(0))

            def sub(js=js, sig=sig):
                return [(int(sg), specs[int(c)][1], specs[int(c)][2]) for sg, c in zip(sig, comp[js])]
            if js_specs:
                # batches of the same structure reuse one device plan: the key
                # is the cells' (slot, algorithm, grid cell) and this JobSpecs
                h = structure_digest()
                for arr in (sig, specs.alg[comp[js]], specs.cell[comp[js]]):
                    h.update(np.ascontiguousarray(arr, dtype=np.int64))
                key = ("jobspecs", id(specs), h.hexdigest())
                run_specs, run_kw = sub, dict(reuse=key, keep=specs)
            else:
                run_specs = sub()
                key = spec_fingerprint(run_specs)
                run_kw = dict(reuse=key)
            if keep:  # the next batch's run overlaps this batch's STOI
                key = (key, nbatch % 2)
                run_kw["reuse"] = key
            nbatch += 1
            rkey = (L, len(pairs), key)
            if keep:
                if rkey in ready:  # the plan's waveforms are still read by that STOI
                    main.wait_event(ready[rkey])
                run_kw["on_plan"] = on_plan
            res = eng.run(nz, run_specs, clean=cl, align=align, want_waveforms=keep, **run_kw)
            if keep:
                ready[rkey] = state["ev"]
            vals[js, 0] = res["sse"]
            vals[js, 1] = snr_db(res["sse"], cpow[sig])
            vals[js, 2] = res["finite"]
            if "lag" in res:
                vals[js, 4] = res["lag"]
                vals[js, 5] = res["xcorr_status"]
            else:
                vals[js, 4:6] = 0
            del res
    for item in inflight:
        collect(item)
    return vals[back]


def gather_records(local, n_total, group=None, device=None):
    """All-gather per-cell records [n_local, 1 + NCOL] (RECORD_FIELDS; 1 + NCOL + 2
    with the quality columns, + 4 with the distortion columns, + 7 with the
    separation columns, + 8 with the wss column) from every rank into one [n_total, width - 1]
    table indexed by cell_id.  The width is the records' own (every rank's
    alike).  Fixed-size rows padded to the largest shard so one
    all_gather_into_tensor moves them."""
    import torch
    import torch.distributed as dist
    dist_on = group is not None or (dist.is_available() and dist.is_initialized())
    world = dist.get_world_size(group) if dist_on else 1
    if dist_on:
        if device is None and dist.get_backend(group) == "nccl":
            # RCCL moves device tensors only: gather on this rank's GPU
            device = torch.device("cuda", torch.cuda.current_device())
    local = np.asarray(local, dtype=np.float64)
    width = local.shape[1] if local.ndim == 2 else 1 + NCOL
    if width < 1 + NCOL:
        raise ValueError(f"gather: records of {width} columns (at least {1 + NCOL})")
    rec = torch.as_tensor(local.reshape(-1, width))
    if dist_on:  # the collective runs at any world size, 1 included
        n = torch.tensor([rec.shape[0]], dtype=torch.int64, device=device)
        counts = torch.zeros(world, dtype=torch.int64, device=device)
        dist.all_gather_into_tensor(counts, n, group=group)
        m = int(counts.max())
        pad = torch.full((m, width), -1.0, dtype=torch.float64)
        pad[:rec.shape[0]] = rec
        pad = pad.to(device) if device is not None else pad
        allrec = torch.empty((world * m, width), dtype=torch.float64, device=pad.device)
        dist.all_gather_into_tensor(allrec, pad, group=group)
        rec = allrec.cpu()
    rec = rec.numpy()
    if len(rec) and rec[:, 0].min() < 0:  # padding rows of the shorter shards
        rec = rec[rec[:, 0] >= 0]
    ids = rec[:, 0].astype(np.int64)
    # every cell exactly once (a count per id: O(n), no sort)
    inrange = len(ids) == 0 or (ids.min() >= 0 and ids.max() < n_total)
    seen = np.bincount(ids, minlength=n_total) if inrange and len(ids) else np.zeros(n_total, np.int64)
    if not inrange or len(ids) != n_total or (len(ids) and seen.max() != 1):
        raise RuntimeError(f"gather: {len(ids)} records for {n_total} cells "
                           f"({len(ids) - int(np.count_nonzero(seen))} duplicates or out of range)")
    if np.array_equal(ids, np.arange(n_total)):
        return rec[:, 1:]  # already in cell order (a view: no copy of the table)
    table = np.full((n_total, width - 1), np.nan)
    table[ids] = rec[:, 1:]
    return table


def _scan_records(sc, rec, ids, tol, start=-1.0):
    """The sequential scan over the strict running maxima of one group (see
    select_best): returns (winner id or -1, score or None)."""
    incumbent, win = start, -1
    for k in rec.tolist():
        if sc[k] > incumbent + tol:
            incumbent, win = float(sc[k]), int(ids[k])
    return win, (incumbent if win >= 0 else None)


def _select_best_blocks(specs, table, col, tol, start=-1.0, sign=1.0, finite_only=False):
    """select_best over a JobSpecs table: each algorithm's cells of all pairs
    as one [pairs, grid] block (the columns of a (pair, algorithm) run are
    contiguous), running maxima along the grid axis in one call.  sign = -1:
    the scan runs on the negated column (the scores returned are negated too)."""
    n_pairs = len(specs) // max(specs.per_pair, 1)
    # the score column with skipped cells at -inf (a finite cell whose score
    # is not NaN), as [pairs, cells of one pair]
    sc_all = sign * np.asarray(table[:n_pairs * specs.per_pair, col], dtype=np.float64)
    ok = (table[:n_pairs * specs.per_pair, 2] != 0) & (sc_all == sc_all)
    if finite_only:
        ok &= np.isfinite(sc_all)
    sc_all = np.where(ok, sc_all, -np.inf).reshape(n_pairs, specs.per_pair)
    found = {}
    off = 0
    for a in specs.algorithms:
        n = len(specs.cells[a])
        if n:
            sc = sc_all[:, off:off + n]
            prev = np.empty_like(sc)
            prev[:, 0] = -np.inf
            np.maximum.accumulate(sc[:, :-1], axis=1, out=prev[:, 1:])
            recs = sc > prev
            for pair in range(n_pairs):
                ids = pair * specs.per_pair + off + np.arange(n)
                found[(pair, a)] = _scan_records(sc[pair], np.flatnonzero(recs[pair]), ids, tol,
                                                 start)
        else:
            for pair in range(n_pairs):
                found[(pair, a)] = (-1, None)
        off += n
    return OrderedDict(((pair, a), found[(pair, a)]) for pair in range(n_pairs)
                       for a in specs.algorithms)


def select_best(specs, table, objective="snr", tol=None):
    """Per (pair, algorithm): the winner of the reference's sequential scan.

    Non-finite cells are skipped like finalize_enhanced returning None
    (speech_enhancement_comparison.py:102-103,173-175); the incumbent starts
    at -1 (:126-141); a NaN score (pystoi failure -> None) is skipped like
    :182-183.  Returns {(pair, alg): (cell_id or -1, score)}.

    "segsnr" / "fwsegsnr" (a quality=True table): the same scan with their
    tolerance, started below every score (SCAN_START): the reference's -1 is a
    floor for scores that are never negative, and these are dB values clamped
    to [-10, 35], so the first scored cell is always taken.

    "llr" / "cep" (a distortion=True table) are minimised: the same scan runs
    on the negated column, started at -inf, so a cell replaces the incumbent
    when its value < incumbent - tol; the score returned is the value itself.

    "sisdr" / "sisir" / "sisar" (a separation=True table) are maximised from
    -inf like the dB objectives above; a value that is not finite is skipped the
    way a NaN is (+inf: a test signal that is the clean one scaled, or no
    interference left, which the tolerance scan could not rank).

    "wss" (a wss=True table) is minimised like "llr"."""
    best = _select_best(specs, table, objective, tol)
    if objective in OBJECTIVES and OBJECTIVES[objective].sign < 0:  # -(-v) is v, bit for bit
        best = OrderedDict((k, (win, None if sc is None else -sc)) for k, (win, sc) in best.items())
    return best


def _select_best(specs, table, objective, tol):
    tol = TOLERANCE[objective] if tol is None else tol
    sign, finite_only = 1.0, False
    if objective in OBJECTIVES:
        f = OBJECTIVES[objective]
        col, sign, finite_only = scores.columns(f)[objective], float(f.sign), f.finite_only
        if np.ndim(table) != 2 or np.shape(table)[1] <= col:
            raise ValueError(f"objective {objective!r} needs a {f.flag}=True table of "
                             f"{scores.width(f)} columns, this one has {np.shape(table)[-1]}")
    elif objective in ("snr", "stoi"):
        col = TABLE_COLUMN[objective]
    else:
        raise ValueError(f"objective {objective!r} is not scored on the device (pesq is absent)")
    scan_start = SCAN_START.get(objective, -1.0)
    if isinstance(specs, JobSpecs) and tol >= 0.0:
        return _select_best_blocks(specs, table, col, tol, scan_start, sign, finite_only)
    groups = OrderedDict()
    if isinstance(specs, JobSpecs):  # (pair, algorithm) runs are contiguous
        per = [len(specs.cells[a]) for a in specs.algorithms]
        start = 0
        for pair in range(len(specs) // max(specs.per_pair, 1)):
            for a, n in zip(specs.algorithms, per):
                groups[(pair, a)] = np.arange(start, start + n)
                start += n
    else:
        for cid, (pair, alg, _) in enumerate(specs):
            groups.setdefault((pair, alg), []).append(cid)
    best = OrderedDict()
    for key, ids in groups.items():
        ids = np.asarray(ids, dtype=np.int64)
        sc = sign * table[ids, col]
        ok = (table[ids, 2] != 0) & (sc == sc)  # finite cell, score not NaN
        if finite_only:
            ok &= np.isfinite(sc)
        sc = np.where(ok, sc, -np.inf)
        incumbent, win = scan_start, -1
        if tol >= 0.0 and len(sc):
            # Only a strict running maximum can replace the incumbent: after
            # any cell j the incumbent is >= sc[j] - tol (it took sc[j], or
            # sc[j] <= incumbent + tol), so a cell at or below an earlier score
            # never clears incumbent + tol and leaves the state alone.  The
            # scan runs over those records only (a few per group).
            prev = np.maximum.accumulate(np.concatenate(([-np.inf], sc[:-1])))
            best[key] = _scan_records(sc, np.flatnonzero(sc > prev), ids, tol, scan_start)
            continue
        else:
            start = 0  # negative tolerance: the plain jump scan
            while start < len(ids):
                hit = np.flatnonzero(sc[start:] > incumbent + tol)
                if len(hit) == 0:
                    break
                k = start + int(hit[0])
                incumbent, win, start = float(sc[k]), int(ids[k]), k + 1
        best[key] = (win, incumbent if win >= 0 else None)
    return best


def run_grid(clean, noisy, specs, compute=None, group=None, device=None, objective="snr",
             extended=False, quality=False, distortion=False, separation=False, wss=False,
             coherence=False, modulation=False):
    """Run every cell of ``specs`` across the ranks of ``group`` (or locally)
    and return (table [n_cells, NCOL] = sse, snr, finite, stoi, lag, xstatus;
    winners).  Every rank
    gets the full table (all_gather); the selection is the deterministic
    sequential scan, identical on every rank.  extended=True: the default
    compute (engine_compute) scores extended STOI into the stoi column; a
    compute function given by the caller scores what it scores.  coherence=True:
    likewise with the CSII's I3 (not together with extended).  modulation=True:
    likewise with the normalized covariance measure ncm (include/cse_ncm.h; not
    together with extended or coherence).  quality=True:
    the table has NCOL + 2 columns (QUALITY_COLUMNS: segsnr, fwsegsnr), filled
    by the default compute; a caller's compute function returns them itself.
    distortion=True: NCOL + 4 columns (the quality columns, NaN without
    quality=True, then DISTORTION_COLUMNS: llr, cep), likewise.
    separation=True: NCOL + 7 columns (the quality and distortion columns, NaN
    unless asked for, then SEPARATION_COLUMNS: sisdr, sisir, sisar), likewise.
    wss=True: NCOL + 8 columns (all of those, NaN unless asked for, then
    WSS_COLUMNS: wss), likewise."""
    import torch.distributed as dist
    stoi_kind = _stoi_switch(extended, coherence, modulation)
    dist_on = dist.is_available() and dist.is_initialized()
    world = dist.get_world_size(group) if dist_on else 1
    rank = dist.get_rank(group) if dist_on else 0
    lengths = [len(x) for x in noisy]
    rank_of, _ = assign_shards(specs, lengths, world)
    ids = np.nonzero(rank_of == rank)[0]
    flags = dict(quality=quality, distortion=distortion, separation=separation, wss=wss)
    fams = scores.requested(**flags)
    ncol = _width(fams)
    if compute is None and (stoi_kind is not True or fams):
        def compute(clean, noisy, specs, ids):
            return engine_compute(clean, noisy, specs, ids, stoi=stoi_kind, **flags)
    compute = compute or engine_compute
    vals = compute(clean, noisy, specs, ids) if len(ids) else np.zeros((0, ncol))
    if np.ndim(vals) != 2 or np.shape(vals)[1] != ncol:
        # the first family's flag is always shown, the others when set
        first = next(iter(FAMILIES))
        raise ValueError(f"compute returned rows of shape {np.shape(vals)}, expected "
                         f"{ncol} columns ({first}={bool(flags[first])}"
                         + "".join(f", {f.flag}=True" for f in fams if f.flag != first) + ")")
    if not dist_on and len(ids) == len(specs):  # one process, every cell in order: no gather
        table = np.asarray(vals, dtype=np.float64)
    else:
        local = np.concatenate([ids[:, None].astype(np.float64), vals], axis=1)
        table = gather_records(local, len(specs), group=group, device=device)
    return table, select_best(specs, table, objective)


NOISE_METHODS = ("percentile", "min_tracking", "true_noise") + tuple(TRACKERS)
# bound on the noise-PSD estimates score_noise_estimators holds at once (f32
# bytes): 4 GiB, 32 estimates of 100 10-s pairs at n_fft 512 / hop 128
NOISE_EST_BYTES = 4 << 30
LOGERR_COLUMNS = {"logerr": 0, "over": 1, "under": 2}


def score_noise_estimators(clean, noisy, estimators, n_fft=512, hop_length=128, eps=1e-10,
                           engine=None, **logerr_kw):
    """LogErr (include/cse_logerr.h) of noise-PSD estimators on pairs.

    clean, noisy: lists of numpy signals as run_grid takes them (a pair is cut
    to its shorter side); estimators: a list of (method, params), method one of
    NOISE_METHODS and params what Engine.noise_estimate takes for it.  Pairs
    are batched by equal length; per batch there is one metrics.NoiseErrPlan
    (logerr_kw: beta, floor, skip_frames, bins) and every estimate is made once
    with Engine.noise_estimate (true_noise from the power of noisy - clean),
    NOISE_EST_BYTES of estimates at a time.  Returns float64
    [pairs][estimators][3] of (logerr, over, under) in dB."""
    import torch
    from .engine import Engine
    from .metrics import NoiseErrPlan
    estimators = [(m, dict(p or {})) for m, p in estimators]
    for m, _ in estimators:
        if m not in NOISE_METHODS:
            raise ValueError(f"unknown noise method {m!r}: one of {NOISE_METHODS}")
    if len(clean) != len(noisy):
        raise ValueError("clean and noisy differ in number")
    eng = engine or Engine()
    out = np.full((len(clean), len(estimators), 3), np.nan)
    by_len = OrderedDict()
    for i, (c, z) in enumerate(zip(clean, noisy)):
        by_len.setdefault(min(len(c), len(z)), []).append(i)
    for L, idx in by_len.items():
        cd = torch.as_tensor(np.stack([np.asarray(clean[i], dtype=np.float64)[:L] for i in idx]),
                             device=eng.device)
        zd = torch.as_tensor(np.stack([np.asarray(noisy[i], dtype=np.float64)[:L] for i in idx]),
                             device=eng.device)
        plan = NoiseErrPlan(cd, zd, n_fft, hop_length, **logerr_kw)
        S = len(idx)
        _, P = eng.stft(zd, n_fft, hop_length, want_y=False)
        Pv = None
        per = max(1, NOISE_EST_BYTES // (S * plan.T * plan.B * 4))
        for k0 in range(0, len(estimators), per):
            chunk = estimators[k0:k0 + per]
            rows = []
            for m, prm in chunk:
                if m == "true_noise":
                    if Pv is None:
                        _, Pv = eng.stft(zd, n_fft, hop_length, x_sub=cd, want_y=False)
                    rows.append(eng.noise_estimate(m, Pv, eps=eps, frames=plan.T, **prm))
                else:
                    rows.append(eng.noise_estimate(m, P, eps=eps, **prm))
            sig = np.tile(np.arange(S), len(chunk))
            t = plan.score(rows, sig).reshape(len(chunk), S, 3)
            out[idx, k0:k0 + len(chunk)] = t.transpose(1, 0, 2)
            del rows
    return out


def select_tracker(means, tol):
    """The sequential best-so-far rule (select_best's semantics) on per-set
    means that are minimised: a later set replaces the incumbent only if it is
    better by more than tol; a mean that is not finite is skipped.  Returns the
    index of the winner, or -1."""
    incumbent, win = math.inf, -1
    for k, v in enumerate(np.asarray(means, dtype=np.float64).tolist()):
        if math.isfinite(v) and v < incumbent - tol:
            incumbent, win = v, k
    return win


def sweep_tracker(clean, noisy, method, ranges, objective="logerr", tol=None, n_fft=512,
                  hop_length=128, eps=1e-10, compute=None, **logerr_kw):
    """Tune one noise tracker on pairs by the LogErr of its estimate.

    ranges: a dict of lists, enumerated by parameter_ranges.grid_cells in the
    reference's order; every set is one (method, params) of
    score_noise_estimators.  objective: "logerr", "over" or "under", the mean
    over pairs, minimised; the winner is chosen by select_tracker with tol
    (default TOLERANCE["logerr"]), so ties within tol keep the earlier set and
    a set whose mean is not finite is skipped.  compute(clean, noisy,
    estimators) -> [pairs][sets][3] replaces score_noise_estimators (tests).
    Returns {"table", "means" ([sets] of the objective), "best_index" (-1 when
    no set has a finite mean), "best_params" (None then), "params" (every set)}.
    The sweep runs on one device; sharding it over ranks is not built."""
    if objective not in LOGERR_COLUMNS:
        raise ValueError(f"objective {objective!r}: one of {tuple(LOGERR_COLUMNS)}")
    if method not in NOISE_METHODS:
        raise ValueError(f"unknown noise method {method!r}: one of {NOISE_METHODS}")
    tol = TOLERANCE["logerr"] if tol is None else tol
    cells = grid_cells(ranges)
    ests = [(method, p) for p in cells]
    if compute is None:
        table = score_noise_estimators(clean, noisy, ests, n_fft=n_fft, hop_length=hop_length,
                                       eps=eps, **logerr_kw)
    else:
        table = compute(clean, noisy, ests)
    table = np.asarray(table, dtype=np.float64)
    if table.shape != (len(clean), len(cells), 3):
        raise ValueError(f"compute returned shape {table.shape}, expected "
                         f"{(len(clean), len(cells), 3)}")
    with np.errstate(invalid="ignore"):
        means = table[:, :, LOGERR_COLUMNS[objective]].mean(axis=0) if len(clean) else \
            np.full(len(cells), np.nan)
    win = select_tracker(means, tol)
    return {"table": table, "means": means, "best_index": win,
            "best_params": dict(cells[win]) if win >= 0 else None, "params": cells}


def _snr_baseline(c, n):
    m = min(len(c), len(n))
    err = np.sum((c[:m] - n[:m]) ** 2)
    return math.inf if err == 0 else float(10 * np.log10(np.sum(c[:m] ** 2) / (err + 1e-10)))


def _device_stoi(clean, test, sr, extended=False, coherence=False, modulation=False):
    from .metrics import calculate_csii, calculate_ncm, calculate_stoi
    if coherence:
        return calculate_csii(clean, test, sr)
    if modulation:
        return calculate_ncm(clean, test, sr)
    return calculate_stoi(clean, test, sr, extended=extended)


def _device_scores(names, clean, test, sr):
    """metrics.calculate_<name> of test against clean for each of ``names``, on
    the device: a tuple, None for a failure."""
    from . import metrics
    return tuple(getattr(metrics, "calculate_" + name)(clean, test, sr) for name in names)


def _opt(v):
    return None if v != v else float(v)


def _finite(v):
    """A separation score for a result row: None unless finite (JSON has no inf)."""
    return float(v) if math.isfinite(v) else None


def optimize_parameters(clean_reference, noisy_audio, sr, algorithm, param_ranges=None,
                        compute=None, stoi_fn=None, extended=False, quality=False,
                        quality_fn=None, distortion=False, distortion_fn=None, separation=False,
                        separation_fn=None, coherence=False, modulation=False):
    """Single-pair, single-algorithm mirror of the reference's
    optimize_parameters (speech_enhancement_comparison.py:109-252), scored by
    STOI and SNR: returns {'stoi': {'score', 'params', 'cell', 'snr'},
    'snr': {'score', 'params', 'cell', 'stoi'}, 'baseline': {'stoi', 'snr'},
    'improvements': {'stoi', 'snr'}, 'table'}; raises ValueError like :233-235
    when no cell produced a finite output.  The 'stoi' entry is None when no
    cell has a STOI value (a compute function that does not score STOI).
    extended=True: the cells and the baseline are scored with extended STOI
    (every 'stoi' value above is then ESTOI) and the result carries
    'extended': True.
    coherence=True: likewise with the CSII's I3 (include/cse_csii.h; every
    'stoi' value is then I3) and 'coherence': True; not together with extended.
    modulation=True: likewise with the normalized covariance measure ncm
    (include/cse_ncm.h; every 'stoi' value is then ncm) and 'modulation': True;
    not together with extended or coherence.
    quality=True: the table has the two quality columns and the result gains
    'segsnr' and 'fwsegsnr' entries shaped like 'stoi' ({'score', 'params',
    'cell', 'snr'}, None when no cell has the score), with their baselines
    (quality_fn(clean, noisy, sr) -> (segsnr, fwsegsnr); default: the device)
    and improvements.
    distortion=True: likewise 'llr' and 'cep' entries from the two distortion
    columns (distortion_fn(clean, noisy, sr) -> (llr, cep) for the baselines);
    both are minimised, so their improvement is baseline - score.
    separation=True: likewise 'sisdr', 'sisir' and 'sisar' entries from the
    three separation columns, each carrying the other two scores of its cell.
    Only 'sisdr' has a baseline and an improvement (separation_fn(clean, noisy,
    sr) -> the noisy input's SI-SDR; default: the device): the noisy input has
    no artifacts to compare with."""
    from .engine import canonical_algo
    if sr != 16000:
        raise ValueError("the device path runs at 16 kHz (prepare_pair resamples to 16 kHz)")
    alg = canonical_algo(algorithm)
    grids = {alg: param_ranges or ALGORITHM_GRIDS[alg]}
    specs = job_specs(1, [alg], grids)
    clean = [np.asarray(clean_reference, np.float64)]
    noisy = [np.asarray(noisy_audio, np.float64)]
    flags = dict(quality=quality, distortion=distortion, separation=separation)
    table, best = run_grid(clean, noisy, specs, compute=compute, extended=extended,
                           coherence=coherence, modulation=modulation, **flags)
    cid, score = best[(0, alg)]
    if cid < 0:
        raise ValueError("Optimization failed for snr - no valid parameters found!")
    base = _snr_baseline(clean[0], noisy[0])
    out = {"snr": {"score": score, "params": dict(specs[cid][2]), "cell": int(cid),
                   "stoi": _opt(table[cid, 3])},
           "baseline": {"snr": base}, "improvements": {"snr": score - base}, "table": table,
           "stoi": None}
    if extended:
        out["extended"] = True
    if coherence:
        out["coherence"] = True
    if modulation:
        out["modulation"] = True
    sid, sscore = select_best(specs, table, "stoi")[(0, alg)]
    if sid >= 0:
        if stoi_fn is None and (extended or coherence or modulation):
            bstoi = _device_stoi(clean[0], noisy[0], sr, extended=extended,
                                 coherence=coherence, modulation=modulation) or 0
        else:
            bstoi = (stoi_fn or _device_stoi)(clean[0], noisy[0], sr) or 0  # :115 "or 0"
        out["stoi"] = {"score": sscore, "params": dict(specs[sid][2]), "cell": int(sid),
                       "snr": float(table[sid, 1])}
        out["baseline"]["stoi"] = bstoi
        out["improvements"]["stoi"] = sscore - bstoi
    for f, base_fn in ((FAMILIES["quality"], quality_fn), (FAMILIES["distortion"], distortion_fn)):
        if not flags[f.flag]:
            continue
        base = None
        for k, name in enumerate(f.names):
            out[name] = None
            qid, qscore = select_best(specs, table, name)[(0, alg)]
            if qid < 0:
                continue
            if base is None:
                base = base_fn(clean[0], noisy[0], sr) if base_fn else \
                    _device_scores(f.names, clean[0], noisy[0], sr)
            out[name] = {"score": qscore, "params": dict(specs[qid][2]), "cell": int(qid),
                         "snr": float(table[qid, 1])}
            b = out["baseline"][name] = base[k] or 0
            out["improvements"][name] = qscore - b if f.sign > 0 else b - qscore
    # separation stays written out: each of its entries carries the other two
    # scores of its cell, and its baseline function returns one score, not one
    # per name, which no record field says
    if separation:
        for name in SEPARATION_COLUMNS:
            out[name] = None
            pid, pscore = select_best(specs, table, name)[(0, alg)]
            if pid < 0:
                continue
            out[name] = {"score": pscore, "params": dict(specs[pid][2]), "cell": int(pid),
                         "snr": float(table[pid, 1])}
            out[name].update({k: _finite(table[pid, c]) for k, c in SEPARATION_COLUMNS.items()
                              if k != name})
            if name == "sisdr":
                base_p = separation_fn(clean[0], noisy[0], sr) if separation_fn else \
                    _device_scores((name,), clean[0], noisy[0], sr)[0]
                out["baseline"][name] = base_p or 0
                out["improvements"][name] = pscore - out["baseline"][name]
    return out


def run_sweep(clean, noisy, stems, out_root, sr=16000, algorithms=None, grids=None,
              group=None, device=None, extended=False, quality=False, distortion=False,
              separation=False, wss=False, coherence=False, modulation=False):
    """The reference's batch driver (main, speech_enhancement_comparison.py:375-473)
    on the device: every pair x algorithm x grid cell scored after
    finalize_enhanced (STOI and SNR), the STOI-best and SNR-best cells per
    (pair, algorithm) selected by the sequential tolerance scan, their
    waveforms written as results_{alg}/{stem}_{alg}_optimized_stoi.wav (the
    reference's name, :303) and ..._optimized_snr.wav, and the summary files
    (results.write_summary) under results_summary/.  Rank 0 writes.
    extended=True: scored and selected by extended STOI; the rows' stoi_* fields
    then hold ESTOI, each row carries "stoi_extended": True, and the file names
    stay the same.
    coherence=True: scored and selected by the CSII's I3 (include/cse_csii.h) in
    the same way; the rows' stoi_* fields then hold I3, each row carries
    "stoi_coherence": True, the noisy baseline is metrics.CsiiPlan's, and the
    file names stay the same.  A pair without mid-level or low-level frames has
    no I3: its stoi fields are None.  Not together with extended.
    modulation=True: scored and selected by the normalized covariance measure ncm
    (include/cse_ncm.h) in the same way; the rows' stoi_* fields then hold ncm,
    each row carries "stoi_modulation": True, the noisy baseline is
    metrics.NcmPlan's, and the file names stay the same.  Not together with
    extended or coherence.
    quality=True: the cells are also scored by segSNR and fwSegSNR; the
    fwSegSNR-best cell's waveform is written as ..._optimized_fwsegsnr.wav and
    each row gains segsnr_noisy, fwsegsnr_noisy, fwsegsnr_best,
    best_params_fwsegsnr and snr_fwsegopt (means in summary_means.json).  The
    segSNR winner is select_best(specs, table, "segsnr")'s.
    distortion=True: the cells are also scored by the LLR and the cepstrum
    distance; the LLR-best (lowest) cell's waveform is written as
    ..._optimized_llr.wav and each row gains llr_noisy, cep_noisy, llr_best,
    best_params_llr and snr_llropt (means in summary_means.json).  The CEP
    winner is select_best(specs, table, "cep")'s.
    separation=True: the cells are also scored by SI-SDR, SI-SIR and SI-SAR
    against the pair's own noisy - clean; the SI-SDR-best cell's waveform is
    written as ..._optimized_sisdr.wav and each row gains sisdr_noisy,
    sisdr_best, that cell's sisir_sisdropt and sisar_sisdropt (how its error
    splits), best_params_sisdr and snr_sisdropt (means in summary_means.json).
    The SI-SIR and SI-SAR winners are select_best's.
    wss=True: the cells are also scored by the weighted spectral slope distance;
    the WSS-best (lowest) cell's waveform is written as ..._optimized_wss.wav and
    each row gains wss_noisy, wss_best, best_params_wss and snr_wssopt (means in
    summary_means.json)."""
    import torch
    import torch.distributed as dist
    from . import metrics, results
    from .engine import Engine
    grids = grids or ALGORITHM_GRIDS
    algorithms = list(algorithms or grids)
    specs = job_specs(len(noisy), algorithms, grids)
    flags = dict(quality=quality, distortion=distortion, separation=separation, wss=wss)
    fams = scores.requested(**flags)
    table, best = run_grid(clean, noisy, specs, group=group, device=device, extended=extended,
                           coherence=coherence, modulation=modulation, **flags)
    rank = dist.get_rank(group) if (dist.is_available() and dist.is_initialized()) else 0
    if rank != 0:
        return None
    best_stoi = select_best(specs, table, "stoi")
    best_lead = {f.flag: select_best(specs, table, f.lead) for f in fams}
    eng = Engine()
    rows = []
    for pair, stem in enumerate(stems):
        c = np.asarray(clean[pair], np.float64)
        n = np.asarray(noisy[pair], np.float64)
        snr_noisy = _snr_baseline(c, n)
        m = min(len(c), len(n))
        cm = torch.as_tensor(c[:m]).cuda().view(1, -1)
        plan = _stoi_plan(_stoi_switch(extended, coherence, modulation), cm)
        nf = torch.as_tensor(n[:m].astype(np.float32)).cuda()
        stoi_noisy = _opt(float(plan.score_async(nf, [0], [0], clip=False).cpu()[0]))
        noisy_kw = {}  # per family, the unprocessed input's <name>_noisy of its baselines
        for f in fams:
            fplan = getattr(metrics, f.plan)(torch.as_tensor(c[:m]).cuda().view(1, -1))
            v = np.atleast_1d(fplan.score(nf, [0], [0], clip=False)[0])
            noisy_kw[f.flag] = {f"{name}_noisy": (_finite if f.finite_only else _opt)(
                v[f.names.index(name)]) for name in f.baselines}
        x = torch.as_tensor(n).cuda().view(1, -1)
        cl = torch.as_tensor(c).cuda().view(1, -1)
        for alg in algorithms:
            cid, score = best[(pair, alg)]
            if cid < 0:
                raise ValueError(f"Optimization failed for snr - no valid parameters found! ({stem}, {alg})")
            sid, sscore = best_stoi[(pair, alg)]
            out_dir = os.path.join(out_root, f"results_{alg}")
            os.makedirs(out_dir, exist_ok=True)
            written, family_kw = [("snr", cid), ("stoi", sid)], {}
            for f in fams:
                k, kscore = best_lead[f.flag][(pair, alg)]
                written.append((f.lead, k))
                conv = _finite if f.finite_only else _opt
                family_kw.update(noisy_kw[f.flag])
                family_kw.update({
                    f"{f.lead}_best": None if k < 0 else float(kscore),
                    f"{f.lead}_params": None if k < 0 else specs[k][2],
                    f"snr_{f.tag}opt": None if k < 0 else float(table[k, 1])})
                # the winner's other scores, for the families whose rows have them
                family_kw.update({
                    f"{name}_{f.tag}opt": None if k < 0 else conv(table[k, col])
                    for name, col in scores.columns(f).items()
                    if f"{name}_{f.tag}opt" in f.row_args})
            for tag, k in written:
                if k < 0:
                    continue
                res = eng.run(x, [(0, alg, specs[k][2])], clean=cl, want_waveforms=True, align=True)
                y = res["y"][0].cpu().numpy().astype(np.float64)
                e = results.shift_and_fit(y, int(res["lag"][0]), len(c))
                results.write_wav_pcm16(os.path.join(out_dir, f"{stem}_{alg}_optimized_{tag}.wav"),
                                        e, sr)
            rows.append(results.result_row(
                stem, alg, sr, snr_noisy, float(score), specs[cid][2], stoi_noisy=stoi_noisy,
                stoi_best=None if sid < 0 else float(sscore),
                stoi_params=None if sid < 0 else specs[sid][2],
                snr_stoiopt=None if sid < 0 else float(table[sid, 1]), **family_kw))
            if extended:
                rows[-1]["stoi_extended"] = True
            if coherence:
                rows[-1]["stoi_coherence"] = True
            if modulation:
                rows[-1]["stoi_modulation"] = True
    results.write_summary(rows, algorithms, os.path.join(out_root, "results_summary"))
    return rows
