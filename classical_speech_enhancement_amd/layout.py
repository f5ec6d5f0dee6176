"""Host-side planning: a spec list becomes the tables the kernels dereference.

Everything here is plain data (numpy arrays, ints, dicts, tuples) and runs
without a device: PlanLayout derives, for one n_fft's cells, the buffer sizes,
the cse_cell_t / cse_noise_job_t tables with their element offsets, and the
ordered list of noise-estimation calls.  engine.GridPlan allocates what the
layout states, uploads the tables and launches.
"""

import math
import os
from collections import namedtuple

import numpy as np

from . import _lib, trackers

# algorithm name (registry names of speech_enhancement_comparison.py:395-401)
# -> (code, eps the reference passes to noise_estimation, param order in cse_cell_t)
ALGOS = {
    "spectralSubtractor": ("SS", 1e-10, ("alpha", "beta")),
    "wiener": ("WIENER", 1e-10, ("alpha", "gain_floor")),
    "mmse": ("MMSE", 1e-12, ("alpha", "ksi_min", "gain_min", "gain_max")),
    "omlsa": ("OMLSA", 1e-10, ("alpha", "ksi_min", "gain_floor", "q", "v_max")),
}
ALIASES = {"ss": "spectralSubtractor", "spectral_subtraction": "spectralSubtractor",
           "wiener_filter": "wiener", "advanced_mmse": "omlsa"}
DEFAULTS = {"mmse": {"noise_mu": 0.98, "gain_max": 1.0}, "omlsa": {"v_max": 80.0}}
# finalize_enhanced alignment (speech_enhancement_comparison.py:38-69) at 16 kHz:
# correlate the first corr_seconds = 2 s, lags within max_shift_s = 0.1 s,
# no alignment below 256 samples
ALIGN_CORR_SAMPLES = 32000
ALIGN_MAX_LAG = 1600
ALIGN_MIN_SAMPLES = 256
# relative per-bin cost used to order waves (longest first)
ALGO_COST = {"SS": 1.0, "WIENER": 1.1, "MMSE": 2.0, "OMLSA": 3.0}


def canonical_algo(name):
    name = ALIASES.get(name, name)
    if name not in ALGOS:
        raise ValueError(f"unknown algorithm {name!r}")
    return name


# hops of the sweep kernels (cse_enhance_cells) and the short hops of
# cse_enhance_cells_short_hop, per n_fft; every other even n_fft in
# [64, 4096] and hop in [1, n_fft] goes to cse_enhance_cells_generic
HOPS = (128, 256)
SHORT_HOPS = {512: (32, 64), 1024: (64,)}
MAIN, SHORT, GENERIC = 0, 1, 2


def route(n_fft, hop):
    """Which enhance kernel runs (n_fft, hop): MAIN, SHORT, GENERIC, or None
    (not supported)."""
    n_fft, hop = int(n_fft), int(hop)
    if n_fft in (512, 1024) and hop in HOPS:
        return MAIN
    if hop in SHORT_HOPS.get(n_fft, ()):
        return SHORT
    if 64 <= n_fft <= 4096 and n_fft % 2 == 0 and 1 <= hop <= n_fft:
        return GENERIC
    return None


def route_refusal(n_fft, hop):
    """Why route(n_fft, hop) is None, one reason per message: an odd n_fft (the
    reference's istft rejects it too), an n_fft outside [64, 4096], or a hop
    outside [1, n_fft]."""
    n_fft, hop = int(n_fft), int(hop)
    if n_fft % 2:
        return f"engine supports an even n_fft only (got n_fft={n_fft})"
    if not 64 <= n_fft <= 4096:
        return f"engine supports n_fft in [64, 4096] (got n_fft={n_fft})"
    return f"engine supports hop in [1, n_fft] (got n_fft={n_fft}, hop={hop})"


def n_frames(length, hop):
    return 1 + int(length) // int(hop)


# the trackers that go beyond the reference live in trackers.py; the names
# callers and tests have imported from here stay importable
TRACKERS = ALL_TRACKERS = trackers.TRACKERS
tracker_values = trackers.tracker_values
MCRA_DEFAULTS, SPP_DEFAULTS, MINSTAT_DEFAULTS, IMCRA_DEFAULTS = (
    t.defaults for t in TRACKERS.values())
mcra_values, spp_values, minstat_values, imcra_values = (t.values for t in TRACKERS.values())
mcra_params, spp_params, minstat_params, imcra_params = (
    (lambda values, t=t: trackers.params(t, values)) for t in TRACKERS.values())
minstat_time_constants = TRACKERS["minstat"].time_constants
imcra_time_constants = TRACKERS["imcra"].time_constants


def noise_key(alg, params, T):
    """Which noise PSD array a cell reads, mirroring each algorithm's pipeline.

    Returns (method, pct, eps, expand, mu, inverse); pct is the estimator's
    parameter slot: the percentile, or for a tracker (trackers.TRACKERS) its
    values tuple (noise_percentile does not enter: cells that differ only in
    it share one estimate):
      - every algorithm estimates with the eps it passes (ss/wiener/omlsa 1e-10,
        mmse 1e-12: spectral_subtractor.py:17, wiener_filter.py:23, mmse.py:17,
        advanced_mmse.py:26);
      - T < 5 -> the static 'simple' estimate for ANY method
        (noise_estimation.py:194-195, before the method is even looked at);
      - expand: SS and OMLSA pass a static (B,1) estimate through
        librosa.util.fix_length(..., size=T, axis=1) (spectral_subtractor.py:40-41,
        advanced_mmse.py:54-55), which ZERO-PADS frames 1..T-1 — frame 0 sees
        the estimate, later frames see 0 (SS) or, after OMLSA's smoothing,
        mu**t times it;
      - the trackers (no counterpart in the reference) are time-varying and
        take min_tracking's place in each pipeline: smoothed by mmse/omlsa,
        inverted with the algorithm's eps for Wiener/MMSE/OMLSA, as they are for SS;
      - mmse/omlsa smooth any time-varying estimate except true_noise
        (mmse.py:48-54, advanced_mmse.py:60-66); mu=None means no smoothing;
      - inverse: Wiener/MMSE/OMLSA read 1/max(N, eps) (their in-loop floor,
        wiener_filter.py:58, mmse.py:71, advanced_mmse.py:87), SS reads N.
    A key is static (one [B] row for all frames) iff expand is False and the
    method is percentile/simple.
    """
    code, eps, _ = ALGOS[alg]
    method = params["noise_method"]
    tracker = tracker_values(params)  # validated at any T
    if T < 5:
        method, pct = "simple", None
    elif tracker:  # time-varying, like min_tracking
        pct = tracker
    elif method == "percentile":
        pct = float(params["noise_percentile"])
    elif method in ("min_tracking", "true_noise"):
        pct = None
    else:
        raise ValueError(f"Unbekannte Methode: {method}")
    static = method in ("percentile", "simple")
    expand = static and T > 1 and code in ("SS", "OMLSA")
    mu = None
    if method != "true_noise" and (expand or not static):
        if code == "MMSE":
            mu = float(params.get("noise_mu", 0.98))
        elif code == "OMLSA":
            mu = float(params["noise_mu"])
    return (method, pct, eps, expand, mu, code != "SS")


def key_is_static(key):
    method, _, _, expand, mu, _ = key
    return method in ("percentile", "simple") and not expand and mu is None


def noise_params(percentile=20.0, min_frames=10, max_fraction=0.30, floor_rel=0.02,
                 adaptive_short=True, window_size=50, smoothing_factor=None, src_frames=0):
    """cse_noise_params_t from the reference's estimator constructor arguments
    (PercentileNoiseEstimator noise_estimation.py:12-13, MinTrackingNoiseEstimator
    :60; defaults as there).  smoothing_factor None -> NaN."""
    prm = _lib.NoiseParams()
    prm.percentile = float(percentile)
    prm.max_fraction = float(max_fraction)
    prm.floor_rel = float(floor_rel)
    prm.smoothing_factor = math.nan if smoothing_factor is None else float(smoothing_factor)
    prm.min_frames = int(min_frames)
    prm.adaptive_short = 1 if adaptive_short else 0
    prm.window_size = int(window_size)
    prm.src_frames = int(src_frames)
    return prm


def specs_by_n_fft(S, L, specs, with_clean, want_g):
    """Validate a spec list and split it by n_fft (ascending): [(n_fft, items)]
    with items = (spec index, signal, canonical algorithm, params), spec order
    preserved."""
    by_fft = {}
    checked = set()
    for idx, (sig, alg, p) in enumerate(specs):
        alg = canonical_algo(alg)  # defaults (DEFAULTS) are applied where a value is read
        hop, nf = p["hop_length"], p["n_fft"]
        if not 0 <= int(sig) < S:
            raise ValueError(f"signal index {sig} out of range")
        ck = (alg, hop, nf, p["noise_method"])
        ck += tracker_values(p)  # and per distinct parameter set of a tracker
        if ck not in checked:  # per distinct (algorithm, hop, n_fft, method)
            r = route(nf, hop)
            if r is None:
                raise ValueError(route_refusal(nf, hop))
            if want_g and r == SHORT:
                raise ValueError(f"gain matrices not at the short hops (n_fft={nf}, hop={hop})")
            noise_key(alg, p, n_frames(L, hop))  # validates the method
            if (p["noise_method"] == "true_noise" and not with_clean
                    and n_frames(L, hop) >= 5):
                raise ValueError("TrueNoiseEstimator requires clean_audio and noisy_audio")
            checked.add(ck)
        by_fft.setdefault(int(nf), []).append((idx, int(sig), alg, p))
    return sorted(by_fft.items())


# A pointer argument of a scheduled library call: element ``off`` of the plan
# buffer named ``buf`` (GridPlan attribute; P and Ptrue: that hop's buffer).
Ref = namedtuple("Ref", "buf off", defaults=(0,))


class PlanLayout:
    """Where everything of one n_fft's cells lives, and what runs on it.

    STFT:   hops, y_base[hop] / y_elems (complex elements of Ybuf), p_shape[hop],
            ptrue_shape[hop] (hops with a true-noise estimate only)
    noise:  keys, pool_off / pool_elems, raw_off / raw_elems, jobs
            (NOISE_JOB_DTYPE), hop_jobs, noise_calls
    cells:  cells (items order), packed / order / split (pack_waves), idx,
            g_offsets / g_elems, units
    align:  align, xc_n, xc_lag_max, head_off, head_elems (0: the heads are the
            whole waveforms), sig
    """

    def __init__(self, n_fft, S, L, items, with_clean, want_y, want_g, align=False,
                 true_len=None, cells_per_group=None):
        self.n_fft, self.S, self.L, self.items = n_fft, S, L, items
        self.true_len = L if true_len is None else int(true_len)
        if not 1 <= self.true_len <= L:
            raise ValueError(f"true_len={self.true_len} not in [1, {L}]")
        B = self.B = n_fft // 2 + 1
        self.hops = sorted({p["hop_length"] for (_, _, _, p) in items})
        self.y_base, off = {}, 0
        for hop in self.hops:
            self.y_base[hop] = off
            off += S * n_frames(L, hop) * B
        self.y_elems = off
        self.p_shape = {h: (S, n_frames(L, h), B) for h in self.hops}
        item_key = self._noise(with_clean)
        # CSE_NO_QUAD (any value: no cse_noise_percentile_quad) is read here,
        # once per layout, not in the step
        no_quad = bool(os.environ.get("CSE_NO_QUAD"))
        self.noise_calls = {hop: self._noise_calls(hop, no_quad) for hop in self.hops}
        # ---- cell table (columns gathered once, written as arrays)
        n = len(items)
        cells = np.zeros(n, dtype=_lib.CELL_DTYPE)
        self.idx = np.fromiter((it[0] for it in items), dtype=np.int64, count=n)
        sig = self.sig = np.fromiter((it[1] for it in items), dtype=np.int64, count=n)
        hop = np.fromiter((it[3]["hop_length"] for it in items), dtype=np.int64, count=n)
        algo = np.fromiter((_lib.ALGO[ALGOS[it[2]][0]] for it in items), dtype=np.int32, count=n)
        kinfo = np.array([self.pool_off[k] for k in item_key], dtype=np.int64).reshape(n, 3)
        T = 1 + L // hop
        ybase = np.zeros(n, dtype=np.int64)
        for h in self.hops:
            ybase[hop == h] = self.y_base[h]
        # finalize_enhanced alignment (speech_enhancement_comparison.py:38-69)
        # correlates each cell's head of xc_n samples: that of its whole
        # waveform where those are wanted, else written in the waveform's place
        self.xc_n = min(L, ALIGN_CORR_SAMPLES)
        self.xc_lag_max = min(ALIGN_MAX_LAG, self.xc_n - 1)
        self.align = bool(align) and with_clean and self.xc_n >= ALIGN_MIN_SAMPLES
        self.head_elems = n * self.xc_n if self.align and not want_y else 0
        if want_y:
            out_off = self.idx * L
        else:
            out_off = np.arange(n, dtype=np.int64) * self.xc_n if self.align else -1
        self.head_off = out_off if self.align else None
        cells["algo"] = algo
        cells["hop"] = hop
        cells["y_offset"] = ybase + sig * T * B
        cells["noise_offset"] = kinfo[:, 0] + sig * kinfo[:, 2]
        cells["noise_stride"] = kinfo[:, 1]
        cells["clean_offset"] = sig * L if with_clean else -1
        cells["out_offset"] = out_off
        goff = (np.concatenate([[0], np.cumsum(T * B)[:-1]]) if want_g
                else np.zeros(n, dtype=np.int64))
        cells["gain_offset"] = goff if want_g else -1
        self.g_offsets = list(zip(goff.tolist(), T.tolist()))
        self.g_elems = int((T * B).sum()) if want_g else 0
        prm = np.zeros((n, 8), dtype=np.float32)
        for c, (_, _, alg, p) in enumerate(items):
            names = ALGOS[alg][2]
            dflt = DEFAULTS.get(alg, {})
            prm[c, :len(names)] = [p[k] if k in p else dflt[k] for k in names]
        cells["param"] = prm
        self.cells = cells
        self.packed, self.order = pack_waves(cells, n_fft, per=cells_per_group)
        self.split = route_slots(self.packed, n_fft)
        # frame-gain evaluations (SURVEY §8(d) unit): sum over cells of frames
        self.units = int(T.sum())

    def _noise(self, with_clean):
        """Noise keys -> pool slices; returns every item's key.  Each key = a
        base estimate (method, pct, eps) in ``raw``, post-processed into
        ``pool`` by one cse_noise_finish job (smoothing, fix_length
        zero-padding, 1/max(.,eps)); base estimates are shared."""
        S, L, B = self.S, self.L, self.B
        # noise key of every item, computed once per distinct
        # (algorithm, hop, method, percentile, noise_mu)
        keys, key_cache = {}, {}
        item_key = []
        for (_, _, alg, p) in self.items:
            hop = p["hop_length"]
            ck = (alg, hop, p["noise_method"], p.get("noise_percentile"), p.get("noise_mu"))
            ck += tracker_values(p)
            k = key_cache.get(ck)
            if k is None:
                k = key_cache[ck] = (hop, noise_key(alg, p, n_frames(L, hop)))
                keys.setdefault(k, None)
            item_key.append(k)
        # jobs grouped by hop: each hop's rows are finished by one
        # cse_noise_finish launch right after that hop's own estimates (all on
        # one stream, so in order; grouping by hop makes each launch's job list
        # one contiguous slice)
        self.keys = sorted(keys, key=lambda k: k[0])
        self.pool_off, noff = {}, 0
        self.raw_off, roff = {}, 0
        self.ptrue_shape = {}
        self.jobs = np.zeros(len(self.keys), dtype=_lib.NOISE_JOB_DTYPE)
        self.hop_jobs = {}  # hop -> (first job, count)
        for j, (hop, key) in enumerate(self.keys):
            T = n_frames(L, hop)
            method, pct, eps, expand, mu, inverse = key
            static = key_is_static(key)
            per_sig = B if static else T * B
            self.pool_off[(hop, key)] = (noff, 0 if static else B, per_sig)
            base = (hop, method, pct, eps)
            if base not in self.raw_off:
                src_static = method in ("percentile", "simple")
                self.raw_off[base] = (roff, 1 if src_static else T)
                roff += S * (B if src_static else T * B)
            r0, src_frames = self.raw_off[base]
            self.jobs[j] = (r0, noff, src_frames, 1 if static else T, float(mu or 0.0),
                            float(eps) if inverse else 0.0)
            first, cnt = self.hop_jobs.get(hop, (j, 0))
            self.hop_jobs[hop] = (first, cnt + 1)
            noff += S * per_sig
            if method == "true_noise" and hop not in self.ptrue_shape:
                if not with_clean:
                    raise ValueError("TrueNoiseEstimator requires clean_audio and noisy_audio")
                self.ptrue_shape[hop] = (S, n_frames(self.true_len, hop), B)
        self.pool_elems, self.raw_elems = noff, max(roff, 1)
        return item_key

    def _noise_calls(self, hop, no_quad):
        """The library calls that fill this hop's rows of ``raw`` and finish
        them into ``pool``, in launch order: [(entry point, arguments before
        the stream)], pointers as Ref."""
        S, B, T = self.S, self.B, n_frames(self.L, hop)
        bases = [b for b in self.raw_off if b[0] == hop]
        P, med, ws = Ref("P"), Ref("med"), Ref("ws")

        def raw(b):
            return None if b is None else Ref("raw", self.raw_off[b][0])

        def pairs(seq):
            return [(seq[k], seq[k + 1] if k + 1 < len(seq) else None)
                    for k in range(0, len(seq), 2)]
        calls = []
        if T >= 5 and any(m in ("percentile", "min_tracking") for (_, m, _, _) in bases):
            calls.append(("cse_noise_median", (P, S, T, B, med)))
        # two eps per IIR + min-filter pass
        for a_, b_ in pairs([b for b in bases if b[1] == "min_tracking"]):
            calls.append(("cse_noise_min_tracking_med",
                          (P, med, S, T, B, float(a_[3]), raw(a_),
                           float(b_[3]) if b_ else 0.0, raw(b_), ws)))
        # percentile estimates in pairs sharing eps: one frame-energy pass per pair
        pc = {}
        for b in bases:
            if b[1] == "percentile":
                pc.setdefault(float(b[3]), []).append(b)
        quad = sorted(pc) if len(pc) == 2 and not no_quad else None
        if quad and all(len(pc[e]) == 2 for e in quad) and \
                sorted(b[2] for b in pc[quad[0]]) == sorted(b[2] for b in pc[quad[1]]):
            # the HEAD grid's case: two percentiles x two eps, four launches
            # (cse_noise_percentile_quad) instead of ten
            pa, pb = sorted(float(b[2]) for b in pc[quad[0]])
            by = {(float(b[2]), float(b[3])): b for e in quad for b in pc[e]}
            calls.append(("cse_noise_percentile_quad",
                          (P, med, S, T, B, pa, pb, quad[0], quad[1],
                           raw(by[(pa, quad[0])]), raw(by[(pa, quad[1])]),
                           raw(by[(pb, quad[0])]), raw(by[(pb, quad[1])]), ws)))
            pc = {}
        for eps, group in pc.items():
            for a_, b_ in pairs(group):
                calls.append(("cse_noise_percentile_med2",
                              (P, med, S, T, B, float(a_[2]), float(b_[2]) if b_ else 0.0, eps,
                               raw(a_), raw(b_), ws)))
        for b in bases:
            _, method, pct, eps = b
            if method == "simple":
                calls.append(("cse_noise_estimate",
                              (0, P, S, T, B, 25.0, float(eps), raw(b), ws)))
            elif method in TRACKERS:  # one call per (parameter set, eps)
                calls.append((TRACKERS[method].entry,
                              (P, S, T, B, trackers.params(TRACKERS[method], pct), float(eps),
                               raw(b))))
            elif method == "true_noise":
                prm = noise_params(src_frames=self.ptrue_shape[hop][1])
                calls.append(("cse_noise_estimate_ex",
                              (2, Ref("Ptrue"), S, T, B, prm, float(eps), raw(b), None)))
        j0, nj = self.hop_jobs[hop]
        calls.append(("cse_noise_finish", (Ref("jobs_d", j0 * _lib.NOISE_JOB_DTYPE.itemsize), nj,
                                           S, B, Ref("raw"), Ref("pool"))))
        return calls


def pack_waves(cells, n_fft, per=None):
    """Group cells into workgroup slot groups (CSE_CELLS_PER_GROUP cells each;
    ``per`` if given, else asked of the library).

    A slot group's cells must share (algo, hop, spectrum, noise, clean, lag) — the
    kernel stages those rows once per workgroup.  Returns (packed cells incl.
    CSE_ALGO_NONE padding, order) with order[i] = index into ``cells`` of packed
    slot i, or -1 for padding.  Groups are ordered longest-first (frames x
    algorithm cost, then by key) so the launch ends on short workgroups;
    neighbours share rows, and the kernel's XCD remap keeps neighbours on one
    XCD's L2.  Groups at the short hops (SHORT_HOPS) come after the sweep
    hops' and the groups of every other shape after those: each class goes to
    a launch of its own (GridPlan.launch, route_slots).  n_fft other than
    512 / 1024 is all generic: one cell per slot (the generic kernel runs one
    workgroup per cell), in the given order.
    Vectorised (numpy): a 100k-cell table packs in milliseconds.
    """
    n = len(cells)
    if n == 0:
        return np.zeros(0, dtype=_lib.CELL_DTYPE), np.zeros(0, dtype=np.int64)
    if int(n_fft) not in (512, 1024):
        return cells.copy(), np.arange(n, dtype=np.int64)
    if per is None:
        per = _lib.cells_per_group(n_fft)
    keys = np.stack([cells[f].astype(np.int64) for f in
                     ("hop", "algo", "y_offset", "noise_offset", "noise_stride",
                      "clean_offset", "lag")], axis=1)
    uniq, inv = np.unique(keys, axis=0, return_inverse=True)  # rows in key order
    inv = inv.reshape(-1)
    G = len(uniq)
    counts = np.bincount(inv, minlength=G)
    nslots = (counts + per - 1) // per
    cost_of = np.zeros(8, dtype=np.float64)
    for name, code in _lib.ALGO.items():
        if code >= 0:
            cost_of[code] = ALGO_COST[name]
    cost = (1 + 16000 // uniq[:, 0]) * cost_of[uniq[:, 1]]
    cls = np.array([_cls(n_fft, h) for h in uniq[:, 0]], dtype=np.int64)
    gorder = np.lexsort((np.arange(G), -cost, cls))     # longest first, then key order
    slot_base = np.zeros(G, dtype=np.int64)
    slot_base[gorder] = np.concatenate([[0], np.cumsum(nslots[gorder])[:-1]])
    # rank of each cell inside its group, in the cells' original order
    by_group = np.argsort(inv, kind="stable")
    first = np.concatenate([[0], np.cumsum(counts)[:-1]])
    rank = np.empty(n, dtype=np.int64)
    rank[by_group] = np.arange(n) - first[inv[by_group]]
    slot = slot_base[inv] + rank // per
    total = int(nslots.sum())
    order = np.full(total * per, -1, dtype=np.int64)
    order[slot * per + rank % per] = np.arange(n)
    packed = np.zeros(len(order), dtype=_lib.CELL_DTYPE)
    real = order >= 0
    packed[real] = cells[order[real]]
    # padding: the group's shared rows, no algorithm, no outputs
    pad = np.nonzero(~real)[0]
    if len(pad):
        lead = order[(pad // per) * per]
        packed[pad] = cells[lead]
        packed["algo"][pad] = -1
        packed["out_offset"][pad] = -1
        packed["gain_offset"][pad] = -1
    return packed, order


def _cls(n_fft, hop):
    """route() for packing: shapes no kernel supports count as generic (that
    kernel's entry point refuses them)."""
    r = route(n_fft, hop)
    return GENERIC if r is None else r


def route_slots(packed, n_fft):
    """(sweep-hop, short-hop, generic) slot counts of a packed table, which
    pack_waves orders that way."""
    per = [0, 0, 0]
    hops, counts = np.unique(packed["hop"], return_counts=True)
    for h, k in zip(hops.tolist(), counts.tolist()):
        per[_cls(n_fft, h)] += int(k)
    return per[MAIN], per[SHORT], per[GENERIC]
