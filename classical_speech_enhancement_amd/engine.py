"""Device orchestration of the STFT frame-gain path on MI355X.

PyTorch-ROCm is used only as the device-memory container and stream provider;
every numeric step is a libcse.so kernel (include/cse.h):

  cse_stft            STFT of every signal at each (n_fft, hop)        [once per group]
  cse_noise_estimate  percentile / min-tracking / true-noise PSDs     [once per group]
  cse_enhance_cells   THE HOT PATH: gain recursion + ISTFT + SNR sums [per grid cell]

A "cell spec" is (signal index, algorithm name, params dict) where params are
the reference plugin's keyword arguments (parameter_ranges.py keys).
"""

import ctypes
import math
from collections import OrderedDict

import numpy as np
import torch

from . import _lib, trackers
# the planning names other modules and the tests import from here stay importable
from .layout import (ALGO_COST, ALGOS, ALIGN_CORR_SAMPLES, ALIGN_MAX_LAG,  # noqa: F401
                     ALIGN_MIN_SAMPLES, DEFAULTS, GENERIC, MAIN, SHORT, PlanLayout, Ref,
                     canonical_algo, n_frames, noise_key, noise_params, pack_waves, route,
                     route_slots, specs_by_n_fft)


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _at(t, k):
    """Pointer to element k of a device tensor (None stays None)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr() + k * t.element_size())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


NOISE_PARAM_KEYS = ("percentile", "min_frames", "max_fraction", "floor_rel", "adaptive_short",
                    "window_size", "smoothing_factor")


class Engine:
    """Runs batches of grid cells over batches of equal-length signals."""

    def __init__(self, device="cuda"):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.CseError("no GPU visible: the HIP engine has no CPU fallback")
        self.device = torch.device(device)
        # key -> ((specs, keep), MultiPlan), most recent last: see run(reuse=...)
        self._plan_cache = OrderedDict()
        self.plan_cache_size = 1
        self._side = None

    # ------------------------------------------------------------------ prep
    def stft(self, x, n_fft, hop, x_sub=None, want_y=True, want_p=True):
        """x: [S, L] float64 cuda -> (Y [S,T,B,2] f32, P [S,T,B] f64)."""
        S, L = x.shape
        T, B = n_frames(L, hop), n_fft // 2 + 1
        Y = torch.empty((S, T, B, 2), dtype=torch.float32, device=x.device) if want_y else None
        P = torch.empty((S, T, B), dtype=torch.float64, device=x.device) if want_p else None
        _lib.check(self.lib.cse_stft(_ptr(x), _ptr(x_sub), S, L, n_fft, hop, _ptr(Y), _ptr(P),
                                     _stream()), "cse_stft")
        return Y, P

    def noise_estimate(self, method, P, percentile=20.0, eps=1e-10, out=None, frames=None,
                       **params):
        """cse_noise_estimate_ex on P [S, T', B] f64.  params: estimator
        constructor parameters (min_frames, max_fraction, floor_rel,
        adaptive_short, window_size, smoothing_factor; noise_estimation.py:12-13,
        :60).  true_noise: P is the power of STFT(noisy - clean) over the
        shorter length, fit to ``frames`` (default T') frames (:149-153).
        A tracker (trackers.TRACKERS): its cse_noise_<method>
        (include/cse_<method>.h) -> [S, T, B] at any T; params are the names of
        its record's defaults."""
        S, Tp, B = P.shape
        if method in trackers.TRACKERS:
            tracker = trackers.TRACKERS[method]
            if frames is not None and int(frames) != Tp:
                raise ValueError("frames applies to true_noise only")
            trackers.check_names(tracker, params)
            prm = trackers.params(tracker, tracker.values(params))
            if out is None:
                out = torch.empty((S, Tp, B), dtype=torch.float32, device=P.device)
            _lib.check(getattr(self.lib, tracker.entry)(_ptr(P), S, Tp, B, ctypes.byref(prm),
                                                        float(eps), _ptr(out), _stream()),
                       tracker.entry)
            return out
        T = Tp if frames is None else int(frames)
        code = {"percentile": 0, "min_tracking": 1, "true_noise": 2, "simple": 0}[method]
        static = method == "percentile" or (T < 5 and method != "true_noise")
        shape = (S, B) if (static and method != "min_tracking") else (S, T, B)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=P.device)
        ws = torch.empty(int(self.lib.cse_noise_workspace_bytes(S, T, B)), dtype=torch.uint8,
                         device=P.device)
        prm = noise_params(percentile=percentile, src_frames=Tp if code == 2 else 0, **params)
        if code != 2 and Tp != T:
            raise ValueError("frames applies to true_noise only")
        _lib.check(self.lib.cse_noise_estimate_ex(code, _ptr(P), S, T, B, ctypes.byref(prm),
                                                  float(eps), _ptr(out), _ptr(ws), _stream()),
                   f"cse_noise_estimate({method})")
        return out

    # ------------------------------------------------------------------ grid
    def plan(self, n_signals, length, specs, with_clean=True, want_waveforms=False,
             want_gains=False, align=False, true_len=None):
        """Build one GridPlan per n_fft for these specs (see GridPlan)."""
        return MultiPlan(self, n_signals, length, specs, with_clean, want_waveforms, want_gains,
                         align, true_len)

    def side_stream(self):
        """A second stream of this engine, kept for its lifetime (work queued
        on it reuses the caching allocator's blocks of earlier calls)."""
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.device)
        return self._side

    def run(self, noisy, specs, clean=None, want_waveforms=False, want_gains=False, align=False,
            true_len=None, reuse=None, keep=None, on_plan=None):
        """Enhance every cell spec; returns a dict of per-spec results.

        noisy/clean: [S, L] float64 cuda tensors (clean may be None if no spec
        uses true_noise and no SNR is wanted).  specs: list of
        (signal_index, algorithm_name, params).  Results (spec order):
          sse [n] f64 numpy, finite [n] bool numpy, and optionally
          'y' [n, L] f32 cuda and 'G' list of [T, B] f32 cuda.
        true_len: TrueNoise estimates use the first true_len samples of noisy
        and clean (a clean reference shorter than the noisy signal,
        noise_estimation.py:128-130); default L.
        reuse: keep the plan (device buffers, cell tables) for a later call
        with the same structure (the plan_cache_size most recent ones).  True: the structure is spec_fingerprint(specs)
        — per cell the signal index, algorithm and params object identity (the
        cached specs keep the params alive; they must not be mutated in
        between).  Or a hashable key the caller derived from the structure;
        specs may then be a zero-argument callable that builds the list, called
        only when the key misses, and ``keep`` is held with the plan (the
        object the key's identities refer to).  The results' 'y' is the plan's
        buffer: the next reusing call overwrites it.
        on_plan: see MultiPlan.execute.
        """
        S, L = noisy.shape
        flags = (S, L, clean is not None, want_waveforms, want_gains, align, true_len)
        mp, key = None, None
        if reuse is not None and reuse is not False:
            if reuse is True:
                specs = specs() if callable(specs) else specs
                reuse = spec_fingerprint(specs)
            key = flags + (reuse,)
            hit = self._plan_cache.get(key)
            if hit is not None:
                mp = hit[1]
                self._plan_cache.move_to_end(key)
        if mp is None:
            specs = specs() if callable(specs) else specs
            if key is not None:  # evict before allocating the new plan's buffers
                while len(self._plan_cache) >= max(self.plan_cache_size, 1):
                    self._plan_cache.popitem(last=False)
            mp = self.plan(S, L, specs, clean is not None, want_waveforms, want_gains, align,
                           true_len)
            if key is not None:
                self._plan_cache[key] = ((specs, keep), mp)
        mp.execute(noisy, clean, on_plan)
        return mp.results()


class GridPlan:
    """Everything one n_fft's cells need, allocated once; execute() only enqueues.

    Buffers (device, resident in HBM across steps):
      Y      [hop][S][T][B] complex64        cse_stft
      P      [S][T][B] f64 per hop           cse_stft (analysis power)
      pool   flat f32: every noise PSD the cells read, at per-key offsets
      cells  packed cse_cell_t table (wave slots, longest-first)
      sse/finite per packed cell; optional y_out / g_out
    execute() issues only kernel launches on the current stream (no host
    sync, no allocation), so it can be timed or captured as a graph.
    """

    # plain data of the layout that this class and its users read as attributes
    FORWARDED = ("n_fft", "S", "L", "B", "true_len", "items", "hops", "y_base", "hop_jobs", "idx",
                 "cells", "order", "split", "g_offsets", "units", "align", "xc_n", "xc_lag_max")

    def __init__(self, eng, n_fft, S, L, items, with_clean, want_y, want_g, y_all=None,
                 align=False, true_len=None):
        # the library and device only, not the Engine: the engine's plan cache
        # holds this plan, and a back reference would make the pair a cycle
        # that only the cyclic collector frees (with the plan's device buffers)
        lib, dev = self.lib, self.device = eng.lib, eng.device
        per = int(lib.cse_cells_per_group(n_fft)) if n_fft in (512, 1024) else None
        lay = self.layout = PlanLayout(n_fft, S, L, items, with_clean, want_y, want_g, align,
                                       true_len, cells_per_group=per)
        for name in self.FORWARDED:
            setattr(self, name, getattr(lay, name))

        def empty(shape, dtype):
            return torch.empty(shape, dtype=dtype, device=dev)

        def upload(table):
            return torch.from_numpy(table.view(np.uint8).copy()).to(dev)
        self.Ybuf = empty(lay.y_elems * 2, torch.float32)
        self.P = {h: empty(shape, torch.float64) for h, shape in lay.p_shape.items()}
        self.Ptrue = {h: empty(shape, torch.float64) for h, shape in lay.ptrue_shape.items()}
        self.pool = empty(lay.pool_elems, torch.float32)
        self.raw = empty(lay.raw_elems, torch.float32)
        self.jobs_d = upload(lay.jobs)
        self.med = empty((S, self.B), torch.float64)
        Tmax = max(n_frames(L, h) for h in self.hops)
        self.ws = empty(int(lib.cse_noise_workspace_bytes(S, Tmax, self.B)), torch.uint8)
        # the layout's noise calls with their offsets turned into pointers once
        # (the buffers stay where they are): prepare_noise only launches
        self.noise_calls = [(name, getattr(lib, name), [self._arg(a, hop) for a in args])
                            for hop, calls in lay.noise_calls.items() for name, args in calls]
        self.n_packed = len(lay.packed)
        self.cells_d = upload(lay.packed)
        self.g_out = (torch.zeros(max(lay.g_elems, 1), dtype=torch.float32, device=dev)
                      if want_g else None)
        self.y_all = y_all
        self.sse_d = torch.zeros(self.n_packed, dtype=torch.float64, device=dev)
        self.fin_d = torch.zeros(self.n_packed, dtype=torch.uint8, device=dev)
        self.clean = None
        self.with_clean = with_clean
        self.rerun = None
        if self.align:  # the heads: of the whole waveforms where those are requested
            self.head = y_all if y_all is not None else empty(lay.head_elems, torch.float32)
            self.head_off = torch.as_tensor(lay.head_off, device=dev)
            self.sig_of = torch.as_tensor(lay.sig.astype(np.int32), device=dev)
            self.xc_ws = empty(int(lib.cse_xcorr_workspace_bytes(S, L, self.xc_n,
                                                                 self.xc_lag_max)), torch.uint8)
            self.lag_d = torch.zeros(len(items), dtype=torch.int32, device=dev)
            self.zero_d = torch.zeros(len(items), dtype=torch.float64, device=dev)
            self.xst_d = torch.zeros(len(items), dtype=torch.int32, device=dev)

    def prepare(self, noisy, clean=None):
        """Group-level analysis: STFTs and every noise row (once per signal batch)."""
        self.prepare_stft(noisy, clean)
        self.prepare_noise(clean)

    # The analysis in two phases: every hop's STFT first, then the noise chains.
    # The STFT (80 KB of LDS per workgroup) cannot take the slot of one finished
    # enhance workgroup, so on a side stream under an enhance launch it waits
    # for the launch's drain, while the noise kernels fit freed slots.  With
    # the STFTs adjacent (TimedJob.prep: of every plan), one drain runs them all
    # and the chains follow inside the next launch; interleaved (STFT, chain,
    # STFT, chain) each STFT waited for a drain of its own and the next launch
    # for the last chain (r05: 168.6 -> 168.2 ms/step at 100 pairs).
    def prepare_stft(self, noisy, clean=None):
        S, L, B = self.S, self.L, self.B
        lib = self.lib
        st = _stream()
        for hop in self.hops:
            T = n_frames(L, hop)
            yv = self.Ybuf[2 * self.y_base[hop]:2 * (self.y_base[hop] + S * T * B)]
            _lib.check(lib.cse_stft(_ptr(noisy), None, S, L, self.n_fft, hop, _ptr(yv),
                                    _ptr(self.P[hop]), st), "cse_stft")
            if hop in self.Ptrue:
                m = self.true_len
                xn, xc = noisy, clean
                if m < L:  # the STFT of the trimmed difference (noise_estimation.py:128-133)
                    xn, xc = noisy[:, :m].contiguous(), clean[:, :m].contiguous()
                _lib.check(lib.cse_stft(_ptr(xn), _ptr(xc), S, m, self.n_fft, hop, None,
                                        _ptr(self.Ptrue[hop]), st), "cse_stft(true)")

    def prepare_noise(self, clean=None):
        """Every hop's noise rows: the layout's call list (PlanLayout.noise_calls)."""
        st = _stream()
        for name, fn, args in self.noise_calls:
            _lib.check(fn(*args, st), name)
        self.clean = clean if self.with_clean else None

    def _arg(self, a, hop):
        if isinstance(a, Ref):
            buf = getattr(self, a.buf)
            return _at(buf[hop] if isinstance(buf, dict) else buf, a.off)
        return ctypes.byref(a) if isinstance(a, ctypes.Structure) else a

    def enhance(self):
        """THE HOT PATH launch: every cell of this n_fft, one kernel."""
        if self.y_all is not None:
            yo, olen = self.y_all, self.L
        elif self.align:
            yo, olen = self.head, self.xc_n
        else:
            yo, olen = None, 0
        self.launch(self.cells_d, self.split, yo, olen, self.g_out, self.sse_d, self.fin_d,
                    _stream(), "cse_enhance_cells")

    def launch(self, cells_d, split, yo, olen, g, sse, fin, st, what):
        """The enhance launches over packed cells, split = (main, short,
        generic) slot counts in that order (pack_waves): the sweep hops
        (cse_enhance_cells, one kernel), the short hops
        (cse_enhance_cells_short_hop), every other shape
        (cse_enhance_cells_generic)."""
        args = (_ptr(self.Ybuf), _ptr(self.pool), _ptr(self.clean), _ptr(yo), olen)
        n_main, n_short, n_gen = split
        k = _lib.CELL_DTYPE.itemsize
        if n_main:
            _lib.check(self.lib.cse_enhance_cells(self.n_fft, self.L, _ptr(cells_d), n_main, *args,
                                                  _ptr(g), _ptr(sse), _ptr(fin), st), what)
        if n_short:
            _lib.check(self.lib.cse_enhance_cells_short_hop(
                self.n_fft, self.L, _at(cells_d, n_main * k), n_short, *args, _at(sse, n_main),
                _at(fin, n_main), st), what + "(short hop)")
        if n_gen:
            o = n_main + n_short
            _lib.check(self.lib.cse_enhance_cells_generic(
                self.n_fft, self.L, _at(cells_d, o * k), n_gen, *args, _ptr(g), _at(sse, o),
                _at(fin, o), st), what + "(generic)")

    def execute(self, noisy, clean=None):
        self.prepare(noisy, clean)
        self.enhance()
        if self.align:
            self.finalize()

    def finalize(self):
        """finalize_enhanced on the device: per-cell cross-correlation lag
        (cse_xcorr_lag), then the cells whose lag is not 0 are scored again
        with the shifted output (cse_enhance_cells with cell.lag, plus the
        clean energy of the zero padding)."""
        lib, st = self.lib, _stream()
        _lib.check(lib.cse_xcorr_prepare(_ptr(self.clean), self.S, self.L, self.xc_n,
                                         self.xc_lag_max, _ptr(self.xc_ws), st),
                   "cse_xcorr_prepare")
        _lib.check(lib.cse_xcorr_lag(_ptr(self.head), _ptr(self.head_off), _ptr(self.sig_of),
                                     len(self.items), self.S, self.xc_n, self.xc_lag_max,
                                     _ptr(self.xc_ws), _ptr(self.lag_d), _ptr(self.zero_d),
                                     _ptr(self.xst_d), None, st), "cse_xcorr_lag")
        lag = self.lag_d.cpu().numpy()
        sel = np.nonzero(lag != 0)[0]
        self.rerun = None
        if len(sel) == 0:
            return
        cells = self.cells[sel].copy()
        cells["lag"] = lag[sel]
        cells["out_offset"] = -1
        cells["gain_offset"] = -1
        packed, order = pack_waves(cells, self.n_fft)
        cd = torch.from_numpy(packed.view(np.uint8).copy()).to(self.device)
        sse = torch.zeros(len(packed), dtype=torch.float64, device=self.device)
        fin = torch.zeros(len(packed), dtype=torch.uint8, device=self.device)
        self.launch(cd, route_slots(packed, self.n_fft), None, 0, None, sse, fin, st,
                    "cse_enhance_cells(aligned)")
        self.rerun = (sel, order, sse, fin)

    def results(self):
        sse_p = self.sse_d.cpu().numpy()
        fin_p = self.fin_d.cpu().numpy().astype(bool)
        real = self.order >= 0
        sse = np.empty(len(self.items))
        fin = np.empty(len(self.items), dtype=bool)
        sse[self.order[real]] = sse_p[real]
        fin[self.order[real]] = fin_p[real]
        self.lag = self.xstatus = None
        if self.align:
            self.lag = self.lag_d.cpu().numpy()
            self.xstatus = self.xst_d.cpu().numpy()
            # a non-finite head aligns at -max_lag (np.argmax over an all-NaN
            # correlation) and is rescored at that lag like any other: the
            # reference checks finiteness only after the shift (:100-103)
            if self.rerun is not None:
                sel, order, sse_r, fin_r = self.rerun
                sr, fr = sse_r.cpu().numpy(), fin_r.cpu().numpy().astype(bool)
                ok = order >= 0
                sse[sel[order[ok]]] = sr[ok] + self.zero_d.cpu().numpy()[sel[order[ok]]]
                fin[sel[order[ok]]] = fr[ok]
        G = None
        if self.g_out is not None:
            G = [self.g_out[g0:g0 + T * self.B].view(T, self.B) for (g0, T) in self.g_offsets]
        return sse, fin, G


class MultiPlan:
    """GridPlans for every n_fft present in a spec list (spec order preserved)."""

    def __init__(self, eng, S, L, specs, with_clean, want_y, want_g, align=False, true_len=None):
        self.n = len(specs)
        self.align = align
        self.want_g = want_g
        self.y_all = (torch.zeros((self.n, L), dtype=torch.float32, device=eng.device)
                      if want_y else None)
        self.plans = [GridPlan(eng, n_fft, S, L, items, with_clean, want_y, want_g, self.y_all,
                               align, true_len)
                      for n_fft, items in specs_by_n_fft(S, L, specs, with_clean, want_g)]
        self.units = sum(p.units for p in self.plans)

    def execute(self, noisy, clean=None, on_plan=None):
        """Per n_fft: analysis (STFTs, noise rows), enhance, alignment.
        on_plan(plan, sse, finite, lag): called once an n_fft's cells are final
        (host-synchronised results in plan.items order; plan.idx maps them to
        spec indices), after the next n_fft's analysis is queued and before its
        enhance is, so the caller can queue work on those cells' outputs on
        another stream without starving the next analysis' small kernels."""
        if self.plans:
            self.plans[0].prepare(noisy, clean)
        for k, p in enumerate(self.plans):
            p.enhance()
            if p.align:
                p.finalize()
            if k + 1 < len(self.plans):
                self.plans[k + 1].prepare(noisy, clean)
            if on_plan is not None:
                sse, fin, _ = p.results()
                on_plan(p, sse, fin, p.lag)

    def results(self):
        sse = np.full(self.n, np.nan)
        fin = np.zeros(self.n, dtype=bool)
        gains = [None] * self.n if self.want_g else None
        lag = np.zeros(self.n, dtype=np.int64) if self.align else None
        xst = np.zeros(self.n, dtype=np.int64) if self.align else None
        for p in self.plans:
            s, f, G = p.results()
            ix = p.idx
            sse[ix], fin[ix] = s, f
            if gains is not None:
                for c, i in enumerate(ix):
                    gains[i] = G[c]
            if lag is not None and p.lag is not None:
                lag[ix], xst[ix] = p.lag, p.xstatus
        out = {"sse": sse, "finite": fin}
        if lag is not None:
            out["lag"], out["xcorr_status"] = lag, xst
        if self.y_all is not None:
            out["y"] = self.y_all
        if gains is not None:
            out["G"] = gains
        return out


def structure_digest():
    """A 128-bit hash object for plan-reuse keys: xxh3 (an order of magnitude
    faster than blake2b on the sweep's 17-MB batch descriptions) when the
    xxhash module is importable, blake2b otherwise."""
    try:
        import xxhash
        return xxhash.xxh3_128()
    except ImportError:
        import hashlib
        return hashlib.blake2b(digest_size=16)


def spec_fingerprint(specs):
    """Digest of a spec list's structure: per cell the signal index, the
    algorithm name and the identity of its params dict (Engine.run(reuse=True))."""
    n = len(specs)
    sig = np.fromiter((s for (s, _, _) in specs), dtype=np.int64, count=n)
    pid = np.fromiter((id(p) for (_, _, p) in specs), dtype=np.int64, count=n)
    algs = {}
    aid = np.fromiter((algs.setdefault(a, len(algs)) for (_, a, _) in specs), dtype=np.int64, count=n)
    h = structure_digest()
    for arr in (sig, pid, aid):
        h.update(arr)
    h.update(repr(sorted(algs.items(), key=lambda kv: kv[1])).encode())
    return h.hexdigest()


def snr_db(sse, clean_power):
    """calculate_snr (evaluation_metrics.py:39-58) from the kernel's error energy."""
    sse = np.asarray(sse, dtype=np.float64)
    with np.errstate(divide="ignore"):
        out = 10.0 * np.log10(clean_power / (sse + 1e-10))
    return np.where(sse == 0, math.inf, out)
