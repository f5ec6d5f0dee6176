"""The online enhancer: the offline path on audio that is still arriving.

``OnlineEnhancer`` runs one algorithm with one parameter set, as a sweep found
it, on S signals that advance in lockstep; include/cse_online.h is the
specification of what the device does per frame.  This module is the host
side of it:

  config()        a cell's (algorithm, params) -> what cse_online_config_t
                  carries; host-only, raises for what the online path refuses
  DeviceCore      the device calls (cse_online_init / prime / push / finish) on
                  torch buffers; no CPU fallback
  OnlineEnhancer  buffers input to whole hops, builds the reflect padding at
                  both ends, holds back spp's first init_frames frames, and
                  trims the emitted padded samples to the caller's positions

The wrapper talks to its core through four methods (prime, push, finish,
reset), so it runs without a device over any object that has them.
"""

import ctypes
from typing import NamedTuple

import numpy as np

from . import _lib, trackers
from .layout import ALGOS, DEFAULTS, canonical_algo

METHODS = ("mcra", "spp")  # the trackers whose state is per bin and of fixed size
WHOLE_CLIP = ("percentile", "min_tracking", "true_noise")
N_FFT_MIN, N_FFT_MAX = 128, 2048


class Config(NamedTuple):
    algorithm: str     # canonical name (layout.ALGOS)
    algo: int          # CSE_ALGO_*
    n_fft: int
    hop: int
    param: tuple       # cse_cell_t.param[8]
    eps: float         # the algorithm's eps (layout.ALGOS)
    mu: float          # noise smoothing, 0.0 = none
    method: str        # "mcra" or "spp"
    values: tuple      # the tracker's validated values (trackers.TRACKERS[method].values)

    @property
    def bins(self):
        return self.n_fft // 2 + 1

    @property
    def first_frames(self):
        """Frames the first device push must carry (spp: init_frames)."""
        return self.values[-1] if self.method == "spp" else 1


def config(algorithm, params):
    """The Config of a cell spec's (algorithm, params); ValueError for a shape
    or noise_method the online path does not run, TypeError for an unknown
    tracker parameter (trackers.check_names)."""
    alg = canonical_algo(algorithm)
    code, eps, names = ALGOS[alg]
    for key in ("n_fft", "hop_length", "noise_method"):
        if key not in params:
            raise ValueError(f"online: params lack {key!r}")
    n_fft, hop, method = params["n_fft"], params["hop_length"], params["noise_method"]
    if method in WHOLE_CLIP:
        raise ValueError(f"online: noise_method {method!r} needs the whole clip "
                         f"(supported: {', '.join(METHODS)})")
    if method in trackers.TRACKERS and method not in METHODS:
        raise ValueError(f"online: noise_method {method!r} keeps state of another size with "
                         f"coupled bins and is not streamed (supported: {', '.join(METHODS)})")
    if method not in METHODS:
        raise ValueError(f"Unbekannte Methode: {method}")
    if (n_fft != int(n_fft) or not N_FFT_MIN <= int(n_fft) <= N_FFT_MAX
            or int(n_fft) & (int(n_fft) - 1)):
        raise ValueError(f"online: n_fft={n_fft} not a power of two in "
                         f"[{N_FFT_MIN}, {N_FFT_MAX}]")
    n_fft = int(n_fft)
    if hop not in (n_fft // 8, n_fft // 4, n_fft // 2):
        raise ValueError(f"online: hop_length={hop} not n_fft/8, n_fft/4 or n_fft/2 "
                         f"(n_fft={n_fft})")
    tracker = trackers.TRACKERS[method]
    prefix = method + "_"
    trackers.check_names(tracker, {k[len(prefix):] for k in params if k.startswith(prefix)})
    values = tracker.values(params, prefix)
    dflt = DEFAULTS.get(alg, {})
    missing = [k for k in names if k not in params and k not in dflt]
    if missing:
        raise ValueError(f"online: {alg} params lack {missing[0]!r}")
    param = [float(params[k]) if k in params else float(dflt[k]) for k in names]
    mu = None
    if code == "MMSE":  # as layout.noise_key: mmse and omlsa smooth a time-varying estimate
        mu = params.get("noise_mu", dflt["noise_mu"])
    elif code == "OMLSA":
        if "noise_mu" not in params:
            raise ValueError("online: omlsa params lack 'noise_mu'")
        mu = params["noise_mu"]
    return Config(alg, _lib.ALGO[code], n_fft, int(hop), tuple(param + [0.0] * (8 - len(param))),
                  float(eps), float(mu or 0.0), method, values)


def abi_config(cfg):
    """cse_online_config_t of a Config."""
    c = _lib.OnlineConfig()
    c.n_fft, c.hop, c.algo, c.noise_method = cfg.n_fft, cfg.hop, cfg.algo, _lib.NOISE[cfg.method]
    c.param[:] = cfg.param
    c.eps, c.mu = cfg.eps, cfg.mu
    for name in METHODS:  # the other tracker's block: its defaults (never read)
        t = trackers.TRACKERS[name]
        vals = cfg.values if name == cfg.method else t.values({})
        setattr(c, name, trackers.params(t, vals))
    return c


class DeviceCore:
    """The device side of one batch of S streams: the state block, the handle
    and the four calls.  Arrays in and out are numpy; every call returns after
    its results are on the host."""

    def __init__(self, cfg, n_streams, want_noise=False):
        import torch
        self.torch = torch
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.CseError("no GPU visible: the HIP engine has no CPU fallback")
        self.cfg, self.S, self.want_noise = cfg, int(n_streams), bool(want_noise)
        nbytes = int(self.lib.cse_online_state_bytes(cfg.n_fft, self.S))
        if nbytes < 0:
            raise _lib.CseError(f"cse_online_state_bytes({cfg.n_fft}, {self.S}) refused")
        self.state = torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda")
        self.handle = _lib.OnlineHandle()
        c = abi_config(cfg)
        _lib.check(self.lib.cse_online_init(ctypes.byref(self.handle), ctypes.byref(c), self.S,
                                            ctypes.c_void_p(self.state.data_ptr())),
                   "cse_online_init")

    def _stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream().cuda_stream)

    def _dev(self, x):
        return self.torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64)).cuda()

    def prime(self, head):
        x = self._dev(head)
        _lib.check(self.lib.cse_online_prime(ctypes.byref(self.handle),
                                             ctypes.c_void_p(x.data_ptr()), self._stream()),
                   "cse_online_prime")
        self.torch.cuda.current_stream().synchronize()  # x is read until here

    def push(self, x):
        torch, cfg = self.torch, self.cfg
        k = x.shape[1] // cfg.hop
        xd = self._dev(x)
        y = torch.empty((self.S, k * cfg.hop), dtype=torch.float32, device="cuda")
        n = (torch.empty((self.S, k, cfg.bins), dtype=torch.float32, device="cuda")
             if self.want_noise else None)
        _lib.check(self.lib.cse_online_push(
            ctypes.byref(self.handle), ctypes.c_void_p(xd.data_ptr()), k,
            ctypes.c_void_p(y.data_ptr()), None if n is None else ctypes.c_void_p(n.data_ptr()),
            self._stream()), "cse_online_push")
        return y.cpu().numpy(), None if n is None else n.cpu().numpy()

    def finish(self):
        cfg = self.cfg
        y = self.torch.empty((self.S, cfg.n_fft - cfg.hop), dtype=self.torch.float32,
                             device="cuda")
        _lib.check(self.lib.cse_online_finish(ctypes.byref(self.handle),
                                              ctypes.c_void_p(y.data_ptr()), self._stream()),
                   "cse_online_finish")
        return y.cpu().numpy()

    def reset(self):
        """Nothing to do: the next prime resets every state."""


class OnlineEnhancer:
    """One algorithm and parameter set on n_streams signals in lockstep.

    push(block) takes float64 samples [n] (one stream) or [S][n], any n >= 0,
    and returns the float32 samples that are final, [m] or [S][m], m >= 0;
    finish() returns the rest.  All results concatenated have the input's
    length and are the offline plugin's output on the whole clip (for clips of
    at least max(5, init_frames) frames; include/cse_online.h).  After finish,
    push raises until reset().  want_noise: every call returns (samples, rows)
    with the tracked noise rows [k][B] or [S][k][B] of the frames it ran.
    core: the object that runs the frames (default: DeviceCore on the GPU).
    """

    def __init__(self, algorithm, params, n_streams=1, want_noise=False, core=None):
        self.cfg = config(algorithm, params)
        if n_streams != int(n_streams) or int(n_streams) < 1:
            raise ValueError(f"online: n_streams={n_streams} not an integer >= 1")
        self.S = int(n_streams)
        self.want_noise = bool(want_noise)
        self.core = DeviceCore(self.cfg, self.S, want_noise) if core is None else core
        self.reset()

    @property
    def latency(self):
        """Samples of look-ahead, at most: output o is final once input
        o + latency is in (CSE_ONLINE_LATENCY; spp's first init_frames frames
        are held back once on top of it)."""
        return self.cfg.n_fft - 1

    def reset(self):
        half = self.cfg.n_fft // 2
        self._pre = np.zeros((self.S, 0))     # input before the reflect head exists
        self._pad = None                      # padded samples the core has not taken
        self._recent = np.zeros((self.S, 0))  # the last n_fft/2 + 1 input samples
        self._n_in = 0
        self._primed = False
        self._frames = 0
        self._returned = 0
        self._finished = False
        self._flat = self.S == 1
        self._half = half
        self.core.reset()

    # ------------------------------------------------------------------ input
    def _block(self, block):
        x = np.asarray(block, dtype=np.float64)
        if x.ndim == 1:
            if self.S != 1:
                raise ValueError(f"online: a 1-D block for {self.S} streams")
            x = x[None, :]
        elif x.ndim == 2 and x.shape[0] == self.S:
            if self._n_in == 0 and self._pre.shape[1] == 0:
                self._flat = False
        else:
            raise ValueError(f"online: block of shape {x.shape} for {self.S} streams")
        return x

    def push(self, block):
        if self._finished:
            raise RuntimeError("online: push after finish (reset() first)")
        x = self._block(block)
        half = self._half
        self._n_in += x.shape[1]
        self._recent = np.concatenate([self._recent, x], axis=1)[:, -(half + 1):]
        if self._pad is None:
            self._pre = np.concatenate([self._pre, x], axis=1)
            if self._pre.shape[1] >= half + 1:  # xp[0, n_fft/2) = x[n_fft/2], ..., x[1]
                self._pad = np.concatenate([self._pre[:, half:0:-1], self._pre], axis=1)
                self._pre = None
        else:
            self._pad = np.concatenate([self._pad, x], axis=1)
        return self._result(*self._advance(False))

    def finish(self):
        if self._finished:
            raise RuntimeError("online: finish after finish (reset() first)")
        half, cfg = self._half, self.cfg
        if self._n_in < half + 1:
            raise ValueError(f"online: reflect padding of n_fft/2 = {half} samples needs at least "
                             f"{half + 1} samples (got {self._n_in})")
        # xp[n_fft/2 + len + j] = x[len - 2 - j]
        self._pad = np.concatenate([self._pad, self._recent[:, -2::-1]], axis=1)
        y, rows = self._advance(True, length=self._n_in)
        tail = self.core.finish()
        self._finished = True
        y = np.concatenate([y, self._trim(tail, self._frames * cfg.hop, self._n_in)], axis=1)
        assert self._returned == self._n_in, (self._returned, self._n_in)
        return self._result(y, rows)

    # ------------------------------------------------------------------ frames
    def _advance(self, final, length=None):
        cfg = self.cfg
        empty = (np.zeros((self.S, 0), dtype=np.float32),
                 np.zeros((self.S, 0, cfg.bins), dtype=np.float32))
        if self._pad is None:
            return empty
        if not self._primed:
            nt = cfg.n_fft - cfg.hop
            if self._pad.shape[1] < nt:
                return empty
            self.core.prime(self._pad[:, :nt])
            self._pad = self._pad[:, nt:]
            self._primed = True
        k = self._pad.shape[1] // cfg.hop
        if self._frames == 0 and k < cfg.first_frames:
            if final:
                raise ValueError(f"online: the clip has {k} frames, fewer than spp's "
                                 f"init_frames={cfg.first_frames}")
            return empty
        if k == 0:
            return empty
        y, rows = self.core.push(self._pad[:, :k * cfg.hop])
        self._pad = self._pad[:, k * cfg.hop:]
        at = self._frames * cfg.hop
        self._frames += k
        return self._trim(y, at, length), rows if rows is not None else empty[1]

    def _trim(self, y, at, length):
        """Emitted padded samples [at, at + m) -> the caller's positions
        [0, length) among them (padded sample p is output sample p - n_fft/2)."""
        lo = max(self._half - at, 0)
        hi = y.shape[1] if length is None else max(min(length + self._half - at, y.shape[1]), lo)
        out = y[:, lo:hi]
        self._returned += out.shape[1]
        return out

    def _result(self, y, rows):
        if self._flat:
            y, rows = y[0], rows[0]
        return (y, rows) if self.want_noise else y
