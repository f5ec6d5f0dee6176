"""The online enhancer: the offline path on audio that is still arriving.

``OnlineEnhancer`` runs one algorithm with one parameter set, as a sweep found
it, on S signals that advance in lockstep; include/cse_online.h is the
specification of what the device does per frame.  This module is the host
side of it:

  config()        a cell's (algorithm, params) -> what cse_online_config_t
                  carries; host-only, raises for what the online path refuses
  DeviceCore      the device calls (cse_online_init / prime / push / finish) on
                  torch buffers; no CPU fallback
  StreamHost      one stream's (or one lockstep batch's) host logic: buffers
                  input to whole hops, builds the reflect padding at both
                  ends, holds back spp's first init_frames frames, and trims
                  the emitted padded samples to the caller's positions; it
                  makes no call
  OnlineEnhancer  a StreamHost and a core, run as soon as input arrives

The wrapper talks to its core through four methods (prime, push, finish,
reset), so it runs without a device over any object that has them.

``OnlinePool`` (include/cse_online_pool.h) serves streams that do not advance
in lockstep: they open and close one at a time, each with parameter values
and a pace of its own, and one step launch advances all that have frames
pending.  ``PoolCore`` is its device side (cse_pool_init / open / step / close
/ drop); the pool talks to it through open, step, close and drop.
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


class StreamHost:
    """The host side of S signals that advance together (a lockstep batch, or
    with S = 1 one stream of a pool): the reflect head once n_fft/2 + 1 samples
    are in, buffering to whole hops, holding back spp's first init_frames
    frames, the reflect tail, and the trimming of emitted padded samples to the
    caller's positions.  It calls nothing: its owner asks what the device
    would get now (head, ready, take) and hands back what came out (emitted).
    """

    def __init__(self, cfg, n_streams=1):
        self.cfg, self.S = cfg, int(n_streams)
        self.half = cfg.n_fft // 2
        self.pre = np.zeros((self.S, 0))     # input before the reflect head exists
        self.pad = None                      # padded samples the device has not taken
        self.recent = np.zeros((self.S, 0))  # the last n_fft/2 + 1 input samples
        self.n_in = 0
        self.primed = False                  # head() has been taken
        self.frames = 0                      # frames taken
        self.at = 0                          # padded samples handed back so far
        self.returned = 0
        self.ended = False

    # ------------------------------------------------------------------ input
    def feed(self, x):
        """x [S][n] float64, any n >= 0."""
        half = self.half
        self.n_in += x.shape[1]
        self.recent = np.concatenate([self.recent, x], axis=1)[:, -(half + 1):]
        if self.pad is None:
            self.pre = np.concatenate([self.pre, x], axis=1)
            if self.pre.shape[1] >= half + 1:  # xp[0, n_fft/2) = x[n_fft/2], ..., x[1]
                self.pad = np.concatenate([self.pre[:, half:0:-1], self.pre], axis=1)
                self.pre = None
        else:
            self.pad = np.concatenate([self.pad, x], axis=1)

    def end(self):
        """The input is complete: the reflect tail follows it.  ValueError, with
        nothing changed, for an input the path cannot finish."""
        half, cfg = self.half, self.cfg
        if self.n_in < half + 1:
            raise ValueError(f"online: reflect padding of n_fft/2 = {half} samples needs at least "
                             f"{half + 1} samples (got {self.n_in})")
        total = 1 + self.n_in // cfg.hop
        if self.frames == 0 and total < cfg.first_frames:
            raise ValueError(f"online: the clip has {total} frames, fewer than spp's "
                             f"init_frames={cfg.first_frames}")
        # xp[n_fft/2 + len + j] = x[len - 2 - j]
        self.pad = np.concatenate([self.pad, self.recent[:, -2::-1]], axis=1)
        self.ended = True

    # ------------------------------------------------------------------ frames
    def ready(self, max_frames=None):
        """Frames the device would get now: every whole hop pending, none
        before the first first_frames frames are; max_frames caps it, but not
        below those first frames."""
        cfg = self.cfg
        if self.pad is None:
            return 0
        have = self.pad.shape[1] - (0 if self.primed else cfg.n_fft - cfg.hop)
        k = max(have, 0) // cfg.hop
        first = cfg.first_frames if self.frames == 0 else 1
        if k < first:
            return 0
        return k if max_frames is None else min(k, max(int(max_frames), first))

    def head(self):
        """xp[:, 0:n_fft - hop], what the prime takes, once it exists; None
        before that and after it has been taken."""
        nt = self.cfg.n_fft - self.cfg.hop
        if self.primed or self.pad is None or self.pad.shape[1] < nt:
            return None
        head, self.pad = self.pad[:, :nt], self.pad[:, nt:]
        self.primed = True
        return head

    def take(self, k):
        """The next k hop padded samples [S][k hop]; they are the device's now."""
        n = k * self.cfg.hop
        x, self.pad = self.pad[:, :n], self.pad[:, n:]
        self.frames += k
        return x

    def emitted(self, y):
        """The next padded samples the device emitted, [S][m] -> the caller's
        positions among them (padded sample p is output sample p - n_fft/2;
        once the input has ended, nothing from its length on)."""
        at, self.at = self.at, self.at + y.shape[1]
        lo = max(self.half - at, 0)
        hi = y.shape[1]
        if self.ended:
            hi = max(min(self.n_in + self.half - at, hi), lo)
        out = y[:, lo:hi]
        self.returned += out.shape[1]
        return out


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
        self._host = StreamHost(self.cfg, self.S)
        self._finished = False
        self._flat = self.S == 1
        self.core.reset()

    def _block(self, block):
        x = np.asarray(block, dtype=np.float64)
        if x.ndim == 1:
            if self.S != 1:
                raise ValueError(f"online: a 1-D block for {self.S} streams")
            x = x[None, :]
        elif x.ndim == 2 and x.shape[0] == self.S:
            if self._host.n_in == 0:
                self._flat = False
        else:
            raise ValueError(f"online: block of shape {x.shape} for {self.S} streams")
        return x

    def push(self, block):
        if self._finished:
            raise RuntimeError("online: push after finish (reset() first)")
        self._host.feed(self._block(block))
        return self._result(*self._advance())

    def finish(self):
        if self._finished:
            raise RuntimeError("online: finish after finish (reset() first)")
        host = self._host
        host.end()
        y, rows = self._advance()
        tail = self.core.finish()
        self._finished = True
        y = np.concatenate([y, host.emitted(tail)], axis=1)
        assert host.returned == host.n_in, (host.returned, host.n_in)
        return self._result(y, rows)

    def _advance(self):
        """Everything the stream host has for the core now, run at once."""
        host, cfg = self._host, self.cfg
        empty = (np.zeros((self.S, 0), dtype=np.float32),
                 np.zeros((self.S, 0, cfg.bins), dtype=np.float32))
        head = host.head()
        if head is not None:
            self.core.prime(head)
        k = host.ready()
        if k == 0:
            return empty
        y, rows = self.core.push(host.take(k))
        return host.emitted(y), rows if rows is not None else empty[1]

    def _result(self, y, rows):
        if self._flat:
            y, rows = y[0], rows[0]
        return (y, rows) if self.want_noise else y


def abi_pool_params(cfg):
    """cse_pool_params_t of a Config: one slot's values."""
    c = abi_config(cfg)
    p = _lib.PoolParams()
    p.param[:] = cfg.param
    p.mu, p.mcra, p.spp = cfg.mu, c.mcra, c.spp
    return p


class PoolCore:
    """The device side of a pool (include/cse_online_pool.h): the state block,
    the work list and the slot table, the handle and its five calls.  Arrays in
    and out are numpy; every call returns after its results are on the host.
    No CPU fallback."""

    def __init__(self, cfg, capacity, want_noise=False):
        import torch
        self.torch = torch
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.CseError("no GPU visible: the HIP engine has no CPU fallback")
        self.cfg, self.capacity, self.want_noise = cfg, int(capacity), bool(want_noise)
        sizes = (int(self.lib.cse_pool_state_bytes(cfg.n_fft, self.capacity)),
                 int(self.lib.cse_pool_work_bytes(self.capacity)))
        if min(sizes) < 0:
            raise _lib.CseError(f"cse_pool_state_bytes({cfg.n_fft}, {self.capacity}) refused")
        self.state, self.work = (torch.empty(max(n, 1), dtype=torch.uint8, device="cuda")
                                 for n in sizes)
        self.slots = (_lib.PoolSlot * max(self.capacity, 1))()
        self.handle = _lib.PoolHandle()
        c = abi_config(cfg)
        _lib.check(self.lib.cse_pool_init(
            ctypes.byref(self.handle), ctypes.byref(c), self.capacity,
            ctypes.c_void_p(self.state.data_ptr()), ctypes.c_void_p(self.work.data_ptr()),
            ctypes.cast(self.slots, ctypes.c_void_p)), "cse_pool_init")

    def _stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream().cuda_stream)

    def _dev(self, x):
        return self.torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64)).cuda()

    def open(self, slot, cfg, head):
        """Slot ``slot`` starts a stream with cfg's values (a Config of the
        pool's shape and method) and the input head [n_fft - hop]."""
        prm = abi_pool_params(cfg)
        x = self._dev(head)
        _lib.check(self.lib.cse_pool_open(ctypes.byref(self.handle), int(slot), ctypes.byref(prm),
                                          ctypes.c_void_p(x.data_ptr()), self._stream()),
                   "cse_pool_open")
        self.torch.cuda.current_stream().synchronize()  # x is read until here

    def step(self, items, x):
        """items: [(slot, k)]; x: their next k hop samples, concatenated in
        that order.  Returns (samples [sum k hop], rows [sum k][B] or None)."""
        torch, cfg = self.torch, self.cfg
        frames = sum(k for _, k in items)
        lst = (_lib.PoolItem * max(len(items), 1))(*[_lib.PoolItem(int(s), int(k))
                                                      for s, k in items])
        xd = self._dev(x)
        y = torch.empty(max(frames * cfg.hop, 1), dtype=torch.float32, device="cuda")
        n = (torch.empty((max(frames, 1), cfg.bins), dtype=torch.float32, device="cuda")
             if self.want_noise else None)
        _lib.check(self.lib.cse_pool_step(
            ctypes.byref(self.handle), ctypes.cast(lst, ctypes.c_void_p), len(items),
            ctypes.c_void_p(xd.data_ptr()), ctypes.c_void_p(y.data_ptr()),
            None if n is None else ctypes.c_void_p(n.data_ptr()), self._stream()), "cse_pool_step")
        return (y[:frames * cfg.hop].cpu().numpy(),
                None if n is None else n[:frames].cpu().numpy())

    def close(self, slot):
        """The slot's last n_fft - hop padded samples; the slot is free."""
        cfg = self.cfg
        y = self.torch.empty(cfg.n_fft - cfg.hop, dtype=self.torch.float32, device="cuda")
        _lib.check(self.lib.cse_pool_close(ctypes.byref(self.handle), int(slot),
                                           ctypes.c_void_p(y.data_ptr()), self._stream()),
                   "cse_pool_close")
        return y.cpu().numpy()

    def drop(self, slot):
        _lib.check(self.lib.cse_pool_drop(ctypes.byref(self.handle), int(slot)), "cse_pool_drop")


class _PoolStream:
    def __init__(self, cfg, slot):
        self.cfg, self.slot = cfg, slot
        self.host = StreamHost(cfg, 1)
        self.opened = False  # the core's open has run


class OnlinePool:
    """Streams that come and go on one device state block
    (include/cse_online_pool.h): one algorithm, shape and noise method per
    pool, parameter values and pace per stream.

    open(overrides) starts a stream with the pool's params merged with
    ``overrides`` and returns its id (never reused); feed(sid, block) buffers
    float64 samples [n], any n >= 0, without device work; step(max_frames)
    runs, in one launch, every stream that has whole frames pending (its first
    first_frames frames, afterwards at least one hop), each by all of them
    (at most max_frames, which does not cut below an spp stream's first
    init_frames), and returns {sid: samples} of the streams it ran: float32,
    final, possibly empty; close(sid) runs what that stream still has, the
    reflect tail and the finish, returns the rest and frees the slot;
    drop(sid) abandons the stream.  Everything one stream returns,
    concatenated, has the length of what was fed and is what
    OnlineEnhancer(algorithm, merged params) returns for that input.
    want_noise: (samples, rows [k][B]) in place of samples.  core: the object
    that runs the slots (default: PoolCore on the GPU).
    """

    SHAPE = ("n_fft", "hop_length", "noise_method")

    def __init__(self, algorithm, params, capacity=1024, want_noise=False, core=None):
        self.algorithm, self.params = algorithm, dict(params)
        self.cfg = config(algorithm, params)
        if capacity != int(capacity) or int(capacity) < 1:
            raise ValueError(f"online: capacity={capacity} not an integer >= 1")
        self.capacity = int(capacity)
        self.want_noise = bool(want_noise)
        self.core = PoolCore(self.cfg, self.capacity, want_noise) if core is None else core
        self._free = list(range(self.capacity))  # kept sorted: the lowest slot goes first
        self._streams = {}
        self._next = 0

    def __len__(self):
        return len(self._streams)

    def merged(self, overrides=None):
        """The pool's params with ``overrides`` over them, and their Config."""
        over = dict(overrides or {})
        cfg = self.cfg
        _, _, names = ALGOS[cfg.algorithm]
        takes = set(names) | set(DEFAULTS.get(cfg.algorithm, {})) | set(self.params)
        if cfg.algo >= _lib.ALGO["MMSE"]:
            takes.add("noise_mu")
        for key, value in over.items():
            if key in self.SHAPE:
                if value != self.params[key]:
                    raise ValueError(f"online: {key}={value!r} is fixed by the pool "
                                     f"({self.params[key]!r})")
            elif key not in takes and not key.startswith(cfg.method + "_"):
                raise TypeError(f"online: {cfg.algorithm} with {cfg.method} takes no "
                                f"parameter {key!r}")
        params = dict(self.params, **over)
        return params, config(self.algorithm, params)

    def open(self, overrides=None):
        _, cfg = self.merged(overrides)
        if not self._free:
            raise RuntimeError(f"online: the pool is full ({self.capacity} streams)")
        sid, self._next = self._next, self._next + 1
        self._streams[sid] = _PoolStream(cfg, self._free.pop(0))
        return sid

    def _get(self, sid):
        if sid not in self._streams:
            raise KeyError(f"online: no open stream {sid!r}")
        return self._streams[sid]

    def feed(self, sid, block):
        x = np.asarray(block, dtype=np.float64)
        if x.ndim != 1:
            raise ValueError(f"online: block of shape {x.shape} for one stream")
        self._get(sid).host.feed(x[None, :])

    def step(self, max_frames=None):
        if max_frames is not None and (max_frames != int(max_frames) or int(max_frames) < 1):
            raise ValueError(f"online: max_frames={max_frames} not an integer >= 1")
        run = [(sid, st, st.host.ready(max_frames)) for sid, st in self._streams.items()]
        return self._run([r for r in run if r[2] > 0])

    def close(self, sid):
        st = self._get(sid)
        st.host.end()  # raises, with the stream as it was, for an input that cannot finish
        k = st.host.ready()
        y, rows = self._run([(sid, st, k)] if k else [], always=sid)[sid]
        if st.opened:
            tail = self.core.close(st.slot)
            y = np.concatenate([y, st.host.emitted(tail[None, :])[0]])
        assert st.host.returned == st.host.n_in, (st.host.returned, st.host.n_in)
        self._release(sid)
        return (y, rows) if self.want_noise else y

    def drop(self, sid):
        st = self._get(sid)
        if st.opened:
            self.core.drop(st.slot)
        self._release(sid)

    def _release(self, sid):
        slot = self._streams.pop(sid).slot
        self._free.append(slot)
        self._free.sort()

    def _run(self, run, always=None):
        """One step of the core for ``run`` = [(sid, stream, k)], after the open
        of every stream it runs for the first time."""
        bins = self.cfg.bins
        outs = {}
        if always is not None:
            outs[always] = (np.zeros(0, dtype=np.float32), np.zeros((0, bins), dtype=np.float32))
        if not run:
            return outs
        for _, st, _ in run:
            head = st.host.head()
            if head is not None:
                self.core.open(st.slot, st.cfg, head[0])
                st.opened = True
        hop = self.cfg.hop
        x = np.concatenate([st.host.take(k)[0] for _, st, k in run])
        y, rows = self.core.step([(st.slot, k) for _, st, k in run], x)
        at = 0
        for sid, st, k in run:
            ys = st.host.emitted(y[None, at * hop:(at + k) * hop])[0]
            rs = rows[at:at + k] if rows is not None else np.zeros((0, bins), dtype=np.float32)
            outs[sid] = (ys, rs)
            at += k
        if always is None and not self.want_noise:
            outs = {sid: o[0] for sid, o in outs.items()}
        return outs


