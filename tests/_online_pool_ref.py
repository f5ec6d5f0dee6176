"""fp64 restatement of include/cse_online_pool.h as a core with the methods
OnlinePool drives (open, step, close, drop): every slot is one
tests/_online_ref._Stream with the parameter values it was opened with.  It
refuses what cse_pool_open / step / close / drop refuse, and counts its calls
so that a test can see what the pool asked of it."""

import functools

import numpy as np

from _online_cases import clip, params_for, run
from _online_ref import RefCore, _Stream

# the second parameter set of a pool's streams, over _online_cases.params_for's
ALT = {
    "mcra": dict(alpha=0.9, gain_floor=0.1, mcra_window_frames=5, mcra_alpha_d=0.85,
                 mcra_delta=3.0),
    "spp": dict(alpha=0.95, q=0.3, noise_mu=0.9, gain_floor=0.05, ksi_min=0.01,
                spp_init_frames=4, spp_alpha_pow=0.8),
}
MARGIN = 1e-9   # cse_spp.h's |pm - ph_max|; for mcra |S - delta Smin| / S


def merged(alg, method, n_fft, hop, alt):
    """BASE = params_for(...), or ALT[method] over it."""
    base = params_for(alg, method, n_fft, hop)
    return dict(base, **ALT[method]) if alt else base


@functools.lru_cache(maxsize=None)
def enhancer_reference(alg, method, n_fft, hop, alt, length, seed):
    """OnlineEnhancer over the fp64 restatement on the whole clip(length,
    seed): (samples, rows, the tracker's margin).  Shared: do not write to it."""
    from classical_speech_enhancement_amd import online
    params = merged(alg, method, n_fft, hop, alt)
    core = RefCore(online.config(alg, params), 1)
    y, rows = run(online.OnlineEnhancer(alg, params, want_noise=True, core=core),
                  clip(length, seed), [])
    margin = core.margins()[0]
    print(f"{alg} {method} {n_fft}/{hop} {'ALT' if alt else 'BASE'} seed {seed}: "
          f"margin {margin:.3e}")
    y.setflags(write=False)
    rows.setflags(write=False)
    return y, rows, margin


class RefPoolCore:
    def __init__(self, cfg, capacity, want_noise=True):
        self.cfg, self.capacity = cfg, capacity
        self.slots = [None] * capacity
        self.calls = {"open": 0, "step": 0, "close": 0, "drop": 0}
        self.used = set()         # every slot that was ever opened
        self.items = []           # the (slot, k) list of every step
        self.margins = {}         # slot -> the tracker margins of the streams it has held

    def _slot(self, slot, want_open):
        assert 0 <= slot < self.capacity, slot
        assert (self.slots[slot] is not None) == want_open, (slot, want_open)

    def open(self, slot, cfg, head):
        self._slot(slot, False)
        assert (cfg.n_fft, cfg.hop, cfg.algo, cfg.method) == (
            self.cfg.n_fft, self.cfg.hop, self.cfg.algo, self.cfg.method)
        assert head.shape == (cfg.n_fft - cfg.hop,)
        self.calls["open"] += 1
        self.used.add(slot)
        self.slots[slot] = _Stream(cfg, head)

    def step(self, items, x):
        self.calls["step"] += 1
        self.items.append(list(items))
        assert len(items) > 0 and len({s for s, _ in items}) == len(items)
        hop = self.cfg.hop
        assert x.shape == (hop * sum(k for _, k in items),)
        ys, rows, at = [], [], 0
        for slot, k in items:
            self._slot(slot, True)
            st = self.slots[slot]
            assert k >= (st.cfg.first_frames if st.t == 0 else 1)
            y, r = st.push(x[at * hop:(at + k) * hop])
            ys.append(y)
            rows.append(r)
            at += k
        return np.concatenate(ys), np.concatenate(rows)

    def _retire(self, slot):
        st, self.slots[slot] = self.slots[slot], None
        self.margins.setdefault(slot, []).append(st.tracker.margin)
        return st

    def close(self, slot):
        self._slot(slot, True)
        self.calls["close"] += 1
        st = self._retire(slot)
        return st.retire(self.cfg.n_fft - self.cfg.hop)

    def drop(self, slot):
        self._slot(slot, True)
        self.calls["drop"] += 1
        self._retire(slot)
