"""The pool of online streams on the device (include/cse_online_pool.h): a
stream's company, pace and slot are invisible bit for bit; every slot is the
offline plugin with its own parameter values, and its tracked rows are
cse_noise_<method>'s; the pool agrees with the lockstep enhancer; a reused slot
is a fresh stream; and the ABI refuses what the header says it refuses before
any launch.  Clips are one second."""

import ctypes
import functools

import numpy as np
import pytest
import torch

from _online_cases import clip, run
from _online_pool_ref import ALT, MARGIN, enhancer_reference, merged
from classical_speech_enhancement_amd import _lib, online, plugins
from conftest import rel_l2, rel_max

pytestmark = pytest.mark.gpu

LENGTH = 16000 + 37
PLUGINS = {"spectralSubtractor": plugins.spectral_subtraction, "wiener": plugins.wiener_filter,
           "mmse": plugins.mmse, "omlsa": plugins.advanced_mmse}
# per pool: its streams in the order they open, (seed, ALT?, frames fed per
# round, the round it opens in).  Stream A is seed 0: third to open, so slot 2,
# beside a stream that gets 1 frame per round and one that gets 3 while A gets
# 8; seed 3 opens in round 5, so that step runs a slot's first frame beside
# slots in mid-stream.
COMPANY = [(1, True, 1, 0), (2, False, 3, 0), (0, False, 8, 0), (3, True, 2, 5)]
POOLS = {
    ("wiener", "mcra", 512, 128): COMPANY,   # mcra_window_frames 8 and 5
    ("omlsa", "spp", 512, 128): COMPANY,     # spp_init_frames 6 and 4
    ("wiener", "mcra", 128, 32): COMPANY,
    ("mmse", "mcra", 2048, 512): [(0, False, 2, 0), (1, False, 1, 0)],
}
STREAMS = [(*shape, seed, alt) for shape, streams in POOLS.items() for seed, alt, _, _ in streams]


def split(params, method):
    """A merged params dict -> the plugin's keyword arguments and the tracker's."""
    prefix = method + "_"
    tracker = {k[len(prefix):]: v for k, v in params.items() if k.startswith(prefix)}
    rest = {k: v for k, v in params.items() if not k.startswith(prefix)}
    return rest, tracker


def alone(alg, method, n_fft, hop, seed, alt, capacity=1):
    """The stream fed whole, the only one of its pool, in slot 0."""
    pool = online.OnlinePool(alg, merged(alg, method, n_fft, hop, False), capacity=capacity,
                             want_noise=True)
    sid = pool.open(ALT[method] if alt else None)
    pool.feed(sid, clip(LENGTH, seed))
    out = pool.step()[sid]
    rest = pool.close(sid)
    return np.concatenate([out[0], rest[0]]), np.concatenate([out[1], rest[1]])


@functools.lru_cache(maxsize=None)
def company(alg, method, n_fft, hop):
    """The pool of POOLS[...] run to the end: {seed: (samples, rows)}, what the
    steps carried, and the slot of every stream.  Shared: do not write to it."""
    streams = POOLS[alg, method, n_fft, hop]
    pool = online.OnlinePool(alg, merged(alg, method, n_fft, hop, False), capacity=len(streams),
                             want_noise=True)
    sid, pos, got, slots, steps = {}, {}, {}, {}, []
    done, rnd = set(), 0
    lead = max(streams, key=lambda s: s[2])[0]  # the stream that is through first
    while lead not in done:
        for seed, alt, frames, opens in streams:
            if opens == rnd:
                sid[seed] = pool.open(ALT[method] if alt else None)
                slots[seed] = pool._get(sid[seed]).slot
                pos[seed], got[seed] = 0, ([], [])
                frames = max(frames, 8)  # enough for the first step (init_frames <= 6)
            if seed in sid and seed not in done:
                x = clip(LENGTH, seed)[pos[seed]:pos[seed] + frames * hop]
                pool.feed(sid[seed], x)
                pos[seed] += len(x)
        out = pool.step()
        steps.append({seed: len(out[s][1]) for seed, s in sid.items() if s in out})
        for seed, s in sid.items():
            if s in out:
                got[seed][0].append(out[s][0])
                got[seed][1].append(out[s][1])
        for seed in sid:
            if seed not in done and pos[seed] == LENGTH:
                rest = pool.close(sid[seed])
                got[seed][0].append(rest[0])
                got[seed][1].append(rest[1])
                done.add(seed)
        rnd += 1
    for seed in sid:  # the others: the rest of the clip at once
        if seed not in done:
            pool.feed(sid[seed], clip(LENGTH, seed)[pos[seed]:])
            rest = pool.close(sid[seed])
            got[seed][0].append(rest[0])
            got[seed][1].append(rest[1])
    res = {seed: (np.concatenate(g[0]), np.concatenate(g[1])) for seed, g in got.items()}
    for y, rows in res.values():
        y.setflags(write=False)
        rows.setflags(write=False)
    return res, steps, slots


def margins_hold(alg, method, n_fft, hop, seeds_alts):
    for seed, alt in seeds_alts:
        margin = enhancer_reference(alg, method, n_fft, hop, alt, LENGTH, seed)[2]
        assert margin >= MARGIN, (alg, method, n_fft, hop, seed, alt, margin)


# ------------------------------------- 5. company, pace and slot are invisible
@pytest.mark.parametrize("alg,method,n_fft,hop", [k for k, v in POOLS.items() if v is COMPANY])
def test_company_pace_and_slot_are_invisible_bit_for_bit(alg, method, n_fft, hop):
    margins_hold(alg, method, n_fft, hop, [(s, a) for s, a, _, _ in COMPANY])
    base_y, base_n = alone(alg, method, n_fft, hop, 0, False)
    assert base_y.shape == (LENGTH,) and base_y.dtype == np.float32
    assert base_n.shape == (1 + LENGTH // hop, n_fft // 2 + 1)
    assert np.isfinite(base_y).all() and np.abs(base_y).max() > 1e-3
    res, steps, slots = company(alg, method, n_fft, hop)
    assert slots == {1: 0, 2: 1, 0: 2, 3: 3}  # A is not in slot 0 here
    # single steps carried items of 1, 3 and 8 frames, and a first step beside mid-stream slots
    assert any(sorted(s.values())[:1] == [1] and {1, 3, 8} <= set(s.values()) for s in steps)
    first = next(i for i, s in enumerate(steps) if 3 in s)
    assert first > 0 and len(steps[first]) == 4
    y, rows = res[0]
    assert y.tobytes() == base_y.tobytes() and rows.tobytes() == base_n.tobytes()
    for seed, alt, _, _ in COMPANY:  # and so for the company itself
        ys, rs = alone(alg, method, n_fft, hop, seed, alt)
        assert res[seed][0].tobytes() == ys.tobytes(), seed
        assert res[seed][1].tobytes() == rs.tobytes(), seed
    assert res[1][0].tobytes() != res[2][0].tobytes()


# --------------------------------------- 6. every slot is the offline plugin
@pytest.mark.parametrize("alg,method,n_fft,hop,seed,alt", STREAMS)
def test_every_slot_is_the_offline_plugin_with_its_own_parameters(alg, method, n_fft, hop, seed,
                                                                  alt):
    margins_hold(alg, method, n_fft, hop, [(seed, alt)])
    params = merged(alg, method, n_fft, hop, alt)
    cfg = online.config(alg, params)
    kw, tracker = split(params, method)
    x = clip(LENGTH, seed)
    y, rows = company(alg, method, n_fft, hop)[0][seed]
    want = PLUGINS[alg](x, 16000, noise_percentile=20.0, **kw, **{method: tracker})
    l2, mx = rel_l2(y, want), rel_max(y, want)
    print(f"{alg} {method} {n_fft}/{hop} seed {seed} {'ALT' if alt else 'BASE'}: "
          f"rel-L2 {l2:.3e} rel-max {mx:.3e}")
    assert y.shape == want.shape and l2 <= 1e-5 and mx <= 1e-5
    # the rows: Engine.noise_estimate of the same clip, equal or adjacent f32 values
    eng = plugins.engine()
    _, P = eng.stft(torch.as_tensor(x).cuda().view(1, -1), n_fft, hop, want_y=False)
    N = eng.noise_estimate(method, P, eps=cfg.eps, **tracker)[0].cpu().numpy().astype(np.float64)
    d = np.abs(rows.astype(np.float64) - N)
    print(f"   rows: max |d| / N {np.max(d / N):.3e}, differing {np.mean(d > 0):.2%}")
    assert rows.shape == N.shape and np.all(d <= 2.0 ** -23 * N)


# ------------------------------------------ 7. against the lockstep enhancer
@pytest.mark.parametrize("alg,method,n_fft,hop,seed,alt", STREAMS)
def test_pool_agrees_with_the_lockstep_enhancer(alg, method, n_fft, hop, seed, alt):
    margins_hold(alg, method, n_fft, hop, [(seed, alt)])
    params = merged(alg, method, n_fft, hop, alt)
    y, rows = company(alg, method, n_fft, hop)[0][seed]
    e = online.OnlineEnhancer(alg, params, n_streams=1, want_noise=True)
    want, want_n = run(e, clip(LENGTH, seed), [])
    l2, mx = rel_l2(y, want), rel_max(y, want)
    d = np.abs(rows.astype(np.float64) - want_n.astype(np.float64))
    print(f"{alg} {method} {n_fft}/{hop} seed {seed} {'ALT' if alt else 'BASE'}: "
          f"samples bit-equal {y.tobytes() == want.tobytes()}, rows bit-equal "
          f"{rows.tobytes() == want_n.tobytes()}, rel-L2 {l2:.3e} rel-max {mx:.3e}")
    assert y.shape == want.shape and l2 <= 1e-5 and mx <= 1e-5
    assert rows.shape == want_n.shape and np.all(d <= 2.0 ** -23 * want_n.astype(np.float64))


# ------------------------------------------------ 8. slot reuse on the device
@pytest.mark.parametrize("alg,method", [("wiener", "mcra"), ("omlsa", "spp")])
def test_a_reused_slot_is_a_fresh_stream(alg, method):
    n_fft, hop = 512, 128
    pool = online.OnlinePool(alg, merged(alg, method, n_fft, hop, False), capacity=2,
                             want_noise=True)
    a, b = pool.open(), pool.open(ALT[method])
    pool.feed(a, clip(LENGTH, 0))
    pool.feed(b, clip(LENGTH, 1)[:8000])
    pool.step()
    pool.close(a)
    c = pool.open(ALT[method])  # A's slot, other values, another clip, beside b mid-stream
    assert pool._get(c).slot == 0 and pool._get(b).slot == 1
    pool.feed(c, clip(LENGTH, 2))
    pool.feed(b, clip(LENGTH, 1)[8000:])
    out = pool.step()[c]
    rest = pool.close(c)
    want = alone(alg, method, n_fft, hop, 2, True)
    assert np.concatenate([out[0], rest[0]]).tobytes() == want[0].tobytes()
    assert np.concatenate([out[1], rest[1]]).tobytes() == want[1].tobytes()
    pool.drop(b)  # mid-stream
    d, e = pool.open(), pool.open()
    assert (pool._get(d).slot, pool._get(e).slot) == (0, 1)  # e has the dropped slot
    pool.feed(e, clip(LENGTH, 3))
    out = pool.step()[e]
    rest = pool.close(e)
    want = alone(alg, method, n_fft, hop, 3, False)
    assert np.concatenate([out[0], rest[0]]).tobytes() == want[0].tobytes()
    assert np.concatenate([out[1], rest[1]]).tobytes() == want[1].tobytes()


# ------------------------------------------------------- 9. ABI refusals
def test_abi_refusals_come_before_any_launch():
    lib = _lib.load()
    params = merged("wiener", "spp", 512, 128, False)  # init_frames = 6
    cfg = online.abi_config(online.config("wiener", params))
    ptr, ref = ctypes.c_void_p(256), ctypes.byref  # never dereferenced: refused first
    err = lambda: lib.cse_last_error().decode()  # noqa: E731

    def refused(rc, word):
        assert rc == -1 and word in err(), (rc, err())

    one = lib.cse_online_state_bytes(512, 1)
    assert lib.cse_pool_state_bytes(512, 3) == 3 * lib.cse_pool_state_bytes(512, 1) > 3 * one
    assert lib.cse_pool_state_bytes(512, 1) % 256 == 0
    assert lib.cse_pool_state_bytes(512, 0) == 0 and lib.cse_pool_work_bytes(0) == 0
    assert lib.cse_pool_state_bytes(512, -1) == -1 and lib.cse_pool_work_bytes(-1) == -1
    for n_fft in (64, 400, 4096):
        assert lib.cse_pool_state_bytes(n_fft, 1) == -1
    assert lib.cse_pool_work_bytes(1024) >= 1024 * 24 and lib.cse_pool_work_bytes(3) % 256 == 0

    h = _lib.PoolHandle()
    slots = (_lib.PoolSlot * 3)()
    sl = ctypes.cast(slots, ctypes.c_void_p)
    refused(lib.cse_pool_init(None, ref(cfg), 3, ptr, ptr, sl), "NULL handle")
    refused(lib.cse_pool_init(ref(h), None, 3, ptr, ptr, sl), "NULL handle or configuration")
    refused(lib.cse_pool_init(ref(h), ref(cfg), -1, ptr, ptr, sl), "capacity=-1")
    for args in ((None, ptr, sl), (ptr, None, sl), (ptr, ptr, None)):
        refused(lib.cse_pool_init(ref(h), ref(cfg), 3, *args), "NULL state, work or slots")
    for field, value, word in (("n_fft", 400, "n_fft=400"), ("hop", 160, "hop=160"),
                               ("algo", 4, "algo=4"), ("noise_method", 5, "coupled bins"),
                               ("noise_method", 6, "coupled bins"),
                               ("noise_method", 0, "whole clip"), ("noise_method", 9, "unknown"),
                               ("eps", 0.0, "eps=0")):
        bad = online.abi_config(online.config("wiener", params))
        setattr(bad, field, value)
        refused(lib.cse_pool_init(ref(h), ref(bad), 3, ptr, ptr, sl), "cse_pool_init: ")
        refused(lib.cse_pool_init(ref(h), ref(bad), 3, ptr, ptr, sl), word)
    bad = online.abi_config(online.config("wiener", params))
    bad.spp.ph_max = 1.5
    refused(lib.cse_pool_init(ref(h), ref(bad), 3, ptr, ptr, sl), "cse_pool_init: prior_h1")

    # a live pool of three slots
    state = torch.zeros(int(lib.cse_pool_state_bytes(512, 3)), dtype=torch.uint8, device="cuda")
    work = torch.zeros(int(lib.cse_pool_work_bytes(3)), dtype=torch.uint8, device="cuda")
    sp, wp = ctypes.c_void_p(state.data_ptr()), ctypes.c_void_p(work.data_ptr())
    assert lib.cse_pool_init(ref(h), ref(cfg), 3, sp, wp, sl) == 0, err()
    assert [(s.frames, s.open) for s in slots] == [(0, 0)] * 3
    x = torch.zeros(16 * 128, dtype=torch.float64, device="cuda")
    y = torch.full((16 * 128,), 7.0, dtype=torch.float32, device="cuda")
    xp, yp = ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(y.data_ptr())

    def items(*pairs):
        return (_lib.PoolItem * max(len(pairs), 1))(*[_lib.PoolItem(s, k) for s, k in pairs])

    def step(lst, n=None, h_=h, x_=xp, y_=yp):
        return lib.cse_pool_step(None if h_ is None else ref(h_), lst,
                                 len(lst) if n is None else n, x_, y_, None, None)

    refused(lib.cse_pool_open(None, 0, None, xp, None), "NULL handle or x_head")
    refused(lib.cse_pool_open(ref(h), 0, None, None, None), "NULL handle or x_head")
    refused(lib.cse_pool_open(ref(h), 3, None, xp, None), "slot=3 outside [0, 3)")
    refused(lib.cse_pool_open(ref(h), -1, None, xp, None), "slot=-1 outside")
    prm = online.abi_pool_params(online.config("wiener", params))
    prm.spp.alpha_pow = 1.0
    refused(lib.cse_pool_open(ref(h), 0, ref(prm), xp, None), "cse_pool_open: alpha_pow")
    prm = online.abi_pool_params(online.config("wiener", params))
    prm.mu = float("nan")
    refused(lib.cse_pool_open(ref(h), 0, ref(prm), xp, None), "mu is NaN")
    refused(lib.cse_pool_close(ref(h), 0, yp, None), "slot=0 is not open")
    refused(lib.cse_pool_drop(ref(h), 0), "slot=0 is not open")
    refused(step(items((0, 6))), "slot=0 is not open")
    assert [s.open for s in slots] == [0, 0, 0]

    prm = online.abi_pool_params(online.config("wiener", dict(params, spp_init_frames=4)))
    assert lib.cse_pool_open(ref(h), 0, None, xp, None) == 0, err()      # cfg's: init_frames 6
    assert lib.cse_pool_open(ref(h), 2, ref(prm), xp, None) == 0, err()  # its own: 4
    assert [(s.open, s.first_frames) for s in slots] == [(1, 6), (0, 0), (1, 4)]
    refused(lib.cse_pool_open(ref(h), 0, None, xp, None), "slot=0 is open")
    before = [(s.frames, s.open, s.first_frames) for s in slots]
    refused(step(items((0, 6)), h_=None), "NULL handle, items, x or y")
    refused(step(None, n=1), "NULL handle, items, x or y")
    refused(step(items((0, 6)), x_=None), "NULL handle, items, x or y")
    refused(step(items((0, 6)), y_=None), "NULL handle, items, x or y")
    refused(step(items((0, 6)), n=-1), "n=-1")
    refused(step(items((2, 4), (3, 1))), "item 1: slot=3 outside [0, 3)")
    refused(step(items((2, 4), (-1, 1))), "slot=-1 outside")
    refused(step(items((2, 4), (1, 1))), "item 1: slot=1 is not open")
    refused(step(items((2, 4), (0, 6), (2, 1))), "item 2: slot=2 listed twice")
    refused(step(items((2, 4), (0, 0))), "item 1: k=0 < 1")
    refused(step(items((2, 4), (0, -3))), "k=-3 < 1")
    refused(step(items((2, 4), (0, 5))), "k=5 < init_frames=6 on an spp slot's first step")
    refused(step(items((0, 6), (2, 3))), "item 1: k=3 < init_frames=4")
    refused(step(items((2, 4), (0, (1 << 30) // 128))), "too many frames")
    assert step(items(), n=0) == 0  # an empty list: nothing launched
    torch.cuda.synchronize()
    assert [(s.frames, s.open, s.first_frames) for s in slots] == before
    assert float(y.min()) == 7.0  # nothing ran

    assert step(items((2, 4), (0, 6))) == 0, err()
    assert [s.frames for s in slots] == [6, 0, 4]
    assert step(items((0, 1), (2, 2))) == 0, err()  # later steps: any k >= 1
    assert [s.frames for s in slots] == [7, 0, 6]
    torch.cuda.synchronize()
    assert float(y[:10 * 128].abs().max()) == 0.0  # silence in, silence out
    assert float(y[10 * 128:].min()) == 7.0        # and nothing past the list's frames
    refused(lib.cse_pool_close(ref(h), 0, None, None), "NULL handle or y_tail")
    refused(lib.cse_pool_close(ref(h), 5, yp, None), "slot=5 outside")
    refused(lib.cse_pool_drop(None, 0), "NULL handle")
    refused(lib.cse_pool_drop(ref(h), 3), "slot=3 outside")
    assert lib.cse_pool_close(ref(h), 0, yp, None) == 0, err()
    assert lib.cse_pool_drop(ref(h), 2) == 0, err()
    assert [s.open for s in slots] == [0, 0, 0]
    refused(lib.cse_pool_close(ref(h), 0, yp, None), "slot=0 is not open")
    refused(lib.cse_pool_drop(ref(h), 2), "slot=2 is not open")
    refused(step(items((0, 1))), "slot=0 is not open")
    torch.cuda.synchronize()
    assert float(y[:384].abs().max()) == 0.0
    # a freed slot opens again, from frame 0
    assert lib.cse_pool_open(ref(h), 2, None, xp, None) == 0, err()
    assert (slots[2].frames, slots[2].open, slots[2].first_frames) == (0, 1, 6)
    # no slots: everything is accepted that names none, and nothing is launched
    h0 = _lib.PoolHandle()
    assert lib.cse_pool_init(ref(h0), ref(cfg), 0, None, None, None) == 0, err()
    assert step(items(), n=0, h_=h0) == 0
    refused(step(items((0, 1)), h_=h0), "slot=0 outside [0, 0)")
    refused(lib.cse_pool_open(ref(h0), 0, None, xp, None), "slot=0 outside [0, 0)")
    torch.cuda.synchronize()
