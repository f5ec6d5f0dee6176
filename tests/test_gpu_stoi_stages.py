"""Every stage of csrc/cse_stoi.hip against the long-double reference of
tests/_stoi_cases.py, per element (needs a GPU).

test_gpu_stoi.py and test_gpu_estoi.py see the kernels through one number per
signal, |STOI_dev - STOI_oracle| <= 1e-8, which a whole frame row wrong by
1e-4 passes.  Here the stages are read back (StoiPlan.stages(),
cell_envelopes(), cell_y10()) and every element of every row < M and band < 15
is held to the bound _stoi_cases.py derives for it: the filter tables, the
clean side's 10-kHz signal, frame energies, kept frames and meta (exact), the
block tables (exact), the clean envelopes, the segment and column statistics,
the cells' envelopes through all four cell kernels, the cells' 10-kHz signals
at other rates, and both phase-B forms in isolation (the device's score
against the long-double phase B of the device's own envelopes).  Each test
prints its worst error / bound and where it occurs.  tests/
test_stoi_cases_host.py proves the conditions this file relies on.
"""

import functools

import numpy as np
import pytest

import _stoi_cases as C

pytestmark = pytest.mark.gpu
LD = C.LD
GATED = [n for n in C.NAMES if n != "none"]


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from classical_speech_enhancement_amd import metrics
    return metrics


def _report(what, frac, where=()):
    print(f"[stoi-stage] {what}: worst error / bound {frac:.3g} at {where}")
    return frac


def _fold(worst, what, f, at):
    """Hold one cell's error / bound to 1 and keep the largest.  A NaN (which
    C.worst reports as inf) fails here: it must not vanish in a max()."""
    assert np.isfinite(f) and f <= 1.0, (what, f, at)
    return max(worst, (f, at))


_DEVICE_ERROR = []


def _run(key, sr, extended):
    """_launch, once per case; after a device error nothing more is launched."""
    if _DEVICE_ERROR:
        pytest.fail(f"not run: an earlier case ended in a device error ({_DEVICE_ERROR[0]!r})")
    try:
        return _launch(key, sr, extended)
    except Exception as e:
        _DEVICE_ERROR.append(e)
        raise


@functools.lru_cache(maxsize=None)
def _launch(key, sr, extended):
    """Prepare the clean side of a case and score its cells; everything read
    back once: the stages, and per cell the score, envelopes and (other rates)
    the 10-kHz signal."""
    import torch
    from classical_speech_enhancement_amd import metrics
    clean, cells = _case(key, sr)
    clean = np.atleast_2d(clean)
    n = clean.shape[1]
    plan = metrics.StoiPlan(torch.as_tensor(clean).cuda(), sr, extended=extended)
    torch.cuda.synchronize()
    st = {k: (v.cpu().numpy().copy() if torch.is_tensor(v) else v) for k, v in plan.stages().items()}
    flat, offs = C.pack([c[0] for c in cells], n)
    yd = torch.as_tensor(flat).cuda()
    out = np.zeros(len(cells))
    env = [None] * len(cells)
    y10 = [None] * len(cells)
    for clip in (False, True):
        ids = [i for i, c in enumerate(cells) if c[2] == clip]
        if not ids:
            continue
        # every byte 0xff: a row the kernel does not write reads back as NaN,
        # not as what an earlier plan of the same sizes left in the block
        plan._scratch_for(len(ids)).fill_(0xFF)
        got = plan.score(yd, offs[ids], [cells[i][3] for i in ids], lag=[cells[i][1] for i in ids],
                         clip=clip)
        e = plan.cell_envelopes(len(ids)).cpu().numpy().copy()
        t = plan.cell_y10(len(ids)).cpu().numpy().copy() if sr != 16000 else None
        for k, i in enumerate(ids):
            out[i], env[i] = got[k], e[k]
            y10[i] = None if t is None else t[k]
    return dict(stages=st, out=out, env=env, y10=y10, cells=cells, clean=clean)


def _case(key, sr):
    """(clean [S, n] or [n], cells [(f32 y, lag, clip, sig)])."""
    if sr != 16000:
        return C.rate_clean(sr, key), [(y, lag, clip, 0) for y, lag, clip in C.rate_cells(sr, key)]
    if key == "pair":
        clean = C.pair_clean()
        n = clean.shape[1]
        cells = []
        for k in range(5):
            sig = (k + 1) % 2  # 1, 0, 1, ...
            name = ("steady", "bursts")[sig]
            tag, y, clip = C.tests_of(name)[k % 3]
            cells.append((np.concatenate([y, np.zeros(n - len(y), dtype=np.float32)]),
                          (0, 7, -203, 1, -7)[k], clip, sig))
        return clean, cells
    if key.startswith("lag:"):
        name = key[4:]
        tag, y, clip = C.tests_of(name)[0]
        return C.clean_of(name), [(y, lag, clip, 0) for lag in C.lags_of(len(y))]
    return C.clean_of(key), [(y, 0, clip, 0) for tag, y, clip in C.tests_of(key)]


@functools.lru_cache(maxsize=None)
def _ref(key, sr=16000, sig=0):
    clean, _ = _case(key, sr)
    return C.clean_side(np.atleast_2d(clean)[sig], sr)


@functools.lru_cache(maxsize=None)
def _cell_ref(key, sr, c):
    y, lag, clip, sig = _case(key, sr)[1][c]
    return C.cell_side(_ref(key, sr, sig), y, lag, clip, sr)


# ---------------------------------------------------------------- the tables
def test_coef(dev):
    """stoi_coef_kernel's [5][128] polyphase table: |dc| <= E_c max |c|, and
    exact zeros outside each phase's tap span and at kk >= 123."""
    got = _run("steady", 16000, False)["stages"]["coef"]
    ref = C.coef16()
    w = C.window_oct(5, 8)
    r, kk = np.arange(5)[:, None], np.arange(C.CST)[None, :]
    outside = (kk >= C.KN) | (np.abs(8 * r - 5 * (kk + C.KLO)) > w.half)
    assert not got[outside].any() and not ref[outside].any()
    assert np.array_equal(got == 0, ref == 0)  # and the sinc's zeros, 8 | (8 r - 5 k)
    f, at = C.worst(np.abs(got - ref).astype(np.float64), w.e_c * float(np.abs(ref).max()))
    assert _report("coef", f, at) <= 1.0


@pytest.mark.parametrize("sr", C.RATES)
def test_hgen(dev, sr):
    got = _run("steady", sr, False)["stages"]["hgen"]
    w = C.window_oct(*C.ratio(sr))
    assert got.shape == w.h.shape
    if sr == 10000:
        assert got[0] == 1.0
        return
    f, at = C.worst(np.abs(got - w.h).astype(np.float64), w.e_c * float(np.abs(w.h).max()))
    assert _report(f"hgen {sr}", f, at) <= 1.0


# ------------------------------------------------------------ the clean side
def _clean_keys():
    keys = [(n, 16000, 0) for n in C.NAMES] + [("pair", 16000, 0), ("pair", 16000, 1)]
    return keys + [(k, sr, 0) for sr in C.RATES for k in C.RATE_GATES]


CLEAN_KEYS = _clean_keys()
_ids = [f"{k}-{sr}-{s}" for k, sr, s in CLEAN_KEYS]


@pytest.mark.parametrize("key,sr,sig", CLEAN_KEYS, ids=_ids)
def test_x10(dev, key, sr, sig):
    got = _run(key, sr, False)["stages"]["x10"][sig]
    r = _ref(key, sr, sig)
    assert got.shape == r.x10.shape
    f, at = C.worst(np.abs(got - r.x10).astype(np.float64), r.d10)
    assert _report(f"x10 {key} {sr}", f, at) <= 1.0


@pytest.mark.parametrize("key,sr,sig", CLEAN_KEYS, ids=_ids)
def test_energy_mask_meta(dev, key, sr, sig):
    st = _run(key, sr, False)["stages"]
    r = _ref(key, sr, sig)
    meta = st["meta"][sig]
    assert list(meta[:5]) == [r.K, r.M, r.J, 1 if r.F else 0, len(r.blocks)]
    assert st["en"].shape[1] == r.F
    assert np.array_equal(st["kf"][sig][:r.K], r.kf)
    f, at = C.worst(np.abs(st["en"][sig] - r.en).astype(np.float64), r.en_bound)
    assert _report(f"en {key} {sr}", f, at) <= 1.0


@pytest.mark.parametrize("key,sr,sig", CLEAN_KEYS, ids=_ids)
def test_btab(dev, key, sr, sig):
    st = _run(key, sr, False)["stages"]
    r = _ref(key, sr, sig)
    assert len(r.blocks) <= st["layout"]["NBLK"]
    for i, b in enumerate(r.blocks):
        want = C.block_row(b)
        got = st["btab"][sig][i]
        spec = want != -9
        assert np.array_equal(got[spec], want[spec]), (i, got, want)


@pytest.mark.parametrize("key,sr,sig", CLEAN_KEYS, ids=_ids)
def test_xtob(dev, key, sr, sig):
    got = _run(key, sr, False)["stages"]["xtob"][sig]
    r = _ref(key, sr, sig)
    f, at = C.worst(np.abs(got[:r.M, :15] - r.env).astype(np.float64), r.env_bound[:, None])
    assert _report(f"xtob {key} {sr}", f, at) <= 1.0


@pytest.mark.parametrize("key,sr,sig", CLEAN_KEYS, ids=_ids)
def test_xtob_from_device_x10(dev, key, sr, sig):
    """The transform alone: xtob against the long-double envelopes of the
    device's own x10, so the resampler's bound (which adds the coefficients'
    E_c coherently over its taps and dwarfs E_FFT) is out of the comparison:
    E_FFT U_f and the 11 u of the window products remain."""
    st = _run(key, sr, False)["stages"]
    r = _ref(key, sr, sig)
    x10 = st["x10"][sig].astype(LD)
    env, Uf, bound = C.envelopes(x10, np.zeros(len(x10)), r.kf)
    f, at = C.worst(np.abs(st["xtob"][sig][:r.M, :15] - env).astype(np.float64), bound[:, None])
    assert _report(f"xtob|x10 {key} {sr}", f, at) <= 1.0


@pytest.mark.parametrize("key,sr", [(k, sr) for sr in C.RATES for k in C.RATE_GATES])
def test_cell_envelopes_from_device_y10(dev, key, sr):
    """The same for the cells at other rates, whose 10-kHz signals are read
    back: the 10-kHz cell kernels' transform against E_FFT U_f alone."""
    run = _run(key, sr, False)
    r = _ref(key, sr, 0)
    if r.J == 0:  # the kernels return before phase A
        return
    worst = (0.0, ())
    for c, (y, lag, clip, sig) in enumerate(run["cells"]):
        y10 = run["y10"][c].astype(LD)
        env, Uf, bound = C.envelopes(y10, np.zeros(len(y10)), r.kf)
        f, at = C.worst(np.abs(run["env"][c][:r.M, :15] - env).astype(np.float64), bound[:, None])
        worst = _fold(worst, "cell env|y10", f, (c, lag) + at)
    assert _report(f"cell env|y10 {key} {sr}", *worst) <= 1.0


@pytest.mark.parametrize("key,sr,sig", CLEAN_KEYS, ids=_ids)
def test_xstat_xcol(dev, key, sr, sig):
    """The statistics against the long-double ones of the device's own xtob:
    norm and mean within gamma_30, the inverses within gamma_30 (1 + kappa);
    xcol from the device's own xstat, its mean within gamma_30 of the mean
    magnitude."""
    st = _run(key, sr, True)["stages"]
    r = _ref(key, sr, sig)
    if r.J == 0:
        return
    g30 = C.gamma(30)
    xt = st["xtob"][sig][:r.M, :15]
    norm, mean, inv, kap = C.segment_stats(xt)
    got = st["xstat"][sig][:r.J, :15]
    fr = [C.worst(np.abs(got[..., 0] - norm).astype(np.float64), g30 * norm.astype(np.float64)),
          C.worst(np.abs(got[..., 1] - mean).astype(np.float64), g30 * mean.astype(np.float64)),
          C.worst(np.abs(got[..., 2] - inv).astype(np.float64), g30 * (1 + kap) * inv.astype(np.float64))]
    cm, ci, kc, mag = C.column_stats(xt, got[..., 1].astype(LD), got[..., 2].astype(LD))
    gc = st["xcol"][sig][:r.J]
    fr += [C.worst(np.abs(gc[..., 0] - cm).astype(np.float64), g30 * mag),
           C.worst(np.abs(gc[..., 1] - ci).astype(np.float64), g30 * (1 + kc) * ci.astype(np.float64))]
    for what, (f, at) in zip(("norm", "mean", "inv", "col mean", "col inv"), fr):
        _report(f"xstat {what} {key} {sr}", f, at)
    assert all(np.isfinite(f) and f <= 1.0 for f, _ in fr), fr
    assert np.array_equal(st["xstat"][sig][:r.J, :15, 3], np.zeros((r.J, 15)))


# ------------------------------------------------------------------ the cells
CELL_KEYS = [(n, 16000) for n in GATED] + [("pair", 16000)] + \
    [(f"lag:{n}", 16000) for n in C.LAG_DESIGNS] + \
    [(k, sr) for sr in C.RATES for k in C.RATE_GATES]
_cids = [f"{k}-{sr}" for k, sr in CELL_KEYS]


@pytest.mark.parametrize("extended", [False, True], ids=["stoi", "estoi"])
@pytest.mark.parametrize("key,sr", CELL_KEYS, ids=_cids)
def test_cell_envelopes(dev, key, sr, extended):
    """cse_stoi_cells / cse_estoi_cells (16 kHz), cse_stoi_cells_sr /
    cse_estoi_cells (other rates): every cell's envelope rows < M."""
    run = _run(key, sr, extended)
    worst = (0.0, ())
    for c, (y, lag, clip, sig) in enumerate(run["cells"]):
        r = _ref(key, sr, sig)
        if r.J == 0:  # the kernels return before phase A
            continue
        cell = _cell_ref(key, sr, c)
        f, at = C.worst(np.abs(run["env"][c][:r.M, :15] - cell.env).astype(np.float64),
                        cell.env_bound[:, None])
        if not cell.env.any():
            assert not run["env"][c][:r.M, :15].any()
        worst = _fold(worst, "cell env", f, (c, lag) + at)
    assert _report(f"cell env {key} {sr} ext={extended}", *worst) <= 1.0


@pytest.mark.parametrize("key,sr", [(k, sr) for sr in C.RATES for k in C.RATE_GATES])
def test_cell_y10(dev, key, sr):
    run = _run(key, sr, False)
    worst = (0.0, ())
    for c, (y, lag, clip, sig) in enumerate(run["cells"]):
        cell = _cell_ref(key, sr, c)
        f, at = C.worst(np.abs(run["y10"][c] - cell.y10).astype(np.float64), cell.d10)
        if sr == 10000:
            assert np.array_equal(run["y10"][c], cell.y10.astype(np.float64))
        worst = _fold(worst, "cell y10", f, (c, lag) + at)
    assert _report(f"cell y10 {key} {sr}", *worst) <= 1.0


@pytest.mark.parametrize("extended", [False, True], ids=["stoi", "estoi"])
@pytest.mark.parametrize("key,sr", [k for k in CELL_KEYS if k[0] != "j0"],
                         ids=[i for i, k in zip(_cids, CELL_KEYS) if k[0] != "j0"])
def test_phase_b_isolated(dev, key, sr, extended):
    """The device's score against the long-double phase B of the device's own
    envelopes: E_B (1 + kappa_max), and E_BE (1 + kappa_r)(1 + lam) for the
    extended form.  A test signal that leaves nothing scores exactly 0."""
    run = _run(key, sr, extended)
    worst = (0.0, ())
    for c, (y, lag, clip, sig) in enumerate(run["cells"]):
        r = _ref(key, sr, sig)
        if r.J == 0:
            continue
        M = int(run["stages"]["meta"][sig][1])
        xt = run["stages"]["xtob"][sig][:M, :15]
        ye = run["env"][c][:M, :15]
        if not ye.any():
            assert run["out"][c] == 0.0, (c, lag)
            continue
        if extended:
            d, kr, lam, _ = C.estoi_b(xt, ye)
            bound = C.E_BE * (1 + kr) * (1 + lam)
        else:
            d, k = C.stoi_b(xt, ye)
            bound = C.E_B * (1 + k)
        f = abs(float(LD(run["out"][c]) - d)) / bound
        assert np.isfinite(run["out"][c]) and np.isfinite(float(d)), (c, lag, run["out"][c], d)
        worst = _fold(worst, "phase B", f, (c, lag))
    assert _report(f"phase B {key} {sr} ext={extended}", *worst) <= 1.0


@pytest.mark.parametrize("extended", [False, True], ids=["stoi", "estoi"])
def test_special_results(dev, extended):
    """Fewer than 30 frames: exactly 1e-5; no frame: NaN; a zero test signal
    and lags that leave nothing in reach of an envelope: exactly 0."""
    assert np.all(_run("j0", 16000, extended)["out"] == 1e-5)
    assert np.all(np.isnan(_run("none", 16000, extended)["out"]))
    run = _run("steady", 16000, extended)
    zero = [t for t, _, _ in C.tests_of("steady")].index("zero")
    assert run["out"][zero] == 0.0
    run = _run("lag:steady", 16000, extended)
    n = run["clean"].shape[1]
    # nothing left, or one sample in the last 230, which reach no envelope
    gone = [c for c in range(len(run["cells"])) if not _cell_ref("lag:steady", 16000, c).env.any()]
    assert {c for c, cell in enumerate(run["cells"]) if abs(cell[1]) >= n} <= set(gone)
    assert 3 <= len(gone) <= 4 and all(run["out"][c] == 0.0 for c in gone)
    assert all(run["out"][c] != 0.0 for c in range(len(run["cells"])) if c not in gone)
