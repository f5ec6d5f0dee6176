"""Minimum-statistics noise tracking, the parts that need no GPU: the numpy
restatement's own properties (tests/_minstat_ref.py, the definition of
include/cse_minstat.h), the two entry points' declarations, exports and
argument checks, and the layout: the parameter tuple, the call list and the
time constants at another frame step."""

import ctypes
import math
import os
import re

import numpy as np
import pytest

import _minstat_ref
from classical_speech_enhancement_amd import _lib, layout, parameter_ranges, search, trackers

HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "cse_minstat.h")
SCALARS = ("alpha_c", "alpha_c_floor", "alpha_max", "alpha_min", "snr_exp", "beta_max", "av",
           "q_eq_min", "q_eq_max")
NAMES = SCALARS + ("slope_q", "slope_max", "sub_windows", "sub_frames")
DEFAULT_VALUES = (0.837, 0.7, 0.98, 0.548, -0.125, 0.894, 2.12, 2.0, 14.0, (0.03, 0.05, 0.06),
                  (8.0, 4.0, 2.0, 1.2), 8, 24)
SIZE = 136


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


@pytest.fixture(scope="module", params=(0, 1, 2))
def stationary(request):
    """(P, N) for 900 frames of stationary exponential power, computed once."""
    P = np.random.default_rng(request.param).exponential(size=(900, 257))
    return P, _minstat_ref.minstat(P)


# ---------------------------------------------------------------- restatement
def test_m_table():
    assert _minstat_ref.m_of(192) == pytest.approx(0.92332623, abs=5e-9)
    assert _minstat_ref.m_of(24) == pytest.approx(0.73206411, abs=5e-9)
    assert _minstat_ref.m_of(12) == pytest.approx(0.63753892, abs=5e-9)
    for d, m in zip(_minstat_ref.TABLE_D, _minstat_ref.TABLE_M):
        assert _minstat_ref.m_of(d) == m
    assert _minstat_ref.m_of(300) == _minstat_ref.m_of(10 ** 6) == 0.94
    ms = [_minstat_ref.m_of(d) for d in range(1, 320)]
    assert all(a <= b for a, b in zip(ms, ms[1:]))


def test_stationary_noise_is_estimated_without_bias(stationary):
    P, N = stationary
    assert N.dtype == np.float32 and N.shape == P.shape
    m = float(N[216:].mean())
    print("mean of N[216:]:", m)
    assert 0.9 <= m <= 1.1


def test_a_rise_is_followed_after_the_window(stationary):
    """x100 from frame 300 on: the estimate stays down while the window of
    D = 192 frames still holds minima from before the rise and is up one
    sub-window later."""
    P, _ = stationary
    up = P.copy()
    up[300:] *= 100.0
    N = _minstat_ref.minstat(up)
    before, after = float(N[492].mean()), float(N[516].mean())
    print("frame means at 492 and 516:", before, after)
    assert before <= 1.3
    assert after >= 70.0


def test_a_fall_is_followed_at_once(stationary):
    P, _ = stationary
    dn = P.copy()
    dn[300:] *= 0.01
    N = _minstat_ref.minstat(dn)
    m = float(N[324].mean())
    print("frame mean at 324:", m)
    assert m <= 0.02


@pytest.mark.parametrize("eps", (1e-10, 1e-12))
def test_zero_power_returns_eps(eps):
    N = _minstat_ref.minstat(np.zeros((130, 33)), eps)
    assert N.dtype == np.float32 and np.array_equal(N, np.full((130, 33), np.float32(eps)))


def test_zero_bin_and_zero_frames_stay_finite():
    P = np.random.default_rng(3).exponential(size=(200, 65))
    P[:, 5] = 0.0
    P[60:100] = 0.0
    N = _minstat_ref.minstat(P)
    assert np.isfinite(N).all() and (N >= np.float32(1e-10)).all()
    assert np.array_equal(N[:, 5], np.full(200, np.float32(1e-10)))


def test_stats_keys_and_shapes():
    t = np.arange(26)[:, None]
    P = np.random.default_rng(26).exponential(size=(26, 257)) * np.where(t < 13, 1, 100)
    st = {}
    N = _minstat_ref.minstat(P, stats=st, sub_windows=3, sub_frames=4)
    assert set(st) == {"margin", "lmin", "kmod"}
    assert st["margin"] >= 1e-9 and st["lmin"] >= 1 and st["kmod"] >= 257
    st3 = {}
    N3 = _minstat_ref.minstat(np.stack([P, 2.0 * P, P]), stats=st3, sub_windows=3, sub_frames=4)
    assert N3.shape == (3, 26, 257) and set(st3) == set(st)
    assert np.array_equal(N3[0], N) and np.array_equal(N3[2], N)
    assert st3["kmod"] >= 3 * 257 and st3["lmin"] >= 2 * st["lmin"]
    # T = 1: the store branch only; the output is the first frame
    st1 = {}
    N1 = _minstat_ref.minstat(P[:1], stats=st1)
    assert st1["lmin"] == 0 and st1["kmod"] == 257
    np.testing.assert_array_equal(N1[0], P[0].astype(np.float32))
    with pytest.raises(TypeError):
        _minstat_ref.minstat(P, window_frames=3)
    assert _minstat_ref.DEFAULTS == layout.MINSTAT_DEFAULTS


# ------------------------------------------------------------------------ ABI
def test_header_declares_the_exports(lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = set(re.findall(r"\b(cse_[a-z0-9_]+)\s*\(", text))
    assert names == set(_lib.EXPORTS_MINSTAT) == {"cse_minstat_default_params",
                                                  "cse_noise_minstat"}
    assert '#include "cse.h"' in text
    assert not set(_lib.EXPORTS_MINSTAT) & (set(_lib.EXPORTS) | set(_lib.EXPORTS_ESTOI) |
                                            set(_lib.EXPORTS_MCRA) | set(_lib.EXPORTS_SEGSNR) |
                                            set(_lib.EXPORTS_SPP))
    for n in _lib.EXPORTS_MINSTAT:
        assert hasattr(lib, n), n
    assert lib.cse_version() == _lib.ABI_VERSION == 5
    assert _lib.NOISE["minstat"] == 5 and "#define CSE_NOISE_MINSTAT 5" in text


def _as_tuple(prm):
    return tuple(getattr(prm, n) for n in SCALARS) + (
        tuple(prm.slope_q), tuple(prm.slope_max), prm.sub_windows, prm.sub_frames)


def test_struct_size_and_defaults(lib):
    assert ctypes.sizeof(_lib.MinstatParams) == SIZE
    assert [f[0] for f in _lib.MinstatParams._fields_] == list(NAMES)
    assert "} cse_minstat_params_t; /* 136 bytes */" in open(HEADER).read()
    # the C struct's size: default_params fills a guarded buffer of 136 bytes exactly
    buf = (ctypes.c_ubyte * (SIZE + 8))(*([0xAB] * (SIZE + 8)))
    lib.cse_minstat_default_params(ctypes.byref(buf))
    assert bytes(buf[SIZE:]) == b"\xab" * 8
    assert b"\xab" * 4 not in bytes(buf[:SIZE])
    got = _as_tuple(_lib.MinstatParams.from_buffer_copy(bytes(buf[:SIZE])))
    assert got == DEFAULT_VALUES
    assert got == tuple(layout.MINSTAT_DEFAULTS[k] for k in NAMES) == layout.minstat_values({})
    assert got == tuple(_minstat_ref.DEFAULTS[k] for k in NAMES)
    assert bytes(layout.minstat_params(layout.minstat_values({}))) == bytes(buf[:SIZE])
    lib.cse_minstat_default_params(None)  # ignored


def _call(lib, P=16, n_sig=0, T=10, B=257, prm="default", eps=1e-10, N=16, **fields):
    """cse_noise_minstat with n_sig = 0 by default: every check runs, nothing
    is launched."""
    if prm == "default":
        prm = _lib.MinstatParams()
        lib.cse_minstat_default_params(ctypes.byref(prm))
        for k, v in fields.items():
            if isinstance(v, tuple):
                getattr(prm, k)[:] = v
            else:
                setattr(prm, k, v)
        prm = ctypes.byref(prm)
    return lib.cse_noise_minstat(ctypes.c_void_p(P) if P else None, n_sig, T, B, prm, eps,
                                 ctypes.c_void_p(N) if N else None, None)


NAN, INF = math.nan, math.inf
BAD_FIELDS = [
    dict(alpha_c=-1e-9), dict(alpha_c=1.0), dict(alpha_c=NAN), dict(alpha_c_floor=-0.1),
    dict(alpha_c_floor=1.0), dict(alpha_c_floor=NAN), dict(alpha_min=-0.1), dict(alpha_min=1.0),
    dict(alpha_min=NAN), dict(beta_max=-0.1), dict(beta_max=1.0), dict(beta_max=NAN),
    dict(alpha_max=0.0), dict(alpha_max=1.0), dict(alpha_max=NAN), dict(snr_exp=1e-9),
    dict(snr_exp=-INF), dict(snr_exp=NAN), dict(av=-1e-9), dict(av=INF), dict(av=NAN),
    dict(q_eq_min=1.99), dict(q_eq_min=NAN), dict(q_eq_min=15.0), dict(q_eq_max=INF),
    dict(q_eq_max=NAN), dict(q_eq_max=1.0), dict(slope_q=(0.0, 0.05, 0.06)),
    dict(slope_q=(0.03, 0.03, 0.06)), dict(slope_q=(0.03, 0.07, 0.06)),
    dict(slope_q=(0.03, 0.05, INF)), dict(slope_q=(NAN, 0.05, 0.06)),
    dict(slope_q=(0.03, 0.05, NAN)), dict(slope_max=(8.0, 4.0, 2.0, 0.99)),
    dict(slope_max=(INF, 4.0, 2.0, 1.2)), dict(slope_max=(8.0, NAN, 2.0, 1.2)),
    dict(sub_windows=0), dict(sub_windows=17), dict(sub_windows=-1), dict(sub_frames=1),
    dict(sub_frames=2 ** 20 + 1), dict(sub_frames=-5)]
_ids = lambda d: "-".join(f"{k}={v}" for k, v in d.items())  # noqa: E731


@pytest.mark.parametrize("bad", [dict(P=None), dict(N=None), dict(prm=None), dict(n_sig=-1),
                                 dict(T=0), dict(B=32), dict(B=2050)] + BAD_FIELDS, ids=_ids)
def test_argument_checks(lib, bad):
    assert _call(lib, **bad) == -1
    assert b"cse_noise_minstat" in lib.cse_last_error(), lib.cse_last_error()


def test_no_signals_launch_nothing(lib):
    assert _call(lib) == 0
    assert _call(lib, B=33, T=1, alpha_c=0.0, alpha_c_floor=0.0, alpha_min=0.0, beta_max=0.0,
                 snr_exp=0.0, av=0.0, sub_windows=1, sub_frames=2) == 0
    assert _call(lib, B=2049, q_eq_min=2.0, q_eq_max=2.0, sub_windows=16,
                 sub_frames=2 ** 20, slope_max=(1.0, 1.0, 1.0, 1.0)) == 0


# --------------------------------------------------------------------- layout
@pytest.mark.parametrize("bad", BAD_FIELDS + [dict(sub_windows=2.5), dict(sub_frames=NAN),
                                              dict(slope_q=(0.03, 0.05)), dict(slope_max=3.0)],
                         ids=_ids)
def test_minstat_values_refuses_what_the_library_refuses(bad):
    (name, _), = bad.items()
    with pytest.raises(ValueError, match="minstat.*" + ("q_eq" if name.startswith("q_eq")
                                                         else name)):
        layout.minstat_values(bad)
    cell = _cell("wiener", "minstat", **{"minstat_" + k: v for k, v in bad.items()})[2]
    with pytest.raises(ValueError, match="minstat"):
        layout.noise_key("wiener", cell, 63)
    with pytest.raises(ValueError, match="minstat"):  # at any T, the simple path included
        layout.noise_key("wiener", cell, 3)


def test_minstat_values_is_hashable_and_reads_the_prefix():
    v = layout.minstat_values({"minstat_av": 1.5, "minstat_slope_q": [0.02, 0.04, 0.07],
                               "minstat_sub_frames": np.int64(12), "av": 9.0}, "minstat_")
    assert v == (0.837, 0.7, 0.98, 0.548, -0.125, 0.894, 1.5, 2.0, 14.0, (0.02, 0.04, 0.07),
                 (8.0, 4.0, 2.0, 1.2), 8, 12)
    assert hash(v) == hash(tuple(v)) and isinstance(v[9], tuple) and isinstance(v[12], int)
    prm = layout.minstat_params(v)
    assert isinstance(prm, _lib.MinstatParams) and _as_tuple(prm) == v
    assert tuple(layout.TRACKERS) == ("mcra", "spp", "minstat", "imcra")
    assert layout.TRACKERS["minstat"].values is layout.minstat_values
    assert bytes(trackers.params(layout.TRACKERS["minstat"], v)) == bytes(layout.minstat_params(v))


def _cell(alg, method, hop=128, pct=20.0, **extra):
    base = {"spectralSubtractor": dict(alpha=1.0, beta=0.05),
            "wiener": dict(alpha=0.98, gain_floor=0.1),
            "mmse": dict(alpha=0.98, ksi_min=0.01, gain_min=0.05, gain_max=1.0),
            "omlsa": dict(alpha=0.9, ksi_min=0.01, gain_floor=0.1, noise_mu=0.95, q=0.4)}[alg]
    return (0, alg, dict(base, n_fft=512, hop_length=hop, noise_percentile=pct,
                         noise_method=method, **extra))


def _layout(specs, L=8000, S=1):
    (n_fft, items), = layout.specs_by_n_fft(S, L, specs, False, False)
    return layout.PlanLayout(n_fft, S, L, items, False, False, False, cells_per_group=16)


def test_noise_key_of_a_minstat_cell():
    T = 63
    want = DEFAULT_VALUES[:6] + (1.5,) + DEFAULT_VALUES[7:]
    for alg, (code, eps, _) in layout.ALGOS.items():
        p = _cell(alg, "minstat", minstat_av=1.5)[2]
        method, slot, e, expand, mu, inverse = layout.noise_key(alg, p, T)
        assert (method, slot, e, expand) == ("minstat", want, eps, False)
        assert inverse == (code != "SS")
        assert mu == {"SS": None, "WIENER": None, "MMSE": 0.98, "OMLSA": 0.95}[code]
        assert not layout.key_is_static((method, slot, e, expand, mu, inverse))
        # noise_percentile does not enter the key; spp_ and mcra_ names are other trackers'
        assert layout.noise_key(alg, dict(p, noise_percentile=3.0, mcra_delta=2.0,
                                          spp_ph_max=0.9), T) == \
            (method, slot, e, expand, mu, inverse)
        for other in ("min_tracking", "mcra", "spp"):
            assert layout.noise_key(alg, dict(p, noise_method=other), T)[2:] == \
                (e, expand, mu, inverse)
        assert layout.noise_key(alg, p, 4) == \
            layout.noise_key(alg, dict(p, noise_method="percentile"), 4)
        assert layout.noise_key(alg, p, 4)[0] == "simple"


def test_one_minstat_call_per_hop_and_parameter_set():
    specs = [_cell("wiener", "minstat", 128, 10.0), _cell("wiener", "minstat", 128, 20.0),
             _cell("spectralSubtractor", "minstat", 128), _cell("omlsa", "minstat", 128),
             _cell("wiener", "minstat", 128, minstat_sub_frames=12, minstat_slope_q=(0.02, 0.04,
                                                                                     0.07)),
             _cell("wiener", "minstat", 256), _cell("wiener", "min_tracking", 128),
             _cell("wiener", "spp", 128), _cell("wiener", "percentile", 256)]
    lay = _layout(specs)
    B = 257
    other = DEFAULT_VALUES[:9] + ((0.02, 0.04, 0.07), DEFAULT_VALUES[10], 8, 12)
    for hop, sets in ((128, [DEFAULT_VALUES, other]), (256, [DEFAULT_VALUES])):
        calls = lay.noise_calls[hop]
        names = [c[0] for c in calls]
        T = 1 + 8000 // hop
        assert names[-1] == "cse_noise_finish" and names.count("cse_noise_finish") == 1
        assert names.count("cse_noise_spp") == (1 if hop == 128 else 0)
        sc = [c[1] for c in calls if c[0] == "cse_noise_minstat"]
        assert len(sc) == len(sets)
        for args, want in zip(sc, sets):
            P, S, T_, B_, prm, eps, N = args
            assert (P, S, T_, B_, eps) == (layout.Ref("P"), 1, T, B, 1e-10)
            assert isinstance(prm, _lib.MinstatParams) and _as_tuple(prm) == want
            assert N.buf == "raw" and lay.raw_off[(hop, "minstat", want, 1e-10)] == (N.off, T)
            assert N.off + T * B <= lay.raw_elems
    lay2 = _layout(specs + [_cell("mmse", "minstat", 128)])
    sc = [c[1] for c in lay2.noise_calls[128] if c[0] == "cse_noise_minstat"]
    assert sorted(a[5] for a in sc) == [1e-12, 1e-10, 1e-10]
    # twins in noise_percentile share the estimate; the table is mcra's but for the call
    a = _layout([_cell("wiener", "minstat", 128, 10.0), _cell("wiener", "minstat", 128, 20.0)])
    m = _layout([_cell("wiener", "mcra", 128, 10.0), _cell("wiener", "mcra", 128, 20.0)])
    assert len(a.raw_off) == 1 and a.cells.tobytes() == m.cells.tobytes()
    assert [n for n, _ in a.noise_calls[128]] == ["cse_noise_minstat", "cse_noise_finish"]
    with pytest.raises(ValueError, match="Unbekannte Methode: minstat2"):
        _layout([_cell("wiener", "minstat2", 128)])


def test_short_clip_takes_the_simple_estimate():
    a = _layout([_cell("wiener", "minstat", 128)], L=300)
    b = _layout([_cell("wiener", "percentile", 128)], L=300)
    assert [c[0] for c in a.noise_calls[128]] == ["cse_noise_estimate", "cse_noise_finish"]
    assert a.keys == b.keys and a.cells.tobytes() == b.cells.tobytes()


def test_time_constants_at_other_frame_steps():
    d = layout.minstat_time_constants(128, 16000)
    assert set(d) == set(layout.MINSTAT_DEFAULTS)
    for k, v in layout.MINSTAT_DEFAULTS.items():
        if isinstance(v, tuple):
            assert d[k] == v
        else:
            assert d[k] == pytest.approx(v, rel=2e-3), k  # the defaults to 3 digits
            assert float(f"{d[k]:.3g}") == float(f"{v:.3g}"), k
    assert (d["sub_windows"], d["sub_frames"]) == (8, 24)
    h = layout.minstat_time_constants(256, 16000)
    assert (h["sub_windows"], h["sub_frames"]) == (8, 12)
    assert h["alpha_max"] == pytest.approx(math.exp(-0.016 / 0.392))
    assert h["snr_exp"] == pytest.approx(-0.25)
    assert layout.minstat_time_constants(8000, 16000)["sub_frames"] == 2  # clipped
    layout.minstat_values(h)  # a valid set
    layout.minstat_values(layout.minstat_time_constants(64, 8000))
    with pytest.raises(ValueError):
        layout.minstat_time_constants(0, 16000)


def test_grids_with_noise_methods_accepts_minstat():
    grids = parameter_ranges.grids_with_noise_methods(("min_tracking", "mcra", "spp", "minstat"))
    for alg, g in grids.items():
        assert g["noise_method"] == ["min_tracking", "mcra", "spp", "minstat"]
        assert parameter_ranges.ALGORITHM_GRIDS[alg]["noise_method"] == ["percentile",
                                                                         "min_tracking"]
    specs = search.job_specs(1, grids=parameter_ranges.grids_with_noise_methods(("minstat",)))
    for a, alg in enumerate(specs.algorithms):
        rep = specs.grid_rep(a, 16000)
        cells = specs.cells[alg]
        assert len(set(rep.tolist())) == len(cells) // 2  # the noise_percentile twins
        assert all(cells[r]["noise_method"] == "minstat" for r in rep)
