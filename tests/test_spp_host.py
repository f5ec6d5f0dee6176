"""SPP-MMSE noise tracking, the parts that need no GPU: the numpy restatement's
own properties (tests/_spp_ref.py, the definition of include/cse_spp.h), the
two entry points' declarations, exports and argument checks, and the layout:
the call list, the shared estimates and the sweep's duplicate cells."""

import ctypes
import math
import os
import re

import numpy as np
import pytest

import _spp_ref
from classical_speech_enhancement_amd import _lib, layout, parameter_ranges, search

HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "cse_spp.h")
# the HEAD grid's noise calls per hop on the commit before this estimator existed
PARENT_HEAD_CALLS = ["cse_noise_median", "cse_noise_min_tracking_med", "cse_noise_percentile_quad",
                     "cse_noise_finish"]
NAMES = ("prior_h1", "xi_opt_db", "alpha_pow", "alpha_ph", "ph_max", "init_frames")
DEFAULT_VALUES = (0.5, 15.0, 0.8, 0.9, 0.99, 5)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def _power(T, B, seed=0):
    return np.random.default_rng(seed).exponential(size=(T, B))


# ---------------------------------------------------------------- restatement
@pytest.mark.parametrize("eps", (1e-10, 1e-12))
def test_zero_power_returns_eps(eps):
    N = _spp_ref.spp(np.zeros((130, 33)), eps)
    assert N.dtype == np.float32 and np.array_equal(N, np.full((130, 33), np.float32(eps)))


def test_one_frame_returns_that_frame():
    """T = 1: lam starts as P[0], est is a convex combination of lam and P[0]."""
    P = _power(1, 33)
    N = _spp_ref.spp(P)
    assert N.shape == (1, 33)
    np.testing.assert_allclose(N[0], P[0], rtol=2.0 ** -23, atol=0)
    # below eps the floor takes over
    assert np.array_equal(_spp_ref.spp(P * 1e-13, 1e-10), np.full((1, 33), np.float32(1e-10)))


def test_fewer_frames_than_init_frames_use_their_mean():
    """T = 3 < init_frames = 5: the start is the mean of the 3 frames, summed in
    order; init_frames 3, 5 and 50 are then the same computation, 2 is not."""
    P = _power(3, 65, 4)
    a = _spp_ref.spp(P, init_frames=5)
    assert np.array_equal(a, _spp_ref.spp(P, init_frames=3))
    assert np.array_equal(a, _spp_ref.spp(P, init_frames=50))
    assert not np.array_equal(a, _spp_ref.spp(P, init_frames=2))
    # alpha_pow -> frame 0's output is the start value but for (1 - alpha_pow) est:
    # with alpha_pow = 0 and ph = 1 (ph_max close to 1, prior close to 1) N[0] = lam0
    lam0 = ((P[0] + P[1]) + P[2]) / 3.0
    n = _spp_ref.spp(P, alpha_pow=0.0, prior_h1=1.0 - 1e-16, ph_max=1.0 - 1e-16)
    np.testing.assert_allclose(n[0], lam0, rtol=2.0 ** -23, atol=0)


def test_constant_power_stays_the_constant():
    for c in (3.7, 1e-6, 250.0):
        N = _spp_ref.spp(np.full((300, 33), c))
        np.testing.assert_allclose(N, np.float32(c), rtol=2.0 ** -23, atol=0, err_msg=str(c))


def test_a_step_down_is_followed_without_a_window():
    """The power falls from 100 to 1 at frame 20.  Below the estimate s < 1, so
    ph stays under prior exp(c0 + c1) / (1 + prior exp(c0 + c1)) = 0.0738 at the
    defaults, and est = ph lam + (1 - ph) P pulls lam to P at the rate
    r = alpha_pow + (1 - alpha_pow) 0.0738 < 0.815 per frame: after n frames
    lam - 1 <= 99 * 0.815**n.  n = 40 frames (0.32 s at hop 128; MCRA's window
    is 125) leave less than 99 * 0.815**40 < 0.03."""
    P = np.full((80, 33), 100.0)
    P[20:] = 1.0
    N = _spp_ref.spp(P).astype(np.float64)
    xi = 10.0 ** 1.5
    g = math.exp(math.log(1.0 / (1.0 + xi)) + xi / (1.0 + xi))
    r = 0.8 + 0.2 * g / (1.0 + g)
    assert r < 0.815
    n = np.arange(1, 61)
    assert np.all(N[20:, 0] - 1.0 <= 99.0 * r ** n * (1 + 1e-6))
    assert np.all(N[20:] >= 1.0 - 1e-6) and N[60:].max() < 1.03
    assert np.allclose(N[:20], 100.0, rtol=1e-6)


def test_a_step_up_is_followed_through_the_guard():
    """The power rises from 1 to 100 at frame 20: ph goes to 1 and lam stands
    still, pm follows ph at alpha_ph (1 - pm falls by 0.9 a frame from above
    0.9, so it is above 1 - ph_max = 0.01 for 40 frames at least and below it
    after 44 at the most); from then on the guard holds ph at ph_max or less
    and each frame moves lam by at least (1 - alpha_pow)(1 - ph_max) = 0.002 of
    its distance to P: from frame 64 on, 100 - lam <= 99 * 0.998**(t - 64).
    Without the guard (ph_max just under 1) lam never moves."""
    P = np.ones((3000, 33))
    P[20:] = 100.0
    st = {}
    N = _spp_ref.spp(P, stats=st).astype(np.float64)
    assert st["clamped_share"] > 0.01
    assert np.all(np.diff(N[:, 0]) >= 0) and N[59, 0] <= 1.0 + 1e-6 and N[64, 0] > 1.0
    t = np.arange(64, 3000)
    assert np.all(100.0 - N[64:, 0] <= 99.0 * 0.998 ** (t - 64) + 1e-6)
    assert N[-1, 0] > 99.0
    stuck = _spp_ref.spp(P, ph_max=1.0 - 1e-16).astype(np.float64)
    assert stuck[-1, 0] < 1.01


def test_stats_count_guard_cap_and_margin():
    t = np.arange(18)[:, None]
    P = _power(18, 257, 18) * np.where(t < 9, 1, 100)
    st = {}
    _spp_ref.spp(P, 1e-12, prior_h1=0.3, xi_opt_db=12, alpha_pow=0.7, alpha_ph=0.5, ph_max=0.9,
                 init_frames=2, stats=st)
    assert 0.1 <= st["clamped_share"] <= 0.3 and st["capped"] >= 1 and st["margin"] >= 1e-9
    st0 = {}
    _spp_ref.spp(np.full((6, 33), 2.0), stats=st0)
    assert st0["clamped_share"] == 0.0 and st0["capped"] == 0
    # pm after frame 0 is 0.9 * 0.5 + 0.1 * ph and only falls towards ph < 0.99
    assert 0.4 < st0["margin"] < 0.99
    big = np.full((2, 33), 1.0)
    big[1] = 1e4  # a = c0 + c1 * 1e4 / lam > 200
    st1 = {}
    _spp_ref.spp(big, stats=st1, init_frames=1)
    assert st1["capped"] == 33
    st3 = {}
    N3 = _spp_ref.spp(np.stack([_power(18, 33, s) for s in range(3)]), stats=st3)
    assert N3.shape == (3, 18, 33) and set(st3) == {"clamped_share", "capped", "margin"}
    assert np.array_equal(N3[2], _spp_ref.spp(_power(18, 33, 2)))


# ------------------------------------------------------------------------ ABI
def test_header_declares_the_exports(lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = set(re.findall(r"\b(cse_[a-z0-9_]+)\s*\(", text))
    assert names == set(_lib.EXPORTS_SPP) == {"cse_spp_default_params", "cse_noise_spp"}
    assert '#include "cse.h"' in text
    assert not set(_lib.EXPORTS_SPP) & (set(_lib.EXPORTS) | set(_lib.EXPORTS_ESTOI) |
                                        set(_lib.EXPORTS_MCRA) | set(_lib.EXPORTS_SEGSNR))
    for n in _lib.EXPORTS_SPP:
        assert hasattr(lib, n), n
    assert lib.cse_version() == _lib.ABI_VERSION == 5
    assert _lib.NOISE["spp"] == 4 and "#define CSE_NOISE_SPP 4" in text


def test_struct_sizes_and_defaults(lib):
    assert ctypes.sizeof(_lib.SppParams) == 48
    assert [f[0] for f in _lib.SppParams._fields_] == list(NAMES) + ["reserved"]
    text = open(HEADER).read()
    assert "} cse_spp_params_t; /* 48 bytes */" in text
    # the C struct's size: default_params fills a guarded buffer of 48 bytes exactly
    buf = (ctypes.c_ubyte * 56)(*([0xAB] * 56))
    lib.cse_spp_default_params(ctypes.byref(buf))
    assert bytes(buf[48:]) == b"\xab" * 8
    prm = _lib.SppParams.from_buffer_copy(bytes(buf[:48]))
    got = tuple(getattr(prm, n) for n in NAMES)
    assert got == DEFAULT_VALUES and prm.reserved == 0
    assert got == tuple(_spp_ref.DEFAULTS[k] for k in NAMES)
    assert got == tuple(layout.SPP_DEFAULTS[k] for k in NAMES) == layout.spp_values({})
    back = layout.spp_params(layout.spp_values({}))
    assert bytes(back) == bytes(buf[:48])
    lib.cse_spp_default_params(None)  # ignored


def _call(lib, P=16, n_sig=1, T=10, B=257, prm="default", eps=1e-10, N=16, **fields):
    if prm == "default":
        prm = _lib.SppParams()
        lib.cse_spp_default_params(ctypes.byref(prm))
        for k, v in fields.items():
            setattr(prm, k, v)
        prm = ctypes.byref(prm)
    return lib.cse_noise_spp(ctypes.c_void_p(P) if P else None, n_sig, T, B, prm, eps,
                             ctypes.c_void_p(N) if N else None, None)


@pytest.mark.parametrize("bad", [
    dict(P=None), dict(N=None), dict(prm=None), dict(n_sig=-1), dict(T=0), dict(B=32),
    dict(B=2050), dict(prior_h1=0.0), dict(prior_h1=1.0), dict(prior_h1=math.nan),
    dict(ph_max=0.0), dict(ph_max=1.0), dict(ph_max=math.nan), dict(alpha_pow=-1e-9),
    dict(alpha_pow=1.0), dict(alpha_pow=math.nan), dict(alpha_ph=-0.1), dict(alpha_ph=1.0),
    dict(alpha_ph=math.nan), dict(xi_opt_db=math.inf), dict(xi_opt_db=-math.inf),
    dict(xi_opt_db=math.nan), dict(init_frames=0), dict(init_frames=-3)],
    ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_argument_checks(lib, bad):
    assert _call(lib, **bad) == -1
    assert b"cse_noise_spp" in lib.cse_last_error(), lib.cse_last_error()


def test_no_signals_launch_nothing(lib):
    assert _call(lib, n_sig=0) == 0
    assert _call(lib, n_sig=0, B=33, T=1, init_frames=1, alpha_pow=0.0, alpha_ph=0.0) == 0
    assert _call(lib, n_sig=0, B=2049, xi_opt_db=-20.0, init_frames=2**31 - 1) == 0
    assert _call(lib, n_sig=0, ph_max=1.0) == -1  # checked all the same


# --------------------------------------------------------------------- layout
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


def test_noise_key_of_an_spp_cell():
    T = 63
    for alg, (code, eps, _) in layout.ALGOS.items():
        p = _cell(alg, "spp", spp_ph_max=0.95)[2]
        method, slot, e, expand, mu, inverse = layout.noise_key(alg, p, T)
        assert (method, slot, e, expand) == ("spp", (0.5, 15.0, 0.8, 0.9, 0.95, 5), eps, False)
        assert inverse == (code != "SS")
        assert mu == {"SS": None, "WIENER": None, "MMSE": 0.98, "OMLSA": 0.95}[code]
        assert not layout.key_is_static((method, slot, e, expand, mu, inverse))
        # noise_percentile does not enter the key; the mcra_ names are another tracker's
        assert layout.noise_key(alg, dict(p, noise_percentile=3.0, mcra_delta=2.0), T) == \
            (method, slot, e, expand, mu, inverse)
        # in every slot but the estimator's it is min_tracking's and mcra's key
        assert layout.noise_key(alg, dict(p, noise_method="min_tracking"), T)[2:] == \
            (e, expand, mu, inverse)
        assert layout.noise_key(alg, dict(p, noise_method="mcra"), T)[2:] == (e, expand, mu, inverse)
        # the reference's fallback comes before the method: T < 5 is 'simple'
        assert layout.noise_key(alg, p, 4) == \
            layout.noise_key(alg, dict(p, noise_method="percentile"), 4)
        assert layout.noise_key(alg, p, 4)[0] == "simple"


def test_one_spp_call_per_hop_and_parameter_set():
    """Mixed with the other methods: every (hop, parameter set) of the spp
    cells is one cse_noise_spp call (per eps the algorithms estimate with: SS,
    Wiener and OMLSA share 1e-10), launched before that hop's finish."""
    specs = [_cell("wiener", "spp", 128, 10.0), _cell("wiener", "spp", 128, 20.0),
             _cell("spectralSubtractor", "spp", 128), _cell("omlsa", "spp", 128),
             _cell("wiener", "spp", 128, spp_xi_opt_db=12, spp_init_frames=2),
             _cell("wiener", "spp", 256), _cell("wiener", "min_tracking", 128),
             _cell("wiener", "mcra", 128), _cell("wiener", "percentile", 256),
             _cell("spectralSubtractor", "percentile", 128)]
    lay = _layout(specs)
    B = 257
    for hop, sets in ((128, [DEFAULT_VALUES, (0.5, 12.0, 0.8, 0.9, 0.99, 2)]),
                      (256, [DEFAULT_VALUES])):
        calls = lay.noise_calls[hop]
        names = [c[0] for c in calls]
        T = 1 + 8000 // hop
        assert names[-1] == "cse_noise_finish" and names.count("cse_noise_finish") == 1
        assert names.count("cse_noise_mcra") == (1 if hop == 128 else 0)
        sc = [c[1] for c in calls if c[0] == "cse_noise_spp"]
        assert len(sc) == len(sets)
        for args, want in zip(sc, sets):
            P, S, T_, B_, prm, eps, N = args
            assert (P, S, T_, B_, eps) == (layout.Ref("P"), 1, T, B, 1e-10)
            assert isinstance(prm, _lib.SppParams)
            assert tuple(getattr(prm, n) for n in NAMES) == want
            assert N.buf == "raw" and lay.raw_off[(hop, "spp", want, 1e-10)] == (N.off, T)
            assert N.off + T * B <= lay.raw_elems
    # mmse estimates with eps 1e-12: a base, and a call, of its own
    lay2 = _layout(specs + [_cell("mmse", "spp", 128)])
    sc = [c[1] for c in lay2.noise_calls[128] if c[0] == "cse_noise_spp"]
    assert sorted(a[5] for a in sc) == [1e-12, 1e-10, 1e-10]
    assert len({a[6].off for a in sc}) == 3


def test_cells_differing_in_noise_percentile_share_the_estimate():
    lay = _layout([_cell("wiener", "spp", 128, 10.0), _cell("wiener", "spp", 128, 20.0),
                   _cell("omlsa", "spp", 128, 10.0), _cell("omlsa", "spp", 128, 20.0)])
    assert len(lay.keys) == 2 and len(lay.raw_off) == 1  # wiener's and omlsa's rows, one base
    c = lay.cells
    assert c["noise_offset"][0] == c["noise_offset"][1] != c["noise_offset"][2]
    assert c["noise_offset"][2] == c["noise_offset"][3]
    assert (c["noise_stride"] == 257).all()  # time-varying rows
    assert [n for n, _ in lay.noise_calls[128]] == ["cse_noise_spp", "cse_noise_finish"]
    j = lay.jobs
    assert j["src_frames"].tolist() == [63, 63] and j["out_frames"].tolist() == [63, 63]
    assert sorted(j["mu"].tolist()) == [0.0, 0.95] and (j["inv_eps"] == 1e-10).all()
    # the same table as mcra's but for the call: spp sits where mcra sits
    m = _layout([_cell("wiener", "mcra", 128, 10.0), _cell("wiener", "mcra", 128, 20.0),
                 _cell("omlsa", "mcra", 128, 10.0), _cell("omlsa", "mcra", 128, 20.0)])
    assert m.cells.tobytes() == c.tobytes() and m.jobs.tobytes() == j.tobytes()
    # a parameter that differs separates the estimates
    two = _layout([_cell("wiener", "spp", 128), _cell("wiener", "spp", 128, spp_alpha_pow=0.7)])
    assert len(two.raw_off) == 2
    assert two.cells["noise_offset"][0] != two.cells["noise_offset"][1]


@pytest.mark.parametrize("bad", [dict(spp_init_frames=0), dict(spp_init_frames=2.5),
                                 dict(spp_init_frames=math.nan), dict(spp_prior_h1=0.0),
                                 dict(spp_prior_h1=1.0), dict(spp_ph_max=1.0),
                                 dict(spp_ph_max=math.nan), dict(spp_alpha_pow=1.0),
                                 dict(spp_alpha_ph=-0.5), dict(spp_alpha_ph=math.nan),
                                 dict(spp_xi_opt_db=math.inf), dict(spp_xi_opt_db=math.nan)],
                         ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_invalid_parameters_raise_at_layout_time(bad):
    with pytest.raises(ValueError, match="spp"):
        _layout([_cell("wiener", "spp", 128), _cell("wiener", "spp", 128, **bad)])
    with pytest.raises(ValueError, match="spp"):
        layout.noise_key("wiener", _cell("wiener", "spp", 128, **bad)[2], 63)
    with pytest.raises(ValueError, match="spp"):  # at any T, the simple path included
        layout.noise_key("wiener", _cell("wiener", "spp", 128, **bad)[2], 3)
    with pytest.raises(ValueError, match="spp"):
        layout.spp_values({k[4:]: v for k, v in bad.items()})
    with pytest.raises(ValueError, match="Unbekannte Methode: spp2"):
        _layout([_cell("wiener", "spp2", 128)])


def test_short_clip_takes_the_simple_estimate():
    a = _layout([_cell("wiener", "spp", 128)], L=300)
    b = _layout([_cell("wiener", "percentile", 128)], L=300)
    assert [c[0] for c in a.noise_calls[128]] == ["cse_noise_estimate", "cse_noise_finish"]
    assert a.keys == b.keys and a.cells.tobytes() == b.cells.tobytes()
    assert a.jobs.tobytes() == b.jobs.tobytes()


def test_head_grid_call_list_is_the_parents():
    specs = parameter_ranges.grid_specs(2, n_fft=512)
    (n_fft, items), = layout.specs_by_n_fft(2, 16000, specs, True, False)
    lay = layout.PlanLayout(n_fft, 2, 16000, items, True, False, False, align=True,
                            cells_per_group=16)
    assert list(lay.noise_calls) == [128, 256]
    for hop, calls in lay.noise_calls.items():
        assert [c[0] for c in calls] == PARENT_HEAD_CALLS
    assert not any(k[1] in ("spp", "mcra") for k in lay.raw_off)


def test_grids_with_noise_methods_and_grid_rep():
    grids = parameter_ranges.grids_with_noise_methods(("spp",))
    assert all(g["noise_method"] == ["spp"] for g in grids.values())
    grids = parameter_ranges.grids_with_noise_methods(("percentile", "spp"))
    assert list(grids) == list(parameter_ranges.ALGORITHM_GRIDS)
    for alg, g in grids.items():
        head = parameter_ranges.ALGORITHM_GRIDS[alg]
        assert list(g) == list(head) and g["noise_method"] == ["percentile", "spp"]
        assert head["noise_method"] == ["percentile", "min_tracking"]  # the default stays
        assert all(g[k] == head[k] and g[k] is not head[k] for k in g if k != "noise_method")
    specs = search.job_specs(1, grids=grids)
    assert len(specs) == len(search.job_specs(1))
    for a, alg in enumerate(specs.algorithms):
        rep = specs.grid_rep(a, 16000)
        cells = specs.cells[alg]
        dup = 0
        for c, p in enumerate(cells):
            if p["noise_method"] == "spp" and p["noise_percentile"] == 20.0:
                twin = dict(p, noise_percentile=10.0)
                assert rep[c] == cells.index(twin) < c, (alg, c)
                dup += 1
            else:
                assert rep[c] == c, (alg, c)
        assert dup == len(cells) // 4
    # the three time-varying methods side by side: three quarters... of each
    # method's cells, half are the twins of the other half; spp and mcra cells
    # with equal parameters are not each other's
    specs3 = search.job_specs(1, grids=parameter_ranges.grids_with_noise_methods(
        ("min_tracking", "mcra", "spp")))
    for a, alg in enumerate(specs3.algorithms):
        rep = specs3.grid_rep(a, 16000)
        cells = specs3.cells[alg]
        assert len(set(rep.tolist())) == len(cells) // 2
        assert all(cells[r]["noise_method"] == p["noise_method"] for r, p in zip(rep, cells))
