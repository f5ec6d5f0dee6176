"""The design of the per-element gain tests (tests/_gain_cases.py) has the
properties tests/test_gpu_gains.py relies on.  Everything here is asserted on
the fp64 reference alone (oracle/gain_ref.py): no device, no torch.

  * the reference is finite and its conditioning kappa stays below the cap:
    everywhere for Wiener, MMSE and OMLSA, on all but 0.1 % of a case for SS;
  * per (bins, algorithm) family, at least 50 elements lie in every regime of
    the recursion: the three ranges of v, both clips of v, gamma on its floor,
    xi on its floor, G on either clip and strictly between them; for SS both
    branches of the max and Y = 0;
  * bins 0, M/2 and M carry an interior gain in at least half the frames;
  * the scaled SS spectra keep |Y|^2 a normal float32.
"""

import numpy as np
import pytest

import _gain_cases as gc

BINS = (257, 513, 33, 201)  # n_fft 512, 1024, 64, 400
FULL = [(B, T) for B in BINS for T in gc.FRAMES]
BANDED = [(B, T, band) for B in (257, 513) for T in (5, 41) for band in ("low", "mid", "high")]
MIN_COUNT = 50


def _main_cells(alg=None):
    return [c for c in gc.cells() if c.spec == "main" and alg in (None, c.alg)]


def test_parameter_vectors_follow_the_layout():
    """param[] in layout.ALGOS' order: OMLSA's gain_floor comes before q."""
    prm = gc.PARAMS["omlsa"][0]
    np.testing.assert_array_equal(gc.param_vector("omlsa", prm)[:5],
                                  np.float32([0.7, 1e-3, 0.05, 0.3, 80.0]))
    for alg, sets in gc.PARAMS.items():
        for prm in sets:
            assert set(prm) == set(gc.ALGOS[alg][2]), (alg, prm)


@pytest.mark.parametrize("B,T", FULL)
def test_design_is_as_described(B, T):
    d = gc.design(B, T)
    inp = gc.inputs(B, T)
    M = B - 1
    Y = inp.Y["main"]
    assert Y.shape == (T, B) and Y.dtype == np.complex64
    assert (Y[:, [0, M]].imag == 0).all()
    assert (Y[:, d.zero_bin] == 0).all()
    assert (Y[d.run[0]:d.run[1], d.run_bin] == 0).all() and d.run[1] > d.run[0]
    assert np.count_nonzero(Y == 0) == T + d.run[1] - d.run[0]
    # plain zeros: np.angle of a negative zero is pi, not the angle(0) = 0 of the kernels
    assert not np.signbit(Y.real[Y == 0]).any() and not np.signbit(Y.imag[Y.imag == 0]).any()
    assert d.N[d.floor_bin] < 1e-12 and (np.delete(d.N, d.floor_bin) >= 1e-10).all()
    assert (d.factor >= 0.5).all() and (d.factor <= 2.0).all()
    # gamma keeps clear of the cancellation gamma - 1 with either noise row
    lg = np.log10(np.delete(d.gamma, d.floor_bin, axis=0))
    assert (np.abs(lg) >= 0.015 - 1e-12).all()
    assert (np.abs(lg - np.log10(d.factor)[None, :]) >= 0.015 - 1e-12).all()
    # and of P - alpha N of SS
    for prm in gc.PARAMS["spectralSubtractor"]:
        la = np.log10(prm["alpha"])
        assert (np.abs(lg - la) >= 0.005 - 1e-12).all()
        assert (np.abs(lg - np.log10(d.factor)[None, :] - la) >= 0.005 - 1e-12).all()
    # P = gamma N is of one magnitude: every bin but the floored one within
    # the 4.5 decades the trajectories span
    P = np.delete(inp.P["main"], d.floor_bin, axis=0)
    live = P[P > 0]
    assert live.min() >= 1e-3 * 10 ** -3.1 and live.max() <= 1e-3 * 10 ** 4.6
    assert abs(inp.P["main"][d.floor_bin, 0] / 2e-9 - 1) < 1e-6
    pad = inp.rows["ss_pad"].data
    assert pad.shape == (T, B) and (pad[1:] == 0).all() and (pad[0] > 0).all()
    assert inp.rows["ss_tv"].data.shape == (T, B) and inp.rows["ss_static"].data.shape == (1, B)
    for eps in (1e-10, 1e-12):
        inv = inp.rows[f"inv_static|{eps:g}"].data
        assert inv.dtype == np.float32 and inv.max() <= np.float32(1.0 / eps)
        assert inv[0, d.floor_bin] == np.float32(1.0 / eps)


@pytest.mark.parametrize("B,T", FULL)
def test_reference_finite_and_conditioned(B, T):
    for c in gc.cells():
        G = gc.gains(B, T, gc.SEED, "all", c)
        k = gc.kappa(B, T, gc.SEED, "all", c)
        assert G.shape == (B, T) and np.isfinite(G).all() and np.isfinite(k).all(), c
        assert (G >= 0).all(), c
        if c.alg == "spectralSubtractor":
            share = float((k > gc.KAPPA_CAP).mean())
            assert share <= gc.SS_EXCLUDED_MAX, (c, share)
        else:
            assert k.max() <= gc.KAPPA_CAP, (c, float(k.max()), np.unravel_index(k.argmax(), k.shape))


@pytest.mark.parametrize("B,T,band", BANDED)
def test_banded_reference_finite(B, T, band):
    d = gc.design(B, T, gc.SEED, band)
    lo, hi = gc.BANDS[band]
    assert d.lev.min() >= lo and d.lev.max() <= hi
    for c in gc.cells(band):
        assert c.spec == "main"
        assert np.isfinite(gc.gains(B, T, gc.SEED, band, c)).all(), c
        assert np.isfinite(gc.waveform(B, T, gc.SEED, band, c, 128)).all(), c


def _count(acc, name, mask):
    acc[name] = acc.get(name, 0) + int(np.count_nonzero(mask))


@pytest.mark.parametrize("B", BINS)
@pytest.mark.parametrize("alg", list(gc.PARAMS))
def test_every_regime_is_reached(B, alg):
    """Element counts per (bins, algorithm) family over its frame counts, noise
    rows and parameter sets."""
    acc = {}
    for T in gc.FRAMES:
        inp = gc.inputs(B, T)
        for c in _main_cells(alg):
            prm = gc.PARAMS[alg][c.pidx]
            G = gc.gains(B, T, gc.SEED, "all", c)
            gam, xi, v = gc.diagnose(B, T, gc.SEED, "all", c)
            if alg == "spectralSubtractor":
                P = inp.P["main"]
                N = np.broadcast_to(inp.rows[c.form].N, P.shape)
                sub = P - prm["alpha"] * N > prm["beta"] * N
                _count(acc, "subtracted", sub & (P > 0))
                _count(acc, "floored", ~sub & (P > 0))
                _count(acc, "Y = 0", P == 0)
                continue
            lo, hi = gc.clip_bounds(alg, prm)
            _count(acc, "gamma at eps", gam == gc.eps_of(alg))
            _count(acc, "xi at its floor", xi == gc.xi_floor(alg, prm))
            if lo >= hi:  # crossed bounds: numpy's clip gives the upper one
                assert (G == hi).all(), c
            _count(acc, "G on the lower clip", (G == lo) & (lo < hi))
            _count(acc, "G on the upper clip", G == hi)
            _count(acc, "G interior", (G > lo) & (G < hi))
            if alg == "wiener":
                continue
            vlo, vhi = gc.v_clip(alg, prm)
            _count(acc, "v <= 4", (v > vlo) & (v <= 4.0) & (v < vhi))
            _count(acc, "4 < v < 11.5", (v > 4.0) & (v < 11.5) & (v < vhi))
            _count(acc, "11.5 <= v < v_max", (v >= 11.5) & (v < vhi))
            _count(acc, "v clipped at v_max", v >= vhi)
            _count(acc, "v on the lower clip", v <= vlo)
    print(B, alg, acc)
    want = {"spectralSubtractor": 3, "wiener": 5, "mmse": 10, "omlsa": 10}[alg]
    assert len(acc) == want, acc
    for name, n in acc.items():
        assert n >= MIN_COUNT, (B, alg, name, n)


@pytest.mark.parametrize("B,T", FULL)
def test_edge_bins_carry_interior_gains(B, T):
    """Bins 0, M/2 and M (DC, the bin the sweep kernels hand to a wave of its
    own, Nyquist): at least half the frames strictly between the clips, for
    every parameter set whose clip bounds do not cross."""
    M = B - 1
    for c in _main_cells():
        if c.alg == "spectralSubtractor":
            continue
        lo, hi = gc.clip_bounds(c.alg, gc.PARAMS[c.alg][c.pidx])
        if lo >= hi:
            continue
        G = gc.gains(B, T, gc.SEED, "all", c)
        for b in (0, M // 2, M):
            n = int(np.count_nonzero((G[b] > lo) & (G[b] < hi)))
            assert 2 * n >= T, (c, b, n, T)


@pytest.mark.parametrize("B,T", FULL)
def test_scaled_ss_spectra_stay_normal(B, T):
    """Every non-zero |Y| of the 2^-30 and 2^-45 spectra is at least 2^-62, so
    |Y|^2 is a normal float32; they reach the rescaled sqrt (Ps < 2^-96) and
    the rescaled phasor (|y| < 2^-50) of gain_bin."""
    inp = gc.inputs(B, T)
    reach_sqrt = reach_phasor = 0
    for name in ("s30", "s45"):
        Y = inp.Y[name].astype(np.complex128)
        a = np.abs(Y)
        assert np.count_nonzero(a) == np.count_nonzero(inp.Y["main"])
        assert a[a > 0].min() >= 2.0 ** -62
        p32 = (inp.Y[name].real ** 2 + inp.Y[name].imag ** 2)
        assert (p32[a > 0] >= np.finfo(np.float32).tiny).all()
        if T > 1:  # frames past the first see N = 0: Ps = P
            reach_sqrt += np.count_nonzero((inp.P[name][:, 1:] < 2.0 ** -96) & (inp.P[name][:, 1:] > 0))
        reach_phasor += np.count_nonzero((np.maximum(np.abs(Y.real), np.abs(Y.imag)) < 2.0 ** -50)
                                         & (a > 0))
    assert reach_phasor >= min(MIN_COUNT, B // 2)
    assert T == 1 or reach_sqrt >= min(MIN_COUNT, B // 2)
