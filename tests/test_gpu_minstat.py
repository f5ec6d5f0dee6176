"""Minimum-statistics noise tracking on the device (needs an MI355X: -m gpu):
the kernel against the numpy restatement of include/cse_minstat.h within one
f32 step, the estimator and the four algorithm plugins against the oracle
composed from its own parts with the restatement as the estimator, and the
sweep over grids that name it.

Measured on an MI355X: see DESIGN.md, section 3.3.
"""

import functools

import numpy as np
import pytest

import _minstat_ref
import oracle
from classical_speech_enhancement_amd import parameter_ranges, search
from classical_speech_enhancement_amd.synth import make_pair
from conftest import rel_l2, rel_max
from oracle import gain_ref

pytestmark = pytest.mark.gpu

TOL = 1e-5
ULP = 2.0 ** -23  # the contract: the restatement's f32 value or its neighbour
# a larger share of unequal elements means the per-bin order of operations was
# not kept (the order of the three sums moved no f32 in a prototype)
MAX_UNEQUAL_SHARE = 1e-4
# (T, B, S) with U = 3, V = 4, so that every branch is reached in few frames:
# the store branch only, the first whole sub-window, the last frame before the
# buffer wraps, the store at t = 12 into slot 0 again, the first local-minimum
# updates with several signals, a B that is no multiple of the wave
SMALL = dict(sub_windows=3, sub_frames=4)
SMALL_CASES = [(1, 33, 1), (4, 33, 1), (5, 33, 1), (12, 33, 1), (13, 257, 1), (14, 257, 3),
               (26, 257, 1), (27, 300, 1),
               # the kernel's other shapes: 2, 3 and 4 bins per lane (B beyond 512, 1024, 1536)
               (27, 513, 2), (18, 1025, 1), (18, 1537, 1)]
# with the defaults: the buffer of 8 sub-windows wraps at t = 192; the largest B
DEFAULT_CASES = [(250, 257, 1), (253, 2049, 1)]
# every field changed; alpha_min and snr_exp such that the smoothing floor
# falls below alpha_min once the power has risen (pow is on the path)
OTHER = dict(alpha_c=0.7, alpha_c_floor=0.5, alpha_max=0.96, alpha_min=0.7, snr_exp=-0.25,
             beta_max=0.8, av=1.5, q_eq_min=2.5, q_eq_max=10.0, slope_q=(0.02, 0.04, 0.07),
             slope_max=(6.0, 3.0, 1.8, 1.1), sub_windows=5, sub_frames=6)
CELLS = {
    "ss": dict(alpha=2.0, beta=0.005),
    "wiener": dict(alpha=0.98, gain_floor=0.1),
    "mmse": dict(alpha=0.98, ksi_min=0.01, gain_min=0.05, gain_max=1.0, noise_mu=0.98),
    "omlsa": dict(alpha=0.9, ksi_min=0.005, gain_floor=0.1, noise_mu=0.95, q=0.4),
}
SHAPES = [(512, 128), (512, 64), (400, 160)]  # sweep kernel, short hop, generic


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from classical_speech_enhancement_amd.engine import Engine
    return Engine()


@pytest.fixture(scope="module")
def P(eng):
    from classical_speech_enhancement_amd import plugins
    return plugins


def _device(eng, power, **kw):
    import torch
    Pd = torch.as_tensor(np.ascontiguousarray(power)).cuda()
    return eng.noise_estimate("minstat", Pd, **kw).cpu().numpy()


def _step_power(T, B, S):
    """Exponential power, multiplied by 100 from frame T // 2 on."""
    t = np.arange(T)[None, :, None]
    return np.random.default_rng(T).exponential(size=(S, T, B)) * np.where(t < T // 2, 1, 100)


def _compare(N, ref, what):
    """The contract of include/cse_minstat.h, the unequal count printed first."""
    assert N.dtype == np.float32 and N.shape == ref.shape
    unequal = int((N != ref).sum())
    err = float(np.max(np.abs(N.astype(np.float64) - ref) / ref))
    print(f"{what}: {unequal} of {ref.size} unequal, max rel error {err / ULP:.3f} * 2^-23")
    assert err <= ULP, (what, err)
    assert unequal <= MAX_UNEQUAL_SHARE * ref.size, (what, unequal, ref.size)


def _kernel_case(eng, T, B, S, **prm):
    power = _step_power(T, B, S)
    st = {}
    ref = _minstat_ref.minstat(power, 1e-10, stats=st, **prm)
    print(f"T={T} B={B} S={S}: {st}")
    # the input's conditions, on the restatement alone
    assert st["margin"] >= 1e-9
    if T >= 14:
        assert st["lmin"] >= 1
    assert st["kmod"] >= B
    _compare(_device(eng, power, eps=1e-10, **prm), ref, f"T={T} B={B} S={S}")


# ------------------------------------------------------ kernel ~ restatement
@pytest.mark.parametrize("T,B,S", SMALL_CASES)
def test_kernel_equals_restatement_short_windows(eng, T, B, S):
    _kernel_case(eng, T, B, S, **SMALL)


@pytest.mark.parametrize("T,B,S", DEFAULT_CASES)
def test_kernel_equals_restatement_defaults(eng, T, B, S):
    _kernel_case(eng, T, B, S)


def test_kernel_equals_restatement_with_sixteen_sub_windows(eng):
    """U = 16: at B = 257 the buffer is in LDS as ever; at B = 1300 it is beyond
    a CU's LDS and the kernel keeps it in registers."""
    for T, B in ((60, 257), (60, 1300)):  # the buffer wraps at t = 48
        _kernel_case(eng, T, B, 1, sub_windows=16, sub_frames=3)


@pytest.mark.parametrize("eps", (1e-10, 1e-12))
def test_zero_power_gives_eps(eng, eps):
    N = _device(eng, np.zeros((2, 130, 257)), eps=eps)
    assert np.array_equal(N, np.full((2, 130, 257), np.float32(eps)))
    assert np.array_equal(N, _minstat_ref.minstat(np.zeros((2, 130, 257)), eps))


def test_zero_bin_and_zero_frames_stay_finite(eng):
    power = np.random.default_rng(3).exponential(size=(1, 200, 65))
    power[:, :, 5] = 0.0
    power[:, 60:100] = 0.0
    N = _device(eng, power)
    assert np.isfinite(N).all()
    assert np.array_equal(N[0, :, 5], np.full(200, np.float32(1e-10)))


def test_non_default_parameters_equal_restatement(eng):
    power = np.random.default_rng(5).exponential(size=(2, 70, 129))
    power[:, 30:50] *= 40.0
    st = {}
    ref = _minstat_ref.minstat(power, 1e-12, stats=st, **OTHER)
    print(st)
    assert st["margin"] >= 1e-9 and st["lmin"] >= 1
    _compare(_device(eng, power, eps=1e-12, **OTHER), ref, "non-default")
    assert not np.array_equal(ref, _minstat_ref.minstat(power, 1e-12))
    # the floor pow(snr, snr_exp) was below alpha_min somewhere: without it
    # (snr_exp = 0) the estimate is another
    assert not np.array_equal(ref, _minstat_ref.minstat(power, 1e-12, **dict(OTHER, snr_exp=0.0)))


def test_bad_parameter_names_and_values_raise(eng):
    power = np.ones((1, 12, 33))
    for name, value in (("sub_windows", 0), ("sub_windows", 17), ("sub_frames", 1),
                        ("sub_frames", 2.5), ("alpha_max", 1.0), ("alpha_c", float("nan")),
                        ("snr_exp", 0.5), ("av", -1.0), ("q_eq_min", 1.5),
                        ("slope_q", (0.05, 0.03, 0.06)), ("slope_max", (8.0, 4.0, 2.0, 0.5))):
        with pytest.raises(ValueError, match=name[:4]):
            _device(eng, power, **{name: value})
    with pytest.raises(ValueError, match="frames"):
        _device(eng, power, frames=13)
    with pytest.raises(TypeError):
        _device(eng, power, window_frames=50)  # mcra's
    with pytest.raises(TypeError):
        _device(eng, power, delta=5.0)  # mcra's
    with pytest.raises(TypeError):
        _device(eng, power, prior_h1=0.4)  # spp's
    with pytest.raises(TypeError):
        _device(eng, power, init_frames=3)  # spp's
    assert _device(eng, power, frames=12).shape == (1, 12, 33)


# ------------------------------------------------------------ the estimator
@functools.lru_cache(maxsize=None)
def _pair(seed, seconds):
    return make_pair(seed, seconds=seconds)


@functools.lru_cache(maxsize=None)
def _analysis(seed, seconds, n_fft, hop):
    """(Y, P) of the oracle's STFT of the pair's noisy signal, computed once."""
    Y = oracle.stft(_pair(seed, seconds)[1], n_fft, hop)
    return Y, np.abs(Y) ** 2


@pytest.mark.parametrize("n_fft,hop", [(512, 128), (512, 64), (400, 160), (2048, 512)])
def test_noise_estimation_matches_restatement(eng, P, n_fft, hop):
    """plugins.noise_estimation(method='minstat') against the restatement
    applied to oracle.stft's power; fp32 storage of an fp64 estimate, rtol 1e-6
    (the bound of the other estimators).  The device STFT and numpy's differ in
    the last bits, which the recursion does not amplify while no comparison is
    closer than that: the margin is printed."""
    noisy = _pair(8, 2.0)[1]
    power = _analysis(8, 2.0, n_fft, hop)[1]
    st = {}
    ref = _minstat_ref.minstat(power.T, 1e-10, stats=st).T.astype(np.float64)
    N = P.noise_estimation(noisy, 16000, method="minstat", n_fft=n_fft, hop_length=hop)
    assert N.shape == ref.shape == (n_fft // 2 + 1, 1 + len(noisy) // hop) and N.dtype == np.float64
    err = float(np.max(np.abs(N - ref) / ref))
    print(f"n_fft={n_fft} hop={hop}: {st}, {int((N != ref).sum())} of {ref.size} unequal, "
          f"max rel error {err:.3e}")
    np.testing.assert_allclose(N, ref, rtol=1e-6, atol=0)


def test_noise_estimation_reads_parameters_like_the_other_estimators(eng, P):
    """The parameters from {**estimator_params, **kwargs} (kwargs win), eps from
    kwargs only."""
    noisy = _pair(8, 2.0)[1]
    power = _analysis(8, 2.0, 512, 128)[1]
    N = P.noise_estimation(noisy, 16000, method="minstat", n_fft=512, hop_length=128,
                           estimator_params=dict(sub_frames=12, av=1.0, alpha_max=0.9, eps=1.0),
                           alpha_max=0.96, eps=1e-12)
    ref = _minstat_ref.minstat(power.T, 1e-12, sub_frames=12, av=1.0, alpha_max=0.96).T
    np.testing.assert_allclose(N, ref.astype(np.float64), rtol=1e-6, atol=0)
    assert N.min() < 1.0  # estimator_params' eps was not the floor


# --------------------------------------------------------------- end to end
def _fn(P, alg):
    return {"ss": P.spectral_subtraction, "wiener": P.wiener_filter, "mmse": P.mmse,
            "omlsa": P.advanced_mmse}[alg]


def _oracle(alg, seed, seconds, n_fft, hop, cell, minstat=None):
    """The oracle's plugin function of gain_ref with the restatement (rounded to
    f32, as the device stores it) in noise_estimation's place."""
    x = _pair(seed, seconds)[1]
    L = len(x)
    Y, power = _analysis(seed, seconds, n_fft, hop)
    eps = 1e-12 if alg == "mmse" else 1e-10
    N = _minstat_ref.minstat(power.T, eps, **(minstat or {})).T.astype(np.float64)
    if alg == "ss":
        N = np.maximum(N, eps)
        S = gain_ref.ss_spectrum(Y, power, N, cell["alpha"], cell["beta"])
        return oracle.fix_length(oracle.istft(S, hop_length=hop, win_length=n_fft, length=L),
                                 size=L)
    if alg == "wiener":
        N = np.maximum(N, eps)
        G = gain_ref.wiener_gains(power, N, cell["alpha"], cell["gain_floor"], eps)
        return oracle.istft(Y * G, hop_length=hop, win_length=n_fft, length=L)
    if alg == "mmse":
        N = gain_ref.smooth_noise(N, cell["noise_mu"])
        G = gain_ref.mmse_gains(power, N, cell["alpha"], cell["ksi_min"], cell["gain_min"],
                                cell["gain_max"], eps)
        return oracle.istft(Y * G, hop_length=hop, win_length=n_fft, length=L)
    N = gain_ref.smooth_noise(np.maximum(N, eps), cell["noise_mu"])
    G = gain_ref.omlsa_gains(power, N, cell["alpha"], cell["ksi_min"], cell["q"],
                             cell["gain_floor"], eps)
    y = oracle.istft(Y * G, hop_length=hop, win_length=n_fft, length=L)
    return oracle.fix_length(y, size=L)


@pytest.mark.parametrize("n_fft,hop", SHAPES)
@pytest.mark.parametrize("alg", list(CELLS))
def test_plugins_match_composed_oracle(P, alg, n_fft, hop):
    noisy = _pair(3, 1.0)[1]
    y = _fn(P, alg)(noisy, 16000, n_fft=n_fft, hop_length=hop, noise_percentile=10.0,
                    noise_method="minstat", **CELLS[alg])
    ref = _oracle(alg, 3, 1.0, n_fft, hop, CELLS[alg])
    e2, em = rel_l2(y, ref), rel_max(y, ref)
    print(f"{alg} {n_fft}/{hop}: rel-L2 {e2:.2e}, rel-max {em:.2e}")
    assert y.dtype == np.float64 and y.shape == ref.shape
    assert e2 <= TOL and em <= TOL, (alg, n_fft, hop, e2, em)


def test_plugin_takes_parameters_through_the_minstat_keyword(P):
    noisy = _pair(3, 1.0)[1]
    prm = dict(sub_windows=4, sub_frames=6, av=1.0, alpha_max=0.9, slope_max=(4.0, 3.0, 2.0, 1.5))
    kw = dict(n_fft=512, hop_length=128, noise_percentile=10.0, noise_method="minstat",
              **CELLS["wiener"])
    y = P.wiener_filter(noisy, 16000, minstat=prm, **kw)
    ref = _oracle("wiener", 3, 1.0, 512, 128, CELLS["wiener"], minstat=prm)
    e2, em = rel_l2(y, ref), rel_max(y, ref)
    print(f"wiener, minstat={prm}: rel-L2 {e2:.2e}, rel-max {em:.2e}")
    assert e2 <= TOL and em <= TOL
    # and they matter: the default parameters give another output
    d = rel_l2(P.wiener_filter(noisy, 16000, **kw), ref)
    print(f"defaults against it: rel-L2 {d:.2e}")
    assert d > 1e-3
    # the other trackers' keywords are not read by a minstat cell
    assert np.array_equal(P.wiener_filter(noisy, 16000, minstat=prm, mcra=dict(delta=2.0),
                                          spp=dict(ph_max=0.9), **kw), y)
    with pytest.raises(ValueError, match="sub_frames"):
        P.wiener_filter(noisy, 16000, minstat=dict(sub_frames=1), **kw)
    with pytest.raises(TypeError):
        P.wiener_filter(noisy, 16000, minstat=dict(window_frames=3), **kw)
    for alg in CELLS:
        with pytest.raises(TypeError):
            _fn(P, alg)(noisy, 16000, n_fft=512, hop_length=128, noise_percentile=10.0,
                        noise_method="minstat", minstat=dict(prior_h1=0.3), **CELLS[alg])


@pytest.mark.parametrize("alg", list(CELLS))
def test_three_frame_clip_is_the_simple_path(P, alg):
    """T = 3 < 5: the reference falls back to the static estimate before it
    looks at the method, so minstat and percentile are the same computation."""
    noisy = _pair(3, 1.0)[1][:300]
    kw = dict(n_fft=512, hop_length=128, noise_percentile=10.0, **CELLS[alg])
    a = _fn(P, alg)(noisy, 16000, noise_method="minstat", **kw)
    b = _fn(P, alg)(noisy, 16000, noise_method="percentile", **kw)
    assert a.shape == (300,) and np.array_equal(a, b)
    n = P.noise_estimation(noisy, 16000, method="minstat", n_fft=512, hop_length=128)
    assert n.shape == (257, 1)
    assert np.array_equal(n, P.noise_estimation(noisy, 16000, method="percentile", n_fft=512,
                                                hop_length=128))


# -------------------------------------------------------------------- sweep
CUT = {"spectralSubtractor": dict(alpha=[1.0, 2.0], beta=[0.05]),
       "mmse": dict(alpha=[0.98], ksi_min=[0.01], gain_min=[0.05, 0.1]),
       "wiener": dict(alpha=[0.98], gain_floor=[0.05, 0.1]),
       "omlsa": dict(alpha=[0.9], ksi_min=[0.01], gain_floor=[0.1], noise_mu=[0.95],
                     q=[0.3, 0.5])}
METHODS = ("min_tracking", "mcra", "spp", "minstat")


def test_sweep_with_minstat_cells(eng):
    import torch
    from classical_speech_enhancement_amd.engine import snr_db
    grids = parameter_ranges.grids_with_noise_methods(METHODS)
    for alg, g in grids.items():
        g.update(CUT[alg], n_fft=[512], hop_length=[128])
    pairs = [_pair(s, 1.0) for s in (0, 3)]
    clean, noisy = [c for c, _ in pairs], [x for _, x in pairs]
    specs = search.job_specs(2, grids=grids)
    assert len(specs) == 2 * 4 * 16
    table, best = search.run_grid(clean, noisy, specs)
    assert table.shape == (len(specs), search.NCOL) and (table[:, 2] == 1).all()
    assert np.isfinite(table[:, :3]).all()  # sse, snr, finite (stoi is not scored here)
    checked = 0
    for cid, (pair, alg, p) in enumerate(specs):
        if p["noise_method"] != "minstat":
            continue
        x = torch.as_tensor(noisy[pair]).cuda().view(1, -1)
        c = torch.as_tensor(clean[pair]).cuda().view(1, -1)
        res = eng.run(x, [(0, alg, p)], clean=c, align=True)
        snr = float(snr_db(res["sse"], float(np.dot(clean[pair], clean[pair])))[0])
        assert table[cid, 1] == snr, (cid, alg, p, table[cid, 1], snr)
        checked += 1
    assert checked == len(specs) // 4
    winners = {k: specs[cid][2] for k, (cid, _) in best.items()}
    assert all(cid >= 0 for cid, _ in best.values())
    for (pair, alg), (cid, score) in best.items():
        assert specs[cid][0] == pair and specs[cid][1] == alg and score == table[cid, 1]
    # the winners' params name their estimator; which one wins is not asserted
    print({k: (p["noise_method"], round(best[k][1], 2)) for k, p in winners.items()})
    assert all(p["noise_method"] in METHODS for p in winners.values())
    by = {m: max(table[cid, 1] for cid, (_, _, p) in enumerate(specs) if p["noise_method"] == m)
          for m in METHODS}
    print("best SNR per estimator:", {m: round(float(v), 2) for m, v in by.items()})
