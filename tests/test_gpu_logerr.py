"""Noise-PSD LogErr on the device (needs an MI355X: -m gpu): cse_logerr_reference
against the numpy restatement of include/cse_logerr.h bit for bit,
cse_logerr_rows against it within the tolerance tests/_logerr_cases.py derives
(1e-9 dB absolute on over, under and every frame value; non-finite values by
class), each row alone against the same row in a launch bit for bit, and the
seven estimators and the mcra sweep end to end.  The device is compared with the
restatement only, never with itself.

Worst differences seen on the MI355X (tolerance 1e-9 dB): 1.8e-15 dB over every
shape, launch, frame and bin range of test_scores_equal_restatement; 1.8e-15 dB
over the seven estimators of test_estimators_end_to_end (8.9e-16 on the two
512 / 128 pairs); cse_logerr_reference equal to the restatement in every bit.
"""

import ctypes

import numpy as np
import pytest

import _logerr_cases as cases
import _logerr_ref as ref
from classical_speech_enhancement_amd import _lib, search

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return Dev()


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class Dev:
    """The two entry points on arrays, through the C ABI."""

    def __init__(self):
        import torch
        self.torch = torch
        self.lib = _lib.load()

    def up(self, a):
        return self.torch.as_tensor(np.ascontiguousarray(a)).cuda()

    def reference(self, Pv, beta):
        S, T, B = Pv.shape
        Pd = self.up(Pv)
        R = self.torch.full_like(Pd, -1.0)
        _lib.check(self.lib.cse_logerr_reference(_ptr(Pd), S, T, B, float(beta), _ptr(R), None),
                   "cse_logerr_reference")
        return R.cpu().numpy()

    def rows(self, R, rows, sig_of, t_stride=None, floor=1e-12, t0=0, bin_lo=0, bin_hi=None,
             frames=True):
        """One launch: the rows packed into one buffer, static rows taking B
        elements and the others T * B.  Returns (table [n, 3], frames [n, 2, T]
        or None)."""
        torch = self.torch
        S, T, B = R.shape
        n = len(rows)
        flat = [np.asarray(N, dtype=np.float32).ravel() for N in rows]
        off = np.concatenate([[0], np.cumsum([len(x) for x in flat])[:-1]]).astype(np.int64)
        st = np.array([B if np.ndim(N) == 2 else 0 for N in rows] if t_stride is None
                      else t_stride, dtype=np.int64)
        Nd = self.up(np.concatenate(flat))
        Rd = R if torch.is_tensor(R) else self.up(R)
        prm = _lib.LogErrParams()
        self.lib.cse_logerr_default_params(ctypes.byref(prm), B)
        prm.floor, prm.t0, prm.bin_lo = floor, t0, bin_lo
        prm.bin_hi = B if bin_hi is None else bin_hi
        scratch = torch.empty(max(int(self.lib.cse_logerr_scratch_bytes(n, T)), 1),
                              dtype=torch.uint8, device="cuda")
        out = torch.full((2, n), -1.0, dtype=torch.float64, device="cuda")
        fr = torch.full((2, n, T), -1.0, dtype=torch.float64, device="cuda") if frames else None
        off_d, st_d = self.up(off), self.up(st)  # alive until the launch has run
        sig_d = self.up(np.asarray(sig_of, dtype=np.int32))
        _lib.check(self.lib.cse_logerr_rows(
            _ptr(Rd), S, T, B, _ptr(Nd), _ptr(off_d), _ptr(st_d), _ptr(sig_d), n, ctypes.byref(prm),
            _ptr(scratch), _ptr(out[0]), _ptr(out[1]), None if fr is None else _ptr(fr[0]),
            None if fr is None else _ptr(fr[1]), None), "cse_logerr_rows")
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        with np.errstate(invalid="ignore"):
            table = np.stack([o[0] + o[1], o[0], o[1]], axis=1)
        return table, (None if fr is None else fr.cpu().numpy().transpose(1, 0, 2))


# ------------------------------------------------------- reference: bit equality
@pytest.mark.parametrize("beta", cases.BETAS)
@pytest.mark.parametrize("T,B", cases.R_SHAPES)
def test_reference_equals_restatement(dev, T, B, beta):
    Pv = cases.power_with_specials(T, B, T * 7 + B)
    assert (Pv == 0).any() and ((Pv > 0) & (Pv < 2.3e-308)).any()
    want = ref.reference(Pv, beta)
    got = dev.reference(Pv, beta)
    diff = np.argwhere(got.view(np.int64) != want.view(np.int64))
    assert len(diff) == 0, (len(diff), diff[:4].tolist())
    if beta == 0.0:
        assert np.array_equal(got, Pv)


# ---------------------------------------------------- scores: derived tolerance
def _launches(T, B):
    out = dict(cases.LAUNCHES)
    if T * B <= 5 * 257:
        out["many"] = cases.MANY
    return out


@pytest.mark.parametrize("T,B", cases.SCORE_SHAPES)
def test_scores_equal_restatement(dev, T, B):
    """Every launch of _logerr_cases at every (t0, bins) set, with the frame
    outputs and, on every other one, without.  Worst difference on the MI355X:
    1.8e-15 dB (8.9e-16 at (1, 33) and (63, 513))."""
    k = cases.SCORE_SHAPES.index((T, B))
    R = cases.score_reference(T, B, k)
    worst, j = 0.0, 0
    for name, launch in _launches(T, B).items():
        rows = cases.make_rows(R, launch, k)
        sig = [s for s, _ in launch]
        for t0, lo, hi in cases.param_sets(T, B):
            want_t, want_f = cases.checked(R, rows, sig, t0=t0, bin_lo=lo, bin_hi=hi)
            frames = j % 2 == 0
            j += 1
            got_t, got_f = dev.rows(R, rows, sig, t0=t0, bin_lo=lo, bin_hi=hi, frames=frames)
            w = cases.same(got_t[:, 1:], want_t[:, 1:])
            w = max(w, cases.same(got_t[:, 0], want_t[:, 0], 2 * cases.TOL))
            if frames:
                w = max(w, cases.same(got_f, want_f))
            print(f"T={T} B={B} {name} t0={t0} bins=[{lo},{hi}) frames={frames}: worst {w:.2e}")
            worst = max(worst, w)
    print(f"T={T} B={B}: worst difference {worst:.2e} dB")


def test_special_values_and_invalid_rows(dev):
    """NaN and +inf in N, both sides below the floor, exact powers of two, and
    the rows the header declares invalid, in one launch."""
    T, B = 5, 33
    R = 2.0 ** np.random.default_rng(0).integers(-20, 4, size=(2, T, B)).astype(np.float64)
    R[1, 2, :4] = 1e-15
    f32 = np.float32
    nan_row = R[0].astype(f32)
    nan_row[3, 32] = np.nan
    inf_row = R[1].astype(f32)
    inf_row[0, 0] = np.inf
    low = R[1].astype(f32)
    low[2, :4] = 1e-20
    rows = [(4.0 * R[0]).astype(f32), nan_row, inf_row, low, (0.125 * R[1][0]).astype(f32),
            R[0].astype(f32), R[0].astype(f32), R[0].astype(f32), R[0].astype(f32)]
    sig = [0, 0, 1, 1, 1, -1, 2, 0, 1]
    st = [B, B, B, B, 0, B, B, B - 1, 1]
    want_t, want_f = ref.score_rows(R, rows, sig, t_stride=st)
    got_t, got_f = dev.rows(R, rows, sig, t_stride=st)
    cases.same(got_t, want_t)
    cases.same(got_f, want_f)
    assert got_t[0, 1] == pytest.approx(10 * np.log10(4.0), abs=1e-12) and got_t[0, 2] == 0.0
    assert np.isnan(got_t[1]).all() and np.isnan(got_f[1, :, 3]).all()
    assert np.isfinite(got_f[1, :, :3]).all()
    assert got_t[2, 1] == np.inf and got_t[2, 2] == 0.0 and got_t[2, 0] == np.inf
    assert got_t[3, 1] == 0.0 and got_t[3, 2] == 0.0
    assert np.isnan(got_t[5:]).all() and np.isnan(got_f[5:]).all()
    # t0 > 0: NaN frames in front, on valid and invalid rows alike
    got_t, got_f = dev.rows(R, rows, sig, t_stride=st, t0=2, bin_lo=4, bin_hi=30)
    want_t, want_f = ref.score_rows(R, rows, sig, t_stride=st, t0=2, bin_lo=4, bin_hi=30)
    cases.same(got_t, want_t)
    cases.same(got_f, want_f)
    assert np.isnan(got_f[:, :, :2]).all()


# ------------------------------------------------------------------ determinism
@pytest.mark.parametrize("T,B", [(5, 257), (65, 257), (9, 2049), (501, 33)])
def test_a_row_alone_gives_the_bits_it_gives_in_a_launch(dev, T, B):
    k = cases.SCORE_SHAPES.index((T, B))
    R = cases.score_reference(T, B, k)
    launch = cases.MANY if T * B <= 5 * 257 else cases.LAUNCHES["mixed"]
    rows = cases.make_rows(R, launch, k)
    sig = [s for s, _ in launch]
    for t0, lo, hi in ((0, 0, B), (T - 1, 1, B - 1)):
        batch_t, batch_f = dev.rows(R, rows, sig, t0=t0, bin_lo=lo, bin_hi=hi)
        rev_t, rev_f = dev.rows(R, rows[::-1], sig[::-1], t0=t0, bin_lo=lo, bin_hi=hi)
        assert np.array_equal(rev_t[::-1].view(np.int64), batch_t.view(np.int64))
        assert np.array_equal(rev_f[::-1].view(np.int64), batch_f.view(np.int64))
        for r in range(0, len(rows), max(1, len(rows) // 6)):
            one_t, one_f = dev.rows(R, [rows[r]], [sig[r]], t0=t0, bin_lo=lo, bin_hi=hi)
            assert np.array_equal(one_t[0].view(np.int64), batch_t[r].view(np.int64)), r
            assert np.array_equal(one_f[0].view(np.int64), batch_f[r].view(np.int64)), r
            no_f, none = dev.rows(R, [rows[r]], [sig[r]], t0=t0, bin_lo=lo, bin_hi=hi,
                                  frames=False)
            assert none is None and np.array_equal(no_f.view(np.int64), one_t.view(np.int64))


# ------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def eng(dev):
    from classical_speech_enhancement_amd.engine import Engine
    return Engine()


@pytest.mark.parametrize("i,seconds,n_fft,hop", cases.PAIRS)
def test_estimators_end_to_end(dev, eng, i, seconds, n_fft, hop):
    """The seven estimators at their defaults, made on the device, scored by
    NoiseErrPlan and by the restatement on the same N and the device's own Pv;
    the plan's R is the restatement's bit for bit; N = R.float() scores below
    1e-6 dB in both parts."""
    from classical_speech_enhancement_amd.metrics import NoiseErrPlan, noise_logerr
    clean, noisy = cases.pair(i, seconds)
    cd, zd = dev.up(clean[None]), dev.up(noisy[None])
    plan = NoiseErrPlan(cd, zd, n_fft, hop)
    _, P = eng.stft(zd, n_fft, hop, want_y=False)
    _, Pv = eng.stft(zd, n_fft, hop, x_sub=cd, want_y=False)
    R = ref.reference(Pv.cpu().numpy(), 0.9)
    assert np.array_equal(plan.R.cpu().numpy().view(np.int64), R.view(np.int64))
    assert (plan.T, plan.B) == R.shape[1:] == (1 + len(clean) // hop, n_fft // 2 + 1)
    ests = [eng.noise_estimate(m, Pv if m == "true_noise" else P) for m in cases.ESTIMATORS]
    assert [e.dim() for e in ests] == [2, 3, 3, 3, 3, 3, 3]
    got_t, got_f = plan.score(ests, [0] * 7, per_frame=True)
    rows = [e[0].cpu().numpy() for e in ests]
    want_t, want_f = cases.checked(R, rows, [0] * 7)
    w = max(cases.same(got_t[:, 1:], want_t[:, 1:]), cases.same(got_f, want_f))
    for m, row in zip(cases.ESTIMATORS, got_t):
        print(f"pair {i} {seconds}s {n_fft}/{hop} {m}: logerr {row[0]:.3f} over {row[1]:.3f} "
              f"under {row[2]:.3f} dB")
    print(f"worst difference {w:.2e} dB")
    assert np.array_equal(got_t[:, 0], got_t[:, 1] + got_t[:, 2])
    # one tensor, sig_of by default, no frames: the same bits
    alone = plan.score(ests[3])
    assert np.array_equal(alone.view(np.int64), got_t[3:4].view(np.int64))
    exact = plan.score(plan.R.float())
    assert 0.0 <= exact[0, 1] < 1e-6 and 0.0 <= exact[0, 2] < 1e-6
    assert ref.score(R[0], R[0].astype(np.float32))[0] < 1e-6
    # the numpy convenience, on plugins.noise_estimation's shapes
    d = noise_logerr(clean, noisy, rows[3].T.astype(np.float64), n_fft, hop, per_frame=True)
    assert (d["logerr"], d["over"], d["under"]) == tuple(got_t[3])
    assert np.array_equal(d["frame_under"], got_f[3, 1])
    d0 = noise_logerr(clean, noisy, rows[0].astype(np.float64)[:, None], n_fft, hop)
    assert (d0["logerr"], d0["over"], d0["under"]) == tuple(got_t[0])
    assert noise_logerr(clean, noisy, rows[0], n_fft, hop) == d0
    for bad in (ests[3][:, :-1], ests[0][:, :-1], ests[3].double(), ests[3].cpu()):
        with pytest.raises(ValueError):
            plan.score(bad)
    with pytest.raises(ValueError):
        plan.score([ests[3], ests[0]])  # two rows, one signal, no sig_of
    with pytest.raises(ValueError):
        plan.score(ests[3], [1])


def test_plan_parameters_reach_the_kernel(dev):
    clean, noisy = cases.pair(1, 0.5)
    from classical_speech_enhancement_amd.metrics import NoiseErrPlan
    cd, zd = dev.up(np.stack([clean, noisy * 0.5])), dev.up(np.stack([noisy, clean]))
    plan = NoiseErrPlan(cd, zd, 64, 16, beta=0.5, floor=1e-9, skip_frames=7, bins=(2, 30))
    N = (plan.R * 3.0).float()
    got_t, got_f = plan.score(N, per_frame=True)
    R = plan.R.cpu().numpy()
    want_t, want_f = cases.checked(R, list(N.cpu().numpy()), [0, 1], floor=1e-9, t0=7, bin_lo=2,
                                   bin_hi=30)
    cases.same(got_t[:, 1:], want_t[:, 1:])
    cases.same(got_f, want_f)
    assert np.isnan(got_f[:, :, :7]).all()
    swapped = plan.score(N, [1, 0])
    assert not np.array_equal(swapped, got_t)


def test_score_noise_estimators_and_sweep(dev, eng):
    """score_noise_estimators over pairs of two lengths, and sweep_tracker over
    mcra on the 512 / 128 pairs and on the 64 / 16 pair: mcra's contract is bit
    equality, so the device's N is _mcra_ref's on the device's P, and the sweep
    must return the restatement's best_index, (0.85, 5, 8)."""
    pairs = [cases.pair(i, s) for i, s, _, _ in cases.PAIRS]
    clean, noisy = [p[0] for p in pairs], [p[1] for p in pairs]
    ests = [(m, {}) for m in cases.ESTIMATORS] + [("mcra", dict(window_frames=8))]
    table = search.score_noise_estimators(clean, noisy, ests)
    assert table.shape == (3, 8, 3) and np.all(np.isfinite(table))
    assert np.array_equal(table[:, :, 0], table[:, :, 1] + table[:, :, 2])
    assert not np.array_equal(table[:, 3], table[:, 7])
    for group, n_fft, hop in (((0, 1), 512, 128), ((2,), 64, 16)):
        cl, nz = [clean[g] for g in group], [noisy[g] for g in group]
        res = search.sweep_tracker(cl, nz, "mcra", cases.SWEEP_RANGES, n_fft=n_fft,
                                   hop_length=hop)
        per_pair = []
        for c, z in zip(cl, nz):
            cd, zd = dev.up(c[None]), dev.up(z[None])
            P = eng.stft(zd, n_fft, hop, want_y=False)[1][0].cpu().numpy()
            Pv = eng.stft(zd, n_fft, hop, x_sub=cd, want_y=False)[1][0].cpu().numpy()
            means, cells = cases.sweep_means(P, Pv)
            cases.check_sweep_gap(means)
            per_pair.append(means)
        want = np.mean(per_pair, axis=0)
        win = cases.check_sweep_gap(want)
        cases.same(res["table"][:, :, 0].T, np.array(per_pair).T, 2 * cases.TOL)
        assert res["params"] == cells
        assert res["best_index"] == win and res["best_params"] == cases.SWEEP_WINNER
        if n_fft == 512:
            assert np.array_equal(res["table"][:, 6], table[:2, 7])  # the same set, the same bits
