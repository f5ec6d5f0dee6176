"""The fp64 oracle STFT that tests/test_gpu_stft.py measures cse_stft against,
checked on the CPU: inside stft_bound of a long-double direct DFT, the right
shape and finite at every case of the table, and on the analytic three-line
spectrum of a windowed cosine.  The frames come from np.pad here and from the
oracle's own index map there, so the reflect rule is checked twice."""

import numpy as np
import pytest

import oracle
import _stft_cases as sc

SMALL = [c for c in sc.CASES if c[0] <= 512]


def test_table_names_every_arm():
    """Every arm of cse_stft's switch, the direct DFT above 2048, hop 1 and
    hop = n_fft, three signals per kernel form, and both T % 4 classes."""
    sizes = {c[0] for c in sc.CASES}
    assert {64, 128, 256, 512, 1024, 2048, 4096, 66, 400, 4000, 4094, 130} <= sizes
    assert {sc.form(c[0]) for c in sc.CASES if c[3] == 3} == {"radix2", "r512", "dft"}
    assert {(1 + c[2] // c[1]) % 16 for c in sc.CASES if c[0] == 512 and c[2] >= 1800} \
        >= {0, 1, 15}
    for n in (64, 130):
        assert any(c[0] == n and c[1] == 1 for c in sc.CASES)
    for n in (64, 512, 400, 4096):
        assert any(c[0] == n and c[1] == n for c in sc.CASES)
    assert any(c[0] > 2048 and sc.form(c[0]) == "dft" for c in sc.CASES)
    assert len({sc.case_id(c) for c in sc.CASES}) == len(sc.CASES)


@pytest.mark.parametrize("case", sc.CASES, ids=sc.case_id)
def test_oracle_shape_finite_and_frames(case):
    """oracle.stft at every case: (n_fft/2 + 1, 1 + len // hop), finite, and
    equal to numpy's rfft of the np.pad-built frames to rounding (the oracle
    takes the same rfft of frames from its own reflect index map: any
    difference is a frame that holds other samples)."""
    n_fft, hop, length, n_sig, _ = case
    x = sc.signals(case)
    assert x.shape == (n_sig, length) and x.dtype == np.float64
    for s in range(n_sig):
        X = oracle.stft(x[s], n_fft=n_fft, hop_length=hop)
        assert X.shape == (n_fft // 2 + 1, 1 + length // hop)
        assert np.all(np.isfinite(X.real)) and np.all(np.isfinite(X.imag))
        fw = sc.frames_windowed(x[s], n_fft, hop)
        ref = np.fft.rfft(fw, axis=1).T
        tol = sc.stft_bound(fw, n_fft)[None, :]
        assert np.all(np.abs(X.real - ref.real) <= tol)
        assert np.all(np.abs(X.imag - ref.imag) <= tol)


@pytest.mark.parametrize("case", SMALL, ids=sc.case_id)
def test_oracle_within_bound_of_longdouble_dft(case):
    n_fft, hop, length, n_sig, _ = case
    x = sc.signals(case)
    worst = 0.0
    for s in range(n_sig):
        X = oracle.stft(x[s], n_fft=n_fft, hop_length=hop)
        fw = sc.frames_windowed(x[s], n_fft, hop)
        tol = sc.stft_bound(fw, n_fft)
        for t in range(fw.shape[0]):
            re, im = sc.direct_dft_longdouble(fw[t])
            err = max(float(np.max(np.abs(X[:, t].real - re))),
                      float(np.max(np.abs(X[:, t].imag - im))))
            assert err <= tol[t], (t, err, tol[t])
            worst = max(worst, err / tol[t]) if tol[t] > 0 else worst
    print(f"{sc.case_id(case)}: worst err / tol {worst:.2e}")


def test_oracle_within_bound_one_frame_of_4094():
    case = next(c for c in sc.CASES if c[0] == 4094)
    n_fft, hop, length, _, _ = case
    x = sc.signals(case)[0]
    X = oracle.stft(x, n_fft=n_fft, hop_length=hop)
    fw = sc.frames_windowed(x, n_fft, hop)
    tol = sc.stft_bound(fw, n_fft)
    t = 2  # an interior frame
    re, im = sc.direct_dft_longdouble(fw[t])
    err = max(float(np.max(np.abs(X[:, t].real - re))), float(np.max(np.abs(X[:, t].imag - im))))
    print(f"4094: err / tol {err / tol[t]:.2e}")
    assert err <= tol[t]


def test_bound_scales_with_the_frame():
    """stft_bound is 2 n_fft 2**-53 sum |xw| per frame: linear in the frame,
    zero for a zero frame, one value per frame."""
    fw = np.array([[1.0, -2.0, 0.5, 0.0], [0.0, 0.0, 0.0, 0.0]])
    b = sc.stft_bound(fw, 64)
    assert b.shape == (2,) and b[1] == 0.0
    assert b[0] == 2 * 64 * 2.0 ** -53 * 3.5
    assert np.array_equal(sc.stft_bound(4 * fw, 64), 4 * b)


@pytest.mark.parametrize("N,hop,k0", sc.PIN_CASES)
def test_analytic_pin_holds_for_the_oracle(N, hop, k0):
    """A cos(2 pi k0 n / N): every interior frame has |X[k0]| = A N / 4,
    |X[k0 +- 1]| = A N / 8 and nothing elsewhere, within the bound."""
    length = sc.pin_length(N, hop)
    x = sc.pin_signal(N, k0, length)
    X = oracle.stft(x, n_fft=N, hop_length=hop)
    tol = sc.stft_bound(sc.frames_windowed(x, N, hop), N)
    ts = sc.pin_interior(N, hop, length)
    assert len(ts) >= 3
    mag = sc.pin_expected(N, k0)
    P = np.abs(X) ** 2
    for t in ts:
        assert np.all(np.abs(P[:, t] - mag ** 2) <= 2 * mag * tol[t] + tol[t] ** 2), t
    assert P[k0, ts[0]] > 1e20 * tol[ts[0]] ** 2  # the pin is not vacuous


@pytest.mark.parametrize("n_fft,hop,length", sc.NORM_CASES)
def test_istft_norm_reference(n_fft, hop, length):
    """The reference of the cse_istft_norm test: 1 / wss where the window sum
    is positive, 1 elsewhere; at hop = n_fft the window's zero falls on output
    samples (hop t - n_fft/2), and only there."""
    inv, dead = sc.istft_norm_ref(n_fft, hop, length)
    assert inv.shape == (length,) and np.all(np.isfinite(inv)) and np.all(inv > 0)
    assert np.all(inv[dead] == 1.0)
    if hop == n_fft:
        want = [o for o in range(length) if (o + n_fft // 2) % hop == 0]
        assert want and list(np.flatnonzero(dead)) == want
    else:
        assert not dead.any()
