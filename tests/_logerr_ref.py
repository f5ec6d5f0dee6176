"""numpy restatement of include/cse_logerr.h (the logarithmic estimation error
of a noise-PSD estimate against a reference noise PSD): the reference recursion
is a loop over frames, vectorised over bins, every line one individually
rounded fp64 operation in the header's order (numpy evaluates a * x + c * y as
two rounded products and a rounded sum); the element lines are the header's;
every sum is taken by math.fsum."""

import math

import numpy as np

DEFAULTS = dict(beta=0.9, floor=1e-12, t0=0, bin_lo=0, bin_hi=None)


def reference(Pv, beta=0.9):
    """Pv [T, B] (or [S, T, B]) float64 -> R of the same shape, float64."""
    Pv = np.asarray(Pv, dtype=np.float64)
    if Pv.ndim == 3:
        return np.stack([reference(p, beta) for p in Pv])
    beta = np.float64(beta)
    omb = np.float64(1.0) - beta
    R = np.empty_like(Pv)
    R[0] = Pv[0]
    for t in range(1, Pv.shape[0]):
        R[t] = beta * R[t - 1] + omb * Pv[t]
    return R


def elements(R, N, floor=1e-12):
    """R [T, B] float64, N [T, B] or [B] float32 -> (o, u), each [T, B] float64."""
    R = np.asarray(R, dtype=np.float64)
    N = np.asarray(N)
    assert N.dtype == np.float32, "the estimate is f32"
    Nd = np.broadcast_to(N.astype(np.float64), R.shape)
    floor = np.float64(floor)
    with np.errstate(all="ignore"):
        Rf = np.where(R < floor, floor, R)
        Nf = np.where(Nd < floor, floor, Nd)
        d = 10.0 * np.log10(Rf / Nf)
        o = np.where(d > 0, 0.0, -d)
        u = np.where(d < 0, 0.0, d)
    return o, u


def _fsum(v):
    """math.fsum with IEEE results for non-finite terms (fsum raises on inf - inf)."""
    v = np.asarray(v, dtype=np.float64).ravel()
    if np.all(np.isfinite(v)):
        return math.fsum(v.tolist())
    with np.errstate(all="ignore"):
        return float(np.sum(v))


def score(R, N, floor=1e-12, t0=0, bin_lo=0, bin_hi=None):
    """One row: returns (over, under, frame_over [T], frame_under [T])."""
    R = np.asarray(R, dtype=np.float64)
    T, B = R.shape
    bin_hi = B if bin_hi is None else int(bin_hi)
    o, u = elements(R, N, floor)
    nb = bin_hi - bin_lo
    n = (T - t0) * nb
    Fo = np.full(T, np.nan)
    Fu = np.full(T, np.nan)
    for t in range(t0, T):
        Fo[t] = _fsum(o[t, bin_lo:bin_hi])
        Fu[t] = _fsum(u[t, bin_lo:bin_hi])
    with np.errstate(all="ignore"):
        over = np.float64(_fsum(Fo[t0:])) / np.float64(n)
        under = np.float64(_fsum(Fu[t0:])) / np.float64(n)
        return float(over), float(under), Fo / np.float64(nb), Fu / np.float64(nb)


def score_rows(R, rows, sig_of, t_stride=None, **prm):
    """R [S, T, B]; rows: list of [T, B] or [B] float32 arrays; sig_of: one
    signal index per row; t_stride: per row, default B for a 2-D row and 0 for
    a 1-D one.  A row whose sig_of lies outside [0, S) or whose t_stride is
    neither 0 nor B scores NaN.  Returns (table [n, 3] of (logerr, over, under),
    frames [n, 2, T])."""
    R = np.asarray(R, dtype=np.float64)
    S, T, B = R.shape
    n = len(rows)
    table = np.full((n, 3), np.nan)
    frames = np.full((n, 2, T), np.nan)
    for r, (N, s) in enumerate(zip(rows, sig_of)):
        N = np.asarray(N)
        st = (B if N.ndim == 2 else 0) if t_stride is None else int(t_stride[r])
        if not 0 <= int(s) < S or st not in (0, B):
            continue
        Nr = N if st == B or N.ndim == 1 else N[0]
        ov, un, fo, fu = score(R[int(s)], Nr, **prm)
        with np.errstate(all="ignore"):
            table[r] = (np.float64(ov) + np.float64(un), ov, un)
        frames[r, 0], frames[r, 1] = fo, fu
    return table, frames
