"""numpy restatement of include/cse_imcra.h (IMCRA noise-PSD tracking, Cohen
2003): vectorised over bins, sequential over frames, every line one
individually rounded fp64 operation in the header's order (numpy evaluates
a * x + c * y as two rounded products and a rounded sum).  xi_min comes from
the C math library (math.pow), as in cse_noise_imcra; exp is numpy's, E1 is
scipy.special.exp1 unless another is passed.  e1_plain is a second E1 in plain
numpy that shares nothing with scipy's or the device's: the power series below
1, the continued fraction (modified Lentz) above."""

import math

import numpy as np

DEFAULTS = dict(alpha=0.92, alpha_s=0.9, alpha_d=0.85, beta=1.47, b_min=1.66, gamma0=4.6,
                gamma1=3.0, zeta0=1.67, xi_min_db=-18.0, sub_windows=8, sub_frames=15)
DBL_MIN = np.finfo(np.float64).tiny
EULER = 0.5772156649015329


def e1_plain(v):
    """E1(v) for v > 0 (array), relative error below 1e-13."""
    v = np.asarray(v, dtype=np.float64)
    out = np.zeros_like(v)
    lo = v < 1.0
    x = v[lo]
    s, term = np.zeros_like(x), np.ones_like(x)
    for k in range(1, 26):  # sum (-1)^(k+1) x^k / (k k!): 1 / (25 25!) < 1e-26
        term = term * (-x / k)
        s = s - term / k
    out[lo] = (-np.log(x) - EULER) + s
    x = v[~lo]
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        b = x + 1.0
        c = np.full_like(x, 1e300)
        d = 1.0 / b
        h = d.copy()
        for i in range(1, 200):  # converged to 1e-16 after about 100 terms at x = 1
            a = -float(i * i)
            b = b + 2.0
            d = 1.0 / (a * d + b)
            c = b + a / c
            h = h * (c * d)
        out[~lo] = h * np.exp(-x)
    return out


def _exp1(v):
    from scipy.special import exp1
    return exp1(v)


def _margin(x, thr):
    """min |x - thr| / thr over the finite x."""
    x = x[np.isfinite(x)]
    return float(np.min(np.abs(x - thr)) / thr) if x.size else np.inf


def imcra(P, eps=1e-10, stats=None, e1=None, **params):
    """P [T, B] (or [S, T, B]) float64 power -> N of the same shape, float32.
    stats (a dict, optional) receives 'margin', the smallest relative distance of
    gmin to gamma0, zeta and zt to zeta0, gmt to 1 and to gamma1, and the counts
    'i1' (I = 1), 'i0' (I = 0), 'q0' (qh = 0), 'qf' (0 < qh < 1) and 'q1'
    (qh = 1).  e1: the exponential integral (default scipy.special.exp1)."""
    unknown = set(params) - set(DEFAULTS)
    if unknown:
        raise TypeError(f"imcra takes no parameter {sorted(unknown)[0]!r}")
    P = np.asarray(P, dtype=np.float64)
    if P.ndim == 3:
        parts = [dict() for _ in P]
        out = [imcra(p, eps, st, e1, **params) for p, st in zip(P, parts)]
        if stats is not None:
            stats["margin"] = float(min(st["margin"] for st in parts))
            for key in ("i1", "i0", "q0", "qf", "q1"):
                stats[key] = int(sum(st[key] for st in parts))
        return np.stack(out)
    e1 = e1 or _exp1
    prm = dict(DEFAULTS, **params)
    a, a_s, a_d, beta, b_min, gamma0, gamma1, zeta0 = (np.float64(prm[k]) for k in (
        "alpha", "alpha_s", "alpha_d", "beta", "b_min", "gamma0", "gamma1", "zeta0"))
    c_a, c_s, c_d = 1.0 - a, 1.0 - a_s, 1.0 - a_d
    xi_min = np.float64(math.pow(10.0, float(prm["xi_min_db"]) / 10.0))
    U, V = int(prm["sub_windows"]), int(prm["sub_frames"])
    T, B = P.shape
    b = np.arange(B)
    m, r = np.where(b == 0, 1, b - 1), np.where(b == B - 1, B - 2, b + 1)

    def sm3(X):
        return (0.25 * X[m] + 0.5 * X) + 0.25 * X[r]

    S = sm3(P[0])
    St = S.copy()
    Smin, Ssw, Stmin, Stsw = S.copy(), S.copy(), St.copy(), St.copy()
    SW, SWt = np.tile(S, (U, 1)), np.tile(St, (U, 1))
    lam = P[0].copy()
    n = lam.copy()
    g2g = np.ones(B)
    N = np.empty((T, B))
    N[0] = n
    margin = np.inf
    cnt = dict(i1=0, i0=0, q0=0, qf=0, q1=0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        for t in range(T):
            Pt = P[t]
            if t >= 1:
                S = a_s * S + c_s * sm3(Pt)
                Smin = np.minimum(Smin, S)
                Ssw = np.minimum(Ssw, S)
            gam = Pt / np.maximum(n, DBL_MIN)
            xi = np.maximum(a * g2g + c_a * np.maximum(gam - 1.0, 0.0), xi_min)
            v = (gam * xi) / (1.0 + xi)
            d = np.maximum(b_min * Smin, DBL_MIN)
            gmin = Pt / d
            zeta = S / d
            I = ((gmin < gamma0) & (zeta < zeta0)).astype(np.float64)
            den = sm3(I)
            num = sm3(I * Pt)
            Stf = np.where(den > 0.0, num / den, St)
            if t >= 1:
                St = a_s * St + c_s * Stf
                Stmin = np.minimum(Stmin, St)
                Stsw = np.minimum(Stsw, St)
            dt = np.maximum(b_min * Stmin, DBL_MIN)
            gmt = Pt / dt
            zt = S / dt
            qh = np.where(zt >= zeta0, 0.0,
                          np.where(gmt <= 1.0, 1.0,
                                   np.where(gmt < gamma1, (gamma1 - gmt) / (gamma1 - 1.0), 0.0)))
            emv = np.exp(-v)
            p = np.where(qh >= 1.0, 0.0,
                         np.where(qh <= 0.0, 1.0,
                                  1.0 / (1.0 + ((qh / (1.0 - qh)) * (1.0 + xi)) * emv)))
            g = xi / (1.0 + xi)
            ee = np.exp(np.minimum(e1(np.maximum(v, DBL_MIN)), 700.0))
            g2g = np.where(Pt == 0.0, 0.0, ((g * g) * ee) * gam)
            ad = a_d + c_d * p
            lam = ad * lam + (1.0 - ad) * Pt
            n = beta * lam
            if t + 1 < T:
                N[t + 1] = n
            if (t + 1) % V == 0:
                k = ((t + 1) // V - 1) % U
                SW[k] = Ssw
                Smin = SW.min(axis=0)
                Ssw = S.copy()
                SWt[k] = Stsw
                Stmin = SWt.min(axis=0)
                Stsw = St.copy()
            margin = min(margin, _margin(gmin, gamma0), _margin(zeta, zeta0), _margin(zt, zeta0),
                         _margin(gmt, 1.0), _margin(gmt, gamma1))
            cnt["i1"] += int(I.sum())
            cnt["i0"] += int(B - I.sum())
            cnt["q0"] += int((qh <= 0.0).sum())
            cnt["q1"] += int((qh >= 1.0).sum())
            cnt["qf"] += int(((qh > 0.0) & (qh < 1.0)).sum())
    if stats is not None:
        stats["margin"] = float(margin)
        stats.update(cnt)
    return np.maximum(N, eps).astype(np.float32)
