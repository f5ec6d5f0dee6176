"""numpy restatement of include/cse_spp.h (SPP-based MMSE noise-PSD tracking,
Gerkmann & Hendriks 2012): vectorised over bins, sequential over frames, every
line one individually rounded fp64 operation in the header's order (numpy
evaluates a * x + c * y as two rounded products and a rounded sum).  The
host-side constants come from the C math library (math.pow, math.log), as in
cse_noise_spp; exp is numpy's."""

import math

import numpy as np

DEFAULTS = dict(prior_h1=0.5, xi_opt_db=15.0, alpha_pow=0.8, alpha_ph=0.9, ph_max=0.99,
                init_frames=5)
DBL_MIN = np.finfo(np.float64).tiny


def spp(P, eps=1e-10, prior_h1=0.5, xi_opt_db=15.0, alpha_pow=0.8, alpha_ph=0.9, ph_max=0.99,
        init_frames=5, stats=None, exp=np.exp):
    """P [T, B] (or [S, T, B]) float64 power -> N of the same shape, float32.
    stats (a dict, optional) receives 'clamped_share', the share of (t, b)
    where the guard lowered ph, 'capped', the count of a cut at 200, and
    'margin', min |pm - ph_max|.  exp: the exponential (a test may perturb it)."""
    P = np.asarray(P, dtype=np.float64)
    if P.ndim == 3:
        parts = [dict() for _ in P]
        out = [spp(p, eps, prior_h1, xi_opt_db, alpha_pow, alpha_ph, ph_max, init_frames, st, exp)
               for p, st in zip(P, parts)]
        if stats is not None:
            stats["clamped_share"] = float(np.mean([st["clamped_share"] for st in parts]))
            stats["capped"] = int(sum(st["capped"] for st in parts))
            stats["margin"] = float(min(st["margin"] for st in parts))
        return np.stack(out)
    T, B = P.shape
    prior_h1, ph_max = np.float64(prior_h1), np.float64(ph_max)
    a_pow, a_ph = np.float64(alpha_pow), np.float64(alpha_ph)
    c_pow, c_ph = 1.0 - a_pow, 1.0 - a_ph
    prior = prior_h1 / (1.0 - prior_h1)
    xi = math.pow(10.0, float(xi_opt_db) / 10.0)
    c0 = np.float64(math.log(1.0 / (1.0 + xi)))
    c1 = np.float64(xi / (1.0 + xi))
    K = min(int(init_frames), T)
    lam = P[0].copy()
    for t in range(1, K):
        lam = lam + P[t]
    lam = lam / np.float64(K)
    pm = np.full(B, prior_h1)
    N = np.empty((T, B), dtype=np.float64)
    clamped, capped, margin = 0, 0, np.inf
    for t in range(T):
        s = P[t] / np.maximum(lam, DBL_MIN)
        a = c0 + c1 * s
        capped += int((a > 200.0).sum())
        a = np.minimum(a, 200.0)
        g = prior * exp(a)
        ph = g / (1.0 + g)
        pm = a_ph * pm + c_ph * ph
        margin = min(margin, float(np.abs(pm - ph_max).min()))
        guard = pm > ph_max
        clamped += int((guard & (ph > ph_max)).sum())
        ph = np.where(guard, np.minimum(ph, ph_max), ph)
        est = ph * lam + (1.0 - ph) * P[t]
        lam = a_pow * lam + c_pow * est
        N[t] = lam
    if stats is not None:
        stats["clamped_share"] = clamped / float(T * B)
        stats["capped"] = capped
        stats["margin"] = margin
    return np.maximum(N, eps).astype(np.float32)
