"""numpy restatement of include/cse_mcra.h (minima-controlled recursive
averaging, Cohen & Berdugo 2002): vectorised over bins, sequential over frames,
every line one individually rounded fp64 operation in the header's order
(numpy evaluates a * x + c * y as two rounded products and a rounded sum)."""

import numpy as np

DEFAULTS = dict(alpha_s=0.8, alpha_d=0.95, alpha_p=0.2, delta=5.0, window_frames=125)


def mcra(P, eps=1e-10, alpha_s=0.8, alpha_d=0.95, alpha_p=0.2, delta=5.0, window_frames=125,
         stats=None):
    """P [T, B] (or [S, T, B]) float64 power -> N of the same shape, float32.
    stats (a dict, optional) receives 'indicator_share', the share of (t, b)
    with I = 1, 'restarts', the number of window restarts, and 'indicator',
    the bool array of I in P's shape."""
    P = np.asarray(P, dtype=np.float64)
    if P.ndim == 3:
        parts = [dict() for _ in P]
        out = np.stack([mcra(p, eps, alpha_s, alpha_d, alpha_p, delta, window_frames, st)
                        for p, st in zip(P, parts)])
        if stats is not None:
            stats["indicator_share"] = float(np.mean([st["indicator_share"] for st in parts]))
            stats["restarts"] = parts[0]["restarts"] if parts else 0
            stats["indicator"] = np.stack([st["indicator"] for st in parts])
        return out
    T, B = P.shape
    a_s, a_d, a_p, delta = (np.float64(v) for v in (alpha_s, alpha_d, alpha_p, delta))
    c_s, c_d, c_p = 1.0 - a_s, 1.0 - a_d, 1.0 - a_p
    L = int(window_frames)
    b = np.arange(B)
    m = np.where(b == 0, 1, b - 1)
    q = np.where(b == B - 1, B - 2, b + 1)

    def sf(t):
        return (0.25 * P[t, m] + 0.5 * P[t]) + 0.25 * P[t, q]
    N = np.empty((T, B), dtype=np.float64)
    ind_all = np.zeros((T, B), dtype=bool)
    restarts = 0
    for t in range(T):
        if t == 0:
            S = sf(0)
            Smin, Stmp = S.copy(), S.copy()
            p = np.zeros(B)
            lam = P[0].copy()
            N[0] = lam
        else:
            S = a_s * S + c_s * sf(t)
            if t % L == 0:
                Smin, Stmp = np.minimum(Stmp, S), S.copy()
                restarts += 1
            else:
                Smin, Stmp = np.minimum(Smin, S), np.minimum(Stmp, S)
        ind = (S > delta * Smin).astype(np.float64)
        ind_all[t] = ind != 0
        p = a_p * p + c_p * ind
        ad = a_d + c_d * p
        lam = ad * lam + (1.0 - ad) * P[t]
        if t + 1 < T:
            N[t + 1] = lam
    if stats is not None:
        stats["indicator_share"] = float(ind_all.mean())
        stats["restarts"] = restarts
        stats["indicator"] = ind_all
    return np.maximum(N, eps).astype(np.float32)
