"""numpy restatement of include/cse_minstat.h (minimum-statistics noise-PSD
tracking, Martin 2001): vectorised over bins, sequential over frames, every
line one individually rounded fp64 operation in the header's order (numpy
evaluates a * x + c * y as two rounded products and a rounded sum).  The three
sums over the bins are numpy's pairwise sums; pow and sqrt are numpy's."""

import math

import numpy as np

DEFAULTS = dict(alpha_c=0.837, alpha_c_floor=0.7, alpha_max=0.98, alpha_min=0.548,
                snr_exp=-0.125, beta_max=0.894, av=2.12, q_eq_min=2.0, q_eq_max=14.0,
                slope_q=(0.03, 0.05, 0.06), slope_max=(8.0, 4.0, 2.0, 1.2), sub_windows=8,
                sub_frames=24)
DBL_MIN = np.finfo(np.float64).tiny
TABLE_D = (1, 2, 5, 8, 10, 15, 20, 30, 40, 60, 80, 120, 140, 160, 180, 220, 260, 300)
TABLE_M = (0.0, 0.26, 0.48, 0.58, 0.61, 0.668, 0.705, 0.762, 0.8, 0.841, 0.865, 0.89, 0.9, 0.91,
           0.92, 0.93, 0.935, 0.94)


def m_of(d):
    """Martin's M(D), interpolated as the header says."""
    d = int(d)
    if d >= TABLE_D[-1]:
        return TABLE_M[-1]
    for i, di in enumerate(TABLE_D):
        if d == di:
            return TABLE_M[i]
        if d < TABLE_D[i + 1]:
            dj, mi, mj = TABLE_D[i + 1], TABLE_M[i], TABLE_M[i + 1]
            si, sj = math.sqrt(di), math.sqrt(dj)
            return mi + (si * sj / math.sqrt(d) - sj) * (mj - mi) / (si - sj)
    raise ValueError(d)


def _rel(a, b):
    """min |a - b| / |b| over the elements where b is finite and non-zero."""
    a, b = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
    ok = np.isfinite(b) & (b != 0.0) & np.isfinite(a)
    if not ok.any():
        return np.inf
    return float(np.min(np.abs(a[ok] - b[ok]) / np.abs(b[ok])))


def minstat(P, eps=1e-10, stats=None, **params):
    """P [T, B] (or [S, T, B]) float64 power -> N of the same shape, float32.
    stats (a dict, optional) receives 'margin', the smallest relative distance
    at a comparison the recursion branches on, 'lmin', the count of
    local-minimum updates, and 'kmod', the count of actmin updates."""
    unknown = set(params) - set(DEFAULTS)
    if unknown:
        raise TypeError(f"minstat takes no parameter {sorted(unknown)[0]!r}")
    P = np.asarray(P, dtype=np.float64)
    if P.ndim == 3:
        parts = [dict() for _ in P]
        out = [minstat(p, eps, st, **params) for p, st in zip(P, parts)]
        if stats is not None:
            stats["margin"] = float(min(st["margin"] for st in parts))
            stats["lmin"] = int(sum(st["lmin"] for st in parts))
            stats["kmod"] = int(sum(st["kmod"] for st in parts))
        return np.stack(out)
    prm = dict(DEFAULTS, **params)
    f = np.float64
    alpha_c, alpha_c_floor, alpha_max, alpha_min = (f(prm[k]) for k in (
        "alpha_c", "alpha_c_floor", "alpha_max", "alpha_min"))
    snr_exp, beta_max, av = f(prm["snr_exp"]), f(prm["beta_max"]), f(prm["av"])
    slope_q = [f(v) for v in prm["slope_q"]]
    slope_max = [f(v) for v in prm["slope_max"]]
    U, V = int(prm["sub_windows"]), int(prm["sub_frames"])
    T, B = P.shape
    M_D, M_V = f(m_of(U * V)), f(m_of(V))
    nd, md2 = f(2.0 * (U * V - 1)) * (1.0 - M_D), 2.0 * M_D
    nv, mv2 = f(2.0 * (V - 1)) * (1.0 - M_V), 2.0 * M_V
    q_lo, q_hi, c_c = 1.0 / f(prm["q_eq_max"]), 1.0 / f(prm["q_eq_min"]), 1.0 - alpha_c
    p = P[0].copy()
    sn2, pb, pminu = p.copy(), p.copy(), p.copy()
    pb2 = p * p
    ac = f(1.0)
    actmin = np.full(B, np.inf)
    actminsub = np.full(B, np.inf)
    buf = np.full((U, B), np.inf)
    lmf = np.zeros(B, dtype=bool)
    subwc, ib = V, -1
    N = np.empty((T, B), dtype=np.float64)
    margin, lmin, kmod = np.inf, 0, 0
    with np.errstate(all="ignore"):
        for t in range(T):
            y = P[t]
            sp, sy, ss = np.sum(p), np.sum(y), np.sum(sn2)
            r = sp / max(sy, DBL_MIN) - 1.0
            acb = 1.0 / (1.0 + r * r)
            ac = alpha_c * ac + c_c * max(acb, alpha_c_floor)
            snr = sp / max(ss, DBL_MIN)
            fl = min(alpha_min, np.power(snr, snr_exp))
            aa = alpha_max * ac
            ql = q_lo / f(t + 1)
            g = p / np.maximum(sn2, DBL_MIN) - 1.0
            ah = np.maximum(aa / (1.0 + g * g), fl)
            p = ah * p + (1.0 - ah) * y
            bt = np.minimum(ah * ah, beta_max)
            pb = bt * pb + (1.0 - bt) * p
            pb2 = bt * pb2 + (1.0 - bt) * (p * p)
            s2 = np.maximum(sn2, DBL_MIN)
            qe = np.maximum(np.minimum((pb2 - pb * pb) / np.maximum(2.0 * (s2 * s2), DBL_MIN),
                                       q_hi), ql)
            qav = np.sum(qe) / f(B)
            bc = 1.0 + av * np.sqrt(qav)
            iq = 1.0 / qe
            bd = 1.0 + nd / (iq - md2)
            bv = 1.0 + nv / (iq - mv2)
            bcp = bc * p
            c = bcp * bd
            margin = min(margin, _rel(c, actmin))
            k = c < actmin
            kmod += int(k.sum())
            actmin = np.where(k, c, actmin)
            actminsub = np.where(k, bcp * bv, actminsub)
            if 1 < subwc < V:
                lmf |= k
                pminu = np.minimum(actminsub, pminu)
                sn2 = pminu.copy()
            elif subwc >= V:
                ib = (ib + 1) % U
                buf[ib] = actmin
                pminu = buf.min(axis=0)
                nsm = slope_max[3]
                for i in range(3):
                    if qav < slope_q[i]:
                        nsm = slope_max[i]
                        break
                margin = min(margin, min(abs(float(qav) - float(q)) / float(q) for q in slope_q))
                cand = lmf & ~k
                if cand.any():
                    hi = nsm * pminu
                    margin = min(margin, _rel(actminsub[cand], pminu[cand]),
                                 _rel(actminsub[cand], hi[cand]))
                    upd = cand & (pminu < actminsub) & (actminsub < hi)
                    lmin += int(upd.sum())
                    pminu = np.where(upd, actminsub, pminu)
                    buf[:, upd] = pminu[upd]
                lmf[:] = False
                actmin = np.full(B, np.inf)
                subwc = 0
            subwc += 1
            N[t] = sn2
    if stats is not None:
        stats["margin"] = float(margin)
        stats["lmin"] = lmin
        stats["kmod"] = kmod
    return np.maximum(N, eps).astype(np.float32)
