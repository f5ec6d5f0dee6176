"""Designs, long-double reference, conditioning and bounds of the per-stage STOI
tests, shared by tests/test_stoi_cases_host.py (the conditions the device test
relies on; runs without a device) and tests/test_gpu_stoi_stages.py (every
stage of csrc/cse_stoi.hip against the reference).  Host-only: numpy and
mpmath; no device, no torch, and nothing of oracle/stoi_ref.py's scipy / FFT
route (the host test compares the two).

The reference restates every stage from the published definitions (Taal et al.
2011 as pystoi 0.4.1 implements it; Jensen & Taal 2016 for the extended form)
in np.longdouble (x87, eps 1.08e-19):

  window_oct      Octave's Kaiser-sinc resampling window, mpmath for I0 and sinc
  coef16          its 16 kHz -> 10 kHz polyphase form c_r[k], [5][128]
  resample16      e10[5q + r] = sum_k c_r[k] e[8q + k], k in [-58, 64]
  resample_any    out[i] = sum_n h[half + i down - n up] e[n]  (resample_poly's
                  (i + pre_rm) down - pre_pad is half + i down)
  clean_side      frame energies in dB, mask, kept frames, K / M / J, the
                  greedy block tables, overlap-add, 512-point DFT as a matrix
                  product, band envelopes, segment statistics
  stoi_b / estoi_b   both phase-B forms from envelopes, with their conditioning

The test signal of a cell is test_signal(): the f32 values shifted by lag, zero
outside [0, len), clipped (results.shift_and_fit).

Bounds.  u = 2^-53, gamma(n) = n u / (1 - n u).  Each constant is derived next
to its definition from the operation counts of the kernel, none from what a
device returned.  Departures from a plain `E x scale` form, with their reason:
  * the envelope bound is E_FFT U_f plus the resampler's bound carried through
    the two window products and Parseval, evaluated per frame: its ratio to
    U_f depends on the frame's crest and on loud neighbours of a quiet frame,
    so no constant covers it;
  * the column mean of xcol is a mean of 15 values of both signs: its bound is
    gamma_30 times the mean of their magnitudes, not of the mean itself;
  * xstat and xcol are compared with the reference evaluated on the device's
    own xtob (the stage in isolation), as phase B is.
"""

import functools
import math
from collections import namedtuple

import mpmath
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
EPS = np.finfo(np.float64).eps
SEED = 20261
FS10 = 10000
FR, HOP, NBAND, NSEG = 256, 128, 15, 30
MAXD, FB, BT, META = 18, 16, 72, 8
T_P, T_SA, T_SB = 3, 3 + MAXD, 3 + MAXD + FB + 1
KLO, KN, CST = -58, 123, 128
KAPPA_CAP = 64.0
LOUD, QUIET = 0.3, 0.3e-4
TINY = np.finfo(LD).tiny
mpmath.mp.dps = 40


def gamma(n):
    return n * U / (1.0 - n * U)


def _ld(v):
    """mpf -> long double (two-double split: 106 bits, more than 64)."""
    hi = float(v)
    return LD(hi) + LD(float(v - hi))


# ----------------------------------------------------------------------------
# the resampling window
# ----------------------------------------------------------------------------
def ratio(sr):
    g = math.gcd(FS10, sr)
    return FS10 // g, sr // g


def half_len(up, down):
    if up == down:
        return 0
    stop = 1.0 / (2.0 * max(up, down))
    return int(math.ceil((60.0 - 8.0) / (28.714 * (stop / 10.0))))


Window = namedtuple("Window", "h half up down rho e_c n_sum")

# relative error of one unnormalised tap as the kernels compute it
# (stoi_coef_kernel, stoi_coef_generic_kernel), against the largest tap:
#   I0 by its series, at most 40 terms at x <= 5.66: term_j carries the 3 j
#   roundings of its recurrence and q's 2, the sum of positive terms one per
#   addition: (3 * 40 + 2 + 40) u = 162 u, twice (numerator and I0(beta));
#   the argument beta sqrt(1 - v^2): 1 - v^2 has an absolute error of 3 u, which
#   the sqrt halves, and I0's logarithmic derivative is below x^2 / 2 with
#   x^2 = beta^2 (1 - v^2): 0.75 beta^2 u = 24 u, plus beta and the product,
#   2 u x <= 12 u;  the quotient 1 u;
#   sinc: sinpi 4 ulp (OpenCL's bound for sinpi), pi, product, quotient 3 u,
#   and where x = 2 stop t is rounded (2 u, other rates) an absolute 2 u of
#   sinc <= 1, which `against the largest tap` covers;  the two scalings 2 u
E_TAP = (2 * 162 + 24 + 12 + 1 + 4 + 3 + 2 + 2) * U


@functools.lru_cache(maxsize=None)
def window_oct(up, down):
    """h[2 half + 1]: pystoi's _resample_window_oct(up, down), normalised to
    unit sum, times up (what resample_poly applies)."""
    half = half_len(up, down)
    if half == 0:
        return Window(np.ones(1, dtype=LD), 0, 1, 1, 1.0, 0.0, 0)
    mpmath.mp.dps = 40
    big = max(up, down)
    beta = mpmath.mpf(0.1102 * (60.0 - 8.7))  # the definition's double
    i0b = mpmath.besseli(0, beta)
    taps = [None] * (2 * half + 1)
    for t in range(half + 1):
        kais = mpmath.besseli(0, beta * mpmath.sqrt(1 - mpmath.mpf(t * t) / (half * half))) / i0b
        x = mpmath.mpf(t) / big  # 2 stop t
        if t % big == 0:  # sin(pi x) of an integer x: exactly 0, not mpmath's 1e-40
            sinc = mpmath.mpf(1 if t == 0 else 0)
        else:
            sinc = mpmath.sin(mpmath.pi * x) / (mpmath.pi * x)
        taps[half + t] = taps[half - t] = kais * mpmath.mpf(up) / big * sinc
    total = mpmath.fsum(taps)
    rho = float(mpmath.fsum(abs(v) for v in taps) / abs(total))
    h = np.array([_ld(up * v / total) for v in taps], dtype=LD)
    # the normaliser: ceil(n / 1024) additions per thread, then a tree of
    # depth 10, on taps of relative error E_TAP: (E_TAP + n_sum u) rho of the
    # sum; the tap itself E_TAP, the quotient and the product by up 2 u
    n_sum = -(-(2 * half + 1) // 1024) + 10
    e_c = E_TAP * (1.0 + rho) + (n_sum * rho + 2) * U
    return Window(h, half, up, down, rho, e_c, n_sum)


@functools.lru_cache(maxsize=None)
def coef16():
    """c[r][kk] = h[290 + 8 r - 5 (kk - 58)] where that tap exists and kk < 123,
    else exactly 0: stoi_coef_kernel's table [5][128]."""
    w = window_oct(5, 8)
    c = np.zeros((5, CST), dtype=LD)
    for r in range(5):
        for kk in range(KN):
            d = 8 * r - 5 * (kk + KLO)
            if -w.half <= d <= w.half:
                c[r, kk] = w.h[w.half + d]
    return c


def test_signal(y, lag, clip):
    """results.shift_and_fit on the f32 values, without its clip unless clip."""
    y = np.asarray(y, dtype=np.float32).astype(np.float64)
    n = len(y)
    out = np.zeros(n)
    if lag >= 0:
        if lag < n:
            out[lag:] = y[:n - lag]
    elif -lag < n:
        out[:n + lag] = y[-lag:]
    return np.clip(out, -1.0, 1.0) if clip else out


def resample16(e):
    """(e10, bound): the 16 kHz polyphase sum and its per-element bound
    gamma_123 sum |c_k| |e_k| + E_c max |c| sum |e_k| (123 fused multiply-adds
    per output in both kernels; the taps outside a phase's span are exact
    zeros, counted all the same)."""
    w = window_oct(5, 8)
    c = coef16()
    e = np.asarray(e, dtype=LD)
    n = len(e)
    n10 = -(-5 * n // 8)
    Q = -(-n10 // 5)
    pad = np.zeros(8 * Q + KN + 58, dtype=LD)
    pad[58:58 + n] = e
    win = np.lib.stride_tricks.sliding_window_view(pad, KN)[::8][:Q]
    awin = np.abs(win)
    out = np.stack([win @ c[r, :KN] for r in range(5)], axis=1).reshape(-1)[:n10]
    cmax = float(np.abs(c).max())
    s1 = awin.sum(axis=1)
    b = np.stack([gamma(KN) * (awin @ np.abs(c[r, :KN])) + w.e_c * cmax * s1 for r in range(5)],
                 axis=1).reshape(-1)[:n10]
    return out, b.astype(np.float64)


def resample_any(e, sr):
    """(out, bound) at any rate: the generic sum, one fused multiply-add per
    tap that meets a sample (stoi_resample_kernel)."""
    up, down = ratio(sr)
    e = np.asarray(e, dtype=LD)
    if up == down:
        return e.copy(), np.zeros(len(e))
    w = window_oct(up, down)
    n = len(e)
    n_out = -(-n * up // down)
    ae = np.abs(e)
    ah = np.abs(w.h)
    hmax = float(ah.max())
    out = np.zeros(n_out, dtype=LD)
    b = np.zeros(n_out)
    for i in range(n_out):
        base = w.half + i * down
        nlo = max(-((w.half - i * down) // up), 0)   # ceil((i down - half) / up)
        nhi = min(base // up, n - 1)
        if nhi < nlo:
            continue
        idx = base - up * np.arange(nlo, nhi + 1)
        seg, aseg = e[nlo:nhi + 1], ae[nlo:nhi + 1]
        out[i] = w.h[idx] @ seg
        b[i] = gamma(nhi - nlo + 1) * float(ah[idx] @ aseg) + w.e_c * hmax * float(aseg.sum())
    return out, b


def to10(e, sr):
    return resample16(e) if sr == 16000 else resample_any(e, sr)


# ----------------------------------------------------------------------------
# frames, mask, blocks
# ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hann():
    """MATLAB hanning(256): 0.5 - 0.5 cos(2 pi (n + 1) / 257)."""
    n = np.arange(1, FR + 1, dtype=LD)
    return LD(0.5) - LD(0.5) * np.cos(2 * _ld(+mpmath.pi) * n / LD(FR + 1))


# absolute error of a window value on the device: cospi 4 ulp (OpenCL's bound)
# of a value <= 1, halved, the argument's two roundings (2 u x 2 pi x 0.5 sin
# <= 2 pi u ... taken whole: 7 u) and the subtraction 1 u
E_WND = 10 * U


def frame_energies(x10, d10):
    """(en [F] in dB, bound [F], lin [F]).  s = sum (w x)^2 over 256 samples: 4
    fused multiply-adds per lane and 6 shuffle additions (gamma_10 <= 12 u with
    the squares' rounding); v = w x moves by |x| (E_WND + u) + w dx, so
    ds / s <= 2 ||dv|| / ||v|| + 12 u;  20 log10(sqrt(s) + eps) then moves by
    (10 / ln 10) ds / s, plus sqrt, the sum with eps, log10 (4 ulp) and the
    product: 7 u |en|."""
    w = hann()
    F = (len(x10) - FR) // HOP + 1 if len(x10) >= FR else 0
    en = np.zeros(F, dtype=LD)
    bound = np.zeros(F)
    ax = np.abs(x10).astype(np.float64)
    wf = w.astype(np.float64)
    for f in range(F):
        sl = slice(HOP * f, HOP * f + FR)
        v = w * x10[sl]
        nv = np.sqrt(v @ v)
        en[f] = 20 * np.log10(nv + LD(EPS))
        if nv > 0:
            dv = ax[sl] * (E_WND + U) + wf * d10[sl]
            rel = 2.0 * float(np.sqrt(dv @ dv)) / float(nv) + 12 * U
        else:
            rel = 0.0  # every sample is zero on both sides: s = 0 exactly
        bound[f] = 10.0 / math.log(10.0) * rel + 7 * U * abs(float(en[f]))
    return en, bound


def kept_frames(en):
    return np.nonzero((en.max() - 40 - en) < 0)[0] if len(en) else np.zeros(0, dtype=np.int64)


def mask_margin(en):
    """min over the frames of |max(e) - 40 - e_f| in dB."""
    return float(np.abs(en.max() - 40 - en).min())


def blocks(kf, M):
    """stoi_select_kernel's greedy block tables, restated: a block takes frames
    while it holds at most FB and its overlap-add rows need at most MAXD
    distinct 10-kHz half-blocks.  Row hl of a block is kept frame h = j0 + hl:
    w[n] e10[kf[h]] (sa) + w[128 + n] e10[kf[h - 1] + 1] (sb, -1 for h = 0)."""
    out = []
    j0 = 0
    while j0 < M:
        p, sa, sb = [], [], []

        def add(v):
            if not p or p[-1] != v:
                p.append(int(v))
            return len(p) - 1

        def row(hl):
            h = j0 + hl
            sb.append(add(kf[h - 1] + 1) if h >= 1 else -1)
            sa.append(add(kf[h]))

        row(0)
        nf = 0
        while nf < FB and j0 + nf < M:
            h = j0 + nf + 1
            pb, pa = kf[h - 1] + 1, kf[h]
            if len(p) + (pb != p[-1]) + (pa != pb) > MAXD:
                break
            row(nf + 1)
            nf += 1
        out.append(dict(D=len(p), j0=j0, nf=nf, p=p, sa=sa, sb=sb))
        j0 += nf
    return out


def block_row(b):
    """A block as the BT ints of its table; -9 where the kernel writes nothing."""
    t = np.full(BT, -9, dtype=np.int64)
    t[0], t[1], t[2] = b["D"], b["j0"], b["nf"]
    t[T_P:T_P + b["D"]] = b["p"]
    t[T_SA:T_SA + b["nf"] + 1] = b["sa"]
    t[T_SB:T_SB + b["nf"] + 1] = b["sb"]
    return t


# ----------------------------------------------------------------------------
# envelopes
# ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def band_edges():
    """pystoi's thirdoct(10000, 512, 15, 150): [lo, hi) bins of the 15 bands."""
    f = np.linspace(0, FS10, 513)[:257]
    k = np.arange(NBAND, dtype=float)
    lo = [int(np.argmin(np.square(f - v))) for v in 150 * 2.0 ** ((2 * k - 1) / 6)]
    hi = [int(np.argmin(np.square(f - v))) for v in 150 * 2.0 ** ((2 * k + 1) / 6)]
    return list(zip(lo, hi))


@functools.lru_cache(maxsize=None)
def _dft():
    tab = 2 * _ld(+mpmath.pi) * np.arange(512, dtype=LD) / 512
    kn = (np.arange(257)[:, None] * np.arange(FR)[None, :]) % 512
    return np.cos(tab)[kn], -np.sin(tab)[kn]


# the transform's share of the envelope bound, in units of U_f = sqrt(sum over
# k <= 256 of |X[f, k]|^2).  Norm-wise, on the half spectrum whose norm is at
# most sqrt(2) U_f: the 256-point complex transform is two register DFT16s of
# four addition levels each (8 u), two inner twiddle products and the table
# product between them, each with a 4-ulp sincospi twiddle (3 x 8 u), the
# split to 512 points two additions and a table product (10 u): 42 u sqrt(2).
# |env_dev - env_ref| <= ||X_dev - X_ref|| on the band's bins (| ||a|| - ||b||
# | <= ||a - b||).  Then per element |X|^2 (3 u), the band sum of at most 45
# positive terms in 4 partial sums (14 u), sqrt and the exact halving: 11 u.
E_FFT = (42 * math.sqrt(2.0) + 11) * U


def envelopes(t10, d10, kf):
    """(env [M, 15], U_f [M], bound [M]) of a 10-kHz signal under the kept
    frames kf: overlap-add of the windowed kept frames, frames of that at hop
    128, windowed, 512-point DFT, band sums.  bound[f] = E_FFT U_f + sqrt(512)
    ||ds_f||: ds, the bound of a frame's sample, is the resampler's bound d10
    through both window products plus 11 u of the sample magnitudes (two
    E_WND, three roundings), and a sample error reaches the half spectrum with
    at most sqrt(512) of its norm (Parseval)."""
    w = hann()
    wf = w.astype(np.float64)
    K = len(kf)
    M = max(K - 1, 0)
    if M == 0:
        return np.zeros((0, NBAND), dtype=LD), np.zeros(0), np.zeros(0)
    n = HOP * (K - 1) + FR
    xs = np.zeros(n, dtype=LD)
    dx = np.zeros(n)
    ax = np.zeros(n)
    a10 = np.abs(t10).astype(np.float64)
    for k, f in enumerate(kf):
        sl, src = slice(HOP * k, HOP * k + FR), slice(HOP * f, HOP * f + FR)
        xs[sl] += w * t10[src]
        dx[sl] += wf * d10[src]
        ax[sl] += a10[src]
    idx = HOP * np.arange(M)[:, None] + np.arange(FR)[None, :]
    s = w[None, :] * xs[idx]
    ds = wf[None, :] * dx[idx] + 11 * U * ax[idx]
    C, S = _dft()
    re, im = C @ s.T, S @ s.T
    P = re * re + im * im  # [257, M]
    Uf = np.sqrt(P.sum(axis=0)).astype(np.float64)
    env = np.stack([np.sqrt(P[lo:hi].sum(axis=0)) for lo, hi in band_edges()], axis=1)
    bound = E_FFT * Uf + math.sqrt(512.0) * np.sqrt((ds * ds).sum(axis=1))
    return env, Uf, bound


# ----------------------------------------------------------------------------
# segment statistics and both phase-B forms, from envelopes
# ----------------------------------------------------------------------------
def segments(env):
    """[J, 30, 15] of env [M, 15]."""
    J = env.shape[0] - NSEG + 1
    return np.stack([env[j:j + NSEG] for j in range(J)])


def _kappa(num, den):
    out = np.zeros(num.shape)
    nz = num > 0
    out[nz] = (num[nz] / np.maximum(den[nz], TINY)).astype(np.float64)
    return out


def segment_stats(env):
    """(norm, mean, inv, kappa), each [J, 15]: the clean side's xstat, inv =
    1 / (||v - mean|| + eps), kappa = ||v|| / ||v - mean||.  On the device
    (stoi_clean_stat_kernel): the norm is 30 fused multiply-adds and a sqrt,
    the mean 29 additions of non-negative values and a quotient: gamma_30 of
    the value each.  The inverse sees the mean's error sqrt(30) gamma_30 mean
    <= gamma_30 ||v|| in the norm of v - mean: gamma_30 (1 + kappa), its own
    30 fused multiply-adds, sqrt, eps and quotient inside gamma_30 / 2 + 4 u."""
    seg = segments(np.asarray(env, dtype=LD))
    norm = np.sqrt((seg * seg).sum(axis=1))
    mean = seg.mean(axis=1)
    c = seg - mean[:, None, :]
    cn = np.sqrt((c * c).sum(axis=1))
    return norm, mean, 1 / (cn + LD(EPS)), _kappa(norm, cn)


def column_stats(env, mean, inv):
    """(mean [J, 30], inv [J, 30], kappa, mag) of the row-normalised segments'
    columns: xr[b] = (x[j + t][b] - mean[j][b]) inv[j][b] (stoi_clean_col_kernel;
    mean and inv are the device's xstat there, and here whatever is passed).
    The column mean is 14 additions and a quotient on values with two roundings
    each, of both signs: gamma_30 mag, mag the mean of |xr|, covers it (17 u);
    the inverse gamma_30 (1 + kappa) as for the rows, kappa = ||xr|| /
    ||xr - mean||."""
    seg = segments(np.asarray(env, dtype=LD))
    xr = (seg - mean[:, None, :]) * inv[:, None, :]
    cm = xr.mean(axis=2)
    c = xr - cm[:, :, None]
    cn = np.sqrt((c * c).sum(axis=2))
    return cm, 1 / (cn + LD(EPS)), _kappa(np.sqrt((xr * xr).sum(axis=2)), cn), \
        np.abs(xr).mean(axis=2).astype(np.float64)


CLIPF = 1 + LD(10) ** (LD(15) / LD(20))

# phase B of one (segment, band), every term in units of u, kappa_y = ||y'|| /
# ||y' - mean||, kappa_x the clean one (stoi_cells_body):
#   y' = min(alpha y, clipf x): alpha = ||x|| / (||y|| + eps) carries xstat's
#   norm (gamma_30), its own (gamma_30 / 2 + 3 u) and the product: 19 u of y'
#   (min is 1-Lipschitz);  its mean 30 u of mean |y'| more: d = y' - mean moves
#   by (19 + 49) u ||y'|| + u ||d|| in norm, (68 kappa_y + 1) u of ||d||, and a
#   normalised correlation moves by at most twice the relative move of d:
#   136 kappa_y + 2;
#   x - mean with xstat's mean (gamma_30 of it): (30 kappa_x + 1);  the 30
#   fused multiply-adds of the product 30, ||d|| 17, xstat's inverse 30 (1 +
#   kappa_x), product and quotient 3;
#   the mean over J x 15 values of magnitude <= 1: about J / 16 + 10 additions
#   per thread and wave, 30 u for J <= 320.
# Sum: 136 kappa_y + 60 kappa_x + 113 <= 256 (1 + kappa_max).
E_B = 256 * U


def stoi_b(xenv, yenv):
    """(d, kappa_max): Taal's intermediate measure averaged over segments and
    bands, from envelopes [M, 15], and the largest conditioning of a clean or
    a processed (segment, band).  A processed segment that is all zero gives
    exactly 0 and counts no kappa."""
    xs, ys = segments(np.asarray(xenv, dtype=LD)), segments(np.asarray(yenv, dtype=LD))
    nx = np.sqrt((xs * xs).sum(axis=1, keepdims=True))
    ny = np.sqrt((ys * ys).sum(axis=1, keepdims=True))
    yp = np.minimum(ys * (nx / (ny + LD(EPS))), xs * CLIPF)
    yc = yp - yp.mean(axis=1, keepdims=True)
    xc = xs - xs.mean(axis=1, keepdims=True)
    nyc = np.sqrt((yc * yc).sum(axis=1, keepdims=True))
    nxc = np.sqrt((xc * xc).sum(axis=1, keepdims=True))
    corr = (yc / (nyc + LD(EPS)) * xc / (nxc + LD(EPS))).sum(axis=1)
    ky = _kappa(np.sqrt((yp * yp).sum(axis=1)), nyc[:, 0])
    kx = _kappa(nx[:, 0], nxc[:, 0])
    return corr.sum() / (corr.shape[0] * NBAND), float(max(ky.max(), kx.max()))


# extended phase B of one (segment, frame), in units of u (estoi_tile), with
# kappa_r the largest row conditioning ||v|| / ||v - mean|| of the segment in
# either signal and lam = 1 / ||column - its mean|| of the row-normalised
# column (entries <= 1 in magnitude) in either signal:
#   a row-normalised entry: y - mean moves by u |.| + 30 u mean |y|, which the
#   inverse norm turns into at most 30 kappa_r / sqrt(30) = 5.5 kappa_r u; the
#   inverse itself 30 (1 + kappa_r) of an entry <= 1: a = 31 + 35.5 kappa_r;
#   a column of 15 such entries moves by sqrt(15) a in norm, its mean by as
#   much again and by its own 16 u ||col||: relative to ||col - mean||,
#   (2 sqrt(15) a + 16 sqrt(15)) lam + 1;  a correlation moves by at most twice
#   that for y, and for x by once through the entries and once through xcol:
#   4 (2 sqrt(15) a + 62) lam + 4;  xcol's own inverse 30 (1 + sqrt(15) lam),
#   the 15 fused multiply-adds, norm and quotients 25;  the mean as above 30.
# Sum: 8 sqrt(15) (31 + 35.5 kappa_r) lam + 365 lam + 89
#      <= 1100 (1 + kappa_r) lam + 365 lam + 89 <= 2048 (1 + kappa_r)(1 + lam).
E_BE = 2048 * U


def rcn(seg):
    """Row (30 frames), then column (15 bands) mean removal and normalisation
    of segments [J, 30, 15]; also kappa_r [J, 15] and lam [J, 30]."""
    c = seg - seg.mean(axis=1, keepdims=True)
    cn = np.sqrt((c * c).sum(axis=1, keepdims=True))
    kr = _kappa(np.sqrt((seg * seg).sum(axis=1)), cn[:, 0])
    r = c / (cn + LD(EPS))
    d = r - r.mean(axis=2, keepdims=True)
    dn = np.sqrt((d * d).sum(axis=2, keepdims=True))
    nz = np.sqrt((r * r).sum(axis=2)) > 0
    lam = np.zeros(dn[:, :, 0].shape)
    lam[nz] = (1 / np.maximum(dn[:, :, 0][nz], TINY)).astype(np.float64)
    kc = _kappa(np.sqrt((r * r).sum(axis=2)), dn[:, :, 0])
    return d / (dn + LD(EPS)), kr, lam, kc


def estoi_b(xenv, yenv):
    """(d, kappa_r max, lam max, kappa_col max) of the extended measure
    (include/cse_estoi.h: no jitter, norm + eps divisors)."""
    xs, ys = segments(np.asarray(xenv, dtype=LD)), segments(np.asarray(yenv, dtype=LD))
    xn, kx, lx, cx = rcn(xs)
    yn, ky, ly, cy = rcn(ys)
    d = (xn * yn).sum() / (NSEG * xs.shape[0])
    return d, float(max(kx.max(), ky.max())), float(max(lx.max(), ly.max())), \
        float(max(cx.max(), cy.max()))


# ----------------------------------------------------------------------------
# the clean side of one signal, and one cell against it
# ----------------------------------------------------------------------------
Clean = namedtuple("Clean", "x10 d10 en en_bound margin kf K M J F n10 blocks env Uf env_bound")


def clean_side(clean, sr=16000):
    x10, d10 = to10(np.asarray(clean, dtype=np.float64), sr)
    en, eb = frame_energies(x10, d10)
    F = len(en)
    if F == 0:
        z = np.zeros(0)
        return Clean(x10, d10, en, eb, np.inf, np.zeros(0, dtype=np.int64), 0, 0, 0, 0, len(x10),
                     [], np.zeros((0, NBAND), dtype=LD), z, z)
    kf = kept_frames(en)
    K = len(kf)
    M = max(K - 1, 0)
    env, Uf, bound = envelopes(x10, d10, kf)
    return Clean(x10, d10, en, eb, mask_margin(en), kf, K, M, max(M - NSEG + 1, 0), F, len(x10),
                 blocks(kf, M), env, Uf, bound)


Cell = namedtuple("Cell", "y10 d10 env Uf env_bound")


def cell_side(ref, y, lag, clip, sr=16000):
    """A cell's 10-kHz test signal and envelopes under the clean side's mask."""
    y10, d10 = to10(test_signal(y, lag, clip), sr)
    env, Uf, bound = envelopes(y10, d10, ref.kf)
    return Cell(y10, d10, env, Uf, bound)


# ----------------------------------------------------------------------------
# the designs: gated white noise from one seed
# ----------------------------------------------------------------------------
def _rng(*key):
    return np.random.default_rng((SEED,) + tuple(key))


def _gated(idx, gate):
    g = np.asarray(gate, dtype=np.float64)
    return _rng(idx, 0).standard_normal(len(g)) * np.where(g > 0, LOUD, QUIET)


def _all(n):
    return np.ones(n)


def _periodic(n, period, width, start=0):
    t = np.arange(n) - start
    return ((t >= 0) & (t % period < width)).astype(np.float64)


def _span(n, *spans):
    g = np.zeros(n)
    for a, b in spans:
        g[a:b] = 1
    return g


def tile_len(J):
    """The shortest all-loud 16-kHz length with J segments: F = K = J + 30."""
    n10 = FR + HOP * (J + 29)
    return -(-8 * n10 // 5)


GATES = {
    "steady": lambda: _all(9600),
    "j1": lambda: _all(6740),
    "j0": lambda: _all(6500),
    "none": lambda: _all(300),
    "bursts": lambda: _periodic(24000, 1120, 480),
    "sparse": lambda: _periodic(24000, 820, 60, 100),
    "gap": lambda: _span(16000, (0, 5000), (11000, 16000)),
    "lead": lambda: _span(16000, (4000, 14000)),
}
for _k in range(1, 8):
    GATES[f"tail{_k}"] = (lambda n: lambda: _all(n))(9600 + _k)
TILE_J = (31, 32, 33, 63, 64, 65, 96, 97)
for _j in TILE_J:
    GATES[f"tile{_j}"] = (lambda n: lambda: _all(n))(tile_len(_j))
NAMES = list(GATES) + ["oneband"]
# what the table of the issue states for each design: K, M, J
EXPECT = {"steady": (45, 44, 15), "j1": (31, 30, 1), "j0": (30, 29, 0), "bursts": (87, 86, 57),
          "sparse": (58, 57, 28)}


@functools.lru_cache(maxsize=None)
def gate(name):
    return _all(9600) if name == "oneband" else GATES[name]()


@functools.lru_cache(maxsize=None)
def clean_of(name):
    """The clean 16-kHz signal of a design (f64)."""
    idx = NAMES.index(name)
    if name == "oneband":
        # white noise limited to 1.0-1.25 kHz: every other band holds leakage only
        x = _rng(idx, 0).standard_normal(9600)
        X = np.fft.rfft(x)
        f = np.fft.rfftfreq(9600, 1 / 16000)
        X[(f < 1000) | (f > 1250)] = 0
        x = np.fft.irfft(X, 9600)
        return LOUD * x / x.std()
    return _gated(idx, gate(name))


SIGNALS = ("noisy", "clipped", "half", "zero", "inverse")


@functools.lru_cache(maxsize=None)
def tests_of(name):
    """The five test signals of a design: (tag, f32 signal, clip)."""
    idx = NAMES.index(name)
    x = clean_of(name)
    g = gate(name)
    n = len(x)
    r = [_rng(idx, k).standard_normal(n) for k in (1, 2, 3)]
    out = [("noisy", x + 0.1 * r[0], False),
           ("clipped", 6 * (x + 0.05 * r[1]), True),
           ("half", 0.5 * x, False),
           ("zero", np.zeros(n), False),
           ("inverse", r[2] * np.where(g > 0, QUIET, LOUD) if g.min() == 0 else LOUD * r[2], False)]
    return [(t, y.astype(np.float32), c) for t, y, c in out]


def lags_of(n):
    return [0, 1, -1, 7, -7, 203, -203, 205, -205, n - 1, -(n - 1), n, -n, n + 5]


def pair_clean():
    """Two signals in one plan: steady, zero-padded to bursts' length, and
    bursts (M < Mmax in both: the per-signal strides)."""
    a, b = clean_of("steady"), clean_of("bursts")
    return np.stack([np.concatenate([a, np.zeros(len(b) - len(a))]), b])


LAG_DESIGNS = ("steady", "gap", "bursts")
OFFSET_STEPS = (1, 3, 6)


def pack(signals, n):
    """The cells' f32 outputs in one flat array at offsets that are no multiples
    of 4 floats (1, 3, 6, ... past the running sum): (flat, offsets)."""
    offs, parts, o = [], [], 0
    for c, y in enumerate(signals):
        step = OFFSET_STEPS[c % 3]
        parts.append(np.zeros(step, dtype=np.float32))
        o += step
        offs.append(o)
        parts.append(np.asarray(y, dtype=np.float32))
        o += n
    parts.append(np.zeros(8, dtype=np.float32))
    return np.concatenate(parts), np.asarray(offs, dtype=np.int64)


# other rates: 0.5 s of the steady and the gap gate
RATES = (10000, 8000, 48000, 22050)
RATE_GATES = ("steady", "gap")


@functools.lru_cache(maxsize=None)
def rate_clean(sr, kind):
    n = sr // 2
    g = _all(n) if kind == "steady" else _span(n, (0, 5 * n // 16), (11 * n // 16, n))
    return _rng(100 + RATES.index(sr), RATE_GATES.index(kind), 0).standard_normal(n) * \
        np.where(g > 0, LOUD, QUIET)


@functools.lru_cache(maxsize=None)
def rate_cells(sr, kind):
    """(f32 signal, lag, clip) of the cells at another rate: lags 0, +-1,
    +-(down + 1), and the clip."""
    x = rate_clean(sr, kind)
    n = len(x)
    r = _rng(100 + RATES.index(sr), RATE_GATES.index(kind), 1).standard_normal(n)
    y = (x + 0.1 * r).astype(np.float32)
    down = ratio(sr)[1]
    return [(y, lag, False) for lag in (0, 1, -1, down + 1, -(down + 1))] + \
        [((6 * (x + 0.05 * r)).astype(np.float32), 0, True), ((0.5 * x).astype(np.float32), 0, False)]


def worst(err, bound):
    """(largest err / bound, its index): 0 / 0 counts as 0, x / 0 as inf, and
    a NaN in err or bound as inf, so that it can pass no comparison."""
    err = np.asarray(err, dtype=np.float64)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = np.where(err == 0, 0.0, err / bound)
    frac = np.where(np.isnan(frac), np.inf, frac)
    if frac.size == 0:
        return 0.0, ()
    i = np.unravel_index(int(np.argmax(frac)), frac.shape)
    return float(frac[i]), tuple(int(v) for v in i)
