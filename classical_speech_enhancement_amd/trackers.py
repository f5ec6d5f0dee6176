"""The noise-PSD trackers that go beyond the reference, one record each.

A tracker is a noise_method whose estimate is time-varying and whose kernel,
parameters and specification live in a header of its own
(include/cse_<name>.h).  Everything the Python layers need to know about one
is its record in TRACKERS; what differs between trackers, the validation of
the parameters, is written out per tracker, and the rest (the ctypes structure,
the unknown-name check, the cell parameters' prefix) is generic over the
record.  Host-only, like layout.py: numpy and _lib's ctypes structures,
neither torch nor a loaded library.
"""

import ctypes
import math
from typing import Callable, NamedTuple, Optional

import numpy as np

from . import _lib


class Tracker(NamedTuple):
    name: str             # the noise_method; cell params carry <name>_<parameter>
    code: int             # CSE_NOISE_<NAME> (_lib.NOISE)
    defaults: dict        # parameter -> default, in the structure's field order
    struct: type          # the ctypes mirror of cse_<name>_params_t
    values: Callable      # (params, prefix="") -> the validated values tuple
    default_entry: str    # cse_<name>_default_params
    entry: str            # cse_noise_<name>
    time_constants: Optional[Callable]  # (hop_length, sr) -> parameter dict, or None


def _whole(v, lo, hi):
    return (isinstance(v, (int, float, np.integer, np.floating)) and math.isfinite(v)
            and v == int(v) and lo <= int(v) <= hi)


def _floats(defaults):
    return tuple(k for k, d in defaults.items() if isinstance(d, float))


# MCRA (include/cse_mcra.h; Cohen & Berdugo 2002, the paper's values for n_fft
# 512 / hop 128 at 16 kHz)
MCRA_DEFAULTS = {"alpha_s": 0.8, "alpha_d": 0.95, "alpha_p": 0.2, "delta": 5.0,
                 "window_frames": 125}


def mcra_values(params, prefix=""):
    """(alpha_s, alpha_d, alpha_p, delta, window_frames) read from ``params``
    under prefix + name, defaults where absent; raises ValueError for what
    cse_noise_mcra refuses."""
    a_s, a_d, a_p, delta = (float(params.get(prefix + k, MCRA_DEFAULTS[k]))
                            for k in ("alpha_s", "alpha_d", "alpha_p", "delta"))
    w = params.get(prefix + "window_frames", MCRA_DEFAULTS["window_frames"])
    for name, a in (("alpha_s", a_s), ("alpha_d", a_d), ("alpha_p", a_p)):
        if not 0.0 <= a < 1.0:
            raise ValueError(f"mcra {name}={a} not in [0, 1)")
    if not delta > 0.0:
        raise ValueError(f"mcra delta={delta} not > 0")
    if w != int(w) or not 2 <= int(w) < 2**31:
        raise ValueError(f"mcra window_frames={w} not an integer >= 2")
    return (a_s, a_d, a_p, delta, int(w))


# SPP-MMSE (include/cse_spp.h; Gerkmann & Hendriks 2012, the paper's values)
SPP_DEFAULTS = {"prior_h1": 0.5, "xi_opt_db": 15.0, "alpha_pow": 0.8, "alpha_ph": 0.9,
                "ph_max": 0.99, "init_frames": 5}


def spp_values(params, prefix=""):
    """(prior_h1, xi_opt_db, alpha_pow, alpha_ph, ph_max, init_frames) read from
    ``params`` under prefix + name, defaults where absent; raises ValueError for
    what cse_noise_spp refuses, and for an init_frames that is no integer."""
    prior, xi, a_pow, a_ph, ph_max = (float(params.get(prefix + k, SPP_DEFAULTS[k]))
                                      for k in ("prior_h1", "xi_opt_db", "alpha_pow", "alpha_ph",
                                                "ph_max"))
    k = params.get(prefix + "init_frames", SPP_DEFAULTS["init_frames"])
    for name, v in (("prior_h1", prior), ("ph_max", ph_max)):
        if not 0.0 < v < 1.0:
            raise ValueError(f"spp {name}={v} not in (0, 1)")
    for name, a in (("alpha_pow", a_pow), ("alpha_ph", a_ph)):
        if not 0.0 <= a < 1.0:
            raise ValueError(f"spp {name}={a} not in [0, 1)")
    if not math.isfinite(xi):
        raise ValueError(f"spp xi_opt_db={xi} not finite")
    if not (isinstance(k, (int, float, np.integer, np.floating)) and math.isfinite(k)
            and k == int(k) and 1 <= int(k) < 2**31):
        raise ValueError(f"spp init_frames={k} not an integer >= 1")
    return (prior, xi, a_pow, a_ph, ph_max, int(k))


# minimum statistics (include/cse_minstat.h; Martin 2001, the paper's time
# constants at an 8-ms frame step: hop 128 at 16 kHz)
MINSTAT_DEFAULTS = {"alpha_c": 0.837, "alpha_c_floor": 0.7, "alpha_max": 0.98, "alpha_min": 0.548,
                    "snr_exp": -0.125, "beta_max": 0.894, "av": 2.12, "q_eq_min": 2.0,
                    "q_eq_max": 14.0, "slope_q": (0.03, 0.05, 0.06),
                    "slope_max": (8.0, 4.0, 2.0, 1.2), "sub_windows": 8, "sub_frames": 24}


def minstat_values(params, prefix=""):
    """(alpha_c, alpha_c_floor, alpha_max, alpha_min, snr_exp, beta_max, av,
    q_eq_min, q_eq_max, slope_q, slope_max, sub_windows, sub_frames) read from
    ``params`` under prefix + name, defaults where absent, slope_q and slope_max
    as tuples; raises ValueError for what cse_noise_minstat refuses, and for
    sub_windows / sub_frames that are no integers."""
    get = lambda k: params.get(prefix + k, MINSTAT_DEFAULTS[k])  # noqa: E731
    v = {k: float(get(k)) for k in _floats(MINSTAT_DEFAULTS)}
    for k, n in (("slope_q", 3), ("slope_max", 4)):
        try:
            v[k] = tuple(float(x) for x in get(k))
        except TypeError:
            v[k] = ()
        if len(v[k]) != n:
            raise ValueError(f"minstat {k}={get(k)!r} not {n} numbers")
    for k in ("alpha_c", "alpha_c_floor", "alpha_min", "beta_max"):
        if not 0.0 <= v[k] < 1.0:
            raise ValueError(f"minstat {k}={v[k]} not in [0, 1)")
    if not 0.0 < v["alpha_max"] < 1.0:
        raise ValueError(f"minstat alpha_max={v['alpha_max']} not in (0, 1)")
    if not (math.isfinite(v["snr_exp"]) and v["snr_exp"] <= 0.0):
        raise ValueError(f"minstat snr_exp={v['snr_exp']} not finite or > 0")
    if not (math.isfinite(v["av"]) and v["av"] >= 0.0):
        raise ValueError(f"minstat av={v['av']} not finite or < 0")
    if not 2.0 <= v["q_eq_min"] <= v["q_eq_max"] < math.inf:
        raise ValueError(f"minstat not 2 <= q_eq_min={v['q_eq_min']} <= "
                         f"q_eq_max={v['q_eq_max']} < inf")
    q = v["slope_q"]
    if not (0.0 < q[0] < q[1] < q[2] < math.inf):
        raise ValueError(f"minstat slope_q={q} not positive and strictly increasing")
    if not all(math.isfinite(x) and x >= 1.0 for x in v["slope_max"]):
        raise ValueError(f"minstat slope_max={v['slope_max']} not all finite and >= 1")
    U, V = get("sub_windows"), get("sub_frames")
    if not _whole(U, 1, 16):
        raise ValueError(f"minstat sub_windows={U} not an integer in [1, 16]")
    if not _whole(V, 2, 2**20):
        raise ValueError(f"minstat sub_frames={V} not an integer in [2, 2^20]")
    return tuple(v.values()) + (int(U), int(V))


def minstat_time_constants(hop_length, sr):
    """The parameter dict for a frame step of hop_length / sr seconds, from the
    time constants behind MINSTAT_DEFAULTS (which are this at 128 / 16000):
    alpha = exp(-step / tau), snr_exp = -step / 0.064, the sub-window's 0.192 s
    in frames (at least 2), U = 8.  The thresholds on the degrees of freedom and
    slope_max stay.  The plugins do not call it on their own."""
    step = float(hop_length) / float(sr)
    if not (step > 0.0 and math.isfinite(step)):
        raise ValueError(f"hop_length={hop_length} sr={sr}: no frame step")
    tau = {"alpha_c": 0.0449, "alpha_max": 0.392, "alpha_min": 0.0133, "beta_max": 0.0717}
    out = dict(MINSTAT_DEFAULTS)
    out.update((k, math.exp(-step / t)) for k, t in tau.items())
    out["snr_exp"] = -step / 0.064
    out["sub_windows"] = 8
    out["sub_frames"] = max(2, int(round(0.192 / step)))
    return out


# IMCRA (include/cse_imcra.h; Cohen 2003, the paper's values for n_fft 512 /
# hop 128 at 16 kHz)
IMCRA_DEFAULTS = {"alpha": 0.92, "alpha_s": 0.9, "alpha_d": 0.85, "beta": 1.47, "b_min": 1.66,
                  "gamma0": 4.6, "gamma1": 3.0, "zeta0": 1.67, "xi_min_db": -18.0,
                  "sub_windows": 8, "sub_frames": 15}


def imcra_values(params, prefix=""):
    """(alpha, alpha_s, alpha_d, beta, b_min, gamma0, gamma1, zeta0, xi_min_db,
    sub_windows, sub_frames) read from ``params`` under prefix + name, defaults
    where absent; raises ValueError for what cse_noise_imcra refuses, and for
    sub_windows / sub_frames that are no integers."""
    get = lambda k: params.get(prefix + k, IMCRA_DEFAULTS[k])  # noqa: E731
    v = {k: float(get(k)) for k in _floats(IMCRA_DEFAULTS)}
    for k in ("alpha", "alpha_s", "alpha_d"):
        if not 0.0 <= v[k] < 1.0:
            raise ValueError(f"imcra {k}={v[k]} not in [0, 1)")
    for k in ("beta", "b_min", "gamma0", "zeta0"):
        if not 0.0 < v[k] < math.inf:
            raise ValueError(f"imcra {k}={v[k]} not finite and > 0")
    if not 1.0 < v["gamma1"] < math.inf:
        raise ValueError(f"imcra gamma1={v['gamma1']} not finite and > 1")
    if not math.isfinite(v["xi_min_db"]):
        raise ValueError(f"imcra xi_min_db={v['xi_min_db']} not finite")
    U, V = get("sub_windows"), get("sub_frames")
    if not _whole(U, 1, 16):
        raise ValueError(f"imcra sub_windows={U} not an integer in [1, 16]")
    if not _whole(V, 1, 2**20):
        raise ValueError(f"imcra sub_frames={V} not an integer in [1, 2^20]")
    return tuple(v.values()) + (int(U), int(V))


def imcra_time_constants(hop_length, sr):
    """The parameter dict for a frame step of hop_length / sr seconds, from the
    time constants behind IMCRA_DEFAULTS (which are this at 128 / 16000, exactly):
    alpha, alpha_s and alpha_d become exp(-step / tau) with tau = -0.008 /
    log(default), that is default ** (step / 0.008); the sub-window's 0.12 s in
    frames (at least 1), U = 8.  beta, b_min and the thresholds stay.  The
    plugins do not call it on their own."""
    step = float(hop_length) / float(sr)
    if not (step > 0.0 and math.isfinite(step)):
        raise ValueError(f"hop_length={hop_length} sr={sr}: no frame step")
    out = dict(IMCRA_DEFAULTS)
    out.update((k, IMCRA_DEFAULTS[k] ** (step / 0.008)) for k in ("alpha", "alpha_s", "alpha_d"))
    out["sub_windows"] = 8
    out["sub_frames"] = max(1, int(math.floor(0.12 / step + 0.5)))
    return out


def _tracker(name, defaults, struct, values, time_constants=None):
    return Tracker(name, _lib.NOISE[name], defaults, struct, values,
                   *_lib.TRACKER_EXPORTS[name], time_constants)


# method -> record, in the order of their codes; a tracker's values tuple is
# the estimator slot of a noise key (layout.noise_key)
TRACKERS = {t.name: t for t in (
    _tracker("mcra", MCRA_DEFAULTS, _lib.McraParams, mcra_values),
    _tracker("spp", SPP_DEFAULTS, _lib.SppParams, spp_values),
    _tracker("minstat", MINSTAT_DEFAULTS, _lib.MinstatParams, minstat_values,
             minstat_time_constants),
    _tracker("imcra", IMCRA_DEFAULTS, _lib.ImcraParams, imcra_values, imcra_time_constants))}


def params(tracker, values):
    """The tracker's cse_<name>_params_t from its values tuple: the structure's
    fields but ``reserved``, in order, are the values."""
    prm = tracker.struct()
    fields = [f for f in tracker.struct._fields_ if f[0] != "reserved"]
    for (name, ctype), x in zip(fields, values):
        if issubclass(ctype, ctypes.Array):
            getattr(prm, name)[:] = x
        else:
            setattr(prm, name, x)
    return prm


def check_names(tracker, given):
    """TypeError for a name in ``given`` that is no parameter of the tracker
    (the alphabetically first such name)."""
    unknown = set(given) - set(tracker.defaults)
    if unknown:
        raise TypeError(f"{tracker.name} takes no parameter {sorted(unknown)[0]!r}")


def tracker_values(params):
    """The values tuple of a cell whose noise_method is a tracker (its
    parameters read as <method>_<name>), () for every other method."""
    method = params["noise_method"]
    return TRACKERS[method].values(params, method + "_") if method in TRACKERS else ()
