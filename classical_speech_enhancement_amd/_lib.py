"""ctypes binding of libcse.so (the C ABI declared in include/cse.h,
include/cse_estoi.h, include/cse_stoi_stages.h, include/cse_mcra.h, include/cse_segsnr.h,
include/cse_spp.h, include/cse_minstat.h, include/cse_imcra.h, include/cse_lpc.h,
include/cse_wss.h, include/cse_sisdr.h, include/cse_logerr.h, include/cse_csii.h,
include/cse_ncm.h, include/cse_online.h and include/cse_online_pool.h).

Entry points that share a signature are declared in one loop: the noise
trackers (TRACKER_EXPORTS) and the waveform scores on the segSNR interface
(CELL_SCORES / CELL_SCORE_EXPORTS).

The product path has no CPU fallback: if the shared library (built for gfx950
by ``__graft_entry__.build()``) is missing, every entry point raises.
"""

import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CSE_LIB", os.path.join(HERE, "libcse.so"))

CSE_OK = 0
# ABI revision this package mirrors (cse_version(); CELL_DTYPE == cse_cell_t,
# NOISE_JOB_DTYPE == cse_noise_job_t, NoiseParams == cse_noise_params_t)
ABI_VERSION = 5
ALGO = {"NONE": -1, "SS": 0, "WIENER": 1, "MMSE": 2, "OMLSA": 3}
NOISE = {"percentile": 0, "min_tracking": 1, "true_noise": 2, "mcra": 3, "spp": 4,
         "minstat": 5, "imcra": 6}

# numpy mirror of cse_cell_t (include/cse.h) — 96 bytes
CELL_DTYPE = np.dtype([
    ("algo", np.int32), ("hop", np.int32), ("y_offset", np.int64),
    ("noise_offset", np.int64), ("noise_stride", np.int64), ("clean_offset", np.int64),
    ("out_offset", np.int64), ("gain_offset", np.int64), ("lag", np.int32),
    ("reserved", np.int32), ("param", np.float32, (8,)),
], align=True)
assert CELL_DTYPE.itemsize == 96

# numpy mirror of cse_noise_job_t — 40 bytes
NOISE_JOB_DTYPE = np.dtype([
    ("src_offset", np.int64), ("dst_offset", np.int64), ("src_frames", np.int32),
    ("out_frames", np.int32), ("mu", np.float64), ("inv_eps", np.float64)], align=True)
assert NOISE_JOB_DTYPE.itemsize == 40


class NoiseParams(ctypes.Structure):
    """cse_noise_params_t: estimator constructor parameters
    (noise_estimation.py:12-13, :60) and the TrueNoise frame fit (:149-153)."""
    _fields_ = [("percentile", ctypes.c_double), ("max_fraction", ctypes.c_double),
                ("floor_rel", ctypes.c_double), ("smoothing_factor", ctypes.c_double),
                ("min_frames", ctypes.c_int32), ("adaptive_short", ctypes.c_int32),
                ("window_size", ctypes.c_int32), ("src_frames", ctypes.c_int32)]


assert ctypes.sizeof(NoiseParams) == 48


class McraParams(ctypes.Structure):
    """cse_mcra_params_t (include/cse_mcra.h): the MCRA tracker's parameters."""
    _fields_ = [("alpha_s", ctypes.c_double), ("alpha_d", ctypes.c_double),
                ("alpha_p", ctypes.c_double), ("delta", ctypes.c_double),
                ("window_frames", ctypes.c_int32), ("reserved", ctypes.c_int32)]


assert ctypes.sizeof(McraParams) == 40


class SppParams(ctypes.Structure):
    """cse_spp_params_t (include/cse_spp.h): the SPP-MMSE tracker's parameters."""
    _fields_ = [("prior_h1", ctypes.c_double), ("xi_opt_db", ctypes.c_double),
                ("alpha_pow", ctypes.c_double), ("alpha_ph", ctypes.c_double),
                ("ph_max", ctypes.c_double), ("init_frames", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


assert ctypes.sizeof(SppParams) == 48


class MinstatParams(ctypes.Structure):
    """cse_minstat_params_t (include/cse_minstat.h): the minimum-statistics
    tracker's parameters."""
    _fields_ = [("alpha_c", ctypes.c_double), ("alpha_c_floor", ctypes.c_double),
                ("alpha_max", ctypes.c_double), ("alpha_min", ctypes.c_double),
                ("snr_exp", ctypes.c_double), ("beta_max", ctypes.c_double),
                ("av", ctypes.c_double), ("q_eq_min", ctypes.c_double),
                ("q_eq_max", ctypes.c_double), ("slope_q", ctypes.c_double * 3),
                ("slope_max", ctypes.c_double * 4), ("sub_windows", ctypes.c_int32),
                ("sub_frames", ctypes.c_int32)]


assert ctypes.sizeof(MinstatParams) == 136


class ImcraParams(ctypes.Structure):
    """cse_imcra_params_t (include/cse_imcra.h): the IMCRA tracker's parameters."""
    _fields_ = [("alpha", ctypes.c_double), ("alpha_s", ctypes.c_double),
                ("alpha_d", ctypes.c_double), ("beta", ctypes.c_double),
                ("b_min", ctypes.c_double), ("gamma0", ctypes.c_double),
                ("gamma1", ctypes.c_double), ("zeta0", ctypes.c_double),
                ("xi_min_db", ctypes.c_double), ("sub_windows", ctypes.c_int32),
                ("sub_frames", ctypes.c_int32)]


assert ctypes.sizeof(ImcraParams) == 80


class LogErrParams(ctypes.Structure):
    """cse_logerr_params_t (include/cse_logerr.h): what the noise-PSD score reads."""
    _fields_ = [("floor", ctypes.c_double), ("t0", ctypes.c_int32), ("bin_lo", ctypes.c_int32),
                ("bin_hi", ctypes.c_int32), ("reserved", ctypes.c_int32)]


assert ctypes.sizeof(LogErrParams) == 24


class OnlineConfig(ctypes.Structure):
    """cse_online_config_t (include/cse_online.h): what the online enhancer runs."""
    _fields_ = [("n_fft", ctypes.c_int32), ("hop", ctypes.c_int32), ("algo", ctypes.c_int32),
                ("noise_method", ctypes.c_int32), ("param", ctypes.c_float * 8),
                ("eps", ctypes.c_double), ("mu", ctypes.c_double), ("mcra", McraParams),
                ("spp", SppParams)]


assert ctypes.sizeof(OnlineConfig) == 152


class OnlineHandle(ctypes.Structure):
    """cse_online_t (include/cse_online.h): the caller-owned host handle."""
    _fields_ = [("cfg", OnlineConfig), ("n_streams", ctypes.c_int64), ("state", ctypes.c_void_p),
                ("frames", ctypes.c_int64), ("primed", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


assert ctypes.sizeof(OnlineHandle) == 184


class PoolParams(ctypes.Structure):
    """cse_pool_params_t (include/cse_online_pool.h): one slot's parameter values."""
    _fields_ = [("param", ctypes.c_float * 8), ("mu", ctypes.c_double), ("mcra", McraParams),
                ("spp", SppParams)]


assert ctypes.sizeof(PoolParams) == 128


class PoolItem(ctypes.Structure):
    """cse_pool_item_t: one entry of a step's list."""
    _fields_ = [("slot", ctypes.c_int32), ("k", ctypes.c_int32)]


assert ctypes.sizeof(PoolItem) == 8


class PoolSlot(ctypes.Structure):
    """cse_pool_slot_t: the library's host bookkeeping of one slot."""
    _fields_ = [("frames", ctypes.c_int64), ("open", ctypes.c_int32),
                ("first_frames", ctypes.c_int32)]


assert ctypes.sizeof(PoolSlot) == 16


class PoolHandle(ctypes.Structure):
    """cse_pool_t: the caller-owned host handle of a pool."""
    _fields_ = [("cfg", OnlineConfig), ("capacity", ctypes.c_int64), ("state", ctypes.c_void_p),
                ("work", ctypes.c_void_p), ("slots", ctypes.POINTER(PoolSlot))]


assert ctypes.sizeof(PoolHandle) == 184

EXPORTS = ("cse_version", "cse_last_error", "cse_cells_per_group", "cse_stft",
           "cse_noise_workspace_bytes", "cse_noise_default_params", "cse_noise_estimate_ex",
           "cse_noise_estimate", "cse_noise_smooth", "cse_noise_median",
           "cse_noise_percentile_med", "cse_noise_percentile_med2", "cse_noise_percentile_quad", "cse_noise_min_tracking_med", "cse_noise_finish",
           "cse_noise_invert", "cse_istft_norm", "cse_enhance_cells", "cse_enhance_cells_short_hop",
           "cse_enhance_cells_generic",
           "cse_xcorr_workspace_bytes", "cse_xcorr_prepare", "cse_xcorr_lag",
           "cse_stoi_workspace_bytes", "cse_stoi_scratch_bytes", "cse_stoi_prepare",
           "cse_stoi_cells", "cse_stoi_workspace_bytes_sr", "cse_stoi_scratch_bytes_sr",
           "cse_stoi_cells_sr")
# include/cse_stoi_stages.h, a header of its own (cse.h's code is part of the
# enhance kernels' pinned source digest): where STOI's stages lie in a workspace
EXPORTS_STOI_STAGES = ("cse_stoi_layout",)
# cse_stoi_layout's out, in order: byte offsets, sizes, constants
STOI_LAYOUT_FIELDS = ("coef64", "meta", "x10", "en", "kf", "btab", "xtob", "xstat", "hgen", "xcol",
                      "total", "n10", "F", "Mmax", "Jmax", "NBLK", "BT", "META", "MAXD", "FB", "ntap")
# include/cse_estoi.h (extended STOI), a header of its own: EXPORTS is what cse.h declares
EXPORTS_ESTOI = ("cse_estoi_workspace_bytes", "cse_estoi_prepare", "cse_estoi_cells")
# the waveform scores that share one interface, each with a header of its own,
# include/cse_<name>.h: segsnr (segmental and frequency-weighted segmental SNR),
# lpc (log-likelihood ratio and LPC cepstrum distance) and wss (weighted spectral
# slope distance); name -> output pointers of cse_<name>_cells
CELL_SCORES = {"segsnr": 2, "lpc": 2, "wss": 1}
CELL_SCORE_EXPORTS = {s: tuple(f"cse_{s}_{e}" for e in ("workspace_bytes", "prepare",
                                                       "scratch_bytes", "cells"))
                      for s in CELL_SCORES}
EXPORTS_SEGSNR, EXPORTS_LPC, EXPORTS_WSS = CELL_SCORE_EXPORTS.values()
# the noise trackers (NOISE's methods after the reference's three), each with a
# header of its own, include/cse_<name>.h: name -> (default-parameters entry,
# estimate entry); the four names are what the per-tracker tests read
TRACKER_EXPORTS = {t: (f"cse_{t}_default_params", f"cse_noise_{t}")
                   for t, code in NOISE.items() if code > 2}
EXPORTS_MCRA, EXPORTS_SPP, EXPORTS_MINSTAT, EXPORTS_IMCRA = TRACKER_EXPORTS.values()
# include/cse_sisdr.h (SI-SDR, SI-SIR and SI-SAR), likewise
EXPORTS_SISDR = ("cse_sisdr_workspace_bytes", "cse_sisdr_prepare", "cse_sisdr_scratch_bytes",
                 "cse_sisdr_cells")
# include/cse_logerr.h (noise-PSD logarithmic estimation error), likewise
EXPORTS_LOGERR = ("cse_logerr_default_params", "cse_logerr_reference", "cse_logerr_scratch_bytes",
                  "cse_logerr_rows")
# include/cse_csii.h (three-level CSII and I3): the segSNR interface with one
# output pointer, [n_cells][4]; no record of CELL_SCORES, whose names are the
# optional score families'
EXPORTS_CSII = ("cse_csii_workspace_bytes", "cse_csii_prepare", "cse_csii_scratch_bytes",
                "cse_csii_cells")
# include/cse_ncm.h (normalized covariance measure and its band-importance form):
# the same interface with the exponent before the one output pointer,
# [n_cells][2]; like CSII no record of CELL_SCORES
EXPORTS_NCM = ("cse_ncm_workspace_bytes", "cse_ncm_prepare", "cse_ncm_scratch_bytes",
               "cse_ncm_cells")
# include/cse_online.h (the stateful online enhancer): a host handle and one
# device state block per batch of streams
EXPORTS_ONLINE = ("cse_online_state_bytes", "cse_online_init", "cse_online_prime",
                  "cse_online_push", "cse_online_finish")
# include/cse_online_pool.h (a pool of online streams with slots that open, step
# and close one by one): a host handle, a host slot table, a device state block
# and a device work list per pool
EXPORTS_POOL = ("cse_pool_state_bytes", "cse_pool_work_bytes", "cse_pool_init", "cse_pool_open",
                "cse_pool_step", "cse_pool_close", "cse_pool_drop")
XCORR_OK, XCORR_FLAT, XCORR_NONFINITE = 0, 1, 2  # FLAT: slow exact path ran (lag exact)


def cells_per_group(n_fft):
    """Cells per workgroup slot group (CSE_CELLS_PER_GROUP of the loaded build)."""
    n = int(load().cse_cells_per_group(int(n_fft)))
    if n <= 0:
        raise CseError(f"n_fft={n_fft} not supported")
    return n


class CseError(RuntimeError):
    pass


_lib = None


def load(path=LIB_PATH):
    """Load libcse.so and declare prototypes (raises if it is missing)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise CseError(f"{path} not built: run __graft_entry__.build() (hipcc --offload-arch=gfx950)")
    lib = ctypes.CDLL(path)
    P = ctypes.c_void_p
    i32, i64, f64 = ctypes.c_int, ctypes.c_int64, ctypes.c_double
    lib.cse_version.restype = i32
    lib.cse_version.argtypes = []
    lib.cse_last_error.restype = ctypes.c_char_p
    lib.cse_last_error.argtypes = []
    lib.cse_cells_per_group.restype = i32
    lib.cse_cells_per_group.argtypes = [i32]
    lib.cse_stft.restype = i32
    lib.cse_stft.argtypes = [P, P, i64, i64, i32, i32, P, P, P]
    lib.cse_noise_workspace_bytes.restype = i64
    lib.cse_noise_workspace_bytes.argtypes = [i64, i32, i32]
    lib.cse_noise_default_params.restype = None
    lib.cse_noise_default_params.argtypes = [P]
    lib.cse_noise_estimate_ex.restype = i32
    lib.cse_noise_estimate_ex.argtypes = [i32, P, i64, i32, i32, P, f64, P, P, P]
    lib.cse_noise_estimate.restype = i32
    lib.cse_noise_estimate.argtypes = [i32, P, i64, i32, i32, f64, f64, P, P, P]
    lib.cse_noise_smooth.restype = i32
    lib.cse_noise_smooth.argtypes = [P, i64, i32, i32, i32, f64, P, P]
    lib.cse_noise_median.restype = i32
    lib.cse_noise_median.argtypes = [P, i64, i32, i32, P, P]
    lib.cse_noise_percentile_med.restype = i32
    lib.cse_noise_percentile_med.argtypes = [P, P, i64, i32, i32, f64, f64, P, P, P]
    lib.cse_noise_percentile_med2.restype = i32
    lib.cse_noise_percentile_med2.argtypes = [P, P, i64, i32, i32, f64, f64, f64, P, P, P, P]
    lib.cse_noise_percentile_quad.restype = i32
    lib.cse_noise_percentile_quad.argtypes = [P, P, i64, i32, i32, f64, f64, f64, f64, P, P, P, P, P,
                                              P]
    lib.cse_noise_min_tracking_med.restype = i32
    lib.cse_noise_min_tracking_med.argtypes = [P, P, i64, i32, i32, f64, P, f64, P, P, P]
    lib.cse_noise_finish.restype = i32
    lib.cse_noise_finish.argtypes = [P, i32, i64, i32, P, P, P]
    lib.cse_noise_invert.restype = i32
    lib.cse_noise_invert.argtypes = [P, i64, f64, P, P]
    lib.cse_istft_norm.restype = i32
    lib.cse_istft_norm.argtypes = [i32, i32, i64, P, P]
    lib.cse_xcorr_workspace_bytes.restype = i64
    lib.cse_xcorr_workspace_bytes.argtypes = [i64, i64, i32, i32]
    lib.cse_xcorr_prepare.restype = i32
    lib.cse_xcorr_prepare.argtypes = [P, i64, i64, i32, i32, P, P]
    lib.cse_xcorr_lag.restype = i32
    lib.cse_xcorr_lag.argtypes = [P, P, P, i64, i64, i32, i32, P, P, P, P, P, P]
    lib.cse_stoi_workspace_bytes.restype = i64
    lib.cse_stoi_workspace_bytes.argtypes = [i64, i64]
    lib.cse_stoi_scratch_bytes.restype = i64
    lib.cse_stoi_scratch_bytes.argtypes = [i64, i64]
    lib.cse_stoi_prepare.restype = i32
    lib.cse_stoi_prepare.argtypes = [P, i64, i64, i32, P, P]
    lib.cse_stoi_cells.restype = i32
    lib.cse_stoi_cells.argtypes = [P, P, P, P, i64, i64, i64, i32, P, P, P, P]
    lib.cse_stoi_workspace_bytes_sr.restype = i64
    lib.cse_stoi_workspace_bytes_sr.argtypes = [i64, i64, i32]
    lib.cse_stoi_scratch_bytes_sr.restype = i64
    lib.cse_stoi_scratch_bytes_sr.argtypes = [i64, i64, i32]
    lib.cse_stoi_cells_sr.restype = i32
    lib.cse_stoi_cells_sr.argtypes = [P, P, P, P, i64, i64, i64, i32, i32, P, P, P, P]
    lib.cse_stoi_layout.restype = i32
    lib.cse_stoi_layout.argtypes = [i64, i64, i32, i32, P, i32]
    lib.cse_estoi_workspace_bytes.restype = i64
    lib.cse_estoi_workspace_bytes.argtypes = [i64, i64, i32]
    lib.cse_estoi_prepare.restype = i32
    lib.cse_estoi_prepare.argtypes = [P, i64, i64, i32, P, P]
    lib.cse_estoi_cells.restype = i32
    lib.cse_estoi_cells.argtypes = [P, P, P, P, i64, i64, i64, i32, i32, P, P, P, P]
    for default_entry, entry in TRACKER_EXPORTS.values():
        getattr(lib, default_entry).restype = None
        getattr(lib, default_entry).argtypes = [P]
        getattr(lib, entry).restype = i32
        getattr(lib, entry).argtypes = [P, i64, i32, i32, P, f64, P, P]
    for score, n_out in CELL_SCORES.items():
        size, prepare, scratch, cells = (getattr(lib, e) for e in CELL_SCORE_EXPORTS[score])
        size.restype = scratch.restype = i64
        size.argtypes = [i64, i64, i32]
        scratch.argtypes = [i64, i64, i32]
        prepare.restype = cells.restype = i32
        prepare.argtypes = [P, i64, i64, i32, P, P]
        # the test signals and their indices, the plan, scratch, the outputs, the stream
        cells.argtypes = [P, P, P, P, i64, i64, i64, i32, i32, P, P] + [P] * n_out + [P]
    lib.cse_csii_workspace_bytes.restype = lib.cse_csii_scratch_bytes.restype = i64
    lib.cse_csii_workspace_bytes.argtypes = [i64, i64, i32]
    lib.cse_csii_scratch_bytes.argtypes = [i64, i64, i32]
    lib.cse_csii_prepare.restype = lib.cse_csii_cells.restype = i32
    lib.cse_csii_prepare.argtypes = [P, i64, i64, i32, P, P]
    lib.cse_csii_cells.argtypes = [P, P, P, P, i64, i64, i64, i32, i32, P, P, P, P]
    lib.cse_ncm_workspace_bytes.restype = lib.cse_ncm_scratch_bytes.restype = i64
    lib.cse_ncm_workspace_bytes.argtypes = [i64, i64, i32]
    lib.cse_ncm_scratch_bytes.argtypes = [i64, i64, i32]
    lib.cse_ncm_prepare.restype = lib.cse_ncm_cells.restype = i32
    lib.cse_ncm_prepare.argtypes = [P, i64, i64, i32, P, P]
    lib.cse_ncm_cells.argtypes = [P, P, P, P, i64, i64, i64, i32, i32, P, P, f64, P, P]
    lib.cse_sisdr_workspace_bytes.restype = i64
    lib.cse_sisdr_workspace_bytes.argtypes = [i64, i64, i32]
    lib.cse_sisdr_prepare.restype = i32
    lib.cse_sisdr_prepare.argtypes = [P, P, i64, i64, i32, P, P]
    lib.cse_sisdr_scratch_bytes.restype = i64
    lib.cse_sisdr_scratch_bytes.argtypes = [i64, i64]
    lib.cse_sisdr_cells.restype = i32
    lib.cse_sisdr_cells.argtypes = [P, P, P, P, i64, i64, i64, i32, P, P, P, P, P, P, P]
    lib.cse_logerr_default_params.restype = None
    lib.cse_logerr_default_params.argtypes = [P, i32]
    lib.cse_logerr_reference.restype = i32
    lib.cse_logerr_reference.argtypes = [P, i64, i32, i32, f64, P, P]
    lib.cse_logerr_scratch_bytes.restype = i64
    lib.cse_logerr_scratch_bytes.argtypes = [i64, i32]
    lib.cse_logerr_rows.restype = i32
    lib.cse_logerr_rows.argtypes = [P, i64, i32, i32, P, P, P, P, i64, P, P, P, P, P, P, P]
    lib.cse_online_state_bytes.restype = i64
    lib.cse_online_state_bytes.argtypes = [i32, i64]
    lib.cse_online_init.restype = lib.cse_online_prime.restype = i32
    lib.cse_online_push.restype = lib.cse_online_finish.restype = i32
    lib.cse_online_init.argtypes = [P, P, i64, P]
    lib.cse_online_prime.argtypes = [P, P, P]
    lib.cse_online_push.argtypes = [P, P, i32, P, P, P]
    lib.cse_online_finish.argtypes = [P, P, P]
    lib.cse_pool_state_bytes.restype = lib.cse_pool_work_bytes.restype = i64
    lib.cse_pool_state_bytes.argtypes = [i32, i64]
    lib.cse_pool_work_bytes.argtypes = [i64]
    for entry in EXPORTS_POOL[2:]:
        getattr(lib, entry).restype = i32
    lib.cse_pool_init.argtypes = [P, P, i64, P, P, P]   # handle, config, capacity, state, work, slots
    lib.cse_pool_open.argtypes = [P, i64, P, P, P]      # handle, slot, params or NULL, x_head, stream
    lib.cse_pool_step.argtypes = [P, P, i32, P, P, P, P]  # handle, items, n, x, y, n_out, stream
    lib.cse_pool_close.argtypes = [P, i64, P, P]        # handle, slot, y_tail, stream
    lib.cse_pool_drop.argtypes = [P, i64]
    lib.cse_enhance_cells.restype = i32
    lib.cse_enhance_cells.argtypes = [i32, i64, P, i64, P, P, P, P, i64, P, P, P, P]
    lib.cse_enhance_cells_short_hop.restype = i32
    lib.cse_enhance_cells_short_hop.argtypes = [i32, i64, P, i64, P, P, P, P, i64, P, P, P]
    lib.cse_enhance_cells_generic.restype = i32
    lib.cse_enhance_cells_generic.argtypes = [i32, i64, P, i64, P, P, P, P, i64, P, P, P, P]
    # the kernels read the cell/job tables laid out as this package packs them:
    # refuse a library of another ABI revision.  The packer (engine.pack_waves)
    # takes the slot-group size from the library itself; it must be usable.
    ver = lib.cse_version()
    if ver != ABI_VERSION:
        raise CseError(f"{path}: ABI version {ver}, this package mirrors {ABI_VERSION} (rebuild)")
    for n_fft in (512, 1024):
        per = lib.cse_cells_per_group(n_fft)
        if per <= 0 or per % 2:
            raise CseError(f"{path}: {per} cells per slot group at n_fft={n_fft}")
    _lib = lib
    return lib


def check(rc, what):
    if rc != CSE_OK:
        msg = load().cse_last_error().decode(errors="replace")
        raise CseError(f"{what} failed ({rc}): {msg}")
