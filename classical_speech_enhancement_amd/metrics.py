"""Scores of the reference's sweep, on the device.

Mirrors of Code/evaluation_metrics.py:
  calculate_stoi                   :30-36   pystoi 0.4.1 stoi(..., extended=False)
                                            -> libcse.so cse_stoi_prepare / cse_stoi_cells
  calculate_snr                    :39-58
  calculate_combined_speech_score  :104-115
  calculate_pesq                   :9-27    the pesq C extension is not in this
                                            image: returns None like the
                                            reference's failure path (:25-27)
  evaluate_audio_quality           :61-101

StoiPlan is the batched form the sweep uses: the clean side (10-kHz clean,
silent-frame mask, band envelopes, segment statistics) is prepared once per
batch of equal-length signals, then any number of cell outputs are scored
against it, each shifted by its alignment lag and clipped like
finalize_enhanced (speech_enhancement_comparison.py:92-106).  The sweep runs
at the reference's working rate, 16 kHz (:381), resampled to 10 kHz inside the
cell kernel; other rates (1-768 kHz, 10 kHz unresampled) go through a generic
fp64 resampler first (cse_stoi_cells_sr).  There is no CPU fallback.

extended=True scores extended STOI (Jensen & Taal 2016; pystoi's
``extended=True``, which the reference never passes) through cse_estoi_prepare /
cse_estoi_cells: the same clean side plus per-(segment, frame) column
statistics, the same resampling, silent-frame removal and band envelopes, then
the row- and column-normalised correlation defined in include/cse_estoi.h
(no jitter; norm + eps divisors).

SegSnrPlan scores the two quality measures of include/cse_segsnr.h, segmental
SNR and frequency-weighted segmental SNR (Hu & Loizou 2008's best non-PESQ
predictor of quality for this project's algorithm families), the same way: the
clean side once per batch (cse_segsnr_prepare), then any number of cells
(cse_segsnr_cells) with STOI's lag / clip test-signal definition.  The
reference scores neither; evaluate_audio_quality adds them only on request.

LpcPlan scores the two envelope-distortion measures of include/cse_lpc.h, the
log-likelihood ratio and the LPC cepstrum distance (lower is better), through
the same interface (cse_lpc_prepare / cse_lpc_cells).

WssPlan scores the weighted spectral slope distance of include/cse_wss.h (Klatt
1982; lower is better) the same way, one score per cell (cse_wss_prepare /
cse_wss_cells).  With it the device delivers every ingredient of Hu & Loizou's
composite measures but PESQ: composite() takes the caller's PESQ values with
LLR, WSS and segSNR and returns CSIG, CBAK and COVL.

CsiiPlan scores the three-level coherence speech intelligibility index of
include/cse_csii.h (Kates & Arehart 2005) and its fit I3, the intelligibility
measure Ma, Hu & Loizou (2009) found to predict best for this project's
algorithm families, through the same interface (cse_csii_prepare /
cse_csii_cells): four values per cell, higher is better.  It is no score family
(scores.FAMILIES): like extended STOI it can take STOI's place as the sweep's
intelligibility column (search: coherence=True), and evaluate_audio_quality adds
it on request (coherence=True).

NcmPlan scores the normalized covariance measure of include/cse_ncm.h, the
measure of the speech-transmission-index family and the other of the two best
predictors in Ma, Hu & Loizou (2009): the squared correlation of the slow band
envelopes of clean and test signal over the whole clip, with the fixed
articulation-index weights (ncm) and with that study's signal-dependent
band-importance weights, the clean band-envelope energy raised to bif_power
(ncm_bif), through cse_ncm_prepare / cse_ncm_cells: two values per cell, higher
is better.  Like CsiiPlan it is no score family: it can take STOI's place as the
sweep's intelligibility column (search: modulation=True), and
evaluate_audio_quality adds it on request (modulation=True).

SiSdrPlan scores the scale-invariant SDR of include/cse_sisdr.h (Le Roux et al.
2019) and, when the batch's noisy signals are given, its split into SI-SIR
(residual interference) and SI-SAR (artifacts) through cse_sisdr_prepare /
cse_sisdr_cells, with the same lag / clip test-signal definition, at any rate.

NoiseErrPlan scores noise-PSD estimates, not waveforms: the logarithmic
estimation error of include/cse_logerr.h against the smoothed power of
noisy - clean (cse_logerr_reference / cse_logerr_rows), split into over- and
under-estimation, per row and on request per frame.

What the waveform plans share is written once: _cell_index checks every
score_async's y and index arrays, SegSnrPlan._launch is the chunked launch of
the three plans on the segSNR interface, and _pair_score is the scalar wrapper
(two equal-length signals, one plan, one score, NaN raises) behind stoi, segsnr,
fwsegsnr, llr, cepstrum_distance and wss.  evaluate_audio_quality's optional
groups follow scores.FAMILIES and find calculate_<name> by name.
"""

import ctypes
import math

import numpy as np
import torch

from . import _lib
from .engine import _ptr, _stream
from .scores import requested

STOI_SR = 16000
# cells per cse_stoi_cells launch: bounds the envelope scratch (Mmax x 64 B per cell)
STOI_CHUNK = 16384


_GPU = None


def _gpu_visible():
    global _GPU
    if _GPU is None:
        _GPU = bool(torch.cuda.is_available())
    return _GPU


def _cell_index(plan, y, y_offset, sig_of, lag):
    """Every plan's checks of score_async's y and index arrays: (y_offset,
    sig_of, lag or None) on the plan's device, and the number of cells.  Host
    arrays are validated against the plan's S and L and uploaded on the current
    stream; cuda tensors get every check that needs no host synchronisation
    (the value ranges are the caller's; the kernels read int64 / int32 / int32)."""
    dev = plan.clean.device
    if y.dtype != torch.float32 or not y.is_cuda:
        raise ValueError("y must be a float32 cuda tensor")
    if torch.is_tensor(y_offset):
        off, sig = y_offset, sig_of
        if not torch.is_tensor(sig):
            raise ValueError("sig_of must be a cuda tensor when y_offset is one")
        if off.dtype != torch.int64 or sig.dtype != torch.int32:
            raise ValueError("device y_offset / sig_of must be int64 / int32")
        if off.device != dev or sig.device != dev:
            raise ValueError("device y_offset / sig_of must live on the clean signal's GPU")
        if not (off.is_contiguous() and sig.is_contiguous()):
            raise ValueError("device y_offset / sig_of must be contiguous")
        n = int(off.numel())
        if int(sig.numel()) != n:
            raise ValueError("y_offset and sig_of differ in length")
    else:
        off_h = np.asarray(y_offset, dtype=np.int64)
        sig_h = np.asarray(sig_of, dtype=np.int32)
        n = len(off_h)
        if len(sig_h) != n:
            raise ValueError("y_offset and sig_of differ in length")
        if n and (int(sig_h.min()) < 0 or int(sig_h.max()) >= plan.S):
            raise ValueError("sig_of out of range")
        if n and (int(off_h.min()) < 0 or int(off_h.max()) + plan.L > y.numel()):
            raise ValueError("a cell's output runs past the end of y")
        off = torch.as_tensor(off_h, device=dev)
        sig = torch.as_tensor(sig_h, device=dev)
    lg = None
    if lag is not None:
        if torch.is_tensor(lag):
            if lag.device != dev:
                raise ValueError("device lag must live on the clean signal's GPU")
            lg = lag.to(torch.int32).contiguous()
        else:
            lg = torch.as_tensor(np.asarray(lag, dtype=np.int32), device=dev)
        if int(lg.numel()) != n:
            raise ValueError("lag and y_offset differ in length")
    return off, sig, lg, n


class StoiPlan:
    """Clean side of STOI for S equal-length signals (clean: [S, L] f64 cuda);
    extended=True: of extended STOI, which the plan then scores."""

    def __init__(self, clean, sr=STOI_SR, extended=False):
        if not _gpu_visible():
            raise _lib.CseError("no GPU visible: the HIP engine has no CPU fallback")
        self.lib = _lib.load()
        clean = clean.contiguous()
        if clean.dtype != torch.float64 or clean.dim() != 2 or not clean.is_cuda:
            raise ValueError("clean must be a [S, L] float64 cuda tensor")
        self.S, self.L = clean.shape
        self.clean = clean
        self.sr = int(sr)
        self.extended = bool(extended)
        size_fn, prepare, name = (
            (self.lib.cse_estoi_workspace_bytes, self.lib.cse_estoi_prepare, "cse_estoi_prepare")
            if self.extended else
            (self.lib.cse_stoi_workspace_bytes_sr, self.lib.cse_stoi_prepare, "cse_stoi_prepare"))
        nbytes = int(size_fn(self.S, self.L, self.sr))
        if nbytes < 0:
            raise NotImplementedError(f"STOI: sample rate {sr} not supported (1000-768000 Hz)")
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=clean.device)
        _lib.check(prepare(_ptr(clean), self.S, self.L, sr, _ptr(self.ws), _stream()), name)
        self._scratch = None

    def _scratch_for(self, n):
        nbytes = max(int(self.lib.cse_stoi_scratch_bytes_sr(n, self.L, self.sr)), 1)
        if self._scratch is None or self._scratch.numel() < nbytes:
            self._scratch = torch.empty(nbytes, dtype=torch.uint8, device=self.clean.device)
        return self._scratch

    def score_async(self, y, y_offset, sig_of, lag=None, clip=True, out=None):
        """Enqueue the STOI of every cell; returns the [n] f64 cuda result.

        y: flat f32 cuda tensor holding every cell's output (>= L samples from
        y_offset[c]); sig_of: clean signal of each cell; lag: alignment lag
        (None = 0).  The test signal of cell c is y[n - lag] (zero outside
        [0, L)), clipped to [-1, 1] when clip.  y_offset / sig_of / lag given
        as host arrays are validated here and uploaded on the current stream;
        given as cuda tensors (int64 / int32 / int32) they are taken as they
        are, with no host synchronisation (the caller validated them)."""
        dev = self.clean.device
        if torch.is_tensor(lag):
            # this plan alone takes a device lag as it is, like the device
            # indices, and with host indices moves a lag tensor to its GPU
            if not torch.is_tensor(y_offset):
                lag = lag.to(dev)
            elif lag.dtype != torch.int32 or lag.device != dev or not lag.is_contiguous() \
                    or lag.numel() != y_offset.numel():
                raise ValueError("device lag must be a contiguous int32 tensor of n entries "
                                 "on the clean signal's GPU")
        off, sig, lg, n = _cell_index(self, y, y_offset, sig_of, lag)
        if out is None:
            out = torch.empty(n, dtype=torch.float64, device=dev)
        for s in range(0, n, STOI_CHUNK):
            m = min(STOI_CHUNK, n - s)
            scratch = self._scratch_for(m)
            args = (_ptr(y), _ptr(off[s:]), None if lg is None else _ptr(lg[s:]), _ptr(sig[s:]),
                    m, self.S, self.L)
            tail = (1 if clip else 0, _ptr(self.ws), _ptr(scratch), _ptr(out[s:]), _stream())
            if self.extended:
                _lib.check(self.lib.cse_estoi_cells(*args, self.sr, *tail), "cse_estoi_cells")
            elif self.sr == STOI_SR:
                _lib.check(self.lib.cse_stoi_cells(*args, *tail), "cse_stoi_cells")
            else:
                _lib.check(self.lib.cse_stoi_cells_sr(*args, self.sr, *tail), "cse_stoi_cells_sr")
        return out

    def score(self, y, y_offset, sig_of, lag=None, clip=True):
        """score_async, synchronised; NaN entries are pystoi failures (None)."""
        return self.score_async(y, y_offset, sig_of, lag, clip).cpu().numpy()

    def layout(self):
        """cse_stoi_layout of this plan's workspace: name -> byte offset, size
        or constant (_lib.STOI_LAYOUT_FIELDS)."""
        out = np.zeros(len(_lib.STOI_LAYOUT_FIELDS), dtype=np.int64)
        _lib.check(self.lib.cse_stoi_layout(self.S, self.L, self.sr, int(self.extended),
                                            out.ctypes.data, len(out)), "cse_stoi_layout")
        return dict(zip(_lib.STOI_LAYOUT_FIELDS, (int(v) for v in out)))

    def stages(self):
        """The clean side's stages as typed views of self.ws (no copy), for
        tests and tools: coef [5, 128] (16 kHz) or None, meta [S, META] (K, M,
        J, ok, nblk), x10 [S, n10], en [S, F], kf [S, F], btab [S, NBLK, BT],
        xtob [S, Mmax, 16], xstat [S, Jmax, 16, 4], hgen [taps] (other rates)
        or None, xcol [S, Jmax, 30, 2] (extended) or None, and "layout".
        Rows >= M, column 15 and entries past K / nblk are unspecified."""
        lay = self.layout()
        S = self.S

        def view(name, dtype, shape):
            n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
            return self.ws[lay[name]:lay[name] + n].view(dtype).view(*shape)

        f64, i32 = torch.float64, torch.int32
        out = {
            "layout": lay,
            "coef": view("coef64", f64, (5, 128)) if self.sr == STOI_SR else None,
            "meta": view("meta", i32, (S, lay["META"])),
            "x10": view("x10", f64, (S, lay["n10"])),
            "en": view("en", f64, (S, lay["F"])),
            "kf": view("kf", i32, (S, lay["F"])),
            "btab": view("btab", i32, (S, lay["NBLK"], lay["BT"])),
            "xtob": view("xtob", f64, (S, lay["Mmax"], 16)),
            "xstat": view("xstat", f64, (S, lay["Jmax"], 16, 4)),
            "hgen": None if self.sr == STOI_SR else view("hgen", f64, (lay["ntap"],)),
            "xcol": view("xcol", f64, (S, lay["Jmax"], 30, 2)) if self.extended else None,
        }
        return out

    def cell_envelopes(self, n):
        """Band envelopes [n, Mmax, 16] of the n <= STOI_CHUNK cells the last
        score / score_async scored (a view of the scratch; rows >= M of the
        cell's signal and column 15 are unspecified)."""
        if not 0 < n <= STOI_CHUNK or self._scratch is None:
            raise ValueError("cell_envelopes: after a score of 1..STOI_CHUNK cells")
        Mmax = self.layout()["Mmax"]
        return self._scratch[:n * Mmax * 128].view(torch.float64).view(n, Mmax, 16)

    def cell_y10(self, n):
        """At rates other than 16 kHz: the 10-kHz test signals [n, n10] of the
        n <= STOI_CHUNK cells the last score scored (the scratch after the
        envelopes)."""
        if self.sr == STOI_SR:
            raise ValueError("cell_y10: 16-kHz cells are resampled inside the cell kernel")
        if not 0 < n <= STOI_CHUNK or self._scratch is None:
            raise ValueError("cell_y10: after a score of 1..STOI_CHUNK cells")
        lay = self.layout()
        o = n * lay["Mmax"] * 128
        return self._scratch[o:o + n * lay["n10"] * 8].view(torch.float64).view(n, lay["n10"])


SEGSNR_RATES = (16000, 8000)
# bound on the scratch of one cse_segsnr_cells launch: the cells per launch come
# from this budget and the library's per-cell figure, never from a fixed count
SEGSNR_SCRATCH_BYTES = 1 << 30
# cells per launch when the kernel needs no scratch (the grid's x dimension)
SEGSNR_MAX_CELLS = 1 << 20


class SegSnrPlan:
    """Clean side of segSNR / fwSegSNR for S equal-length signals (clean:
    [S, L] f64 cuda) at 16 or 8 kHz."""

    # the library's four entry points are _PREFIX + _workspace_bytes / _prepare /
    # _scratch_bytes / _cells; _WHICH names the two score columns (LpcPlan
    # scores through the same code with its own)
    _PREFIX = "cse_segsnr"
    _LABEL = "segSNR"
    _WHICH = ("segsnr", "fwsegsnr")

    def _fn(self, name):
        return getattr(self.lib, f"{self._PREFIX}_{name}")

    def __init__(self, clean, sr=STOI_SR):
        if not _gpu_visible():
            raise _lib.CseError("no GPU visible: the HIP engine has no CPU fallback")
        self.lib = _lib.load()
        clean = clean.contiguous()
        if clean.dtype != torch.float64 or clean.dim() != 2 or not clean.is_cuda:
            raise ValueError("clean must be a [S, L] float64 cuda tensor")
        self.S, self.L = clean.shape
        self.clean = clean
        self.sr = int(sr)
        nbytes = int(self._fn("workspace_bytes")(self.S, self.L, self.sr))
        if nbytes < 0:
            raise NotImplementedError(
                f"{self._LABEL}: sample rate {sr} not supported (16000, 8000 Hz)")
        self.ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=clean.device)
        _lib.check(self._fn("prepare")(_ptr(clean), self.S, self.L, self.sr, _ptr(self.ws),
                                       _stream()), f"{self._PREFIX}_prepare")
        self._scratch = None

    def cells_per_launch(self):
        """Cells of one launch: SEGSNR_SCRATCH_BYTES over the library's scratch
        per cell at this length and rate; SEGSNR_MAX_CELLS when it needs none."""
        per = int(self._fn("scratch_bytes")(1, self.L, self.sr))
        if per <= 0:
            return SEGSNR_MAX_CELLS
        return int(max(1, min(SEGSNR_MAX_CELLS, SEGSNR_SCRATCH_BYTES // per)))

    def _scratch_for(self, n):
        nbytes = int(self._fn("scratch_bytes")(n, self.L, self.sr))
        if nbytes <= 0:
            return None
        if self._scratch is None or self._scratch.numel() < nbytes:
            self._scratch = torch.empty(nbytes, dtype=torch.uint8, device=self.clean.device)
        return self._scratch

    def score_async(self, y, y_offset, sig_of, lag=None, clip=True, out=None, which="both"):
        """Enqueue both scores of every cell; returns the [n, 2] f64 cuda result
        (segsnr, fwsegsnr).  The arguments are StoiPlan.score_async's: host
        index arrays are validated and uploaded, cuda tensors (int64 / int32 /
        int32) are taken as they are.  which="segsnr" / "fwsegsnr" computes
        that score alone (the other column is NaN; "segsnr" skips the
        transforms)."""
        dev = self.clean.device
        first, second = self._WHICH
        if which not in ("both", first, second):
            raise ValueError(f"which={which!r}: 'both', {first!r} or {second!r}")
        off, sig, lg, n = _cell_index(self, y, y_offset, sig_of, lag)
        if out is None:
            out = torch.empty((n, 2), dtype=torch.float64, device=dev)
        if out.shape != (n, 2) or out.dtype != torch.float64 or not out.is_contiguous():
            raise ValueError("out must be a contiguous [n, 2] float64 tensor")
        # the library writes one column each: planar scratch rows, then one copy
        cols = torch.full((2, n), float("nan"), dtype=torch.float64, device=dev)
        self._launch(y, off, sig, lg, n, clip, (None if which == second else cols[0],
                                                None if which == first else cols[1]))
        out.copy_(cols.t())
        return out

    def _launch(self, y, off, sig, lg, n, clip, outs):
        """The cells kernel over n cells, cells_per_launch() at a time; outs: one
        [n] f64 row per output pointer of the entry point, None for a score that
        is not asked for."""
        step = self.cells_per_launch()
        for s in range(0, n, step):
            m = min(step, n - s)
            scratch = self._scratch_for(m)
            _lib.check(self._fn("cells")(
                _ptr(y), _ptr(off[s:]), None if lg is None else _ptr(lg[s:]), _ptr(sig[s:]), m,
                self.S, self.L, self.sr, 1 if clip else 0, _ptr(self.ws),
                None if scratch is None else _ptr(scratch),
                *(None if o is None else _ptr(o[s:]) for o in outs), _stream()),
                f"{self._PREFIX}_cells")

    def score(self, y, y_offset, sig_of, lag=None, clip=True, which="both"):
        """score_async, synchronised: [n, 2] numpy (segsnr, fwsegsnr); NaN: no
        frame, or no non-silent frame."""
        return self.score_async(y, y_offset, sig_of, lag, clip, which=which).cpu().numpy()


class LpcPlan(SegSnrPlan):
    """Clean side of the LLR / LPC cepstrum distance (include/cse_lpc.h) for S
    equal-length signals at 16 or 8 kHz: SegSnrPlan's interface on
    cse_lpc_prepare / cse_lpc_cells.  score_async returns [n, 2] (llr, cep);
    which="llr" / "cep" computes that score alone (the other column is NaN;
    "llr" skips the cepstrum recursion).  Clips of more than 1536 frames (11.5 s)
    select through scratch the library sizes; the launches are chunked by it."""

    _PREFIX = "cse_lpc"
    _LABEL = "LLR/CEP"
    _WHICH = ("llr", "cep")


class WssPlan(SegSnrPlan):
    """Clean side of the weighted spectral slope distance (include/cse_wss.h) for
    S equal-length signals at 16 or 8 kHz: SegSnrPlan's construction, checks and
    launch chunking on cse_wss_prepare / cse_wss_cells, with one score per cell
    (lower is better).  Clips of more than 1536 frames (11.5 s) select through
    scratch the library sizes."""

    _PREFIX = "cse_wss"
    _LABEL = "WSS"
    _WHICH = ("wss",)

    def score_async(self, y, y_offset, sig_of, lag=None, clip=True, out=None):
        """Enqueue the score of every cell; returns the [n] f64 cuda result.  The
        arguments are SegSnrPlan.score_async's."""
        off, sig, lg, n = _cell_index(self, y, y_offset, sig_of, lag)
        if out is None:
            out = torch.empty(n, dtype=torch.float64, device=self.clean.device)
        if out.shape != (n,) or out.dtype != torch.float64 or not out.is_contiguous():
            raise ValueError("out must be a contiguous [n] float64 tensor")
        self._launch(y, off, sig, lg, n, clip, (out,))
        return out

    def score(self, y, y_offset, sig_of, lag=None, clip=True):
        """score_async, synchronised: [n] numpy; NaN: no frame, or no non-silent
        frame."""
        return self.score_async(y, y_offset, sig_of, lag, clip).cpu().numpy()


class CsiiPlan(SegSnrPlan):
    """Clean side of the three-level CSII and I3 (include/cse_csii.h) for S
    equal-length signals at 16 or 8 kHz: SegSnrPlan's construction, checks and
    launch chunking on cse_csii_prepare / cse_csii_cells, with four values per
    cell (csii_high, csii_mid, csii_low, i3; higher is better).  A level with no
    frame scores NaN, and I3 is NaN when the mid or the low level has none."""

    _PREFIX = "cse_csii"
    _LABEL = "CSII"
    _WHICH = ("csii_high", "csii_mid", "csii_low", "i3")

    def score_async(self, y, y_offset, sig_of, lag=None, clip=True, out=None, which="all"):
        """Enqueue the four values of every cell; returns the [n, 4] f64 cuda
        result.  The arguments are SegSnrPlan.score_async's.  which="i3" (or
        another name of _WHICH) returns that column alone, [n]; the kernel
        computes all four either way."""
        if which != "all" and which not in self._WHICH:
            raise ValueError(f"which={which!r}: 'all' or one of {self._WHICH}")
        off, sig, lg, n = _cell_index(self, y, y_offset, sig_of, lag)
        dev = self.clean.device
        if which != "all":
            table = torch.empty((n, 4), dtype=torch.float64, device=dev)
            self._launch(y, off, sig, lg, n, clip, (table,))
            col = table[:, self._WHICH.index(which)]
            if out is None:
                return col.contiguous()
            if out.shape != (n,) or out.dtype != torch.float64:
                raise ValueError("out must be a [n] float64 tensor")
            out.copy_(col)
            return out
        if out is None:
            out = torch.empty((n, 4), dtype=torch.float64, device=dev)
        if out.shape != (n, 4) or out.dtype != torch.float64 or not out.is_contiguous():
            raise ValueError("out must be a contiguous [n, 4] float64 tensor")
        self._launch(y, off, sig, lg, n, clip, (out,))
        return out

    def score(self, y, y_offset, sig_of, lag=None, clip=True, which="all"):
        """score_async, synchronised: [n, 4] numpy (or [n] for one column)."""
        return self.score_async(y, y_offset, sig_of, lag, clip, which=which).cpu().numpy()


class NcmPlan(SegSnrPlan):
    """Clean side of the normalized covariance measure (include/cse_ncm.h) for S
    equal-length signals at 16 or 8 kHz: SegSnrPlan's construction, checks and
    launch chunking on cse_ncm_prepare / cse_ncm_cells, with two values per cell
    (ncm, with the fixed articulation-index weights, and ncm_bif, with the clean
    band-envelope energies raised to bif_power as weights; higher is better).
    The clean side does not depend on the exponent: bif_power is the plan's
    default, and score_async takes another per call.  Clips of fewer than 12
    frames and all-zero clean signals score NaN."""

    _PREFIX = "cse_ncm"
    _LABEL = "NCM"
    _WHICH = ("ncm", "ncm_bif")

    def __init__(self, clean, sr=STOI_SR, bif_power=1.0):
        self.bif_power = _bif_power(bif_power)
        super().__init__(clean, sr)

    def score_async(self, y, y_offset, sig_of, lag=None, clip=True, out=None, which="both",
                    bif_power=None):
        """Enqueue both values of every cell; returns the [n, 2] f64 cuda result
        (ncm, ncm_bif).  The arguments are SegSnrPlan.score_async's.
        which="ncm" / "ncm_bif" returns that column alone, [n]; the kernel
        computes both either way.  bif_power: the exponent of this call (default:
        the plan's)."""
        if which != "both" and which not in self._WHICH:
            raise ValueError(f"which={which!r}: 'both' or one of {self._WHICH}")
        p = self.bif_power if bif_power is None else _bif_power(bif_power)
        off, sig, lg, n = _cell_index(self, y, y_offset, sig_of, lag)
        dev = self.clean.device
        if which != "both":
            table = torch.empty((n, 2), dtype=torch.float64, device=dev)
            self._launch(y, off, sig, lg, n, clip, (table,), p)
            col = table[:, self._WHICH.index(which)]
            if out is None:
                return col.contiguous()
            if out.shape != (n,) or out.dtype != torch.float64:
                raise ValueError("out must be a [n] float64 tensor")
            out.copy_(col)
            return out
        if out is None:
            out = torch.empty((n, 2), dtype=torch.float64, device=dev)
        if out.shape != (n, 2) or out.dtype != torch.float64 or not out.is_contiguous():
            raise ValueError("out must be a contiguous [n, 2] float64 tensor")
        self._launch(y, off, sig, lg, n, clip, (out,), p)
        return out

    def _launch(self, y, off, sig, lg, n, clip, outs, bif_power):
        """SegSnrPlan._launch with the exponent before the output pointer; outs:
        one contiguous [n, 2] table."""
        step = self.cells_per_launch()
        for s in range(0, n, step):
            m = min(step, n - s)
            scratch = self._scratch_for(m)
            _lib.check(self._fn("cells")(
                _ptr(y), _ptr(off[s:]), None if lg is None else _ptr(lg[s:]), _ptr(sig[s:]), m,
                self.S, self.L, self.sr, 1 if clip else 0, _ptr(self.ws),
                None if scratch is None else _ptr(scratch), bif_power, _ptr(outs[0][s:]),
                _stream()), f"{self._PREFIX}_cells")

    def score(self, y, y_offset, sig_of, lag=None, clip=True, which="both", bif_power=None):
        """score_async, synchronised: [n, 2] numpy (or [n] for one column)."""
        return self.score_async(y, y_offset, sig_of, lag, clip, which=which,
                                bif_power=bif_power).cpu().numpy()


def _bif_power(p):
    """The band-importance exponent as a finite float >= 0, or ValueError."""
    p = float(p)
    if not (math.isfinite(p) and p >= 0.0):
        raise ValueError(f"bif_power={p!r}: a finite number >= 0")
    return p


class SiSdrPlan:
    """Clean side of SI-SDR / SI-SIR / SI-SAR (include/cse_sisdr.h) for S
    equal-length signals (clean: [S, L] f64 cuda, any rate).  noisy ([S, L] f64
    cuda) gives the interference noisy - clean; without it only SI-SDR is
    defined.  zero_mean removes the means of the signals first (the sums are
    centred)."""

    _WHICH = ("sisdr", "sisir", "sisar")

    def __init__(self, clean, noisy=None, zero_mean=True):
        if not _gpu_visible():
            raise _lib.CseError("no GPU visible: the HIP engine has no CPU fallback")
        self.lib = _lib.load()
        clean = clean.contiguous()
        if clean.dtype != torch.float64 or clean.dim() != 2 or not clean.is_cuda:
            raise ValueError("clean must be a [S, L] float64 cuda tensor")
        if noisy is not None:
            noisy = noisy.contiguous()
            if noisy.dtype != torch.float64 or noisy.shape != clean.shape or \
                    noisy.device != clean.device:
                raise ValueError("noisy must be a float64 cuda tensor of clean's shape and device")
        self.S, self.L = clean.shape
        if self.L < 1:
            raise ValueError("SI-SDR expects non-empty signals")
        self.clean = clean
        self.with_noise = noisy is not None
        self.zero_mean = bool(zero_mean)
        nbytes = int(self.lib.cse_sisdr_workspace_bytes(self.S, self.L, int(self.with_noise)))
        self.ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=clean.device)
        _lib.check(self.lib.cse_sisdr_prepare(
            _ptr(clean), None if noisy is None else _ptr(noisy), self.S, self.L,
            int(self.zero_mean), _ptr(self.ws), _stream()), "cse_sisdr_prepare")

    def score_async(self, y, y_offset, sig_of, lag=None, clip=True, out=None, which="all"):
        """Enqueue the scores of every cell; returns the [n, 3] f64 cuda result
        (sisdr, sisir, sisar).  The arguments are StoiPlan.score_async's: host
        index arrays are validated and uploaded, cuda tensors (int64 / int32 /
        int32) are taken as they are.  which="sisdr" computes SI-SDR alone
        (the other columns are NaN; the interference is not read); a plan made
        without noisy scores nothing else."""
        dev = self.clean.device
        if which not in ("all", "sisdr"):
            raise ValueError(f"which={which!r}: 'all' or 'sisdr'")
        off, sig, lg, n = _cell_index(self, y, y_offset, sig_of, lag)
        if out is None:
            out = torch.empty((n, 3), dtype=torch.float64, device=dev)
        if out.shape != (n, 3) or out.dtype != torch.float64 or not out.is_contiguous():
            raise ValueError("out must be a contiguous [n, 3] float64 tensor")
        # the library writes one column each: planar rows, then one copy
        cols = torch.full((3, n), float("nan"), dtype=torch.float64, device=dev)
        parts = which == "all" and self.with_noise
        for s in range(0, n, SEGSNR_MAX_CELLS):
            m = min(SEGSNR_MAX_CELLS, n - s)
            _lib.check(self.lib.cse_sisdr_cells(
                _ptr(y), _ptr(off[s:]), None if lg is None else _ptr(lg[s:]), _ptr(sig[s:]), m,
                self.S, self.L, 1 if clip else 0, _ptr(self.clean), _ptr(self.ws), None,
                _ptr(cols[0, s:]), _ptr(cols[1, s:]) if parts else None,
                _ptr(cols[2, s:]) if parts else None, _stream()), "cse_sisdr_cells")
        out.copy_(cols.t())
        return out

    def score(self, y, y_offset, sig_of, lag=None, clip=True, which="all"):
        """score_async, synchronised: [n, 3] numpy (sisdr, sisir, sisar); NaN,
        +inf and -inf as include/cse_sisdr.h's IEEE rules give them."""
        return self.score_async(y, y_offset, sig_of, lag, clip, which=which).cpu().numpy()


def _pair_signals(x, y, what):
    """Two equal-length non-empty 1-D signals as float64, or the scalars' errors."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    if x.shape != y.shape:
        raise Exception(f"x and y should have the same length, found {x.shape} and {y.shape}")
    if x.ndim != 1 or x.size == 0:
        raise ValueError(f"{what} expects non-empty 1-D signals")
    return x, y


def _pair_score(cls, x, y, what, which=None, nan_message="no non-silent 30-ms frame", **plan_kw):
    """One score of y against the clean x through a one-signal plan of ``cls``:
    its column ``which`` when the plan scores several; a NaN raises."""
    x, y = _pair_signals(x, y, what)
    plan = cls(torch.as_tensor(x).cuda().view(1, -1), **plan_kw)
    yd = torch.as_tensor(y.astype(np.float32)).cuda()
    if which is None:
        v = float(plan.score(yd, [0], [0], clip=False)[0])
    else:
        v = float(plan.score(yd, [0], [0], clip=False, which=which)[0, cls._WHICH.index(which)])
    if math.isnan(v):
        raise ValueError(nan_message)
    return v


def si_sdr(x, y, noisy=None, zero_mean=True):
    """SI-SDR in dB (include/cse_sisdr.h) of y against the clean x; with noisy
    (the unprocessed input, x plus the interference) the triple (si_sdr, si_sir,
    si_sar).  Values may be +-inf or NaN as the header's IEEE rules give them."""
    x, y = _pair_signals(x, y, "si_sdr")
    nz = None
    if noisy is not None:
        nz = np.asarray(noisy, dtype=np.float64)
        if nz.shape != x.shape:
            raise Exception(f"x and noisy should have the same length, found {x.shape} and "
                            f"{nz.shape}")
        nz = torch.as_tensor(nz).cuda().view(1, -1)
    plan = SiSdrPlan(torch.as_tensor(x).cuda().view(1, -1), nz, zero_mean=zero_mean)
    yd = torch.as_tensor(y.astype(np.float32)).cuda()
    v = plan.score(yd, [0], [0], clip=False)[0]
    return float(v[0]) if noisy is None else (float(v[0]), float(v[1]), float(v[2]))


def calculate_sisdr(clean_reference, test_audio, sr):
    """si_sdr with calculate_stoi's shape: trim to the common length, None on
    failure (a NaN score included).  sr is not used: the score has no rate."""
    def fn(x, y, _sr):
        v = si_sdr(x, y)
        if math.isnan(v):
            raise ValueError("SI-SDR is undefined (an all-zero signal)")
        return v
    return _calculate_quality(fn, "SI-SDR", clean_reference, test_audio, sr)


class NoiseErrPlan:
    """Reference side of the noise-PSD logarithmic estimation error
    (include/cse_logerr.h) for S equal-length pairs (clean, noisy: [S, L] f64
    cuda): the power of STFT(noisy - clean) at (n_fft, hop_length), smoothed
    over frames with ``beta`` (cse_logerr_reference).  ``R`` ([S, T, B] f64
    cuda) is that reference PSD, ``T`` and ``B`` its frames and bins.  floor,
    skip_frames (the first scored frame) and bins ((lo, hi), default every bin)
    are what every score() of the plan uses.  beta = 0.9 is this project's
    default, a time constant of about 80 ms at the grid's 8-ms hop."""

    def __init__(self, clean, noisy, n_fft, hop_length, beta=0.9, floor=1e-12, skip_frames=0,
                 bins=None):
        if not _gpu_visible():
            raise _lib.CseError("no GPU visible: the HIP engine has no CPU fallback")
        from .engine import Engine
        for name, x in (("clean", clean), ("noisy", noisy)):
            if not torch.is_tensor(x) or x.dtype != torch.float64 or x.dim() != 2 or \
                    not x.is_cuda:
                raise ValueError(f"{name} must be a [S, L] float64 cuda tensor")
        if noisy.shape != clean.shape or noisy.device != clean.device:
            raise ValueError("noisy must have clean's shape and device")
        eng = Engine(clean.device)
        self.lib = eng.lib
        self.S = int(clean.shape[0])
        _, Pv = eng.stft(noisy.contiguous(), int(n_fft), int(hop_length), x_sub=clean.contiguous(),
                         want_y=False)
        self.T, self.B = int(Pv.shape[1]), int(Pv.shape[2])
        self.prm = _lib.LogErrParams()
        self.lib.cse_logerr_default_params(ctypes.byref(self.prm), self.B)
        self.prm.floor = float(floor)
        self.prm.t0 = int(skip_frames)
        if bins is not None:
            self.prm.bin_lo, self.prm.bin_hi = int(bins[0]), int(bins[1])
        self.beta = float(beta)
        self.R = torch.empty_like(Pv)
        _lib.check(self.lib.cse_logerr_reference(_ptr(Pv), self.S, self.T, self.B, self.beta,
                                                 _ptr(self.R), _stream()), "cse_logerr_reference")

    def _rows(self, N):
        if not torch.is_tensor(N) or N.dtype != torch.float32 or not N.is_cuda or \
                N.device != self.R.device:
            raise ValueError("an estimate must be a float32 cuda tensor on the plan's device")
        if N.dim() == 3 and tuple(N.shape[1:]) == (self.T, self.B):
            return N.contiguous(), self.T * self.B, self.B
        if N.dim() == 2 and int(N.shape[1]) == self.B:
            return N.contiguous(), self.B, 0
        raise ValueError(f"an estimate must be [n, {self.T}, {self.B}] or [n, {self.B}], "
                         f"found {tuple(N.shape)}")

    def score(self, N, sig_of=None, per_frame=False):
        """N: f32 cuda [n, T, B] (time-varying estimates) or [n, B] (static
        ones), or a list mixing both, the rows counted through the list.
        sig_of: the signal of every row (default 0..S-1 when n == S).  Returns
        float64 numpy [n, 3] of (logerr, over, under) in dB, logerr = over +
        under; per_frame=True also returns [n, 2, T] (frame_over, frame_under;
        NaN before skip_frames).  Values follow include/cse_logerr.h's IEEE
        rules; a wrong shape raises ValueError."""
        parts = [self._rows(x) for x in (N if isinstance(N, (list, tuple)) else [N])]
        n = sum(int(p[0].shape[0]) for p in parts)
        if sig_of is None:
            if n != self.S:
                raise ValueError(f"sig_of is needed: {n} rows for {self.S} signals")
            sig_of = np.arange(self.S)
        sig_h = np.asarray(sig_of, dtype=np.int32).reshape(-1)
        if len(sig_h) != n:
            raise ValueError(f"sig_of has {len(sig_h)} entries for {n} rows")
        if n and (int(sig_h.min()) < 0 or int(sig_h.max()) >= self.S):
            raise ValueError("sig_of out of range")
        dev = self.R.device
        cols = torch.empty((2, n), dtype=torch.float64, device=dev)
        fr = torch.empty((2, n, self.T), dtype=torch.float64, device=dev) if per_frame else None
        done = 0
        for x, row_stride, t_stride in parts:
            m = int(x.shape[0])
            if m == 0:
                continue
            off = torch.arange(m, dtype=torch.int64, device=dev) * row_stride
            st = torch.full((m,), t_stride, dtype=torch.int64, device=dev)
            sig = torch.as_tensor(sig_h[done:done + m], device=dev)
            nbytes = int(self.lib.cse_logerr_scratch_bytes(m, self.T))
            scratch = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
            _lib.check(self.lib.cse_logerr_rows(
                _ptr(self.R), self.S, self.T, self.B, _ptr(x), _ptr(off), _ptr(st), _ptr(sig), m,
                ctypes.byref(self.prm), _ptr(scratch), _ptr(cols[0, done:]), _ptr(cols[1, done:]),
                None if fr is None else _ptr(fr[0, done:]),
                None if fr is None else _ptr(fr[1, done:]), _stream()), "cse_logerr_rows")
            done += m
        c = cols.cpu().numpy()
        table = np.empty((n, 3), dtype=np.float64)
        with np.errstate(invalid="ignore"):
            table[:, 0] = c[0] + c[1]
        table[:, 1], table[:, 2] = c[0], c[1]
        if not per_frame:
            return table
        return table, np.ascontiguousarray(fr.cpu().numpy().transpose(1, 0, 2))


def noise_logerr(clean, noisy, N, n_fft, hop_length, per_frame=False, **kw):
    """LogErr in dB (include/cse_logerr.h) of one noise-PSD estimate N of the
    pair (clean, noisy), numpy in and out.  N is shaped as
    plugins.noise_estimation returns it: (B, T), (B, 1) or (B,).  kw: beta,
    floor, skip_frames, bins of NoiseErrPlan.  Returns {logerr, over, under},
    with per_frame=True also frame_over and frame_under ([T])."""
    c = np.asarray(clean, dtype=np.float64)
    z = np.asarray(noisy, dtype=np.float64)
    if c.ndim != 1 or c.shape != z.shape or c.size == 0:
        raise ValueError("clean and noisy must be non-empty 1-D signals of equal length")
    plan = NoiseErrPlan(torch.as_tensor(c).cuda().view(1, -1), torch.as_tensor(z).cuda().view(1, -1),
                        n_fft, hop_length, **kw)
    N = np.asarray(N, dtype=np.float32)
    if N.ndim == 1:
        N = N[:, None]
    if N.ndim != 2 or N.shape[0] != plan.B or N.shape[1] not in (1, plan.T):
        raise ValueError(f"N must be ({plan.B}, {plan.T}), ({plan.B}, 1) or ({plan.B},), "
                         f"found {N.shape}")
    Nd = torch.as_tensor(np.ascontiguousarray(N.T)).cuda()
    Nd = Nd.view(1, plan.B) if N.shape[1] == 1 and plan.T != 1 else Nd.view(1, plan.T, plan.B)
    res = plan.score(Nd, [0], per_frame=per_frame)
    t = res[0] if per_frame else res
    out = {"logerr": float(t[0, 0]), "over": float(t[0, 1]), "under": float(t[0, 2])}
    if per_frame:
        out["frame_over"], out["frame_under"] = res[1][0, 0], res[1][0, 1]
    return out


def llr(x, y, fs):
    """Log-likelihood ratio (include/cse_lpc.h) of y against the clean x; lower is better."""
    return _pair_score(LpcPlan, x, y, "llr", "llr", sr=fs)


def cepstrum_distance(x, y, fs):
    """LPC cepstrum distance (include/cse_lpc.h) of y against the clean x; lower is better."""
    return _pair_score(LpcPlan, x, y, "cep", "cep", sr=fs)


def wss(x, y, fs):
    """Weighted spectral slope distance (include/cse_wss.h) of y against the clean
    x; lower is better."""
    return _pair_score(WssPlan, x, y, "wss", sr=fs)


def csii(x, y, fs):
    """(CSII_high, CSII_mid, CSII_low, I3) of y against the clean x
    (include/cse_csii.h); higher is better.  A level without frames gives NaN,
    and so does I3 without mid or low frames."""
    x, y = _pair_signals(x, y, "csii")
    plan = CsiiPlan(torch.as_tensor(x).cuda().view(1, -1), sr=fs)
    yd = torch.as_tensor(y.astype(np.float32)).cuda()
    return tuple(float(v) for v in plan.score(yd, [0], [0], clip=False)[0])


def calculate_csii(clean_reference, test_audio, sr):
    """I3 with calculate_stoi's shape: trim to the common length, None on
    failure (a clip with no mid-level or no low-level frame included)."""
    def fn(x, y, fs):
        v = csii(x, y, fs)[3]
        if math.isnan(v):
            raise ValueError("I3 is undefined (no mid-level or no low-level 30-ms frame)")
        return v
    return _calculate_quality(fn, "CSII", clean_reference, test_audio, sr)


def _coherence(clean_reference, noisy_audio, enhanced_audio, sr):
    """csii_high_*, csii_mid_*, csii_low_* (noisy, enhanced) and i3_noisy,
    i3_enhanced, i3_improvement; {} on failure."""
    try:
        n = min(len(clean_reference), len(noisy_audio), len(enhanced_audio))
        c = np.asarray(clean_reference)[:n]
        v_noisy = csii(c, np.asarray(noisy_audio)[:n], sr)
        v_enh = csii(c, np.asarray(enhanced_audio)[:n], sr)
        out = {}
        for k, name in enumerate(CsiiPlan._WHICH):
            out[f"{name}_noisy"], out[f"{name}_enhanced"] = v_noisy[k], v_enh[k]
        out["i3_improvement"] = v_enh[3] - v_noisy[3]
        return out
    except (NotImplementedError, _lib.CseError):
        raise  # no device / unsupported: not a score failure
    except Exception as e:  # calculate_stoi's catch-all
        print(f"CSII calculation failed: {e}")
        return {}


def ncm(x, y, fs, bif_power=1.0):
    """(ncm, ncm_bif) of y against the clean x (include/cse_ncm.h); higher is
    better.  bif_power: the exponent of ncm_bif's band weights.  A clip of fewer
    than 12 frames (0.12 s) and an all-zero clean signal give NaN."""
    x, y = _pair_signals(x, y, "ncm")
    p = _bif_power(bif_power)  # refused before anything goes to the device
    plan = NcmPlan(torch.as_tensor(x).cuda().view(1, -1), sr=fs, bif_power=p)
    yd = torch.as_tensor(y.astype(np.float32)).cuda()
    return tuple(float(v) for v in plan.score(yd, [0], [0], clip=False)[0])


def calculate_ncm(clean_reference, test_audio, sr):
    """ncm with calculate_stoi's shape: trim to the common length, None on
    failure (a clip of fewer than 12 frames or an all-zero clean signal
    included)."""
    def fn(x, y, fs):
        v = ncm(x, y, fs)[0]
        if math.isnan(v):
            raise ValueError("NCM is undefined (fewer than 12 30-ms frames, or a zero clean signal)")
        return v
    return _calculate_quality(fn, "NCM", clean_reference, test_audio, sr)


def _modulation(clean_reference, noisy_audio, enhanced_audio, sr):
    """ncm_* and ncm_bif_* (noisy, enhanced) and ncm_improvement; {} on failure."""
    try:
        n = min(len(clean_reference), len(noisy_audio), len(enhanced_audio))
        c = np.asarray(clean_reference)[:n]
        v_noisy = ncm(c, np.asarray(noisy_audio)[:n], sr)
        v_enh = ncm(c, np.asarray(enhanced_audio)[:n], sr)
        out = {}
        for k, name in enumerate(NcmPlan._WHICH):
            out[f"{name}_noisy"], out[f"{name}_enhanced"] = v_noisy[k], v_enh[k]
        out["ncm_improvement"] = v_enh[0] - v_noisy[0]
        return out
    except (NotImplementedError, _lib.CseError):
        raise  # no device / unsupported: not a score failure
    except Exception as e:  # calculate_stoi's catch-all
        print(f"NCM calculation failed: {e}")
        return {}


def composite(pesq, llr, wss, segsnr):
    """(CSIG, CBAK, COVL): Hu & Loizou's (2008) composite predictions of the
    signal-distortion, background-intrusiveness and overall-quality ratings, the
    regressions of Loizou's composite.m:

        CSIG = 3.093 - 1.029 LLR + 0.603 PESQ - 0.009 WSS
        CBAK = 1.634 + 0.478 PESQ - 0.007 WSS + 0.063 segSNR
        COVL = 1.594 + 0.805 PESQ - 0.512 LLR - 0.007 WSS

    each clamped to [1, 5].  Plain numpy on the host: the arguments broadcast
    against each other and a NaN in one gives NaN in what depends on it.  pesq
    is the caller's (ITU-T P.862 is not scored here); llr, wss and segsnr are
    this project's variants (include/cse_lpc.h, cse_wss.h, cse_segsnr.h), which
    leave exactly-silent clean frames out, so on clips with exact-zero pauses
    the composites differ from composite.m's."""
    pesq, llr, wss, segsnr = (np.asarray(v, dtype=np.float64) for v in (pesq, llr, wss, segsnr))
    csig = 3.093 - 1.029 * llr + 0.603 * pesq - 0.009 * wss
    cbak = 1.634 + 0.478 * pesq - 0.007 * wss + 0.063 * segsnr
    covl = 1.594 + 0.805 * pesq - 0.512 * llr - 0.007 * wss
    # np.clip keeps NaN
    return tuple(np.clip(v, 1.0, 5.0)[()] for v in (csig, cbak, covl))


def segsnr(x, y, fs):
    """Segmental SNR in dB (include/cse_segsnr.h) of y against the clean x."""
    return _pair_score(SegSnrPlan, x, y, "segsnr", "segsnr", sr=fs)


def fwsegsnr(x, y, fs):
    """Frequency-weighted segmental SNR in dB (include/cse_segsnr.h)."""
    return _pair_score(SegSnrPlan, x, y, "fwsegsnr", "fwsegsnr", sr=fs)


def _calculate_quality(fn, name, clean_reference, test_audio, sr):
    try:
        n = min(len(clean_reference), len(test_audio))
        return fn(np.asarray(clean_reference)[:n], np.asarray(test_audio)[:n], sr)
    except (NotImplementedError, _lib.CseError):
        raise  # no device / unsupported: not a score failure
    except Exception as e:  # calculate_stoi's catch-all
        print(f"{name} calculation failed: {e}")
        return None


def calculate_segsnr(clean_reference, test_audio, sr):
    """segsnr with calculate_stoi's shape: trim to the common length, None on failure."""
    return _calculate_quality(segsnr, "segSNR", clean_reference, test_audio, sr)


def calculate_fwsegsnr(clean_reference, test_audio, sr):
    """fwsegsnr with calculate_stoi's shape: trim to the common length, None on failure."""
    return _calculate_quality(fwsegsnr, "fwSegSNR", clean_reference, test_audio, sr)


def calculate_llr(clean_reference, test_audio, sr):
    """llr with calculate_stoi's shape: trim to the common length, None on failure."""
    return _calculate_quality(llr, "LLR", clean_reference, test_audio, sr)


def calculate_cep(clean_reference, test_audio, sr):
    """cepstrum_distance with calculate_stoi's shape: trim to the common length, None on failure."""
    return _calculate_quality(cepstrum_distance, "CEP", clean_reference, test_audio, sr)


def calculate_wss(clean_reference, test_audio, sr):
    """wss with calculate_stoi's shape: trim to the common length, None on failure."""
    return _calculate_quality(wss, "WSS", clean_reference, test_audio, sr)


def stoi(x, y, fs_sig, extended=False):
    """pystoi ``stoi(x, y, fs_sig, extended=False)`` on the device; with
    extended=True, extended STOI as include/cse_estoi.h defines it."""
    return _pair_score(StoiPlan, x, y, "stoi", sr=fs_sig, extended=extended,
                       nan_message="no 256-sample frame at 10 kHz")  # pystoi: empty frame array


def calculate_stoi(clean_reference, test_audio, sr, extended=False):
    """evaluation_metrics.calculate_stoi (:30-36): trim to the common length,
    None on failure.  extended=True scores extended STOI the same way."""
    try:
        n = min(len(clean_reference), len(test_audio))
        return stoi(np.asarray(clean_reference)[:n], np.asarray(test_audio)[:n], sr,
                    extended=extended)
    except (NotImplementedError, _lib.CseError):
        raise  # no device / unsupported: not a score failure
    except Exception as e:  # the reference's catch-all
        print(f"STOI calculation failed: {e}")
        return None


def calculate_pesq(clean_reference, test_audio, sr):
    """evaluation_metrics.calculate_pesq (:9-27).  The ITU-T P.862 `pesq`
    extension is not available in this image; like the reference when the
    call fails, report and return None."""
    print("PESQ calculation failed: the pesq extension is not available")
    return None


def calculate_snr(clean, processed):
    """evaluation_metrics.calculate_snr (:39-58)."""
    try:
        clean = np.asarray(clean)
        processed = np.asarray(processed)
        m = min(len(clean), len(processed))
        clean, processed = clean[:m], processed[:m]
        noise = clean - processed
        p_signal = np.sum(clean ** 2)
        p_noise = np.sum(noise ** 2)
        if p_noise == 0:
            return float("inf")
        return float(10 * np.log10(p_signal / (p_noise + 1e-10)))
    except Exception as e:
        print(f"SNR calculation failed: {e}")
        return None


def calculate_combined_speech_score(stoi_score, pesq_score):
    """evaluation_metrics.calculate_combined_speech_score (:104-115)."""
    if stoi_score is None:
        stoi_score = 0
    if pesq_score is None:
        pesq_score = 0
    return 0.5 * stoi_score + 0.5 * (max(0, pesq_score) / 4.5)


def _separation(clean_reference, noisy_audio, enhanced_audio):
    """sisdr_enhanced, sisir_enhanced and sisar_enhanced, and sisdr_noisy with
    sisdr_improvement (the noisy input's SI-SAR carries no meaning:
    include/cse_sisdr.h); {} on failure."""
    try:
        n = min(len(clean_reference), len(noisy_audio), len(enhanced_audio))
        c, z = np.asarray(clean_reference)[:n], np.asarray(noisy_audio)[:n]
        sdr, sir, sar = si_sdr(c, np.asarray(enhanced_audio)[:n], noisy=z)
        base = si_sdr(c, z)
        return {"sisdr_noisy": base, "sisdr_enhanced": sdr, "sisdr_improvement": sdr - base,
                "sisir_enhanced": sir, "sisar_enhanced": sar}
    except (NotImplementedError, _lib.CseError):
        raise  # no device / unsupported: not a score failure
    except Exception as e:  # calculate_stoi's catch-all
        print(f"SI-SDR calculation failed: {e}")
        return {}


def evaluate_audio_quality(clean_reference, noisy_audio, enhanced_audio, sr, algorithm_name="",
                           quality=False, distortion=False, separation=False, wss=False,
                           coherence=False, modulation=False):
    """evaluation_metrics.evaluate_audio_quality (:61-101), same keys;
    quality=True adds segsnr_* and fwsegsnr_* (noisy, enhanced, improvement);
    distortion=True adds llr_* and cep_* likewise, their improvement being
    noisy - enhanced (lower is better); separation=True adds sisdr_enhanced,
    sisir_enhanced and sisar_enhanced, and sisdr_noisy with sisdr_improvement;
    wss=True adds wss_noisy, wss_enhanced and wss_improvement (noisy - enhanced);
    coherence=True adds csii_high_*, csii_mid_* and csii_low_* (noisy, enhanced)
    and i3_noisy, i3_enhanced and i3_improvement (include/cse_csii.h; a level
    without frames gives NaN); modulation=True adds ncm_noisy, ncm_enhanced,
    ncm_bif_noisy, ncm_bif_enhanced and ncm_improvement (include/cse_ncm.h, at
    the default exponent)."""
    results = {}
    s_noisy = calculate_stoi(clean_reference, noisy_audio, sr)
    s_enh = calculate_stoi(clean_reference, enhanced_audio, sr)
    if s_noisy is not None and s_enh is not None:
        results["stoi_noisy"] = s_noisy
        results["stoi_enhanced"] = s_enh
        results["stoi_improvement"] = s_enh - s_noisy
    p_noisy = calculate_pesq(clean_reference, noisy_audio, sr)
    p_enh = calculate_pesq(clean_reference, enhanced_audio, sr)
    if p_noisy is not None and p_enh is not None:
        results["pesq_noisy"] = p_noisy
        results["pesq_enhanced"] = p_enh
        results["pesq_improvement"] = p_enh - p_noisy
    snr_val = calculate_snr(clean_reference, enhanced_audio)
    if snr_val is not None:
        results["snr_enhanced"] = snr_val
    for f in requested(quality=quality, distortion=distortion, separation=separation, wss=wss):
        if f.plan_takes_noisy:  # scored against the noisy input's interference
            results.update(_separation(clean_reference, noisy_audio, enhanced_audio))
            continue
        for key in f.names:
            fn = globals()["calculate_" + key]
            v_noisy = fn(clean_reference, noisy_audio, sr)
            v_enh = fn(clean_reference, enhanced_audio, sr)
            if v_noisy is not None and v_enh is not None:
                results[f"{key}_noisy"] = v_noisy
                results[f"{key}_enhanced"] = v_enh
                results[f"{key}_improvement"] = v_enh - v_noisy if f.sign > 0 else v_noisy - v_enh
    if coherence:
        results.update(_coherence(clean_reference, noisy_audio, enhanced_audio, sr))
    if modulation:
        results.update(_modulation(clean_reference, noisy_audio, enhanced_audio, sr))
    if algorithm_name:
        print(f"\n{'=' * 60}\nEvaluation: {algorithm_name}\n{'=' * 60}")
    if "stoi_noisy" in results:
        print(f"STOI: {results['stoi_noisy']:.4f} -> {results['stoi_enhanced']:.4f} "
              f"(+{results['stoi_improvement']:.4f})")
    if "snr_enhanced" in results:
        print(f"SNR (Enhanced): {results['snr_enhanced']:.2f} dB")
    for key, label in (("segsnr", "segSNR"), ("fwsegsnr", "fwSegSNR")):
        if f"{key}_noisy" in results:
            print(f"{label}: {results[key + '_noisy']:.2f} -> {results[key + '_enhanced']:.2f} dB")
    for key, label in (("llr", "LLR"), ("cep", "CEP")):
        if f"{key}_noisy" in results:
            print(f"{label}: {results[key + '_noisy']:.3f} -> {results[key + '_enhanced']:.3f}")
    if "wss_noisy" in results:
        print(f"WSS: {results['wss_noisy']:.2f} -> {results['wss_enhanced']:.2f}")
    if "sisdr_enhanced" in results:
        print(f"SI-SDR: {results['sisdr_noisy']:.2f} -> {results['sisdr_enhanced']:.2f} dB "
              f"(SI-SIR {results['sisir_enhanced']:.2f}, SI-SAR {results['sisar_enhanced']:.2f})")
    if "i3_noisy" in results:
        print(f"I3: {results['i3_noisy']:.4f} -> {results['i3_enhanced']:.4f} (CSII mid "
              f"{results['csii_mid_noisy']:.4f} -> {results['csii_mid_enhanced']:.4f})")
    if "ncm_noisy" in results:
        print(f"NCM: {results['ncm_noisy']:.4f} -> {results['ncm_enhanced']:.4f} (band-importance "
              f"form {results['ncm_bif_noisy']:.4f} -> {results['ncm_bif_enhanced']:.4f})")
    return results
