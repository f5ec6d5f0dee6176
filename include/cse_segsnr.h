/*
 * cse_segsnr.h — segmental SNR (segSNR) and frequency-weighted segmental SNR
 * (fwSegSNR) on the device, next to the STOI entry points of cse.h (same
 * conventions: caller-owned device memory, asynchronous on `stream`, CSE_OK or
 * a negative code and a cse_last_error message, no allocation in the library).
 *
 * fwSegSNR (Tribolet, Noll, McDermott & Crochiere, ICASSP 1978) is, among the
 * objective measures that are not PESQ, the one Hu & Loizou (IEEE TASLP 16(1),
 * 2008) found to correlate best with subjective quality for spectral
 * subtraction, Wiener, MMSE and log-MMSE enhancers; segSNR is its plain
 * sibling on the same frames.  The reference scores neither, so this header
 * is the specification: Loizou's comp_snr / comp_fwseg as pysepm's SNRseg /
 * fwSNRseg restate them, with the two differences stated below.
 *
 * Rates: sr = 16000 and 8000 only (the size functions return -1 otherwise).
 *
 * Inputs: x[n], the clean signal, f64, length len.  y[n], the cell's test
 * signal exactly as cse_stoi_cells defines it: y[n - lag], zero outside
 * [0, len), clipped to [-1, 1] when clip.
 *
 * Constants: W = round(0.03 sr) (480, 240); hop = W / 4; NFFT = 2^ceil(log2(2W))
 * (1024, 512); H = NFFT / 2; EPS = 2^-52.  J = floor(len / hop) - 4 frames,
 * frame j covering samples [j hop, j hop + W); J < 1 gives NaN for both scores.
 * Window w[i] = 0.5 (1 - cos(2 pi (i + 1) / (W + 1))), i < W (MATLAB hanning,
 * strictly positive).
 *
 * Silent frames (difference 1 from Loizou): a frame whose W clean samples are
 * all exactly 0 is silent and left out of both means.  The mask is made once
 * per clean signal from the f64 samples.  Ja = number of non-silent frames;
 * Ja = 0 gives NaN for both scores.  (Clean against clean then scores 35 on a
 * clip with pauses.)
 *
 * segSNR, per non-silent frame, with xf = x w and yf = y w:
 *   s = sum xf^2,  e = sum (xf - yf)^2,
 *   v = 10 log10(s / (e + EPS) + EPS) clamped to [-10, 35];
 *   the score is the mean of v over the Ja frames.
 *
 * fwSegSNR, per non-silent frame:
 *   X[k] = |FFT_NFFT(xf)[k]|, Y[k] likewise, k < H, each divided by (its sum
 *   over k < H) + EPS (difference 2 from Loizou: an all-zero test frame gives
 *   zeros, not NaN).
 *   25 critical-band filters over the H bins, with cent_i and band_i in Hz:
 *     f0_i = floor(cent_i / (sr/2) H),  bw_i = band_i / (sr/2) H,
 *     F[i][k] = exp(-11 ((k - f0_i) / bw_i)^2 + ln(band_0) - ln(band_i)),
 *     entries not above exp(-30 / (2 * 2.303)) set to 0.
 *   cent = 50, 120, 190, 260, 330, 400, 470, 540, 617.372, 703.378, 798.717,
 *     904.128, 1020.38, 1148.30, 1288.72, 1442.54, 1610.70, 1794.16, 1993.93,
 *     2211.08, 2446.71, 2701.97, 2978.04, 3276.17, 3597.63
 *   band = 70 (seven times), 77.3724, 86.0056, 95.3398, 105.411, 116.256,
 *     127.914, 140.423, 153.823, 168.154, 183.457, 199.776, 217.153, 235.631,
 *     255.255, 276.072, 298.126, 321.465, 346.136
 *   (comp_fwseg's tables, used unchanged at both rates as pysepm does.)
 *   ce = F X, pe = F Y, Wt = ce^0.2, err = max((ce - pe)^2, EPS),
 *   snr_i = 10 log10(ce_i^2 / err_i); a band with ce_i = 0 contributes 0 to
 *   the numerator.  Frame value: sum Wt snr / (sum Wt + EPS) clamped to
 *   [-10, 35]; the score is the mean over the Ja frames.
 *
 * Precision: the clean side (cse_segsnr_prepare) is computed in fp64 and
 * stored as f32 (s as f64).  The cell kernel works in fp32 from the windowed
 * frame on; frame sums and the mean over frames accumulate in fp64.
 *
 * cse_segsnr_workspace_bytes: bytes of the clean-side workspace; -1 when the
 *   rate is not supported or a count is negative.
 * cse_segsnr_prepare: builds the clean side once per batch of n_sig equal-
 *   length signals (clean: [n_sig][len] f64): the filter table, the f32 clean
 *   samples, and per frame the silent mask, s, ce[25], Wt[25] and sum Wt; Ja
 *   per signal.
 * cse_segsnr_scratch_bytes: bytes of per-launch scratch (0: the cell kernel
 *   keeps everything on chip; `scratch` may then be NULL); -1 as above.
 * cse_segsnr_cells: y, y_offset, lag (NULL = 0), sig_of as in cse_stoi_cells.
 *   segsnr[c] / fwsegsnr[c] = the scores of cell c; either pointer may be NULL
 *   (a NULL fwsegsnr skips the transforms), not both.  n_cells == 0 launches
 *   nothing.  CSE_EINVAL for NULL required pointers, negative counts, len < 1
 *   or an unsupported sr.
 */
#ifndef CSE_SEGSNR_H_
#define CSE_SEGSNR_H_

#include "cse.h"

#ifdef __cplusplus
extern "C" {
#endif

int64_t cse_segsnr_workspace_bytes(int64_t n_sig, int64_t len, int sr);
int cse_segsnr_prepare(const double* clean, int64_t n_sig, int64_t len, int sr, void* workspace,
                       cse_stream_t stream);
int64_t cse_segsnr_scratch_bytes(int64_t n_cells, int64_t len, int sr);
int cse_segsnr_cells(const float* y, const int64_t* y_offset, const int32_t* lag,
                     const int32_t* sig_of, int64_t n_cells, int64_t n_sig, int64_t len, int sr,
                     int clip, const void* workspace, void* scratch, double* segsnr,
                     double* fwsegsnr, cse_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* CSE_SEGSNR_H_ */
