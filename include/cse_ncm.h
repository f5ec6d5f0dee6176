/*
 * cse_ncm.h — the normalized covariance measure (NCM) and its signal-dependent
 * band-importance form on the device, next to the CSII entry points of
 * cse_csii.h (same conventions: caller-owned device memory, asynchronous on
 * `stream`, CSE_OK or a negative code and a cse_last_error message, no
 * allocation in the library; the checks come before any device work).
 *
 * NCM is the measure of the speech-transmission-index family: it compares the
 * slow temporal envelopes (modulations up to about 16 Hz) of the clean and the
 * test signal in each critical band over the whole clip, through the squared
 * correlation of the two envelopes.  Ma, Hu & Loizou (JASA 125(5), 2009) found
 * it, with CSII, the best predictor of the intelligibility of speech processed
 * by spectral subtraction, Wiener, MMSE and log-MMSE enhancers, and proposed
 * weighting the bands by the clean band-envelope energy raised to a power in
 * place of fixed articulation-index weights.  The reference scores no NCM, so
 * this header is the specification.  It is this project's variant: the frames,
 * transform and Gaussian critical-band filters of cse_segsnr.h stand in for
 * NCM's Butterworth bank and Hilbert envelopes.  Higher is better; both values
 * lie in [0, 1].
 *
 * Rates: sr = 16000 and 8000 only (the size functions return -1 otherwise).
 *
 * Inputs: x[n], the clean signal, f64, length len.  y[n], the cell's test
 * signal exactly as cse_segsnr.h defines it: y[n - lag], zero outside
 * [0, len), clipped to [-1, 1] when clip.
 *
 * Frames and band envelopes: W, hop, NFFT, H, J = floor(len / hop) - 4, the
 * frames, the strictly positive Hann window w and the 25 critical-band filters
 * F[i][k] are those of cse_segsnr.h.  All J frames are used: there is no
 * silent-frame mask, pauses are part of the modulation.  Per frame j and band i
 *   e_j[i] = sqrt(sum_k F[i][k] |S_j[k]|^2),  S_j = FFT_NFFT of the windowed
 *   frame, k < H.
 * The frame rate is sr / hop = 133.3 Hz at both rates.
 *
 * Envelope samples (low-pass and decimation by 4, to 33.3 Hz):
 *   g[d] = 0.5 (1 - cos(2 pi (d + 1) / 9)), d < 8;  M = floor((J - 8) / 4) + 1;
 *   E_m[i] = sum_{d<8} g[d] e_{4m+d}[i], m < M, the taps added in increasing d.
 *   J < 12 (M < 2) gives NaN for both outputs.
 *   Ex comes from the clean signal and Ey from the test signal.
 *
 * Per band i, sums over m in increasing order:
 *   mu = (sum Ex_m) / M,  dx_m = Ex_m - mu,  vx = sum dx_m^2,  sxx = sum Ex_m^2,
 *   cxy = sum dx_m Ey_m  (no mean of Ey is needed, since sum dx = 0),
 *   sy = sum Ey_m,  syy = sum Ey_m^2,  vy = max(syy - sy^2 / M, 0),
 *   r2 = min(cxy^2 / (vx vy), 1) when vx > 2^-40 sxx and vy > 2^-40 syy,
 *   otherwise r2 = 0: an envelope that moves by less than f32 rounding carries
 *   no modulation.  The same rule covers an all-zero y and a constant band.
 *   SNR = 10 log10(max(r2, 2^-100) / max(1 - r2, 2^-100)) clamped to [-15, 15],
 *   TI_i = (SNR + 15) / 30.
 *
 * Scores:
 *   ncm     = sum_i A_i TI_i / sum_i A_i with the 25 articulation-index weights
 *             A_i listed in cse_csii.h;
 *   ncm_bif = sum_i Wb_i TI_i / sum_i Wb_i with Wb_i = sxx_i^p, the
 *             signal-dependent band-importance form: the clean band-envelope
 *             energy raised to a power.  p (bif_power) is the caller's, a finite
 *             double >= 0; p = 0 gives the plain mean of TI (0^0 = 1).  The
 *             default of the Python layer, p = 1, is this project's choice.
 *   Both are NaN when sum_i sxx_i = 0 (an all-zero clean signal).
 *
 * Consequences:
 *   Scaling y leaves both values unchanged.
 *   y = x gives 1 and 1.
 *   An all-zero y gives 0 and 0.
 *   M = 2 gives |r| = 1 in every band that moves, so very short clips score
 *   high: the small-sample bias cse_csii.h also documents.
 *
 * Precision: the clean side (cse_ncm_prepare) is fp64 throughout.  The cell
 * kernel works in fp32 from the windowed frame through e_j[i]: the transform,
 * the powers, the band sums and the square root.  E_m and the running sums are
 * fp64, and so are r2, the logarithm, the weights sxx^p and both weighted sums.
 * Every sum has a fixed order: the same call twice gives the same bits.  No
 * atomics.
 *
 * cse_ncm_workspace_bytes: bytes of the clean-side workspace (per signal the
 *   band envelopes e[J][25], dx[M][25], vx[25] and sxx[25] as f64 and the
 *   dead-band flags: 0.34 MB for 10 s at 16 kHz); -1 when the rate is not
 *   supported or a count is negative.
 * cse_ncm_prepare: builds the clean side once per batch of n_sig equal-length
 *   signals (clean: [n_sig][len] f64).  It does not depend on bif_power.
 * cse_ncm_scratch_bytes: bytes of per-launch scratch (0: the cell kernel keeps
 *   everything on chip; `scratch` may be NULL); -1 as above.
 * cse_ncm_cells: y, y_offset, lag (NULL = 0), sig_of as in cse_stoi_cells.
 *   ncm[2 c + 0..1] = ncm and ncm_bif of cell c.  n_cells == 0 launches
 *   nothing.  CSE_EINVAL for NULL required pointers, negative counts, len < 1,
 *   an unsupported sr, or a negative or non-finite bif_power.
 */
#ifndef CSE_NCM_H_
#define CSE_NCM_H_

#include "cse.h"

#ifdef __cplusplus
extern "C" {
#endif

int64_t cse_ncm_workspace_bytes(int64_t n_sig, int64_t len, int sr);
int cse_ncm_prepare(const double* clean, int64_t n_sig, int64_t len, int sr, void* workspace,
                    cse_stream_t stream);
int64_t cse_ncm_scratch_bytes(int64_t n_cells, int64_t len, int sr);
int cse_ncm_cells(const float* y, const int64_t* y_offset, const int32_t* lag,
                  const int32_t* sig_of, int64_t n_cells, int64_t n_sig, int64_t len, int sr,
                  int clip, const void* workspace, void* scratch, double bif_power, double* ncm,
                  cse_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* CSE_NCM_H_ */
