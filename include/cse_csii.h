/*
 * cse_csii.h — the three-level coherence speech intelligibility index (CSII)
 * and I3 on the device, next to the WSS entry points of cse_wss.h (same
 * conventions: caller-owned device memory, asynchronous on `stream`, CSE_OK or
 * a negative code and a cse_last_error message, no allocation in the library;
 * the checks come before any device work).
 *
 * CSII (Kates & Arehart, JASA 117(4), 2005) separates what of the test signal
 * is linearly related to the clean speech from what is not (noise, distortion,
 * musical noise) through the magnitude-squared coherence, on three level ranges
 * of the clean speech, and folds the mid and low ranges into one index, I3.
 * Ma, Hu & Loizou (JASA 125(5), 2009) found it the best predictor of the
 * intelligibility of speech processed by spectral subtraction, Wiener, MMSE
 * and log-MMSE enhancers.  The reference scores no CSII, so this header is the
 * specification.  Higher is better; every value lies in [0, 1].
 *
 * Rates: sr = 16000 and 8000 only (the size functions return -1 otherwise).
 *
 * Inputs: x[n], the clean signal, f64, length len.  y[n], the cell's test
 * signal exactly as cse_segsnr.h defines it: y[n - lag], zero outside
 * [0, len), clipped to [-1, 1] when clip.
 *
 * Constants, frames, window and filters: W, hop, NFFT, H, J, the frames, the
 * strictly positive Hann window w and the 25 critical-band filters F[i][k] are
 * those of cse_segsnr.h (the same tables, the same floor).  J < 1 gives NaN
 * for all four outputs.
 *
 * Level of a frame, in fp64 on the clean side, unwindowed:
 *   s_j = sum of x[n]^2 over the frame's W samples;
 *   S   = sum of x[n]^2 over n < len;
 *   a_j = s_j len,  b = S W  (the frame's mean power against the clip's);
 *   high: a_j >= b;  mid: 0.1 b <= a_j < b;  low: 0.001 b <= a_j < 0.1 b.
 *   A frame below that is in no level, and so is every frame when S = 0:
 *   exact-zero pauses drop out without a separate mask.
 *   n_L = number of frames of level L.
 *
 * Spectra: X_j[k] and Y_j[k] = FFT_NFFT of the windowed frame, k < H.
 *
 * Per level L and bin k, sums over the frames j of L:
 *   Pxy = sum X_j conj(Y_j),  Pxx = sum |X_j|^2,  Pyy = sum |Y_j|^2,
 *   MSC_L[k] = min(|Pxy|^2 / (Pxx Pyy), 1), and 0 where Pxx Pyy = 0.
 *
 * Per frame j of L and band i:
 *   num = sum_k F[i][k] MSC_L[k] |Y_j[k]|^2,
 *   den = sum_k F[i][k] (1 - MSC_L[k]) |Y_j[k]|^2,
 *   q = num / max(den, 2^-100),
 *   SDR = 10 log10(max(q, 2^-100)) clamped to [-15, 15],  T = (SDR + 15) / 30.
 *   Frame value c_j = sum_i A_i T_ij / sum_i A_i with the articulation-index
 *   weights of the 25 bands (the ones comp_fwseg lists):
 *   A = 0.003, 0.003, 0.003, 0.007, 0.010, 0.016, 0.016, 0.017, 0.017, 0.022,
 *       0.027, 0.028, 0.030, 0.032, 0.034, 0.035, 0.037, 0.036, 0.036, 0.033,
 *       0.030, 0.029, 0.027, 0.026, 0.026.
 *
 * Scores:
 *   CSII_L = the mean of c_j over the frames of L; NaN when n_L = 0.
 *   I3 = 1 / (1 + exp(-(-3.47 + 1.84 CSII_low + 9.99 CSII_mid))), Kates &
 *   Arehart's fit; NaN when CSII_low or CSII_mid is NaN.
 *
 * Consequences:
 *   Scaling y leaves every value unchanged.
 *   y = x gives 1, 1, 1 and I3 = 0.99977.
 *   An all-zero y gives 0, 0, 0 and I3 = 1 / (1 + e^3.47).
 *   A level with one frame has MSC = 1 and scores 1: the known small-sample
 *   bias of the coherence estimate, so short clips score high.
 *   A clip with no mid or no low frame has no I3 (NaN).
 *
 * Precision: the clean side (cse_csii_prepare) is computed in fp64: the
 * levels, and Pxx from the fp64 spectra; X and Pxx are stored as f32.  The cell
 * kernel works in fp32 from the windowed frame on: the transform, Pxy, Pyy, the
 * band sums and the logarithms.  The quotient of MSC_L[k] and 1 - MSC_L[k] are
 * formed in fp64 from the f32 sums (the product Pxx Pyy cannot underflow there)
 * and stored as f32.  The sums over the bands of a frame, the mean over frames
 * and I3 are fp64.  Every sum has a fixed order: the same call twice gives the
 * same bits.  No atomics.
 *
 * cse_csii_workspace_bytes: bytes of the clean-side workspace (per signal the
 *   level counts, the frame indices ordered by level, Pxx[3][H] and the spectra
 *   X[J][H] as f32 complex: 5.4 MB for 10 s at 16 kHz); -1 when the rate is not
 *   supported or a count is negative.
 * cse_csii_prepare: builds the clean side once per batch of n_sig equal-length
 *   signals (clean: [n_sig][len] f64).
 * cse_csii_scratch_bytes: bytes of per-launch scratch (0: the cell kernel keeps
 *   everything on chip; `scratch` may be NULL); -1 as above.
 * cse_csii_cells: y, y_offset, lag (NULL = 0), sig_of as in cse_stoi_cells.
 *   csii[4 c + 0..3] = CSII_high, CSII_mid, CSII_low and I3 of cell c.
 *   n_cells == 0 launches nothing.  CSE_EINVAL for NULL required pointers,
 *   negative counts, len < 1 or an unsupported sr.
 */
#ifndef CSE_CSII_H_
#define CSE_CSII_H_

#include "cse.h"

#ifdef __cplusplus
extern "C" {
#endif

int64_t cse_csii_workspace_bytes(int64_t n_sig, int64_t len, int sr);
int cse_csii_prepare(const double* clean, int64_t n_sig, int64_t len, int sr, void* workspace,
                     cse_stream_t stream);
int64_t cse_csii_scratch_bytes(int64_t n_cells, int64_t len, int sr);
int cse_csii_cells(const float* y, const int64_t* y_offset, const int32_t* lag,
                   const int32_t* sig_of, int64_t n_cells, int64_t n_sig, int64_t len, int sr,
                   int clip, const void* workspace, void* scratch, double* csii,
                   cse_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* CSE_CSII_H_ */
