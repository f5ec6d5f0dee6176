/*
 * cse_lpc.h — log-likelihood ratio (LLR) and LPC cepstrum distance (CEP) on the
 * device, next to the segSNR entry points of cse_segsnr.h (same conventions:
 * caller-owned device memory, asynchronous on `stream`, CSE_OK or a negative
 * code and a cse_last_error message, no allocation in the library).
 *
 * Both compare the LPC spectral envelopes of the clean and the test signal
 * frame by frame; lower is better.  In Hu & Loizou (IEEE TASLP 16(1), 2008) the
 * LLR ties with fwSegSNR as the best non-PESQ predictor of overall quality for
 * spectral subtraction, Wiener, MMSE and log-MMSE enhancers and is the best
 * predictor of signal distortion; the cepstrum distance comes next.  The
 * reference scores neither, so this header is the specification: Loizou's
 * comp_llr / comp_cep, with the three differences stated below.
 *
 * Rates: sr = 16000 and 8000 only (the size functions return -1 otherwise).
 *
 * Inputs: x[n], the clean signal, f64, length len.  y[n], the cell's test
 * signal exactly as cse_stoi_cells defines it: y[n - lag], zero outside
 * [0, len), clipped to [-1, 1] when clip.
 *
 * Constants: W = round(0.03 sr) (480, 240); hop = W / 4; J = floor(len / hop) - 4
 * frames, frame j covering samples [j hop, j hop + W).  Window
 * w[i] = 0.5 (1 - cos(2 pi (i + 1) / (W + 1))), i < W.  Order P = 16 at 16 kHz,
 * 10 at 8 kHz.
 *
 * Silent frames (difference 1 from Loizou): a frame whose W clean samples are
 * all exactly 0 is silent and left out.  The mask is made once per clean signal
 * from the f64 samples.  Ja = number of frames kept; J < 1 or Ja = 0 gives NaN
 * for both scores.
 *
 * Per kept frame, with xf = x w and yf = y w, for both signals:
 *   autocorrelation  R[k] = sum_{i < W - k} f[i] f[i + k],  k = 0..P;
 *   Levinson-Durbin on R gives the monic predictor A[0..P], A[0] = 1:
 *     E_0 = R[0]; at step i = 1..P
 *       k_i = -(R[i] + sum_{j=1}^{i-1} A[j] R[i - j]) / E_{i-1},
 *       A'[j] = A[j] + k_i A[i - j] for j < i,  A'[i] = k_i,
 *       E_i = (1 - k_i^2) E_{i-1}.
 *     If at step i `E_{i-1} > 0` is false or `|k_i| < 1` is false the recursion
 *     stops and the coefficients of order >= i are 0 (difference 2: Loizou's
 *     lpcoeff has no guard and returns NaN for an all-zero test frame).
 *   LLR:  llr_j = log((A_y T(R_x) A_y^T) / (A_x T(R_x) A_x^T)), T(R_x) the
 *     Toeplitz matrix of the clean autocorrelation, clamped to [0, 2]; a ratio
 *     that is not finite or not > 0 gives 2.  (Difference 3 from the plain
 *     comp_llr: the clamp at 2 is the one Hu & Loizou apply before averaging.)
 *     The quadratic form is sum_k m_k R_x[k] rho[k], rho[k] = sum_j A[j] A[j + k],
 *     m_0 = 1, m_k = 2 for k > 0.
 *   Cepstrum of a predictor: c_1 = -A[1],
 *     c_n = -(A[n] + (1 / n) sum_{k=1}^{n-1} k c_k A[n - k]),  n = 2..P;
 *     cep_j = min(10, (10 / ln 10) sqrt(2 sum_{n=1}^{P} (c_x[n] - c_y[n])^2));
 *     a value that is not finite gives 10.
 *
 * Per cell: each score is the mean of the n95 smallest of its Ja frame values,
 * n95 = (19 Ja + 10) div 20 in integers (MATLAB's round(0.95 Ja) without a
 * floating product: half rounds up, Ja = 30 gives 29, Ja = 10 gives 10).
 *
 * Precision: fp64 from the windowed sample on, on both sides: the window, the
 * autocorrelations, both recursions, the quadratic forms, the logarithm and
 * the square root.  (An all-f32 evaluation returns NaN on ten exact harmonics,
 * whose prediction error is 1e-7 of R[0].)  A frame's two values are then stored
 * as f32 (round to nearest) for the selection of the n95 smallest, and their
 * mean accumulates in fp64.
 *
 * cse_lpc_workspace_bytes: bytes of the clean-side workspace; -1 when the rate
 *   is not supported or a count is negative.
 * cse_lpc_prepare: builds the clean side once per batch of n_sig equal-length
 *   signals (clean: [n_sig][len] f64): per frame the silent mask, R_x[0..P],
 *   the denominator A_x T(R_x) A_x^T and c_x[1..P] (f64); Ja and n95 per
 *   signal.
 * cse_lpc_scratch_bytes: bytes of per-launch scratch: 0 while J <= 1536 (the
 *   cell kernel selects in LDS; `scratch` may then be NULL), else room for two
 *   f32 values per frame and cell; -1 as above.
 * cse_lpc_cells: y, y_offset, lag (NULL = 0), sig_of as in cse_stoi_cells.
 *   llr[c] / cep[c] = the scores of cell c; either pointer may be NULL (a NULL
 *   cep skips the cepstrum recursion), not both.  n_cells == 0 launches
 *   nothing.  CSE_EINVAL for NULL required pointers, negative counts, len < 1
 *   or an unsupported sr; the checks come before any device work.
 */
#ifndef CSE_LPC_H_
#define CSE_LPC_H_

#include "cse.h"

#ifdef __cplusplus
extern "C" {
#endif

int64_t cse_lpc_workspace_bytes(int64_t n_sig, int64_t len, int sr);
int cse_lpc_prepare(const double* clean, int64_t n_sig, int64_t len, int sr, void* workspace,
                    cse_stream_t stream);
int64_t cse_lpc_scratch_bytes(int64_t n_cells, int64_t len, int sr);
int cse_lpc_cells(const float* y, const int64_t* y_offset, const int32_t* lag,
                  const int32_t* sig_of, int64_t n_cells, int64_t n_sig, int64_t len, int sr,
                  int clip, const void* workspace, void* scratch, double* llr, double* cep,
                  cse_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* CSE_LPC_H_ */
