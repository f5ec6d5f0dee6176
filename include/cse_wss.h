/*
 * cse_wss.h — weighted spectral slope distance (WSS) on the device, next to the
 * segSNR entry points of cse_segsnr.h and the LLR / CEP ones of cse_lpc.h (same
 * conventions: caller-owned device memory, asynchronous on `stream`, CSE_OK or
 * a negative code and a cse_last_error message, no allocation in the library).
 *
 * WSS (Klatt, ICASSP 1982) compares the slopes of the critical-band spectrum
 * between adjacent bands, weighted towards the spectral peaks, so it reacts to
 * formants that are shifted or flattened; lower is better.  It is the third
 * ingredient, with the LLR and PESQ, of Hu & Loizou's composite measures CSIG,
 * CBAK and COVL (IEEE TASLP 16(1), 2008).  The reference scores no WSS, so this
 * header is the specification: Loizou's comp_wss as pysepm's wss restates it,
 * with the one difference stated below.
 *
 * Rates: sr = 16000 and 8000 only (the size functions return -1 otherwise).
 *
 * Inputs: x[n], the clean signal, f64, length len.  y[n], the cell's test
 * signal exactly as cse_segsnr.h defines it: y[n - lag], zero outside
 * [0, len), clipped to [-1, 1] when clip.
 *
 * Constants, frames and window: W, hop, NFFT, H, J, the frames and the strictly
 * positive Hann window w are those of cse_segsnr.h (W = 480 / 240, hop = W / 4,
 * NFFT = 1024 / 512, H = NFFT / 2, J = floor(len / hop) - 4).
 *
 * Silent frames (the difference from Loizou): a frame whose W clean samples are
 * all exactly 0 is silent and left out, as in cse_segsnr.h.  The mask is made
 * once per clean signal from the f64 samples.  Ja = number of frames kept;
 * J < 1 or Ja = 0 gives NaN.
 *
 * Filters: the 25 critical-band filters F[i][k] over the H bins are those of
 * cse_segsnr.h: the same tables, the same floor.
 *
 * Band energies and slopes, per kept frame and for both signals, f = the
 * windowed frame:
 *   S[k] = |FFT_NFFT(f)[k]|^2, k < H (the power, not divided by its sum);
 *   e_i = sum_k F[i][k] S[k];  E_i = 10 log10(max(e_i, 1e-10)), i = 0..24;
 *   slopes s_i = E_{i+1} - E_i, i = 0..23.
 *   (An all-zero test frame has E_i = -100 in every band and a finite value.)
 *
 * Nearest peak P_i, i = 0..23: Loizou's rule as it stands, quirk included, so
 * that values compare with published ones.
 *   If s_i > 0:  n = i; while n < 24 and s_n > 0: n += 1;  P_i = E_{n-1}.
 *     (The rightward search returns the band before the last rising step, one
 *     below the local maximum.)
 *   Otherwise:   n = i; while n >= 0 and s_n <= 0: n -= 1;  P_i = E_{n+1}.
 *
 * Weights, Kmax = 20 and Kloc = 1, per signal:
 *   Wmax_i = Kmax / (Kmax + max_j E_j - E_i),  j = 0..24;
 *   Wloc_i = Kloc / (Kloc + P_i - E_i);
 *   W_i = Wmax_i Wloc_i.
 *   (P_i >= E_i by the rule above, so both denominators are >= their constant.)
 *   Wt_i = (Wx_i + Wy_i) / 2.
 *
 * Frame value: d = sum_i Wt_i (sx_i - sy_i)^2 / sum_i Wt_i over i = 0..23.
 * Cell score: the mean of the n95 smallest of the Ja frame values,
 * n95 = (19 Ja + 10) div 20 in integers as in cse_lpc.h (MATLAB's
 * round(0.95 Ja) without a floating product: Ja = 30 gives 29, Ja = 10 gives 10).
 *
 * Precision: the clean side (cse_wss_prepare) is computed in fp64 and stored as
 * f32: E_x[25], from which the cell kernel takes sx in f32, and Wx[24].  The
 * cell kernel works in fp32 from the windowed frame on (each E_i rounded to f32
 * on its own, so two bands at the floor have slope exactly 0); the frame's two sums
 * over i and the mean over frames accumulate in fp64.  A frame's value is
 * stored as f32 (round to nearest) for the selection of the n95 smallest.
 *
 * cse_wss_workspace_bytes: bytes of the clean-side workspace; -1 when the rate
 *   is not supported or a count is negative.
 * cse_wss_prepare: builds the clean side once per batch of n_sig equal-length
 *   signals (clean: [n_sig][len] f64): per frame the silent mask, E_x[25] and
 *   Wx[24]; Ja and n95 per signal.
 * cse_wss_scratch_bytes: bytes of per-launch scratch: 0 while J <= 1536 (the
 *   cell kernel selects in LDS; `scratch` may then be NULL), else room for one
 *   f32 value per frame and cell; -1 as above.
 * cse_wss_cells: y, y_offset, lag (NULL = 0), sig_of as in cse_stoi_cells.
 *   wss[c] = the score of cell c.  n_cells == 0 launches nothing.  CSE_EINVAL
 *   for NULL required pointers, negative counts, len < 1 or an unsupported sr;
 *   the checks come before any device work.
 */
#ifndef CSE_WSS_H_
#define CSE_WSS_H_

#include "cse.h"

#ifdef __cplusplus
extern "C" {
#endif

int64_t cse_wss_workspace_bytes(int64_t n_sig, int64_t len, int sr);
int cse_wss_prepare(const double* clean, int64_t n_sig, int64_t len, int sr, void* workspace,
                    cse_stream_t stream);
int64_t cse_wss_scratch_bytes(int64_t n_cells, int64_t len, int sr);
int cse_wss_cells(const float* y, const int64_t* y_offset, const int32_t* lag,
                  const int32_t* sig_of, int64_t n_cells, int64_t n_sig, int64_t len, int sr,
                  int clip, const void* workspace, void* scratch, double* wss,
                  cse_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* CSE_WSS_H_ */
