/*
 * cse_estoi.h — extended STOI (ESTOI) on the device, next to the STOI entry
 * points of cse.h (same conventions: caller-owned device memory, asynchronous
 * on `stream`, CSE_OK or a negative code and a cse_last_error message).
 *
 * Jensen & Taal, "An Algorithm for Predicting the Intelligibility of Speech
 * Masked by Modulated Noise Maskers", IEEE/ACM TASLP 2016: the score made for
 * fluctuating maskers (music, babble).  pystoi 0.4.1 computes it as
 * stoi(x, y, fs_sig, extended=True); the reference calls pystoi with
 * extended=False only (evaluation_metrics.py:30-36), so no reference output
 * holds an ESTOI value and the score is defined here, as a restatement of
 * pystoi's extended branch.
 *
 * Everything up to the 15 one-third-octave band envelopes is cse_stoi_*'s
 * (resampling to 10 kHz, silent-frame removal, 512-point STFT, bands), and so
 * are both special cases, which pystoi takes before it looks at `extended`:
 * fewer than 30 STFT frames after the silent-frame removal -> 1e-5; no
 * 256-sample frame at 10 kHz -> NaN (calculate_stoi's None).  Then, with
 * X[j] = x_tob[:, j:j+30] and Y[j] likewise, both (J, 15, 30):
 *
 *   rcn(A): A = A - mean(A, axis=2);  A = A / (norm(A, axis=2) + EPS)
 *             (each band row over its 30 frames)
 *           A = A - mean(A, axis=1);  A = A / (norm(A, axis=1) + EPS)
 *             (each frame column over its 15 bands)
 *   ESTOI = sum(rcn(X) * rcn(Y)) / (30 J),      EPS = 2^-52
 *
 * No clipping, no energy matching.  One stated difference from pystoi: pystoi
 * adds EPS * standard_normal jitter before each of the two normalisations and
 * divides by the bare norm; here there is no jitter and the divisor is
 * norm + EPS, the guard of the plain-STOI branch.  A zero-norm row or column
 * then becomes zeros, not random numbers (an all-zero test signal scores
 * exactly 0); every other input agrees with the jittered form to about 1e-11.
 *
 * cse_estoi_workspace_bytes: bytes of the extended workspace, the workspace of
 *   cse_stoi_workspace_bytes_sr followed by the clean side's column statistics
 *   (16 bytes per segment and frame); -1 when the rate is not supported.
 * cse_estoi_prepare: cse_stoi_prepare plus those statistics.  The workspace it
 *   fills also serves cse_stoi_cells and cse_stoi_cells_sr.
 * cse_estoi_cells: like cse_stoi_cells_sr (same test-signal definition, lag,
 *   clip, scratch of cse_stoi_scratch_bytes_sr, n_cells < 65536 per call at
 *   rates other than 16 kHz), on a workspace of cse_estoi_prepare at the same
 *   n_sig, len and sr; estoi[c] = the ESTOI value of cell c.
 */
#ifndef CSE_ESTOI_H_
#define CSE_ESTOI_H_

#include "cse.h"

#ifdef __cplusplus
extern "C" {
#endif

int64_t cse_estoi_workspace_bytes(int64_t n_sig, int64_t len, int sr); /* -1: rate unsupported */
int cse_estoi_prepare(const double* clean, int64_t n_sig, int64_t len, int sr, void* workspace,
                      cse_stream_t stream);
int cse_estoi_cells(const float* y, const int64_t* y_offset, const int32_t* lag,
                    const int32_t* sig_of, int64_t n_cells, int64_t n_sig, int64_t len, int sr,
                    int clip, const void* workspace, void* scratch, double* estoi,
                    cse_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* CSE_ESTOI_H_ */
