/*
 * cse_mcra.h — minima-controlled recursive averaging (MCRA) noise-PSD tracking
 * on the device, next to the estimators of cse.h (same conventions:
 * caller-owned device memory, asynchronous on `stream`, CSE_OK or a negative
 * code and a cse_last_error message).
 *
 * Cohen & Berdugo, "Noise Estimation by Minima Controlled Recursive Averaging
 * for Robust Speech Enhancement", IEEE Signal Processing Letters 9(1), 2002:
 * a causal per-bin tracker steered by a speech-presence probability, which
 * needs no clean signal.  The reference has no such estimator
 * (noise_estimation.py knows percentile, min_tracking and true_noise), so
 * this header is the specification.
 *
 * Input P[s][t][b] = |Y|^2 in fp64, as cse_stft writes it: T frames,
 * B = n_fft/2 + 1 bins.  Every bin is independent given its two neighbours in
 * P.  Each line is one individually rounded fp64 operation, in this order
 * (no FMA contraction; 1 - alpha_* are computed once in fp64):
 *
 *   m = (b == 0 ? 1 : b-1),  q = (b == B-1 ? B-2 : b+1)
 *                            mirror: the real signal's full spectrum
 *   Sf(t)  = (0.25 P[t][m] + 0.5 P[t][b]) + 0.25 P[t][q]
 *   t = 0:   S = Sf(0); Smin = Stmp = S; p = 0; lam = P[0][b]; N[0] = lam
 *   t >= 1:  S = alpha_s S + (1 - alpha_s) Sf(t)       two products, then the sum
 *            if t % L == 0: Smin = min(Stmp, S); Stmp = S
 *            else:          Smin = min(Smin, S); Stmp = min(Stmp, S)
 *   every t: I  = (S > delta Smin) ? 1 : 0
 *            p  = alpha_p p + (1 - alpha_p) I
 *            ad = alpha_d + (1 - alpha_d) p
 *            lam = ad lam + (1 - ad) P[t][b]
 *            if t + 1 < T: N[t+1] = lam                predictive: N[t] never contains P[t]
 *   output:  N[s][t][b] = (float) max(N[t], eps)       f32 [n_sig][T][B]
 *
 * L = window_frames.  The threshold I is a discontinuity, so the contract is
 * bit equality with a restatement in the same order, not a tolerance.
 *
 * cse_mcra_default_params: the paper's values for n_fft 512 / hop 128 at
 *   16 kHz: alpha_s 0.8, alpha_d 0.95, alpha_p 0.2, delta 5, window_frames 125.
 * cse_noise_mcra: the estimate above for n_sig signals.  CSE_EINVAL (-1) when
 *   P, N or prm is NULL; n_sig < 0, T < 1 or B outside [33, 2049]; alpha_s,
 *   alpha_d or alpha_p outside [0, 1); delta not greater than 0 (NaN
 *   included); window_frames < 2.  n_sig == 0 launches nothing and returns
 *   CSE_OK.  No workspace.
 */
#ifndef CSE_MCRA_H_
#define CSE_MCRA_H_

#include "cse.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CSE_NOISE_MCRA 3 /* the method's number next to cse.h's CSE_NOISE_* */

typedef struct {
    double alpha_s;        /* smoothing of the local energy S */
    double alpha_d;        /* smoothing of the noise estimate in speech absence */
    double alpha_p;        /* smoothing of the speech-presence probability */
    double delta;          /* speech present where S > delta Smin */
    int32_t window_frames; /* L: length of the minimum search window */
    int32_t reserved;
} cse_mcra_params_t; /* 40 bytes */

void cse_mcra_default_params(cse_mcra_params_t* prm);
int cse_noise_mcra(const double* P, int64_t n_sig, int T, int B, const cse_mcra_params_t* prm,
                   double eps, float* N, cse_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* CSE_MCRA_H_ */
