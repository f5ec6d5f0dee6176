/*
 * cse_spp.h — SPP-based MMSE noise-PSD tracking on the device, next to the
 * estimators of cse.h and cse_mcra.h (same conventions: caller-owned device
 * memory, asynchronous on `stream`, CSE_OK or a negative code and a
 * cse_last_error message).
 *
 * Gerkmann & Hendriks, "Unbiased MMSE-Based Noise Power Estimation With Low
 * Complexity and Low Tracking Delay", IEEE Transactions on Audio, Speech, and
 * Language Processing 20(4), 2012: a causal per-bin tracker driven by one soft
 * speech-presence probability (SPP) under a fixed a-priori SNR.  No minimum
 * search, no window, no bias compensation; it needs no clean signal.  The
 * reference has no such estimator (noise_estimation.py knows percentile,
 * min_tracking and true_noise), so this header is the specification.
 *
 * Input P[s][t][b] = |Y|^2 in fp64, as cse_stft writes it: T frames,
 * B = n_fft/2 + 1 bins.  Every bin is independent.  Each line is one
 * individually rounded fp64 operation, in this order (no FMA contraction;
 * exp is the math library's fp64 exp; 1 - alpha_* are computed once in fp64):
 *
 *   host, once:  prior = prior_h1 / (1 - prior_h1)
 *                xi    = pow(10, xi_opt_db / 10)
 *                c0    = log(1 / (1 + xi));   c1 = xi / (1 + xi)
 *                K     = min(init_frames, T)
 *   init:        lam = (((P[0][b] + P[1][b]) + ...) + P[K-1][b]) / K
 *                                           sequential sum, then one division
 *                pm  = prior_h1
 *   every t in [0, T):
 *                s   = P[t][b] / max(lam, DBL_MIN)
 *                a   = min(c0 + c1 * s, 200)      product, then sum, then min
 *                g   = prior * exp(a)
 *                ph  = g / (1 + g)
 *                pm  = alpha_ph * pm + (1 - alpha_ph) * ph
 *                                           two products, then the sum
 *                if pm > ph_max: ph = min(ph, ph_max)
 *                                           the paper's guard against stagnation
 *                est = ph * lam + (1 - ph) * P[t][b]
 *                lam = alpha_pow * lam + (1 - alpha_pow) * est
 *                N[t] = lam                 the paper's form: N[t] contains P[t]
 *   output:      N[s][t][b] = (float) max(N[t], eps)       f32 [n_sig][T][B]
 *
 * ph = g / (1 + g) is the paper's P(H1 | y) = 1 / (1 + (P(H0)/P(H1)) (1 + xi)
 * exp(-s xi / (1 + xi))); est is its E(|N|^2 | y).  Zero power gives exactly
 * eps (est = 0).  What a non-finite P yields is not part of the contract.
 *
 * The contract is a tolerance, not bit equality: the only discontinuity is the
 * guard, and exp is the only operation whose last bit may differ between two
 * math libraries.  A device value equals that of a restatement in the same
 * order, or its f32 neighbour: |N_dev - N_ref| <= 2^-23 N_ref, on inputs where
 * the restatement's min |pm - ph_max| is at least 1e-9.
 *
 * cse_spp_default_params: the paper's values: prior_h1 0.5, xi_opt_db 15,
 *   alpha_pow 0.8, alpha_ph 0.9, ph_max 0.99, init_frames 5.
 * cse_noise_spp: the estimate above for n_sig signals.  CSE_EINVAL (-1) when
 *   P, N or prm is NULL; n_sig < 0, T < 1 or B outside [33, 2049]; prior_h1 or
 *   ph_max outside (0, 1); alpha_pow or alpha_ph outside [0, 1); xi_opt_db not
 *   finite (NaN counts as outside everywhere); init_frames < 1.  n_sig == 0
 *   launches nothing and returns CSE_OK.  No workspace.
 */
#ifndef CSE_SPP_H_
#define CSE_SPP_H_

#include "cse.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CSE_NOISE_SPP 4 /* the method's number next to cse.h's CSE_NOISE_* */

typedef struct {
    double prior_h1;     /* a-priori probability of speech presence P(H1) */
    double xi_opt_db;    /* the fixed a-priori SNR under H1, in dB */
    double alpha_pow;    /* smoothing of the noise power estimate */
    double alpha_ph;     /* smoothing of the speech-presence probability */
    double ph_max;       /* where the smoothed probability exceeds it, ph is capped to it */
    int32_t init_frames; /* frames averaged into the initial estimate */
    int32_t reserved;
} cse_spp_params_t; /* 48 bytes */

void cse_spp_default_params(cse_spp_params_t* prm);
int cse_noise_spp(const double* P, int64_t n_sig, int T, int B, const cse_spp_params_t* prm,
                  double eps, float* N, cse_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* CSE_SPP_H_ */
