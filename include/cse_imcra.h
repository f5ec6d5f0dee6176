/*
 * cse_imcra.h — improved minima-controlled recursive averaging (IMCRA)
 * noise-PSD tracking on the device, next to the estimators of cse.h,
 * cse_mcra.h, cse_spp.h and cse_minstat.h (same conventions: caller-owned
 * device memory, asynchronous on `stream`, CSE_OK or a negative code and a
 * cse_last_error message).
 *
 * Cohen, "Noise Spectrum Estimation in Adverse Environments: Improved Minima
 * Controlled Recursive Averaging", IEEE Transactions on Speech and Audio
 * Processing 11(5), 2003: the noise estimator designed for OMLSA.  Against
 * MCRA (cse_mcra.h) it has a second smoothing and minimum-tracking pass over
 * the bins that a rough decision found free of speech, a soft a-priori
 * speech-absence probability that also looks at the a-priori SNR, and a bias
 * factor.  It needs no clean signal.  The reference has no such estimator
 * (noise_estimation.py knows percentile, min_tracking and true_noise), so this
 * header is the specification.
 *
 * Input P[s][t][b] = |Y|^2 in fp64, as cse_stft writes it: T frames,
 * B = n_fft/2 + 1 bins.  Each line is one individually rounded fp64 operation,
 * in this order (no FMA contraction; exp is the math library's fp64 exp; E1 is
 * the exponential integral, below; 1 - alpha_* and
 * xi_min = pow(10, xi_min_db / 10) are computed once in fp64).  U =
 * sub_windows, V = sub_frames.
 *
 *   m = (b == 0 ? 1 : b-1),  r = (b == B-1 ? B-2 : b+1)
 *                            mirror: the real signal's full spectrum
 *   sm3(X)[b] = (0.25 X[m] + 0.5 X[b]) + 0.25 X[r]       for any row X
 *
 *   t = 0:   S = St = sm3(P[0])[b]; Smin = Ssw = S; SW[u] = S, u < U
 *            Stmin = Stsw = St; SWt[u] = St
 *            lam = P[0][b]; N[0] = lam; g2g = 1
 *   t >= 1:  S = alpha_s S + (1 - alpha_s) sm3(P[t])[b]   two products, then the sum
 *            Smin = min(Smin, S); Ssw = min(Ssw, S)
 *   every t: gam  = P[t][b] / max(N[t], DBL_MIN)
 *            xi   = max(alpha g2g + (1 - alpha) max(gam - 1, 0), xi_min)
 *            v    = gam xi / (1 + xi)                     (gam * xi), then the quotient
 *            d    = max(b_min Smin, DBL_MIN);  gmin = P[t][b] / d;  zeta = S / d
 *            I[b] = (gmin < gamma0 && zeta < zeta0) ? 1 : 0      the rough decision
 *            den  = sm3(I)[b];  num = sm3(I .* P[t])[b]   needs I of bins m and r
 *            Stf  = den > 0 ? num / den : St
 *     t >= 1:  St = alpha_s St + (1 - alpha_s) Stf
 *              Stmin = min(Stmin, St);  Stsw = min(Stsw, St)
 *            dt   = max(b_min Stmin, DBL_MIN);  gmt = P[t][b] / dt;  zt = S / dt
 *            qh   = zt >= zeta0 ? 0 : gmt <= 1 ? 1
 *                   : gmt < gamma1 ? (gamma1 - gmt) / (gamma1 - 1) : 0
 *            p    = qh >= 1 ? 0 : qh <= 0 ? 1
 *                   : 1 / (1 + ((qh / (1 - qh)) (1 + xi)) exp(-v))
 *            g2g  = P[t][b] == 0 ? 0
 *                   : (((xi / (1 + xi)) (xi / (1 + xi))) exp(min(E1(max(v, DBL_MIN)), 700))) gam
 *            ad   = alpha_d + (1 - alpha_d) p
 *            lam  = ad lam + (1 - ad) P[t][b]
 *            if t + 1 < T: N[t+1] = beta lam              predictive, like mcra
 *            if (t + 1) % V == 0:  k = ((t + 1) / V - 1) % U
 *                SW[k] = Ssw;  Smin = min over u of SW[u];  Ssw = S
 *                SWt[k] = Stsw;  Stmin = min over u of SWt[u];  Stsw = St
 *   output:  N[s][t][b] = (float) max(N[t], eps)          f32 [n_sig][T][B]
 *
 * I .* P[t] is the product of the two rows, bin by bin.  g2g is G_H1^2 gamma
 * of the previous frame, with G_H1 = xi / (1 + xi) exp(E1(v) / 2): the
 * decision-directed estimate of the a-priori SNR.  qh is the paper's a-priori
 * speech-absence probability, p its speech-presence probability.  The bins
 * are coupled through the rough decision: the second pass of bin b reads I of
 * bins m and r of the same frame.
 *
 * Zero power gives exactly eps.  Constant power c gives N[0] = c and
 * N[t >= 1] = beta c to rounding: the bias factor beta is the paper's (its
 * eq. 18 compensates the bias of the recursive average in speech absence), it
 * is not taken out here.  What a non-finite P yields is not part of the
 * contract.
 *
 * E1(v) = int_v^inf exp(-x) / x dx, for v in [DBL_MIN, inf), with a relative
 * error of at most 1e-13; it is 0 above 745.  Its implementation is free.
 *
 * The contract is a tolerance, not bit equality, because exp, E1 and the
 * divisions may differ in the last bit between two libraries.  A device value
 * equals that of a restatement in the same order, or its f32 neighbour:
 * |N_dev - N_ref| <= 2^-23 N_ref, on inputs where the restatement's smallest
 * relative distance of a compared quantity to its threshold is at least 1e-9.
 * The compared quantities are gmin against gamma0, zeta and zt against zeta0,
 * gmt against 1 and against gamma1.
 *
 * cse_imcra_default_params: the paper's values at n_fft 512 / hop 128, 16 kHz:
 *   alpha 0.92, alpha_s 0.9, alpha_d 0.85, beta 1.47, b_min 1.66, gamma0 4.6,
 *   gamma1 3, zeta0 1.67, xi_min_db -18, sub_windows 8, sub_frames 15.
 * cse_noise_imcra: the estimate above for n_sig signals.  CSE_EINVAL (-1) when
 *   P, N or prm is NULL; n_sig < 0, T < 1 or B outside [33, 2049]; alpha,
 *   alpha_s or alpha_d outside [0, 1); beta, b_min, gamma0 or zeta0 not finite
 *   and > 0; gamma1 not finite and > 1; xi_min_db not finite (NaN counts as
 *   outside everywhere); sub_windows outside [1, 16]; sub_frames outside
 *   [1, 2^20].  n_sig == 0 launches nothing and returns CSE_OK.  No workspace.
 */
#ifndef CSE_IMCRA_H_
#define CSE_IMCRA_H_

#include "cse.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CSE_NOISE_IMCRA 6 /* the method's number next to cse.h's CSE_NOISE_* */

typedef struct {
    double alpha;        /* decision-directed weight of the a-priori SNR */
    double alpha_s;      /* smoothing of S and S~ */
    double alpha_d;      /* smoothing of the noise estimate in speech absence */
    double beta;         /* bias compensation */
    double b_min;        /* bias of the minimum */
    double gamma0;       /* rough decision: gamma_min below it */
    double gamma1;       /* q^ falls to 0 at gamma~_min = gamma1 */
    double zeta0;        /* rough decision and q^: zeta below it */
    double xi_min_db;    /* floor of the a-priori SNR, in dB */
    int32_t sub_windows; /* U: sub-windows in the minimum search window */
    int32_t sub_frames;  /* V: frames per sub-window */
} cse_imcra_params_t; /* 80 bytes */

void cse_imcra_default_params(cse_imcra_params_t* prm);
int cse_noise_imcra(const double* P, int64_t n_sig, int T, int B, const cse_imcra_params_t* prm,
                    double eps, float* N, cse_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* CSE_IMCRA_H_ */
