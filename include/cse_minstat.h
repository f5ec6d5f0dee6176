/*
 * cse_minstat.h — minimum-statistics noise-PSD tracking on the device, next to
 * the estimators of cse.h, cse_mcra.h and cse_spp.h (same conventions:
 * caller-owned device memory, asynchronous on `stream`, CSE_OK or a negative
 * code and a cse_last_error message).
 *
 * R. Martin, "Noise Power Spectral Density Estimation Based on Optimal
 * Smoothing and Minimum Statistics", IEEE Transactions on Speech and Audio
 * Processing 9(5), 2001: the periodogram is smoothed with a time- and
 * frequency-dependent optimal smoothing parameter, the minimum of the smoothed
 * power over a window of D = U V frames (kept as U sub-window minima) is
 * tracked per bin, and its bias is compensated from an estimate of the
 * smoothed power's variance.  It needs no clean signal.  The reference has no
 * such estimator (its min_tracking is an IIR, a 51-tap minimum filter and a
 * median floor), so this header is the specification.
 *
 * Input P[s][t][b] = |Y|^2 in fp64, as cse_stft writes it: T frames,
 * B = n_fft/2 + 1 bins.  Each line is one individually rounded fp64 operation
 * (a line with several: in the order its brackets give, left to right
 * otherwise), no FMA contraction; pow and sqrt are the math library's fp64
 * functions.  Sigma is a sum over the B bins of a frame in an order the
 * implementation chooses; TINY = DBL_MIN; U = sub_windows, V = sub_frames.
 *
 *   host, once:  M_D = M(U V);  M_V = M(V)        Martin's table, below
 *                nd  = (2 (U V - 1)) (1 - M_D);   md2 = 2 M_D
 *                nv  = (2 (V - 1)) (1 - M_V);     mv2 = 2 M_V
 *                q_lo = 1 / q_eq_max;  q_hi = 1 / q_eq_min;  c_c = 1 - alpha_c
 *   state per signal: ac, subwc, ib; per bin: p, sn2, pb, pb2, pminu, actmin,
 *                actminsub, lmf (a flag), buf[U]
 *   init:        p = sn2 = pb = pminu = P[0][b];  pb2 = p p;  ac = 1
 *                actmin = actminsub = +inf;  buf[0..U) = +inf;  lmf = 0
 *                subwc = V;  ib = -1
 *   every t in [0, T), with y = P[t][b]:
 *                sp  = Sigma p;  sy = Sigma y;  ss = Sigma sn2
 *                                           p, sn2 as frame t-1 left them
 *                r   = sp / max(sy, TINY) - 1
 *                acb = 1 / (1 + r r)
 *                ac  = alpha_c ac + c_c max(acb, alpha_c_floor)
 *                snr = sp / max(ss, TINY)
 *                fl  = min(alpha_min, pow(snr, snr_exp))
 *                                           C's pow, also at 0 and +inf
 *                aa  = alpha_max ac
 *                ql  = q_lo / (t + 1)
 *     per bin:   g   = p / max(sn2, TINY) - 1
 *                ah  = max(aa / (1 + g g), fl)
 *                p   = ah p + (1 - ah) y    two products, then the sum
 *                bt  = min(ah ah, beta_max)
 *                pb  = bt pb + (1 - bt) p
 *                pb2 = bt pb2 + (1 - bt) (p p)
 *                s2  = max(sn2, TINY)
 *                qe  = max(min((pb2 - pb pb) / max(2 (s2 s2), TINY), q_hi), ql)
 *                qav = (Sigma qe) / B
 *                bc  = 1 + av sqrt(qav)
 *     per bin:   iq  = 1 / qe
 *                bd  = 1 + nd / (iq - md2)
 *                bv  = 1 + nv / (iq - mv2)
 *                c   = (bc p) bd
 *                k   = c < actmin
 *                if k: actmin = c;  actminsub = (bc p) bv
 *     if 1 < subwc < V:
 *       per bin: lmf |= k;  pminu = min(actminsub, pminu);  sn2 = pminu
 *     else if subwc >= V:
 *                ib  = (ib + 1) % U
 *       per bin: buf[ib] = actmin;  pminu = min over buf[0..U)
 *                nsm = slope_max[i], i the first with qav < slope_q[i], else 3
 *       per bin: if lmf and not k and pminu < actminsub < nsm pminu:
 *                    pminu = actminsub;  buf[0..U) = pminu
 *                lmf = 0;  actmin = +inf
 *                subwc = 0
 *     subwc += 1
 *                N[t] = sn2        subwc == 1 and the second branch leave sn2
 *   output:      N[s][t][b] = (float) max(N[t], eps)       f32 [n_sig][T][B]
 *
 * Martin's table of M(D) for the bias of a minimum over D frames:
 *   D = 1, 2, 5, 8, 10, 15, 20, 30, 40, 60, 80, 120, 140, 160, 180, 220, 260, 300
 *   M = 0, .26, .48, .58, .61, .668, .705, .762, .8, .841, .865, .89, .9, .91,
 *       .92, .93, .935, .94
 * at a tabulated d the entry; for adjacent D_i < d < D_j
 *   M = M_i + (sqrt(D_i) sqrt(D_j) / sqrt(d) - sqrt(D_j)) (M_j - M_i)
 *             / (sqrt(D_i) - sqrt(D_j));
 * d >= 300 gives 0.94.  M(192) = 0.92332623, M(24) = 0.73206411.
 *
 * The guards (TINY, ql, the bounds on qe) are this project's: they make zero
 * power well defined.  All-zero P gives exactly eps everywhere; a zero bin or a
 * run of zero frames yields no NaN or inf.  What a non-finite P yields is not
 * part of the contract.
 *
 * The contract is a tolerance, not bit equality, because the order of the
 * three sums is the implementation's.  On inputs where a restatement in this
 * order has a margin of at least 1e-9, a device value is the restatement's f32
 * value or its neighbour: |N_dev - N_ref| <= 2^-23 N_ref.  The margin is the
 * smallest relative distance at any comparison the recursion branches on: c
 * against a finite non-zero actmin, qav against each slope_q where nsm is
 * chosen, actminsub against pminu and against nsm pminu on bins with lmf and
 * not k.
 *
 * cse_minstat_default_params: Martin's time constants at an 8-ms frame step
 *   (hop 128 at 16 kHz): alpha_c 0.837, alpha_c_floor 0.7, alpha_max 0.98,
 *   alpha_min 0.548, snr_exp -0.125, beta_max 0.894, av 2.12, q_eq_min 2,
 *   q_eq_max 14, slope_q {0.03, 0.05, 0.06}, slope_max {8, 4, 2, 1.2},
 *   sub_windows 8, sub_frames 24 (D = 192 frames = 1.536 s).
 * cse_noise_minstat: the estimate above for n_sig signals.  CSE_EINVAL (-1)
 *   when P, N or prm is NULL; n_sig < 0, T < 1 or B outside [33, 2049];
 *   alpha_c, alpha_c_floor, alpha_min or beta_max outside [0, 1); alpha_max
 *   outside (0, 1); snr_exp not finite or > 0; av not finite or < 0; not
 *   2 <= q_eq_min <= q_eq_max < inf (q_eq_min >= 2 > 2 * 0.94 keeps both bias
 *   denominators positive); slope_q not positive and strictly increasing; any
 *   slope_max not finite or < 1; sub_windows outside [1, 16]; sub_frames
 *   outside [2, 2^20].  NaN counts as outside everywhere.  n_sig == 0 launches
 *   nothing and returns CSE_OK.  No workspace: the state is in registers and
 *   LDS (where sub_windows times the bins exceeds the LDS, from sub_windows 10
 *   on at B = 2049, in registers that spill: correct, and slow).
 */
#ifndef CSE_MINSTAT_H_
#define CSE_MINSTAT_H_

#include "cse.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CSE_NOISE_MINSTAT 5 /* the method's number next to cse.h's CSE_NOISE_* */

typedef struct {
    double alpha_c;       /* smoothing of the correction factor ac */
    double alpha_c_floor; /* lower bound of the correction term */
    double alpha_max;     /* upper bound of the smoothing parameter */
    double alpha_min;     /* its lower bound at low SNR */
    double snr_exp;       /* exponent of the SNR in that lower bound (<= 0) */
    double beta_max;      /* upper bound of the variance estimate's smoothing */
    double av;            /* weight of sqrt(mean 1/Q_eq) in the bias correction */
    double q_eq_min;      /* bounds of the equivalent degrees of freedom */
    double q_eq_max;
    double slope_q[3];    /* thresholds on the mean inverse degrees of freedom */
    double slope_max[4];  /* allowed rise of a local minimum per sub-window */
    int32_t sub_windows;  /* U */
    int32_t sub_frames;   /* V: frames per sub-window */
} cse_minstat_params_t; /* 136 bytes */

void cse_minstat_default_params(cse_minstat_params_t* prm);
int cse_noise_minstat(const double* P, int64_t n_sig, int T, int B,
                      const cse_minstat_params_t* prm, double eps, float* N, cse_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* CSE_MINSTAT_H_ */
