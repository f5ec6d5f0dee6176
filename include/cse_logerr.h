/*
 * cse_logerr.h — the logarithmic estimation error (LogErr) of a noise-PSD
 * estimate against a reference noise PSD, on the device, next to the entry
 * points of cse_sisdr.h and cse_mcra.h (same conventions: caller-owned device
 * memory, asynchronous on `stream`, CSE_OK or a negative code and a
 * cse_last_error message, no allocation in the library, all argument checks
 * before any device work).
 *
 * The noise trackers of cse_mcra.h, cse_spp.h, cse_minstat.h and cse_imcra.h
 * are judged in the literature by the mean absolute distance in dB between
 * their estimate and a reference noise PSD made from the noise alone (Hendriks,
 * Jensen & Heusdens 2008; Gerkmann & Hendriks 2012 use it in their
 * evaluations), split into the part where the estimate is too large and the
 * part where it is too small (Taghia et al. 2011): over-estimation makes a gain
 * rule attenuate speech, under-estimation leaves residual and musical noise.
 * The sweep knows the noise exactly (noisy - clean), so it can score an
 * estimate without running an enhancement algorithm on top of it.  The
 * reference scores nothing of the kind, so this header is the specification.
 *
 * Reference PSD (cse_logerr_reference).  Pv[s][t][b] is the fp64 power of
 * STFT(noisy - clean), exactly as cse_stft(x, x_sub, ...) writes P: T frames,
 * B = n_fft/2 + 1 bins.  R is fp64 [n_sig][T][B], per (signal, bin):
 *
 *   R[0] = Pv[0]
 *   R[t] = beta R[t-1] + (1 - beta) Pv[t]          t >= 1
 *
 * The two products and the sum are each rounded on their own (no FMA
 * contraction), and 1 - beta is computed once in fp64: the contract is bit
 * equality with a restatement in the same order.  beta must lie in [0, 1);
 * beta = 0 makes R = Pv.  The smoothing constant is a parameter: 0.9, a time
 * constant of roughly 80 ms at a hop of 8 ms, is the default this project's
 * Python layer chose, not a value taken from one of the papers above.
 *
 * Score (cse_logerr_rows).  A row r is one estimate of one signal: f32 at
 * N + n_offset[r], frame t starting t * t_stride[r] elements further on.
 * t_stride[r] = B is a time-varying estimate [T][B] (the trackers,
 * min_tracking, true_noise); t_stride[r] = 0 is a static [B] row (percentile).
 * sig_of[r] selects the signal whose R the row is scored against.  prm holds
 *   floor            > 0 and finite            (default 1e-12)
 *   t0               first scored frame        (default 0)
 *   bin_lo, bin_hi   scored bins [bin_lo, bin_hi)   (default [0, B))
 * Per scored element (t in [t0, T), b in [bin_lo, bin_hi)), each line one
 * rounded fp64 operation:
 *
 *   Rf = (R[t][b] < floor) ? floor : R[t][b]
 *   Nf = ((double)N[t][b] < floor) ? floor : (double)N[t][b]
 *   d  = 10 * log10(Rf / Nf)          one division, log10, one product
 *   o  = (d > 0) ? 0 : -d             over-estimation  (N too large)
 *   u  = (d < 0) ? 0 : d              under-estimation (N too small)
 *
 * The selects are written this way so that a NaN in N (or R) reaches both o
 * and u.  Beyond that plain IEEE holds: N = +inf gives o = +inf, u = 0.  With
 * nb = bin_hi - bin_lo and n = (T - t0) nb:
 *
 *   Fo[t] = sum_b o,  Fu[t] = sum_b u                       t in [t0, T)
 *   frame_over[r][t]  = Fo[t] / nb    (NaN for t < t0)      likewise frame_under
 *   over[r]  = (sum_t Fo[t]) / n,     under[r] = (sum_t Fu[t]) / n
 *
 * Each quotient is one fp64 division by (double)nb or (double)n.  The order of
 * the sums is free, so against a restatement the contract is a tolerance.
 * LogErr itself is over + under, one fp64 addition the caller takes.
 *
 * A row whose sig_of lies outside [0, n_sig), or whose t_stride is neither 0
 * nor B, scores NaN (over, under and every frame value) and reads nothing of
 * N or R: the tables are device arrays, so the host cannot check them.
 *
 * Determinism: a row's outputs depend on its own inputs only (its N, its
 * signal's R, T, B and prm).  Scored alone or at any position in a launch of
 * any n_rows it returns the same bits: no floating-point atomics, and the
 * shape of both reductions is fixed by T, B and prm alone.
 *
 * cse_logerr_default_params: floor 1e-12, t0 0, bins [0, B).
 * cse_logerr_reference: CSE_EINVAL (-1) when Pv or R is NULL; n_sig < 0, T < 1
 *   or B outside [33, 2049]; beta outside [0, 1), NaN included.  n_sig == 0
 *   launches nothing and returns CSE_OK.  R may not alias Pv.
 * cse_logerr_scratch_bytes: bytes of per-launch scratch: 16 n_rows T (Fo and
 *   Fu of every row and frame, between the two kernels); -1 on a negative
 *   count.
 * cse_logerr_rows: over[r] and under[r], f64 [n_rows]; frame_over and
 *   frame_under, f64 [n_rows][T], both or neither NULL.  CSE_EINVAL when R, N,
 *   n_offset, t_stride, sig_of, prm, over or under is NULL, or scratch is NULL
 *   while rows are to be scored; only one of the frame outputs is NULL; a count
 *   is negative; T < 1; B outside [33, 2049]; floor is not finite and > 0; t0
 *   outside [0, T); the bin range is empty or leaves [0, B].  n_rows == 0 or
 *   n_sig == 0 launches nothing and returns CSE_OK.
 */
#ifndef CSE_LOGERR_H_
#define CSE_LOGERR_H_

#include "cse.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    double floor;    /* both PSDs are raised to this before the quotient */
    int32_t t0;      /* first scored frame */
    int32_t bin_lo;  /* scored bins [bin_lo, bin_hi) */
    int32_t bin_hi;
    int32_t reserved;
} cse_logerr_params_t; /* 24 bytes */

void cse_logerr_default_params(cse_logerr_params_t* prm, int B);
int cse_logerr_reference(const double* Pv, int64_t n_sig, int T, int B, double beta, double* R,
                         cse_stream_t stream);
int64_t cse_logerr_scratch_bytes(int64_t n_rows, int T);
int cse_logerr_rows(const double* R, int64_t n_sig, int T, int B, const float* N,
                    const int64_t* n_offset, const int64_t* t_stride, const int32_t* sig_of,
                    int64_t n_rows, const cse_logerr_params_t* prm, void* scratch, double* over,
                    double* under, double* frame_over, double* frame_under, cse_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* CSE_LOGERR_H_ */
