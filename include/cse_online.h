/*
 * cse_online.h — the stateful online enhancer: the offline path (cse_stft, a
 * noise tracker, cse_noise_finish, the gain recursion and the inverse
 * transform of cse_enhance_cells_generic) run frame by frame on audio that is
 * still arriving, for S concurrent signals in lockstep.  Same conventions as
 * cse.h: caller-owned device memory, asynchronous on `stream`, CSE_OK or a
 * negative code and a cse_last_error message.  The reference has no such path
 * (its plugins take the finished clip), so this header is the specification.
 *
 * FRAMING.  The caller feeds the reflect-padded signal
 *   xp[p] = x[reflect(p - n_fft/2)],  p in [0, len + n_fft)
 * (np.pad(x, n_fft/2, mode="reflect"), as cse_stft pads).  Frame t covers
 * xp[t hop, t hop + n_fft); a clip of len samples has T = 1 + len / hop frames;
 * the window is periodic Hann, w(n) = 0.5 - 0.5 cos(2 pi n / n_fft), fp64.
 * cse_online_prime takes xp[0, n_fft - hop); every frame pushed afterwards
 * brings hop more samples.  The head of xp needs x[0, n_fft/2]: the first
 * frame can be pushed once n_fft/2 + 1 samples of x are known; the tail
 * (x[len - 2 - j] at xp[n_fft/2 + len + j]) once len is.
 *
 * PER FRAME t (counted from the prime), in this order, per signal:
 *   1. Analysis: X = DFT(w xp[t hop ...]) by a radix-2 decimation-in-time FFT
 *      in fp64 (the order of cse_stft's radix-2 form); the imaginary parts of
 *      bins 0 and n_fft/2 are exact zeros; P = Re^2 + Im^2 in fp64;
 *      Y = (float) X.  (cse_stft runs n_fft 512 in another order, so there P
 *      may differ from cse_stft's in the last bits.)
 *   2. The tracker's step for frame t exactly as its header states it, every
 *      operation individually rounded in fp64:
 *        mcra (cse_mcra.h)  N[t] = lam before frame t enters (predictive);
 *                           frame 0 initialises S, Smin, Stmp, p, lam; the
 *                           window restarts where t % window_frames == 0
 *        spp (cse_spp.h)    N[t] = lam after frame t enters; lam starts as the
 *                           sequential mean of P over the first K = init_frames
 *                           frames, so the first push must carry k >= K frames
 *                           (they are transformed twice, as cse_noise_spp reads
 *                           them twice)
 *      n[t] = (float) max(N[t], eps): the row cse_noise_<method> writes; it is
 *      what n_out receives.
 *   3. The row's post-processing as cse_noise_finish does it, fp64 math:
 *        s_0 = n[0],  s_t = mu s_{t-1} + (1 - mu) n[t]     two products, one sum
 *      with mu = clip(mu, 0, 0.9999), mu = 0 where the algorithm does not
 *      smooth; the gain reads (float) s_t for CSE_ALGO_SS and
 *      1 / max((float) s_t, (float) eps) in f32 for the others.
 *   4. The gain of `algo` with param[8] as in cse_cell_t, through the device
 *      functions of cse_enhance_cells_generic (gain_bin<1024, ALGO>): f32, the
 *      decision-directed state of the previous frame, alpha_t = 0 at t = 0.
 *   5. x_t = irfft(Y G) as a complex n_fft/2-point radix-2 inverse FFT in f32,
 *      times w, added into the overlap ring (cse_enhance_cells_generic's code).
 *
 * EMISSION.  After frame t the padded samples [t hop, (t + 1) hop) are final:
 * no later frame touches them.  Each is divided, in fp64, by the sum of w^2
 * over the frames <= t that cover it, in ascending frame order; a sum
 * <= DBL_MIN leaves the sample unscaled (cse_istft_norm).  That sum is the
 * offline normalisation of the sample whatever T turns out to be.
 * cse_online_finish emits the remaining n_fft - hop samples
 * [T hop, (T - 1) hop + n_fft) the same way.  Output sample o of the caller's
 * signal is padded sample o + n_fft/2: the caller drops the first n_fft/2
 * emitted samples and everything from len on.  Nothing is clipped.
 *
 * LATENCY.  Output sample o is final once input sample o + n_fft - 1 is in
 * (the frame that closes o's hop reaches that far): CSE_ONLINE_LATENCY(n_fft)
 * = n_fft - 1 samples of look-ahead at most, n_fft - hop at least.  With spp
 * the first K frames are held back once, (K - 1) hop more before the first
 * output.
 *
 * EQUALITY WITH OFFLINE.  The offline path replaces every estimator by the
 * static "simple" estimate when T < 5 (noise_estimation.py:194-195), and
 * cse_noise_spp averages min(init_frames, T) frames.  A stream does not know T,
 * so the same samples as the offline path are claimed for
 * T >= max(5, init_frames) only; the waveform then agrees to the project's
 * parity bound (1e-5 relative), the tracked rows to one f32 step.
 *
 * STATE.  One device block of cse_online_state_bytes(n_fft, n_streams) bytes,
 * 256-byte aligned, per batch.  Per signal it holds (B = n_fft/2 + 1):
 *   f64 [n_fft]         input tail: the last n_fft - hop samples of xp seen
 *   f64 [5][B]          tracker: mcra S, Smin, Stmp, p, lam; spp lam, pm
 *   f64 [B]             the mu recursion's s
 *   f32 [B]             the decision-directed state
 *   f32 [n_fft]         the overlap ring (hop of it zero between frames)
 * The size does not depend on hop, algorithm or method.  The frame counter
 * (window restarts, first-frame forms, ring position) is common to the batch
 * and lives in the host handle.  The library allocates nothing.
 *
 * cse_online_t is a caller-owned host structure of plain data; the calls on
 * one handle are made from one thread at a time, in stream order.
 *
 * cse_online_state_bytes: the block's size; -1 for an unsupported n_fft or
 *   n_streams < 0.
 * cse_online_init: checks the configuration and fills the handle; no device
 *   work (cse_online_prime overwrites all state that a frame reads).
 *   CSE_EINVAL with a message naming the case for: a NULL pointer; n_streams
 *   < 0; n_fft not a power of two in [128, 2048]; hop not n_fft/8, n_fft/4 or
 *   n_fft/2; an unknown algorithm; a noise method other than CSE_NOISE_MCRA /
 *   CSE_NOISE_SPP (minstat and imcra: state of another size, coupled bins;
 *   percentile, min_tracking and true_noise need the whole clip); tracker
 *   parameters their own entry point refuses; eps not > 0; mu NaN.
 * cse_online_prime: x_head [S][n_fft - hop] f64 -> the input tail; every other
 *   state is reset (frame counter 0).  Also the way to reset a handle.
 * cse_online_push: k frames.  x [S][k hop] f64 (the next samples of xp),
 *   y [S][k hop] f32 (padded samples [t0 hop, (t0 + k) hop)), n_out
 *   [S][k][B] f32 or NULL.  One workgroup per signal loops over the k frames;
 *   the per-frame work does not depend on k, so the outputs do not depend on
 *   how the frames are split over pushes.  CSE_EINVAL before any launch for:
 *   NULL handle, x or y; k < 0; a handle not primed or already finished;
 *   k < init_frames on spp's first push.  k == 0 or n_streams == 0 launch
 *   nothing and return CSE_OK.
 * cse_online_finish: y_tail [S][n_fft - hop] f32; afterwards push is refused
 *   until the next cse_online_prime.
 *
 * Streams that start and end one by one, with parameter values and a pace of
 * their own: cse_online_pool.h.
 */
#ifndef CSE_ONLINE_H_
#define CSE_ONLINE_H_

#include "cse.h"
#include "cse_mcra.h"
#include "cse_spp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CSE_ONLINE_LATENCY(n_fft) ((n_fft) - 1)

typedef struct cse_online_config {
    int32_t n_fft;        /* power of two in [128, 2048] */
    int32_t hop;          /* n_fft/8, n_fft/4 or n_fft/2 */
    int32_t algo;         /* CSE_ALGO_SS .. CSE_ALGO_OMLSA */
    int32_t noise_method; /* CSE_NOISE_MCRA or CSE_NOISE_SPP */
    float param[8];       /* as cse_cell_t.param */
    double eps;           /* the algorithm's eps: floor of the tracked row and of its inverse */
    double mu;            /* noise smoothing (mmse, omlsa); 0 = none */
    cse_mcra_params_t mcra; /* read for CSE_NOISE_MCRA */
    cse_spp_params_t spp;   /* read for CSE_NOISE_SPP */
} cse_online_config_t;      /* 152 bytes */

typedef struct cse_online {
    cse_online_config_t cfg;
    int64_t n_streams;
    void* state;     /* the device block */
    int64_t frames;  /* frames pushed since the prime */
    int32_t primed;  /* 1 between cse_online_prime and cse_online_finish */
    int32_t reserved;
} cse_online_t;      /* 184 bytes */

int64_t cse_online_state_bytes(int n_fft, int64_t n_streams);
int cse_online_init(cse_online_t* h, const cse_online_config_t* cfg, int64_t n_streams,
                    void* state);
int cse_online_prime(cse_online_t* h, const double* x_head, cse_stream_t stream);
int cse_online_push(cse_online_t* h, const double* x, int k, float* y, float* n_out,
                    cse_stream_t stream);
int cse_online_finish(cse_online_t* h, float* y_tail, cse_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* CSE_ONLINE_H_ */
