// SPP-based MMSE noise-PSD tracking (include/cse_spp.h; Gerkmann & Hendriks
// 2012) on device.
//
// One thread per (signal, bin), bins along threadIdx.x: every frame row is read
// and written by consecutive lanes.  The time loop is the header's sequential
// recurrence, every operation rounded on its own.  Unlike MCRA's, the whole
// frame hangs on the previous frame's lam (lam -> divide -> exp -> divide ->
// est -> lam; only the pm line is off the chain), so nothing of a later frame
// can run under an earlier one: a wave is one dependent fp64 chain, and with
// one wave per SIMD the kernel runs at that chain's latency.  What is kept out
// of the chain's way is memory: a block of SPP_U frames of the bin (no
// neighbours: 8 doubles against MCRA's 24) is fetched into registers ahead of
// the recurrence, as mcra_kernel does, and the f32 stores wait for nothing.  A
// block is one basic block: the guard is a select.  The state (lam, pm) stays
// in registers; no LDS, no scratch.  One wave per workgroup: the sweep's shape
// has about 500 waves for 1,024 SIMDs, and single-wave workgroups spread over
// all CUs.
//
// The first K = min(init_frames, T) frames are read twice: for the initial
// mean, then by the loop.
#include "cse_common.hpp"

#include <float.h>
#include <math.h>

#include "../../include/cse_spp.h"

namespace cse {

#ifndef CSE_SPP_U
#define CSE_SPP_U 8
#endif
constexpr int SPP_U = CSE_SPP_U;  // frames per prefetch block

struct SppK {  // the header's host-side constants and the complements 1 - alpha
    double prior, c0, c1, a_ph, c_ph, ph_max, a_pow, c_pow, prior_h1;
};

// one frame of the recurrence: updates lam and pm from P[t][b], returns N[t]
__device__ __forceinline__ double spp_frame(double& lam, double& pm, const SppK& k, double p) {
#pragma clang fp contract(off)
    const double s = p / fmax(lam, DBL_MIN);
    const double a = fmin(k.c0 + k.c1 * s, 200.0);
    const double g = k.prior * exp(a);
    const double ph = g / (1.0 + g);
    pm = k.a_ph * pm + k.c_ph * ph;
    const double pc = pm > k.ph_max ? fmin(ph, k.ph_max) : ph;  // a select: no branch in a block
    const double est = pc * lam + (1.0 - pc) * p;
    lam = k.a_pow * lam + k.c_pow * est;
    return lam;
}

// the parameter checks of cse_noise_spp, under the caller's name (the online
// enhancer, cse_online.hip, includes this file with CSE_SPP_DEVICE_ONLY)
static int spp_check_params(const char* name, const cse_spp_params_t* prm) {
    // every range written so that NaN fails
    CSE_CHECK_ARG(prm->prior_h1 > 0.0 && prm->prior_h1 < 1.0 && prm->ph_max > 0.0 &&
                      prm->ph_max < 1.0,
                  "%s: prior_h1=%g ph_max=%g not both in (0, 1)", name, prm->prior_h1,
                  prm->ph_max);
    CSE_CHECK_ARG(prm->alpha_pow >= 0.0 && prm->alpha_pow < 1.0 && prm->alpha_ph >= 0.0 &&
                      prm->alpha_ph < 1.0,
                  "%s: alpha_pow=%g alpha_ph=%g not both in [0, 1)", name, prm->alpha_pow,
                  prm->alpha_ph);
    CSE_CHECK_ARG(isfinite(prm->xi_opt_db), "%s: xi_opt_db=%g not finite", name, prm->xi_opt_db);
    CSE_CHECK_ARG(prm->init_frames >= 1, "%s: init_frames=%d < 1", name, prm->init_frames);
    return CSE_OK;
}

// the header's host-side constants
static SppK spp_constants(const cse_spp_params_t* prm) {
    // the base through a volatile: pow stays the library's pow (no exp10 in its place)
    volatile double ten = 10.0;
    const double xi = pow(ten, prm->xi_opt_db / 10.0);
    SppK k;
    k.prior = prm->prior_h1 / (1.0 - prm->prior_h1);
    k.c0 = log(1.0 / (1.0 + xi));
    k.c1 = xi / (1.0 + xi);
    k.a_ph = prm->alpha_ph;
    k.c_ph = 1.0 - prm->alpha_ph;
    k.ph_max = prm->ph_max;
    k.a_pow = prm->alpha_pow;
    k.c_pow = 1.0 - prm->alpha_pow;
    k.prior_h1 = prm->prior_h1;
    return k;
}

#ifndef CSE_SPP_DEVICE_ONLY
__global__ void __launch_bounds__(64) spp_kernel(const double* __restrict__ P, int T, int B,
                                                 int nblk, SppK k, int K, double eps,
                                                 float* __restrict__ N) {
    const int b = (int)(blockIdx.x % (unsigned)nblk) * 64 + (int)threadIdx.x;
    const int64_t sig = blockIdx.x / (unsigned)nblk;
    if (b >= B) return;
    const double* Ps = P + sig * (int64_t)T * B + b;
    float* Ns = N + sig * (int64_t)T * B + b;
    // the initial estimate: the mean of the first K frames, summed in order
    double lam = Ps[0];
#pragma unroll 4
    for (int t = 1; t < K; ++t) lam = lam + Ps[(int64_t)t * B];
    lam = lam / (double)K;
    double pm = k.prior_h1;
    constexpr int U = SPP_U;
    const int full = (T / U) * U;  // frames [0, full) in whole blocks
    int t = 0;
    if (full > 0) {
        double nxt[U], cur[U];
#pragma unroll
        for (int u = 0; u < U; ++u) nxt[u] = Ps[(int64_t)u * B];
        for (; t < full; t += U) {
#pragma unroll
            for (int u = 0; u < U; ++u) cur[u] = nxt[u];
            if (t + U < full) {  // uniform: the next block's loads run under this block's chain
#pragma unroll
                for (int u = 0; u < U; ++u) nxt[u] = Ps[(int64_t)(t + U + u) * B];
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                Ns[(int64_t)(t + u) * B] = (float)fmax(spp_frame(lam, pm, k, cur[u]), eps);
        }
    }
    for (; t < T; ++t)
        Ns[(int64_t)t * B] = (float)fmax(spp_frame(lam, pm, k, Ps[(int64_t)t * B]), eps);
}

#endif  // !CSE_SPP_DEVICE_ONLY

}  // namespace cse

#ifndef CSE_SPP_DEVICE_ONLY
using namespace cse;

extern "C" void cse_spp_default_params(cse_spp_params_t* prm) {
    if (!prm) return;
    prm->prior_h1 = 0.5;
    prm->xi_opt_db = 15.0;
    prm->alpha_pow = 0.8;
    prm->alpha_ph = 0.9;
    prm->ph_max = 0.99;
    prm->init_frames = 5;
    prm->reserved = 0;
}

extern "C" int cse_noise_spp(const double* P, int64_t n_sig, int T, int B,
                             const cse_spp_params_t* prm, double eps, float* N,
                             cse_stream_t stream) {
    CSE_CHECK_ARG(P != nullptr && N != nullptr && prm != nullptr,
                  "cse_noise_spp: P, N or params is NULL");
    CSE_CHECK_ARG(n_sig >= 0 && T >= 1 && B >= 33 && B <= 2049,
                  "cse_noise_spp: bad shape n_sig=%lld T=%d B=%d (B in [33, 2049])",
                  (long long)n_sig, T, B);
    if (spp_check_params("cse_noise_spp", prm) != CSE_OK) return CSE_EINVAL;
    const int nblk = ceil_div(B, 64);
    CSE_CHECK_ARG(n_sig * nblk <= 0x7fffffffLL, "cse_noise_spp: n_sig=%lld too many for one launch",
                  (long long)n_sig);
    if (n_sig == 0) return CSE_OK;
    const SppK k = spp_constants(prm);
    const int K = prm->init_frames < T ? prm->init_frames : T;
    hipLaunchKernelGGL(spp_kernel, dim3((unsigned)(n_sig * nblk)), dim3(64), 0,
                       (hipStream_t)stream, P, T, B, nblk, k, K, eps, N);
    CSE_CHECK_LAUNCH("cse_noise_spp");
    return CSE_OK;
}
#endif  // !CSE_SPP_DEVICE_ONLY
