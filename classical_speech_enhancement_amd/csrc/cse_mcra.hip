// MCRA noise-PSD tracking (include/cse_mcra.h; Cohen & Berdugo 2002) on device.
//
// One thread per (signal, bin), bins along threadIdx.x: every frame row is read
// and written by consecutive lanes.  The time loop is the header's sequential
// recurrence, every operation rounded on its own (the speech-presence
// threshold is a discontinuity: a reassociated or contracted form would be a
// different estimator), so the work is one long dependent fp64 chain per
// wave.  What can overlap it are the loads: a block of MCRA_U frames (the bin
// and its two neighbours, which hit the cache lines the row's own load
// brought in) is fetched ahead of the recurrence into registers, as
// cse_noise.hip's iir_kernel does; and within a block the S / Smin chain of
// the later frames, which does not depend on p and lam of the earlier ones.
// The state (S, Smin, Stmp, p, lam) stays in registers; no LDS.  One wave per
// workgroup: the sweep's shape has about 500 waves for 1,024 SIMDs, and
// single-wave workgroups spread over all CUs.
//
// The estimate is predictive (N[t+1] is written after frame t), so the last
// frame of P is never read.
#include "cse_common.hpp"

#include "../../include/cse_mcra.h"

namespace cse {

#ifndef CSE_MCRA_U
#define CSE_MCRA_U 8
#endif
constexpr int MCRA_U = CSE_MCRA_U;  // frames per prefetch block

struct McraK {  // the parameters and their complements, computed once on the host
    double a_s, c_s, a_d, c_d, a_p, c_p, delta;
};

struct McraState {
    double S, Smin, Stmp, p, lam;
};

struct McraRow {  // P[t][m], P[t][b], P[t][q]
    double m, c, q;
};

// Sf(t) = (0.25 P[t][m] + 0.5 P[t][b]) + 0.25 P[t][q]
__device__ __forceinline__ double mcra_sf(const McraRow& r) {
#pragma clang fp contract(off)
    return (0.25 * r.m + 0.5 * r.c) + 0.25 * r.q;
}

// the frame's S, Smin and Stmp (t >= 1), then (1 - alpha_p) I.  restart:
// t % L == 0, wave-uniform; written as selects so that a block of frames stays
// one basic block and the scheduler can run one frame's p / lam chain under
// the next frame's S chain (a lone wave per SIMD has nothing else to hide the
// fp64 latency with).  The product (1 - alpha_p) I is exact for I in {0, 1}.
__device__ __forceinline__ double mcra_presence(McraState& s, const McraK& k, double sf,
                                                bool restart) {
#pragma clang fp contract(off)
    s.S = k.a_s * s.S + k.c_s * sf;
    s.Smin = fmin(restart ? s.Stmp : s.Smin, s.S);
    s.Stmp = restart ? s.S : fmin(s.Stmp, s.S);
    return s.S > k.delta * s.Smin ? k.c_p : 0.0;
}

// p, ad and lam of a frame from its (1 - alpha_p) I and P[t][b]
__device__ __forceinline__ void mcra_track(McraState& s, const McraK& k, double ci, double pc) {
#pragma clang fp contract(off)
    s.p = k.a_p * s.p + ci;
    const double ad = k.a_d + k.c_d * s.p;
    s.lam = ad * s.lam + (1.0 - ad) * pc;
}

// the parameter checks of cse_noise_mcra, under the caller's name (the online
// enhancer, cse_online.hip, includes this file with CSE_MCRA_DEVICE_ONLY)
static int mcra_check_params(const char* name, const cse_mcra_params_t* prm) {
    const double al[3] = {prm->alpha_s, prm->alpha_d, prm->alpha_p};
    for (int i = 0; i < 3; ++i)  // written so that NaN fails
        CSE_CHECK_ARG(al[i] >= 0.0 && al[i] < 1.0,
                      "%s: alpha_s=%g alpha_d=%g alpha_p=%g not all in [0, 1)", name, al[0], al[1],
                      al[2]);
    CSE_CHECK_ARG(prm->delta > 0.0, "%s: delta=%g not > 0", name, prm->delta);
    CSE_CHECK_ARG(prm->window_frames >= 2, "%s: window_frames=%d < 2", name, prm->window_frames);
    return CSE_OK;
}

static McraK mcra_constants(const cse_mcra_params_t* prm) {
    McraK k;
    k.a_s = prm->alpha_s;
    k.c_s = 1.0 - prm->alpha_s;
    k.a_d = prm->alpha_d;
    k.c_d = 1.0 - prm->alpha_d;
    k.a_p = prm->alpha_p;
    k.c_p = 1.0 - prm->alpha_p;
    k.delta = prm->delta;
    return k;
}

#ifndef CSE_MCRA_DEVICE_ONLY
__global__ void __launch_bounds__(64) mcra_kernel(const double* __restrict__ P, int T, int B,
                                                  int nblk, McraK k, int L, double eps,
                                                  float* __restrict__ N) {
    const int b = (int)(blockIdx.x % (unsigned)nblk) * 64 + (int)threadIdx.x;
    const int64_t sig = blockIdx.x / (unsigned)nblk;
    if (b >= B) return;
    const int m = b == 0 ? 1 : b - 1, q = b == B - 1 ? B - 2 : b + 1;
    const double* Ps = P + sig * (int64_t)T * B;
    float* Ns = N + sig * (int64_t)T * B + b;
    auto load = [&](int t) {
        const double* row = Ps + (int64_t)t * B;
        return McraRow{row[m], row[b], row[q]};
    };
    // frame 0 (T == 1: the row is its own last frame, which only N[0] reads)
    const McraRow r0 = load(0);
    McraState s;
    s.S = mcra_sf(r0);
    s.Smin = s.Stmp = s.S;
    s.p = 0.0;
    s.lam = r0.c;
    Ns[0] = (float)fmax(s.lam, eps);
    if (T == 1) return;
    {
#pragma clang fp contract(off)
        mcra_track(s, k, s.S > k.delta * s.Smin ? k.c_p : 0.0, r0.c);
    }
    Ns[B] = (float)fmax(s.lam, eps);
    // frames [1, T-1): frame t writes N[t+1]
    constexpr int U = MCRA_U;
    const int end = T - 1;
    const int full = 1 + ((end > 1 ? end - 1 : 0) / U) * U;  // frames [1, full) in whole blocks
    int t = 1;
    int64_t next = L;  // the next restart frame (t % L == 0)
    if (full > 1) {
        McraRow nxt[U];
        double sf[U], pc[U], ci[U];  // the current block: Sf(t), P[t][b], (1 - alpha_p) I
#pragma unroll
        for (int u = 0; u < U; ++u) nxt[u] = load(1 + u);
        for (; t < full; t += U) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                sf[u] = mcra_sf(nxt[u]);
                pc[u] = nxt[u].c;
            }
            if (t + U < full) {  // uniform: the next block's loads run under this block's chain
#pragma unroll
                for (int u = 0; u < U; ++u) nxt[u] = load(t + U + u);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool restart = t + u == next;
                next += restart ? L : 0;
                ci[u] = mcra_presence(s, k, sf[u], restart);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                mcra_track(s, k, ci[u], pc[u]);
                Ns[(int64_t)(t + u + 1) * B] = (float)fmax(s.lam, eps);
            }
        }
    }
    for (; t < end; ++t) {
        const McraRow r = load(t);
        const bool restart = t == next;
        next += restart ? L : 0;
        const double ci = mcra_presence(s, k, mcra_sf(r), restart);
        mcra_track(s, k, ci, r.c);
        Ns[(int64_t)(t + 1) * B] = (float)fmax(s.lam, eps);
    }
}

#endif  // !CSE_MCRA_DEVICE_ONLY

}  // namespace cse

#ifndef CSE_MCRA_DEVICE_ONLY
using namespace cse;

extern "C" void cse_mcra_default_params(cse_mcra_params_t* prm) {
    if (!prm) return;
    prm->alpha_s = 0.8;
    prm->alpha_d = 0.95;
    prm->alpha_p = 0.2;
    prm->delta = 5.0;
    prm->window_frames = 125;
    prm->reserved = 0;
}

extern "C" int cse_noise_mcra(const double* P, int64_t n_sig, int T, int B,
                              const cse_mcra_params_t* prm, double eps, float* N,
                              cse_stream_t stream) {
    CSE_CHECK_ARG(P != nullptr && N != nullptr && prm != nullptr,
                  "cse_noise_mcra: P, N or params is NULL");
    CSE_CHECK_ARG(n_sig >= 0 && T >= 1 && B >= 33 && B <= 2049,
                  "cse_noise_mcra: bad shape n_sig=%lld T=%d B=%d (B in [33, 2049])",
                  (long long)n_sig, T, B);
    if (mcra_check_params("cse_noise_mcra", prm) != CSE_OK) return CSE_EINVAL;
    const int nblk = ceil_div(B, 64);
    CSE_CHECK_ARG(n_sig * nblk <= 0x7fffffffLL, "cse_noise_mcra: n_sig=%lld too many for one launch",
                  (long long)n_sig);
    if (n_sig == 0) return CSE_OK;
    const McraK k = mcra_constants(prm);
    hipLaunchKernelGGL(mcra_kernel, dim3((unsigned)(n_sig * nblk)), dim3(64), 0,
                       (hipStream_t)stream, P, T, B, nblk, k, (int)prm->window_frames, eps, N);
    CSE_CHECK_LAUNCH("cse_noise_mcra");
    return CSE_OK;
}
#endif  // !CSE_MCRA_DEVICE_ONLY
