// IMCRA noise-PSD tracking (include/cse_imcra.h; Cohen 2003) on device.
//
// Lanes are bins, the time loop is the header's sequential recurrence, every
// operation rounded on its own (the comparisons are discontinuities: a
// reassociated or contracted form would be another estimator).
//
// The bins are coupled: the second pass of bin b needs the rough decision I of
// bins b - 1 and b + 1 of the same frame, and I hangs on the first pass's
// state (S, Smin).  The first pass of a bin depends on P[b-1 .. b+1] only, so
// a wave recomputes it for one bin beyond each of its ends instead of waiting
// for another wave: a wave of 64 lanes covers 62 bins and two halo bins, whose
// lanes run the same code and store nothing.  Inside the wave, I is the
// comparison's lane mask (a ballot), and a lane reads its neighbours' bits
// from it with a shift: no LDS exchange, no barrier, waves independent as in
// cse_mcra.hip.  Carrying the neighbours' first pass in each lane's own
// registers instead would have cost three first passes (six divisions) a
// frame; one workgroup per signal would have cost a barrier a frame.
//
// The sub-window minima SW / SWt are indexed by the run-time slot k: they are
// in LDS ([slot][lane], 2 U KB a wave), written and scanned once in V frames.
// The rest of the state is in registers; no scratch.  A block of IMCRA_UB
// frame rows (the bin and its two neighbours) is fetched ahead of the
// recurrence, as mcra_kernel does.  One wave per workgroup: the sweep's shape
// has about 500 waves for 1,024 SIMDs.
//
// The estimate is predictive (N[t+1] is written after frame t), so the last
// frame of P is read only where T == 1.
#include "cse_common.hpp"

#include <float.h>
#include <math.h>

#include "../../include/cse_imcra.h"
#include "cse_e1.hpp"

namespace cse {

#ifndef CSE_IMCRA_UB
#define CSE_IMCRA_UB 8
#endif
constexpr int IMCRA_UB = CSE_IMCRA_UB;  // frames per prefetch block
constexpr int IMCRA_BINS = 62;          // bins a wave stores: 64 lanes less the two halo lanes

struct ImcraK {  // the parameters, their complements and xi_min, computed once on the host
    double a, c_a, a_s, c_s, a_d, c_d, beta, b_min, gamma0, gamma1, g1m1, zeta0, xi_min;
    int U, V;
};

struct ImcraState {
    double S, Smin, Ssw, St, Stmin, Stsw, lam, g2g, n;  // n: N[t], before the eps floor
};

struct ImcraRow {  // P[t][m], P[t][b], P[t][r]
    double m, c, r;
};

// sm3: (0.25 X[m] + 0.5 X[b]) + 0.25 X[r]
__device__ __forceinline__ double imcra_sm3(double m, double c, double r) {
#pragma clang fp contract(off)
    return (0.25 * m + 0.5 * c) + 0.25 * r;
}

// One frame of the header's recurrence, after which s.n is N[t+1].  FIRST: t == 0,
// where S and St are the initial values.  Every lane of the wave must be here
// (the ballot); left / right: where this lane's I[m] and I[r] sit in the mask.
template <bool FIRST>
__device__ __forceinline__ void imcra_frame(ImcraState& s, const ImcraK& k, const ImcraRow& p,
                                            int left, int right) {
#pragma clang fp contract(off)
    if (!FIRST) {
        s.S = k.a_s * s.S + k.c_s * imcra_sm3(p.m, p.c, p.r);
        s.Smin = fmin(s.Smin, s.S);
        s.Ssw = fmin(s.Ssw, s.S);
    }
    const double gam = p.c / fmax(s.n, DBL_MIN);
    const double xi = fmax(k.a * s.g2g + k.c_a * fmax(gam - 1.0, 0.0), k.xi_min);
    const double xi1 = 1.0 + xi;
    const double v = (gam * xi) / xi1;
    // the rough decision, and the neighbours' through the lane mask
    const double d = fmax(k.b_min * s.Smin, DBL_MIN);
    const double gmin = p.c / d, zeta = s.S / d;
    const bool ib = gmin < k.gamma0 && zeta < k.zeta0;
    const unsigned long long mask = __ballot(ib);
    const double i_c = ib ? 1.0 : 0.0;
    const double i_m = (mask >> left) & 1ull ? 1.0 : 0.0;
    const double i_r = (mask >> right) & 1ull ? 1.0 : 0.0;
    const double den = imcra_sm3(i_m, i_c, i_r);
    const double num = imcra_sm3(i_m * p.m, i_c * p.c, i_r * p.r);
    const double stf = den > 0.0 ? num / den : s.St;
    if (!FIRST) {
        s.St = k.a_s * s.St + k.c_s * stf;
        s.Stmin = fmin(s.Stmin, s.St);
        s.Stsw = fmin(s.Stsw, s.St);
    }
    const double dt = fmax(k.b_min * s.Stmin, DBL_MIN);
    const double gmt = p.c / dt, zt = s.S / dt;
    const double qh = zt >= k.zeta0 ? 0.0
                      : gmt <= 1.0  ? 1.0
                      : gmt < k.gamma1 ? (k.gamma1 - gmt) / k.g1m1
                                       : 0.0;
    const double emv = exp(-v);
    const double pp = 1.0 / (1.0 + ((qh / (1.0 - qh)) * xi1) * emv);
    const double ph = qh >= 1.0 ? 0.0 : qh <= 0.0 ? 1.0 : pp;
    const double g = xi / xi1;
    const double ee = exp(fmin(e1(fmax(v, DBL_MIN), emv), 700.0));
    s.g2g = p.c == 0.0 ? 0.0 : ((g * g) * ee) * gam;
    const double ad = k.a_d + k.c_d * ph;
    s.lam = ad * s.lam + (1.0 - ad) * p.c;
    s.n = k.beta * s.lam;
}

// the end of a sub-window: slot k takes the sub-window's minimum, the minimum
// over all slots is the new running one, the next sub-window starts at S / St
__device__ __forceinline__ void imcra_roll(ImcraState& s, double* sw, int U, int k) {
    double* swt = sw + U * 64;
    sw[k * 64] = s.Ssw;
    swt[k * 64] = s.Stsw;
    double a = sw[0], b = swt[0];
    for (int u = 1; u < U; ++u) {
        a = fmin(a, sw[u * 64]);
        b = fmin(b, swt[u * 64]);
    }
    s.Smin = a;
    s.Stmin = b;
    s.Ssw = s.S;
    s.Stsw = s.St;
}

__global__ void __launch_bounds__(64) imcra_kernel(const double* __restrict__ P, int T, int B,
                                                   int nblk, ImcraK k, double eps,
                                                   float* __restrict__ N) {
    extern __shared__ double imcra_sw[];  // SW[U][64], then SWt[U][64]
    const int lane = (int)threadIdx.x;
    const int bi = (int)(blockIdx.x % (unsigned)nblk) * IMCRA_BINS - 1 + lane;
    const int64_t sig = blockIdx.x / (unsigned)nblk;
    // a halo lane beyond the spectrum runs the end bin again; no lane leaves
    // before the last ballot
    const int b = bi < 0 ? 0 : bi > B - 1 ? B - 1 : bi;
    const bool own = lane >= 1 && lane <= IMCRA_BINS && bi < B;
    const int m = b == 0 ? 1 : b - 1, r = b == B - 1 ? B - 2 : b + 1;
    // where I[m] and I[r] sit in the wave's mask: the lanes beside this one, the
    // mirrored one at the spectrum's ends (only lanes that store need them)
    const int left = b == 0 ? lane + 1 : lane - 1;
    const int right = b == B - 1 ? lane - 1 : lane + 1;
    const int li = left & 63, ri = right & 63;
    const double* Ps = P + sig * (int64_t)T * B;
    float* Ns = N + sig * (int64_t)T * B + b;
    double* sw = imcra_sw + lane;
    auto load = [&](int t) {
        const double* row = Ps + (int64_t)t * B;
        return ImcraRow{row[m], row[b], row[r]};
    };
    const int U = k.U;
    // frame 0
    const ImcraRow r0 = load(0);
    ImcraState s;
    s.S = s.St = imcra_sm3(r0.m, r0.c, r0.r);
    s.Smin = s.Ssw = s.S;
    s.Stmin = s.Stsw = s.St;
    s.lam = s.n = r0.c;
    s.g2g = 1.0;
    if (own) Ns[0] = (float)fmax(s.n, eps);
    if (T == 1) return;
    for (int u = 0; u < 2 * U; ++u) sw[u * 64] = s.S;
    int slot = 0;        // ((t + 1) / V - 1) % U at the next roll
    int64_t next = k.V;  // the next t + 1 that is a multiple of V
    auto roll = [&](int t1) {  // after frame t1 - 1; uniform
        if (t1 == next) {
            imcra_roll(s, sw, U, slot);
            slot = slot + 1 == U ? 0 : slot + 1;
            next += k.V;
        }
    };
    imcra_frame<true>(s, k, r0, li, ri);
    if (own) Ns[B] = (float)fmax(s.n, eps);
    roll(1);
    // frames [1, T-1): frame t writes N[t+1]
    constexpr int UB = IMCRA_UB;
    const int end = T - 1;
    const int full = 1 + ((end > 1 ? end - 1 : 0) / UB) * UB;  // frames [1, full) in whole blocks
    int t = 1;
    if (full > 1) {
        ImcraRow nxt[UB], cur[UB];
#pragma unroll
        for (int u = 0; u < UB; ++u) nxt[u] = load(1 + u);
        for (; t < full; t += UB) {
#pragma unroll
            for (int u = 0; u < UB; ++u) cur[u] = nxt[u];
            if (t + UB < full) {  // uniform: the next block's loads run under this block's chain
#pragma unroll
                for (int u = 0; u < UB; ++u) nxt[u] = load(t + UB + u);
            }
#pragma unroll
            for (int u = 0; u < UB; ++u) {
                imcra_frame<false>(s, k, cur[u], li, ri);
                if (own) Ns[(int64_t)(t + u + 1) * B] = (float)fmax(s.n, eps);
                roll(t + u + 1);
            }
        }
    }
    for (; t < end; ++t) {
        imcra_frame<false>(s, k, load(t), li, ri);
        if (own) Ns[(int64_t)(t + 1) * B] = (float)fmax(s.n, eps);
        roll(t + 1);
    }
}

}  // namespace cse

using namespace cse;

extern "C" void cse_imcra_default_params(cse_imcra_params_t* prm) {
    if (!prm) return;
    prm->alpha = 0.92;
    prm->alpha_s = 0.9;
    prm->alpha_d = 0.85;
    prm->beta = 1.47;
    prm->b_min = 1.66;
    prm->gamma0 = 4.6;
    prm->gamma1 = 3.0;
    prm->zeta0 = 1.67;
    prm->xi_min_db = -18.0;
    prm->sub_windows = 8;
    prm->sub_frames = 15;
}

extern "C" int cse_noise_imcra(const double* P, int64_t n_sig, int T, int B,
                               const cse_imcra_params_t* prm, double eps, float* N,
                               cse_stream_t stream) {
    CSE_CHECK_ARG(P != nullptr && N != nullptr && prm != nullptr,
                  "cse_noise_imcra: P, N or params is NULL");
    CSE_CHECK_ARG(n_sig >= 0 && T >= 1 && B >= 33 && B <= 2049,
                  "cse_noise_imcra: bad shape n_sig=%lld T=%d B=%d (B in [33, 2049])",
                  (long long)n_sig, T, B);
    // every range written so that NaN fails
    const double al[3] = {prm->alpha, prm->alpha_s, prm->alpha_d};
    for (int i = 0; i < 3; ++i)
        CSE_CHECK_ARG(al[i] >= 0.0 && al[i] < 1.0,
                      "cse_noise_imcra: alpha=%g alpha_s=%g alpha_d=%g not all in [0, 1)", al[0],
                      al[1], al[2]);
    const double pos[4] = {prm->beta, prm->b_min, prm->gamma0, prm->zeta0};
    for (int i = 0; i < 4; ++i)
        CSE_CHECK_ARG(pos[i] > 0.0 && isfinite(pos[i]),
                      "cse_noise_imcra: beta=%g b_min=%g gamma0=%g zeta0=%g not all finite and > 0",
                      pos[0], pos[1], pos[2], pos[3]);
    CSE_CHECK_ARG(prm->gamma1 > 1.0 && isfinite(prm->gamma1),
                  "cse_noise_imcra: gamma1=%g not finite and > 1", prm->gamma1);
    CSE_CHECK_ARG(isfinite(prm->xi_min_db), "cse_noise_imcra: xi_min_db=%g not finite",
                  prm->xi_min_db);
    CSE_CHECK_ARG(prm->sub_windows >= 1 && prm->sub_windows <= 16,
                  "cse_noise_imcra: sub_windows=%d not in [1, 16]", prm->sub_windows);
    CSE_CHECK_ARG(prm->sub_frames >= 1 && prm->sub_frames <= (1 << 20),
                  "cse_noise_imcra: sub_frames=%d not in [1, 2^20]", prm->sub_frames);
    const int nblk = ceil_div(B, IMCRA_BINS);
    CSE_CHECK_ARG(n_sig * nblk <= 0x7fffffffLL,
                  "cse_noise_imcra: n_sig=%lld too many for one launch", (long long)n_sig);
    if (n_sig == 0) return CSE_OK;
    // the base through a volatile: pow stays the library's pow (no exp10 in its place)
    volatile double ten = 10.0;
    ImcraK k;
    k.a = prm->alpha;
    k.c_a = 1.0 - prm->alpha;
    k.a_s = prm->alpha_s;
    k.c_s = 1.0 - prm->alpha_s;
    k.a_d = prm->alpha_d;
    k.c_d = 1.0 - prm->alpha_d;
    k.beta = prm->beta;
    k.b_min = prm->b_min;
    k.gamma0 = prm->gamma0;
    k.gamma1 = prm->gamma1;
    k.g1m1 = prm->gamma1 - 1.0;
    k.zeta0 = prm->zeta0;
    k.xi_min = pow(ten, prm->xi_min_db / 10.0);
    k.U = prm->sub_windows;
    k.V = prm->sub_frames;
    const size_t lds = (size_t)2 * k.U * 64 * sizeof(double);  // at most 16 KB
    hipLaunchKernelGGL(imcra_kernel, dim3((unsigned)(n_sig * nblk)), dim3(64), lds,
                       (hipStream_t)stream, P, T, B, nblk, k, eps, N);
    CSE_CHECK_LAUNCH("cse_noise_imcra");
    return CSE_OK;
}
