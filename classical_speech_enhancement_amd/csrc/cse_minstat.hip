// Minimum-statistics noise-PSD tracking (include/cse_minstat.h; Martin 2001) on
// device.
//
// A frame cannot finish without all bins of its signal (the smoothing
// parameter and the bias correction hang on sums over the bins), so the unit
// of work is a signal: one workgroup per signal, the bins spread over its
// lanes, NPL bins per lane (bin = thread + j * threads: a frame row is read
// and written by consecutive lanes).  What every frame touches stays in
// registers: per bin p, sn2, pb, pb2, pminu, actmin, actminsub and the flag.
// The circular buffer of sub-window minima is touched once in V frames and
// lives in LDS, [slot][bin] so that consecutive lanes read consecutive doubles;
// a thread reads and writes its own bins only, so the buffer needs no barrier.
// At the largest B and U = 8 it is 140 KB of the CU's 160 KB.  Where U * B is
// beyond that (U >= 10 at B = 2049) the buffer is a register array of 16 slots
// instead, written by selects on the uniform slot number so that no index is
// dynamic; that variant spills at the large B it exists for and is the slow,
// correct path of a corner nobody is expected to visit.
//
// Two reductions sit on the serial chain of a frame: Sigma qe, and at the
// frame's end (Sigma p, Sigma sn2) for the next frame.  Sigma y of the next
// frame depends on the input alone and rides in that second reduction as a
// third value.  Within a wave a sum is DPP row operations and v_readlane (as
// in cse_segsnr.hip); across the waves each wave's lane 0 leaves its sum in
// LDS and, after one workgroup barrier, every thread adds the nw values in the
// same order, so all threads hold the same bits and every uniform quantity
// (ac, fl, bc, nsm, the sub-window counters) is computed redundantly per wave,
// once per frame and not once per bin, with no second barrier.  The two
// reductions use LDS slots of their own, which makes two barriers per frame
// enough.  A single-wave workgroup has no barrier and touches no LDS.
//
// pow is off the chain wherever its result cannot matter: fl = min(alpha_min,
// pow(snr, snr_exp)) is alpha_min for every snr below a threshold the host
// computes with a relative slack of 1e-9 (pow is monotone far within that), and
// only frames beyond it call pow.  The branch is uniform.
//
// Loads: a ring of PF frame rows per lane (4, or 2 from four bins per lane on);
// the row of frame t + PF is requested when frame t is taken from the ring, so
// the chain does not wait for memory.  The f32 stores wait for nothing.
#include "cse_common.hpp"

#include <float.h>
#include <math.h>

#include "../../include/cse_minstat.h"

namespace cse {
namespace ms {

#ifndef CSE_MINSTAT_NARROW
#define CSE_MINSTAT_NARROW 256
#endif
constexpr int MAXT = 512;                 // most threads per workgroup
// Up to MAX_NPL bins per lane a workgroup has at most this many threads, so
// that each of its waves has a SIMD of its own: every wave runs the frame's
// uniform part too, and two waves on one SIMD take turns at its fp64 pipe.
constexpr int NARROW = CSE_MINSTAT_NARROW;
constexpr int MAXW = 8;                   // most waves per workgroup
constexpr int MAX_NPL = 5;                // ceil(2049 / 512)
constexpr int UREG = 16;                  // slots of the register variant of the buffer
constexpr int64_t LDS_ROOM = 160 * 1024 - 1024;  // for the buffer, beside the reduction slots
static_assert(MAXT == 64 * MAXW && NARROW % 64 == 0 && NARROW >= 64 && NARROW <= MAXT,
              "whole waves, at most MAXW");

struct MsK {  // the header's host-side constants
    double alpha_c, c_c, ac_floor, alpha_max, alpha_min, snr_pow_from, beta_max, av;
    double q_lo, q_hi, nd, md2, nv, mv2, nb;
    int U, V;
};

struct MsRare {  // what only a frame in many reads: kept in LDS, not in SGPRs
    double snr_exp, slope_q[3], slope_max[4];
};

// Sum over the 64 lanes of a wave, all active; every lane gets the result
// (cse_segsnr.hip's: DPP within a row of 16 lanes, v_readlane for the rows).
// Every lane is active and every control used here reads a lane of the same
// row, so no lane keeps an old value: mov_dpp, which needs no zeroed target.
template <int CTRL>
__device__ __forceinline__ double dpp_add(double v) {
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xF, 0xF, true);
    return v + __hiloint2double(hi, lo);
}

__device__ __forceinline__ double row_sum_of(double v, int lane) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane),
                            __builtin_amdgcn_readlane(__double2loint(v), lane));
}

__device__ __forceinline__ double wave_sum(double v) {
    v = dpp_add<0xB1>(v);   // quad_perm [1, 0, 3, 2]
    v = dpp_add<0x4E>(v);   // quad_perm [2, 3, 0, 1]
    v = dpp_add<0x141>(v);  // row_half_mirror
    v = dpp_add<0x140>(v);  // row_mirror
    return (row_sum_of(v, 0) + row_sum_of(v, 16)) + (row_sum_of(v, 32) + row_sum_of(v, 48));
}

// Sums of NV values over the workgroup; every thread gets the same bits.
// red: NV * MAXW doubles of LDS that no other reduction in flight uses.
template <int NV>
__device__ __forceinline__ void block_sum(double (&v)[NV], double* red, int lane, int wave,
                                          int nw) {
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = wave_sum(v[i]);
    if (nw == 1) return;  // uniform
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) red[i * MAXW + wave] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        double s = red[i * MAXW];
        for (int w = 1; w < nw; ++w) s = s + red[i * MAXW + w];
        v[i] = s;
    }
}

// The circular buffer of sub-window minima of a thread's NPL bins.
template <int NPL, bool IN_LDS>
struct SubMin;

template <int NPL>
struct SubMin<NPL, true> {  // LDS: slot w of bin j at (w * NPL + j) * nt + tid
    double* base;
    int nt;
    __device__ __forceinline__ void init(double* lds, int tid, int nt_, int U, double inf) {
        base = lds + tid;
        nt = nt_;
        for (int i = 0; i < U * NPL; ++i) base[i * nt] = inf;
    }
    // v into slot ib; returns the minimum over the U slots
    __device__ __forceinline__ double store_min(int j, int ib, int U, double v, double inf) {
        base[(ib * NPL + j) * nt] = v;
        double m = inf;
        for (int w = 0; w < U; ++w) m = fmin(m, base[(w * NPL + j) * nt]);
        return m;
    }
    __device__ __forceinline__ void fill(int j, int U, bool up, double m) {
        if (up)
            for (int w = 0; w < U; ++w) base[(w * NPL + j) * nt] = m;
    }
};

template <int NPL>
struct SubMin<NPL, false> {  // registers: selects on the uniform slot number, no dynamic index
    double buf[NPL][UREG];
    __device__ __forceinline__ void init(double*, int, int, int, double inf) {
#pragma unroll
        for (int j = 0; j < NPL; ++j)
#pragma unroll
            for (int w = 0; w < UREG; ++w) buf[j][w] = inf;
    }
    __device__ __forceinline__ double store_min(int j, int ib, int, double v, double inf) {
        double m = inf;  // slots from U on stay +inf
#pragma unroll
        for (int w = 0; w < UREG; ++w) {
            buf[j][w] = w == ib ? v : buf[j][w];
            m = fmin(m, buf[j][w]);
        }
        return m;
    }
    __device__ __forceinline__ void fill(int j, int U, bool up, double m) {
#pragma unroll
        for (int w = 0; w < UREG; ++w) buf[j][w] = (up && w < U) ? m : buf[j][w];
    }
};

template <int NPL, bool IN_LDS>
__global__ void __launch_bounds__(MAXT) minstat_kernel(const double* __restrict__ P, int T, int B,
                                                       MsK k, MsRare kr, double eps,
                                                       float* __restrict__ N) {
#pragma clang fp contract(off)
#ifdef CSE_MINSTAT_PF  // for measurements of the ring's depth
    constexpr int PF = CSE_MINSTAT_PF;
#else
    constexpr int PF = NPL >= 4 ? 2 : 4;  // frames in the ring of prefetched rows
#endif
    __shared__ double red_a[MAXW], red_b[3 * MAXW];
    __shared__ MsRare rare;
    extern __shared__ double sub_lds[];  // U * NPL * threads doubles when IN_LDS
    const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
    const int lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
    const int64_t sig = blockIdx.x;
    const double* Ps = P + sig * (int64_t)T * B;
    float* Ns = N + sig * (int64_t)T * B;
    const double INF = __longlong_as_double(0x7ff0000000000000LL);
    const int U = k.U, V = k.V;
    if (tid == 0) rare = kr;
    __syncthreads();

    bool valid[NPL];
    int bin[NPL];
#pragma unroll
    for (int j = 0; j < NPL; ++j) {
        const int b = tid + j * nt;
        valid[j] = b < B;
        bin[j] = valid[j] ? b : 0;
    }
    // the ring of prefetched rows: ring[u] holds frame t with t % PF == u; rows
    // from T on and the lanes past B read as 0 (all of their state stays 0)
    double ring[PF][NPL];
#pragma unroll
    for (int u = 0; u < PF; ++u)
#pragma unroll
        for (int j = 0; j < NPL; ++j)
            ring[u][j] = (valid[j] && u < T) ? Ps[(int64_t)u * B + bin[j]] : 0.0;

    double p[NPL], sn2[NPL], pb[NPL], pb2[NPL], pminu[NPL], actmin[NPL], actminsub[NPL];
    SubMin<NPL, IN_LDS> sub;
    sub.init(sub_lds, tid, nt, U, INF);
    bool lmf[NPL];
    double s3[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < NPL; ++j) {
        p[j] = sn2[j] = pb[j] = pminu[j] = ring[0][j];
        pb2[j] = p[j] * p[j];
        actmin[j] = actminsub[j] = INF;
        lmf[j] = false;
        s3[0] = s3[0] + p[j];
    }
    s3[1] = s3[2] = s3[0];  // Sigma p = Sigma sn2 = Sigma y of frame 0
    block_sum<3>(s3, red_b, lane, wave, nw);
    double sp = s3[0], ss = s3[1], sy = s3[2];
    double ac = 1.0;
    int subwc = V, ib = -1;

    for (int t0 = 0; t0 < T; t0 += PF) {
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            const int t = t0 + u;
            if (t >= T) break;  // uniform
            double y[NPL];
#pragma unroll
            for (int j = 0; j < NPL; ++j) {
                y[j] = ring[u][j];
                ring[u][j] = (valid[j] && t + PF < T) ? Ps[(int64_t)(t + PF) * B + bin[j]] : 0.0;
            }
            // uniform over the frame
            const double r = sp / fmax(sy, DBL_MIN) - 1.0;
            const double acb = 1.0 / (1.0 + r * r);
            ac = k.alpha_c * ac + k.c_c * fmax(acb, k.ac_floor);
            const double snr = sp / fmax(ss, DBL_MIN);
            double fl = k.alpha_min;
            if (!(snr < k.snr_pow_from)) fl = fmin(k.alpha_min, pow(snr, rare.snr_exp));
            const double aa = k.alpha_max * ac;
            const double ql = k.q_lo / (double)(t + 1);
            double qe[NPL];
            double qs[1] = {0.0};
#pragma unroll
            for (int j = 0; j < NPL; ++j) {
                const double g = p[j] / fmax(sn2[j], DBL_MIN) - 1.0;
                const double ah = fmax(aa / (1.0 + g * g), fl);
                p[j] = ah * p[j] + (1.0 - ah) * y[j];
                const double bt = fmin(ah * ah, k.beta_max);
                pb[j] = bt * pb[j] + (1.0 - bt) * p[j];
                pb2[j] = bt * pb2[j] + (1.0 - bt) * (p[j] * p[j]);
                const double s2 = fmax(sn2[j], DBL_MIN);
                const double var = pb2[j] - pb[j] * pb[j];
                qe[j] = fmax(fmin(var / fmax(2.0 * (s2 * s2), DBL_MIN), k.q_hi), ql);
                qs[0] = qs[0] + (valid[j] ? qe[j] : 0.0);
            }
            block_sum<1>(qs, red_a, lane, wave, nw);
            const double qav = qs[0] / k.nb;
            const double bc = 1.0 + k.av * sqrt(qav);
            bool kk[NPL];
#pragma unroll
            for (int j = 0; j < NPL; ++j) {
                const double iq = 1.0 / qe[j];
                const double bd = 1.0 + k.nd / (iq - k.md2);
                const double bv = 1.0 + k.nv / (iq - k.mv2);
                const double bcp = bc * p[j];
                const double c = bcp * bd;
                const double cs = bcp * bv;
                kk[j] = c < actmin[j];
                actmin[j] = kk[j] ? c : actmin[j];
                actminsub[j] = kk[j] ? cs : actminsub[j];
            }
            if (subwc > 1 && subwc < V) {
#pragma unroll
                for (int j = 0; j < NPL; ++j) {
                    lmf[j] = lmf[j] || kk[j];
                    pminu[j] = fmin(actminsub[j], pminu[j]);
                    sn2[j] = pminu[j];
                }
            } else if (subwc >= V) {
                ib = ib + 1 == U ? 0 : ib + 1;
                const double nsm = qav < rare.slope_q[0]   ? rare.slope_max[0]
                                   : qav < rare.slope_q[1] ? rare.slope_max[1]
                                   : qav < rare.slope_q[2] ? rare.slope_max[2]
                                                           : rare.slope_max[3];
#pragma unroll
                for (int j = 0; j < NPL; ++j) {
                    double m = sub.store_min(j, ib, U, actmin[j], INF);
                    const bool up = lmf[j] && !kk[j] && m < actminsub[j] &&
                                    actminsub[j] < nsm * m;
                    m = up ? actminsub[j] : m;
                    sub.fill(j, U, up, m);
                    pminu[j] = m;
                    lmf[j] = false;
                    actmin[j] = INF;
                }
                subwc = 0;
            }
            subwc += 1;
            // the frame's output, and the three sums the next frame starts from
            s3[0] = s3[1] = s3[2] = 0.0;
#pragma unroll
            for (int j = 0; j < NPL; ++j) {
                if (valid[j]) Ns[(int64_t)t * B + bin[j]] = (float)fmax(sn2[j], eps);
                s3[0] = s3[0] + p[j];
                s3[1] = s3[1] + sn2[j];
                s3[2] = s3[2] + ring[(u + 1) % PF][j];
            }
            block_sum<3>(s3, red_b, lane, wave, nw);
            sp = s3[0];
            ss = s3[1];
            sy = s3[2];
        }
    }
}

// Martin's M(D) (the header's table and interpolation)
static double m_of(int d) {
    static const int D[18] = {1, 2, 5, 8, 10, 15, 20, 30, 40, 60, 80, 120, 140, 160, 180, 220, 260,
                              300};
    static const double M[18] = {0.0,   0.26,  0.48, 0.58, 0.61, 0.668, 0.705, 0.762, 0.8,
                                 0.841, 0.865, 0.89, 0.9,  0.91, 0.92,  0.93,  0.935, 0.94};
    if (d >= D[17]) return M[17];
    for (int i = 0; i < 17; ++i) {
        if (d == D[i]) return M[i];
        if (d < D[i + 1]) {
            const double si = sqrt((double)D[i]), sj = sqrt((double)D[i + 1]);
            return M[i] + (si * sj / sqrt((double)d) - sj) * (M[i + 1] - M[i]) / (si - sj);
        }
    }
    return M[17];
}

// false: no such instantiation, or the LDS the buffer needs was refused
template <bool IN_LDS>
static bool launch(int npl, dim3 grid, dim3 block, size_t lds, hipStream_t st, const double* P,
                   int T, int B, const MsK& k, const MsRare& kr, double eps, float* N) {
    switch (npl) {
#define CSE_MS_CASE(n)                                                                          \
    case n:                                                                                     \
        if (lds > 48 * 1024 &&                                                                  \
            hipFuncSetAttribute((const void*)minstat_kernel<n, IN_LDS>,                         \
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=        \
                hipSuccess)                                                                     \
            return false;                                                                       \
        hipLaunchKernelGGL((minstat_kernel<n, IN_LDS>), grid, block, lds, st, P, T, B, k, kr,   \
                           eps, N);                                                             \
        return true;
        CSE_MS_CASE(1)
        CSE_MS_CASE(2)
        CSE_MS_CASE(3)
        CSE_MS_CASE(4)
        CSE_MS_CASE(5)
#undef CSE_MS_CASE
    }
    return false;
}

}  // namespace ms
}  // namespace cse

using namespace cse;

extern "C" void cse_minstat_default_params(cse_minstat_params_t* prm) {
    if (!prm) return;
    prm->alpha_c = 0.837;
    prm->alpha_c_floor = 0.7;
    prm->alpha_max = 0.98;
    prm->alpha_min = 0.548;
    prm->snr_exp = -0.125;
    prm->beta_max = 0.894;
    prm->av = 2.12;
    prm->q_eq_min = 2.0;
    prm->q_eq_max = 14.0;
    prm->slope_q[0] = 0.03;
    prm->slope_q[1] = 0.05;
    prm->slope_q[2] = 0.06;
    prm->slope_max[0] = 8.0;
    prm->slope_max[1] = 4.0;
    prm->slope_max[2] = 2.0;
    prm->slope_max[3] = 1.2;
    prm->sub_windows = 8;
    prm->sub_frames = 24;
}

extern "C" int cse_noise_minstat(const double* P, int64_t n_sig, int T, int B,
                                 const cse_minstat_params_t* prm, double eps, float* N,
                                 cse_stream_t stream) {
    CSE_CHECK_ARG(P != nullptr && N != nullptr && prm != nullptr,
                  "cse_noise_minstat: P, N or params is NULL");
    CSE_CHECK_ARG(n_sig >= 0 && T >= 1 && B >= 33 && B <= 2049,
                  "cse_noise_minstat: bad shape n_sig=%lld T=%d B=%d (B in [33, 2049])",
                  (long long)n_sig, T, B);
    // every range written so that NaN fails
    CSE_CHECK_ARG(prm->alpha_c >= 0.0 && prm->alpha_c < 1.0 && prm->alpha_c_floor >= 0.0 &&
                      prm->alpha_c_floor < 1.0 && prm->alpha_min >= 0.0 && prm->alpha_min < 1.0 &&
                      prm->beta_max >= 0.0 && prm->beta_max < 1.0,
                  "cse_noise_minstat: alpha_c=%g alpha_c_floor=%g alpha_min=%g beta_max=%g not all "
                  "in [0, 1)",
                  prm->alpha_c, prm->alpha_c_floor, prm->alpha_min, prm->beta_max);
    CSE_CHECK_ARG(prm->alpha_max > 0.0 && prm->alpha_max < 1.0,
                  "cse_noise_minstat: alpha_max=%g not in (0, 1)", prm->alpha_max);
    CSE_CHECK_ARG(isfinite(prm->snr_exp) && prm->snr_exp <= 0.0,
                  "cse_noise_minstat: snr_exp=%g not finite or > 0", prm->snr_exp);
    CSE_CHECK_ARG(isfinite(prm->av) && prm->av >= 0.0, "cse_noise_minstat: av=%g not finite or < 0",
                  prm->av);
    CSE_CHECK_ARG(prm->q_eq_min >= 2.0 && prm->q_eq_min <= prm->q_eq_max && isfinite(prm->q_eq_max),
                  "cse_noise_minstat: not 2 <= q_eq_min=%g <= q_eq_max=%g < inf", prm->q_eq_min,
                  prm->q_eq_max);
    CSE_CHECK_ARG(prm->slope_q[0] > 0.0 && prm->slope_q[0] < prm->slope_q[1] &&
                      prm->slope_q[1] < prm->slope_q[2] && isfinite(prm->slope_q[2]),
                  "cse_noise_minstat: slope_q=(%g, %g, %g) not positive and strictly increasing",
                  prm->slope_q[0], prm->slope_q[1], prm->slope_q[2]);
    for (int i = 0; i < 4; ++i)
        CSE_CHECK_ARG(isfinite(prm->slope_max[i]) && prm->slope_max[i] >= 1.0,
                      "cse_noise_minstat: slope_max[%d]=%g not finite or < 1", i,
                      prm->slope_max[i]);
    CSE_CHECK_ARG(prm->sub_windows >= 1 && prm->sub_windows <= 16,
                  "cse_noise_minstat: sub_windows=%d not in [1, 16]", prm->sub_windows);
    CSE_CHECK_ARG(prm->sub_frames >= 2 && prm->sub_frames <= (1 << 20),
                  "cse_noise_minstat: sub_frames=%d not in [2, 2^20]", prm->sub_frames);
    CSE_CHECK_ARG(n_sig <= 0x7fffffffLL, "cse_noise_minstat: n_sig=%lld too many for one launch",
                  (long long)n_sig);
    if (n_sig == 0) return CSE_OK;
    const int U = prm->sub_windows, V = prm->sub_frames;
    const double m_d = ms::m_of(U * V), m_v = ms::m_of(V);
    ms::MsK k;
    k.alpha_c = prm->alpha_c;
    k.c_c = 1.0 - prm->alpha_c;
    k.ac_floor = prm->alpha_c_floor;
    k.alpha_max = prm->alpha_max;
    k.alpha_min = prm->alpha_min;
    ms::MsRare kr;
    kr.snr_exp = prm->snr_exp;
    // below this snr pow(snr, snr_exp) exceeds alpha_min by more than pow's
    // error, so fl = alpha_min without the call (snr_exp <= 0: pow falls in snr)
    k.snr_pow_from = (prm->alpha_min == 0.0 || prm->snr_exp == 0.0)
                         ? HUGE_VAL
                         : pow(prm->alpha_min, 1.0 / prm->snr_exp) * (1.0 - 1e-9);
    k.beta_max = prm->beta_max;
    k.av = prm->av;
    k.q_lo = 1.0 / prm->q_eq_max;
    k.q_hi = 1.0 / prm->q_eq_min;
    k.nd = (2.0 * (double)(U * V - 1)) * (1.0 - m_d);
    k.md2 = 2.0 * m_d;
    k.nv = (2.0 * (double)(V - 1)) * (1.0 - m_v);
    k.mv2 = 2.0 * m_v;
    k.nb = (double)B;
    for (int i = 0; i < 3; ++i) kr.slope_q[i] = prm->slope_q[i];
    for (int i = 0; i < 4; ++i) kr.slope_max[i] = prm->slope_max[i];
    k.U = U;
    k.V = V;
    int npl = ceil_div(B, ms::NARROW);
    if (npl > ms::MAX_NPL) npl = ceil_div(B, ms::MAXT);
    const int nt = ceil_div(ceil_div(B, npl), 64) * 64;
    const dim3 grid((unsigned)n_sig), block((unsigned)nt);
    hipStream_t st = (hipStream_t)stream;
    const int64_t lds = (int64_t)U * npl * nt * (int64_t)sizeof(double);
    const bool ok = lds <= ms::LDS_ROOM
                        ? ms::launch<true>(npl, grid, block, (size_t)lds, st, P, T, B, k, kr, eps,
                                           N)
                        : ms::launch<false>(npl, grid, block, 0, st, P, T, B, k, kr, eps, N);
    if (!ok) {
        (void)hipGetLastError();
        set_error("cse_noise_minstat: B=%d U=%d: %d bins per lane (at most %d) or %lld bytes of "
                  "LDS refused", B, U, npl, ms::MAX_NPL, (long long)lds);
        return CSE_ELAUNCH;
    }
    CSE_CHECK_LAUNCH("cse_noise_minstat");
    return CSE_OK;
}
