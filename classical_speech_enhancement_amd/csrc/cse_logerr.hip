// Logarithmic estimation error of noise-PSD estimates (include/cse_logerr.h)
// on the device.
//
// logerr_reference_kernel: the first-order recursion R[t] = beta R[t-1] +
// (1 - beta) Pv[t].  One lane per (signal, bin), bins along threadIdx.x, so
// every frame row is read and written by consecutive lanes; serial over frames,
// every operation rounded on its own.  As in cse_mcra.hip a block of REF_U
// frames is loaded ahead of the dependent chain, and a workgroup is one wave
// (100 x 257 chains are about 500 waves for 1,024 SIMDs).
//
// logerr_frames_kernel: per element one f64 load of R, one f32 load of N, an
// fp64 division and an fp64 log10.  A workgroup of four waves takes one signal
// and FT consecutive frames and walks every row of that signal, so the frames'
// R is fetched from HBM once and found in cache by the later rows.  The rows
// of a signal are found on the device: each wave reads sig_of / t_stride 64
// rows at a time and takes the rows a ballot marks, in ascending order.  A wave
// owns whole frames (t = first + wave + NW j); lane l takes the bins
// bin_lo + l + 64 i in ascending i, BU of them loaded before the first is
// used, into one (o, u) accumulator pair, then a butterfly over the wave.  So
// Fo[t] and Fu[t] are summed in a shape fixed by the bin range alone, whatever
// else the launch holds.  They go to the scratch, [n_rows][T][2].
//
// logerr_rows_kernel: one workgroup per row sums the scratch over frames
// (lane l takes t0 + l + NT i, butterfly, the waves in order), divides, and
// writes the frame values.  Rows the header declares invalid are written NaN
// here and matched by no workgroup of the frames kernel.
#include "cse_common.hpp"

#include <math.h>

#include "../../include/cse_logerr.h"

namespace cse {
namespace logerr {

constexpr int REF_U = 8;   // frames per prefetch block of the reference kernel
constexpr int NT = 256;    // threads per workgroup of the two score kernels
constexpr int NW = NT / 64;
constexpr int FT = 16;     // frames per workgroup of the frames kernel
constexpr int BU = 4;      // bins in flight per lane

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// ---------------------------------------------------------------------------
// reference PSD
// ---------------------------------------------------------------------------
__device__ __forceinline__ double ref_step(double r, double p, double beta, double omb) {
#pragma clang fp contract(off)
    const double a = beta * r;
    const double c = omb * p;
    return a + c;
}

__global__ void __launch_bounds__(64) logerr_reference_kernel(const double* __restrict__ Pv, int T,
                                                              int B, int nblk, double beta,
                                                              double omb, double* __restrict__ R) {
    const int b = (int)(blockIdx.x % (unsigned)nblk) * 64 + (int)threadIdx.x;
    const int64_t sig = blockIdx.x / (unsigned)nblk;
    if (b >= B) return;
    const double* p = Pv + sig * (int64_t)T * B + b;
    double* r = R + sig * (int64_t)T * B + b;
    double acc = p[0];
    r[0] = acc;
    int t = 1;
    constexpr int U = REF_U;
    const int full = 1 + ((T - 1) / U) * U;  // frames [1, full) in whole blocks
    if (full > 1) {
        double nxt[U], cur[U];
#pragma unroll
        for (int u = 0; u < U; ++u) nxt[u] = p[(int64_t)(1 + u) * B];
        for (; t < full; t += U) {
#pragma unroll
            for (int u = 0; u < U; ++u) cur[u] = nxt[u];
            if (t + U < full) {  // uniform: the next block's loads run under this block's chain
#pragma unroll
                for (int u = 0; u < U; ++u) nxt[u] = p[(int64_t)(t + U + u) * B];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                acc = ref_step(acc, cur[u], beta, omb);
                r[(int64_t)(t + u) * B] = acc;
            }
        }
    }
    for (; t < T; ++t) {
        acc = ref_step(acc, p[(int64_t)t * B], beta, omb);
        r[(int64_t)t * B] = acc;
    }
}

// ---------------------------------------------------------------------------
// score, first kernel: Fo[t], Fu[t] of every valid row
// ---------------------------------------------------------------------------
// the header's element lines; o and u are added to the lane's sums
__device__ __forceinline__ void element(double r, float n, double floor, double& so, double& su) {
#pragma clang fp contract(off)
    const double rf = (r < floor) ? floor : r;
    const double nd = (double)n;
    const double nf = (nd < floor) ? floor : nd;
    const double q = rf / nf;
    const double d = 10.0 * log10(q);
    const double o = (d > 0.0) ? 0.0 : -d;
    const double u = (d < 0.0) ? 0.0 : d;
    so += o;
    su += u;
}

// one frame of one row: the wave's sums over the bins [lo, hi)
__device__ __forceinline__ void frame_sums(const double* __restrict__ Rt,
                                           const float* __restrict__ Nt, int lo, int hi, int lane,
                                           double floor, double& fo, double& fu) {
    double so = 0.0, su = 0.0;
    for (int b0 = lo + lane; b0 < hi; b0 += 64 * BU) {  // b0 < hi: the first bin is the lane's own
        double r[BU];
        float n[BU];
#pragma unroll
        for (int k = 0; k < BU; ++k) {
            const int b = b0 + 64 * k;
            const bool in = b < hi;
            r[k] = in ? Rt[b] : 1.0;
            n[k] = in ? Nt[b] : 1.0f;
        }
#pragma unroll
        for (int k = 0; k < BU; ++k) {
            if (b0 + 64 * k < hi) element(r[k], n[k], floor, so, su);
        }
    }
    fo = wave_sum(so);
    fu = wave_sum(su);
}

__global__ void __launch_bounds__(NT) logerr_frames_kernel(
    const double* __restrict__ R, int T, int B, int nfb, const float* __restrict__ N,
    const int64_t* __restrict__ n_offset, const int64_t* __restrict__ t_stride,
    const int32_t* __restrict__ sig_of, int64_t n_rows, double floor, int t0, int lo, int hi,
    double* __restrict__ F) {
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int sig = (int)(blockIdx.x / (unsigned)nfb);
    const int first = t0 + (int)(blockIdx.x % (unsigned)nfb) * FT;
    const int last = min(first + FT, T);  // frames [first, last), wave-uniform
    const double* Rs = R + (int64_t)sig * T * B;
    for (int64_t base = 0; base < n_rows; base += 64) {
        const int64_t mine = base + lane;
        bool take = false;
        if (mine < n_rows) {
            const int64_t st = t_stride[mine];
            take = sig_of[mine] == sig && (st == 0 || st == (int64_t)B);
        }
        uint64_t todo = __ballot(take);
        while (todo) {
            const int k = __ffsll((unsigned long long)todo) - 1;
            todo &= todo - 1;
            const int64_t row = base + k;  // wave-uniform
            const int64_t st = t_stride[row];
            const float* Nr = N + n_offset[row];
            double* Fr = F + row * (int64_t)T * 2;
            for (int t = first + wave; t < last; t += NW) {
                double fo, fu;
                frame_sums(Rs + (int64_t)t * B, Nr + (int64_t)t * st, lo, hi, lane, floor, fo, fu);
                if (lane == 0) {
                    Fr[2 * t] = fo;
                    Fr[2 * t + 1] = fu;
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------
// score, second kernel: the row's totals and frame values
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(NT) logerr_rows_kernel(
    const double* __restrict__ F, int T, int B, const int64_t* __restrict__ t_stride,
    const int32_t* __restrict__ sig_of, int64_t n_sig, int t0, double dnb, double dn,
    double* __restrict__ over, double* __restrict__ under, double* __restrict__ frame_over,
    double* __restrict__ frame_under) {
    __shared__ double red[NW][2];
    const int tid = (int)threadIdx.x;
    const int64_t row = blockIdx.x;
    const int64_t st = t_stride[row];
    const int32_t sg = sig_of[row];
    const bool valid = sg >= 0 && (int64_t)sg < n_sig && (st == 0 || st == (int64_t)B);  // uniform
    const double nan = __builtin_nan("");
    const double* Fr = F + row * (int64_t)T * 2;
    double so = 0.0, su = 0.0;
    for (int t = tid; t < T; t += NT) {
        double fo = nan, fu = nan;
        if (valid && t >= t0) {
            const double a = Fr[2 * t], c = Fr[2 * t + 1];
            so += a;
            su += c;
            fo = a / dnb;
            fu = c / dnb;
        }
        if (frame_over != nullptr) {
            frame_over[row * (int64_t)T + t] = fo;
            frame_under[row * (int64_t)T + t] = fu;
        }
    }
    so = wave_sum(so);
    su = wave_sum(su);
    if ((tid & 63) == 0) {
        red[tid >> 6][0] = so;
        red[tid >> 6][1] = su;
    }
    __syncthreads();
    if (tid == 0) {
        double a = red[0][0], c = red[0][1];
        for (int w = 1; w < NW; ++w) {
            a += red[w][0];
            c += red[w][1];
        }
        over[row] = valid ? a / dn : nan;
        under[row] = valid ? c / dn : nan;
    }
}

}  // namespace logerr
}  // namespace cse

using namespace cse;
using namespace cse::logerr;

extern "C" void cse_logerr_default_params(cse_logerr_params_t* prm, int B) {
    if (!prm) return;
    prm->floor = 1e-12;
    prm->t0 = 0;
    prm->bin_lo = 0;
    prm->bin_hi = B;
    prm->reserved = 0;
}

extern "C" int cse_logerr_reference(const double* Pv, int64_t n_sig, int T, int B, double beta,
                                    double* R, cse_stream_t stream) {
    CSE_CHECK_ARG(Pv != nullptr && R != nullptr, "cse_logerr_reference: Pv or R is NULL");
    CSE_CHECK_ARG(n_sig >= 0 && T >= 1 && B >= 33 && B <= 2049,
                  "cse_logerr_reference: bad shape n_sig=%lld T=%d B=%d (B in [33, 2049])",
                  (long long)n_sig, T, B);
    CSE_CHECK_ARG(beta >= 0.0 && beta < 1.0, "cse_logerr_reference: beta=%g not in [0, 1)", beta);
    const int nblk = ceil_div(B, 64);
    CSE_CHECK_ARG(n_sig * nblk <= 0x7fffffffLL,
                  "cse_logerr_reference: n_sig=%lld too many for one launch", (long long)n_sig);
    if (n_sig == 0) return CSE_OK;
    hipLaunchKernelGGL(logerr_reference_kernel, dim3((unsigned)(n_sig * nblk)), dim3(64), 0,
                       (hipStream_t)stream, Pv, T, B, nblk, beta, 1.0 - beta, R);
    CSE_CHECK_LAUNCH("cse_logerr_reference");
    return CSE_OK;
}

extern "C" int64_t cse_logerr_scratch_bytes(int64_t n_rows, int T) {
    if (n_rows < 0 || T < 0) return -1;
    return n_rows * (int64_t)T * 2 * (int64_t)sizeof(double);
}

extern "C" int cse_logerr_rows(const double* R, int64_t n_sig, int T, int B, const float* N,
                               const int64_t* n_offset, const int64_t* t_stride,
                               const int32_t* sig_of, int64_t n_rows,
                               const cse_logerr_params_t* prm, void* scratch, double* over,
                               double* under, double* frame_over, double* frame_under,
                               cse_stream_t stream) {
    CSE_CHECK_ARG(R != nullptr && N != nullptr && n_offset != nullptr && t_stride != nullptr &&
                      sig_of != nullptr && prm != nullptr && over != nullptr && under != nullptr,
                  "cse_logerr_rows: R, N, a row table, params, over or under is NULL");
    CSE_CHECK_ARG((frame_over == nullptr) == (frame_under == nullptr),
                  "cse_logerr_rows: frame_over and frame_under must both be given or both NULL");
    CSE_CHECK_ARG(n_sig >= 0 && n_rows >= 0 && T >= 1 && B >= 33 && B <= 2049,
                  "cse_logerr_rows: bad shape n_sig=%lld n_rows=%lld T=%d B=%d (B in [33, 2049])",
                  (long long)n_sig, (long long)n_rows, T, B);
    CSE_CHECK_ARG(prm->floor > 0.0 && prm->floor <= 1.7976931348623157e308,
                  "cse_logerr_rows: floor=%g not finite and > 0", prm->floor);
    CSE_CHECK_ARG(prm->t0 >= 0 && prm->t0 < T, "cse_logerr_rows: t0=%d outside [0, %d)", prm->t0, T);
    CSE_CHECK_ARG(prm->bin_lo >= 0 && prm->bin_lo < prm->bin_hi && prm->bin_hi <= B,
                  "cse_logerr_rows: bins [%d, %d) empty or outside [0, %d]", prm->bin_lo,
                  prm->bin_hi, B);
    const int nfb = ceil_div(T - prm->t0, FT);
    CSE_CHECK_ARG(n_sig * nfb <= 0x7fffffffLL && n_rows <= 0x7fffffffLL,
                  "cse_logerr_rows: n_sig=%lld or n_rows=%lld too many for one launch",
                  (long long)n_sig, (long long)n_rows);
    if (n_rows == 0 || n_sig == 0) return CSE_OK;
    CSE_CHECK_ARG(scratch != nullptr, "cse_logerr_rows: scratch is NULL");
    const double dnb = (double)(prm->bin_hi - prm->bin_lo);
    const double dn = (double)((int64_t)(T - prm->t0) * (prm->bin_hi - prm->bin_lo));
    double* F = (double*)scratch;
    hipLaunchKernelGGL(logerr_frames_kernel, dim3((unsigned)(n_sig * nfb)), dim3(NT), 0,
                       (hipStream_t)stream, R, T, B, nfb, N, n_offset, t_stride, sig_of, n_rows,
                       prm->floor, (int)prm->t0, (int)prm->bin_lo, (int)prm->bin_hi, F);
    CSE_CHECK_LAUNCH("cse_logerr_rows (frames)");
    hipLaunchKernelGGL(logerr_rows_kernel, dim3((unsigned)n_rows), dim3(NT), 0, (hipStream_t)stream,
                       (const double*)F, T, B, t_stride, sig_of, n_sig, (int)prm->t0, dnb, dn, over,
                       under, frame_over, frame_under);
    CSE_CHECK_LAUNCH("cse_logerr_rows (rows)");
    return CSE_OK;
}
