// Normalized covariance measure and its band-importance form
// (include/cse_ncm.h) on device.
//
// The frames, the transform and the 25 critical-band sums are fwSegSNR's
// (cse_segfft.hpp; cse_segsnr.hip describes them): one workgroup per cell, one
// wave per frame, the cell's test signal staged in LDS a chunk of FCH
// consecutive frames at a time with the last W - hop samples carried over, so
// each sample comes from memory once per cell.  A frame leaves one row of 25
// band envelopes e_j[i] (f32) in LDS.
//
// An envelope sample E_m needs the rows of frames 4m .. 4m + 7, which cross
// the chunks, so the rows live in a ring of 2 FCH frames indexed by the frame
// number: a chunk's rows stay until the chunk after the next one is
// transformed, and the last seven rows a sample can reach back for are always
// there.  After a chunk's barrier, thread i < 25 of wave 0 owns band i: it
// forms every E_m whose eight frames are complete, in increasing m, in fp64,
// and adds to the band's three running sums (cxy, sy, syy) in registers.  The
// other waves wait at the next chunk's staging barrier meanwhile, which also
// orders these reads before the next chunk's rows are written.  No sum depends
// on timing, so a call repeats to the bit.
//
// The epilogue is wave 0's: the 25 transmission indices, the weights sxx^p and
// the two weighted sums as fp64 wave sums.  The exponent enters only here, so
// the clean side does not depend on it.
//
// The clean side (cse_ncm_prepare), fp64: one wave per frame leaves e_j[i] in
// the workspace; one workgroup per signal then walks m per band twice (the mean
// first) and stores dx[M][25], vx, sxx and the dead-band flags.  The cell
// kernel never transforms x.
#include <cmath>

#include "cse_segfft.hpp"

#include "../../include/cse_ncm.h"

namespace cse {
namespace ncm {

using namespace seg;

constexpr int PNT = 256;      // clean-side frame kernel: threads per workgroup
constexpr int PNW = PNT / 64;
constexpr int TAPS = 8;       // envelope low-pass
constexpr int DEC = 4;        // decimation
constexpr int RING = 2 * FCH; // rows of band envelopes kept in LDS
constexpr int RS = 32;        // row stride of the ring (25 bands)
constexpr double TINY = 7.8886090522101181e-31;  // 2^-100
constexpr double DEAD = 9.0949470177292824e-13;  // 2^-40
static_assert(FCH % DEC == 0 && FCH >= TAPS, "a sample reaches back less than one chunk");

// the articulation-index weight of band i (include/cse_csii.h)
__device__ __forceinline__ double band_importance(int i) {
    constexpr double A[NB] = {0.003, 0.003, 0.003, 0.007, 0.010, 0.016, 0.016, 0.017, 0.017,
                              0.022, 0.027, 0.028, 0.030, 0.032, 0.034, 0.035, 0.037, 0.036,
                              0.036, 0.033, 0.030, 0.029, 0.027, 0.026, 0.026};
    return A[i];
}

// g[d] = 0.5 (1 - cos(2 pi (d + 1) / 9))
__device__ __forceinline__ void taps(double (&g)[TAPS]) {
#pragma unroll
    for (int d = 0; d < TAPS; ++d) g[d] = 0.5 * (1.0 - cospi(2.0 * (double)(d + 1) / 9.0));
}

struct Layout {
    int64_t J, M;
    int64_t env, dx, vx, sxx, dead, total;  // byte offsets
};

static Layout layout(int64_t n_sig, int64_t len, int H) {
    Layout L;
    L.J = frames_of(len, H / 16 * 15 / 4);
    L.M = L.J >= TAPS ? (L.J - TAPS) / DEC + 1 : 0;
    L.env = 0;                                        // f64 [n_sig][J][NB]
    L.dx = up256(n_sig * L.J * NB * 8);               // f64 [n_sig][M][NB]
    L.vx = L.dx + up256(n_sig * L.M * NB * 8);        // f64 [n_sig][RS]
    L.sxx = L.vx + up256(n_sig * RS * 8);             // f64 [n_sig][RS]
    L.dead = L.sxx + up256(n_sig * RS * 8);           // int [n_sig][RS]: 1 = the band does not move
    L.total = L.dead + up256(n_sig * RS * 4);
    return L;
}

// ---------------------------------------------------------------------------
// clean side
// ---------------------------------------------------------------------------
template <int H>
__global__ void __launch_bounds__(PNT) ncm_frames_kernel(const double* __restrict__ x, int64_t len,
                                                         int64_t J, Bands bands,
                                                         double* __restrict__ env) {
    using C = Cfg<H>;
    __shared__ cx<double> buf[PNW][C::BUF];
    __shared__ double wnd[C::W];
    __shared__ double fv[NB * FWP];
    __shared__ int flo[32], fn[32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < C::W; i += PNT) {  // hann_fill, written out (see there)
        double s, c;
        sincospi(2.0 * (double)(i + 1) / (double)(C::W + 1), &s, &c);
        wnd[i] = 0.5 * (1.0 - c);
    }
    stage_filters<double>(bands, H, fv, flo, fn, tid, PNT);
    __syncthreads();
    const int64_t f = (int64_t)blockIdx.x * PNW + wave;
    if (f >= J) return;  // wave-uniform; no workgroup barrier below
    const int64_t sig = blockIdx.y;
    const double* xs = x + sig * len + f * C::HOP;
    Twiddles<double, H> tw;
    tw.init(lane);
    cx<double> v[C::R];
#pragma unroll
    for (int q = 0; q < C::R; ++q) {
        v[q] = {0.0, 0.0};
        if (q < C::NIN) {
            const int n = lane + 64 * q;
            if (n < C::W / 2) v[q] = {xs[2 * n] * wnd[2 * n], xs[2 * n + 1] * wnd[2 * n + 1]};
        }
    }
    wave_fft<double, H>(buf[wave], v, tw, lane);
    wave_powers<double, H>(buf[wave], tw, lane);
    const double acc = wave_band<double>((const double*)buf[wave], fv, flo, fn, lane);
    if (lane < NB) env[(sig * J + f) * NB + lane] = sqrt(acc);
}

// One workgroup of one wave per signal; thread i < 25 walks band i's envelope
// samples in increasing m, twice: the mean, then dx, vx and sxx.
__global__ void __launch_bounds__(64) ncm_stats_kernel(const double* __restrict__ env, int64_t J,
                                                       int64_t M, double* __restrict__ dx,
                                                       double* __restrict__ vx,
                                                       double* __restrict__ sxx,
                                                       int* __restrict__ dead) {
    const int i = threadIdx.x;
    const int64_t sig = blockIdx.x;
    if (i >= NB) {
        if (i < RS) {
            vx[sig * RS + i] = 0.0;
            sxx[sig * RS + i] = 0.0;
            dead[sig * RS + i] = 1;
        }
        return;
    }
    double g[TAPS];
    taps(g);
    const double* e = env + sig * J * NB + i;
    double* d = dx + sig * M * NB + i;
    double sum = 0.0;
    for (int64_t m = 0; m < M; ++m) {
        double E = 0.0;
#pragma unroll
        for (int t = 0; t < TAPS; ++t) E += g[t] * e[(DEC * m + t) * NB];
        d[m * NB] = E;
        sum += E;
    }
    const double mu = sum / (double)M;
    double v = 0.0, s = 0.0;
    for (int64_t m = 0; m < M; ++m) {
        const double E = d[m * NB], dd = E - mu;
        d[m * NB] = dd;
        v += dd * dd;
        s += E * E;
    }
    vx[sig * RS + i] = v;
    sxx[sig * RS + i] = s;
    dead[sig * RS + i] = v > DEAD * s ? 0 : 1;
}

// ---------------------------------------------------------------------------
// cells
// ---------------------------------------------------------------------------
struct CellArgs {
    const float* y;
    const int64_t* y_offset;
    const int32_t* lag;
    const int32_t* sig_of;
    int64_t len, J, M;
    int clip;
    double p;
    Bands bands;
    const double* dx;
    const double* vx;
    const double* sxx;
    const int* dead;
    double* out;
};

template <int H>
__global__ void __launch_bounds__(NT, 4) ncm_cells_kernel(CellArgs a) {
    using C = Cfg<H>;
    __shared__ cx<float> buf[NW][C::BUF];
    __shared__ __attribute__((aligned(8))) float sy[C::SPAN];
    __shared__ __attribute__((aligned(8))) float wnd[C::W];
    __shared__ float fv[NB * FWP];
    __shared__ int flo[32], fn[32];
    __shared__ float ring[RING * RS];  // e_j[i] of frame j at row j % RING
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t cell = blockIdx.x;
    const double nan = quiet_nan();
    if (a.M < 2) {  // uniform over the grid
        if (tid < 2) a.out[2 * cell + tid] = nan;
        return;
    }
    const int64_t sig = a.sig_of[cell];
    const int lag = a.lag ? a.lag[cell] : 0;
    const float* yc = a.y + a.y_offset[cell];
    const bool clip = a.clip != 0;
    hann_fill(wnd, C::W, tid, NT);
    stage_filters<float>(a.bands, H, fv, flo, fn, tid, NT);
    Twiddles<float, H> tw;
    tw.init(lane);
    // thread i < 25: the running sums of band i and the next sample to form
    double g[TAPS];
    taps(g);
    double cxy = 0.0, sum_y = 0.0, syy = 0.0;
    int64_t m = 0;
    const double* dxs = a.dx + sig * a.M * NB + tid;
    for (int64_t f0 = 0; f0 < a.J; f0 += FCH) {
        const int nf = (int)((a.J - f0) < FCH ? (a.J - f0) : FCH);
        const int span = (nf - 1) * C::HOP + C::W;
        const int64_t base = f0 * C::HOP;
        int start = 0;
        if (f0 > 0) {  // the previous chunk was a full one: keep its last W - hop samples
            float cy = 0.0f;
            if (tid < C::CARRY) cy = sy[FCH * C::HOP + tid];
            __syncthreads();
            if (tid < C::CARRY) sy[tid] = cy;
            start = C::CARRY;
        }
        for (int i = start + tid; i < span; i += NT)
            sy[i] = cell_sample(yc, base + i, a.len, lag, clip);
        __syncthreads();  // the samples (and, the first time, window and filters) are staged
        for (int fr = wave; fr < nf; fr += NW) {
            const int fs = fr * C::HOP;
            cx<float> v[C::R];
#pragma unroll
            for (int q = 0; q < C::R; ++q) {
                v[q] = {0.0f, 0.0f};
                if (q < C::NIN) {
                    const int n = lane + 64 * q;
                    if (n < C::W / 2) {
                        const float2 yy = *(const float2*)&sy[fs + 2 * n];
                        const float2 ww = *(const float2*)&wnd[2 * n];
                        v[q] = {yy.x * ww.x, yy.y * ww.y};
                    }
                }
            }
            wave_fft<float, H>(buf[wave], v, tw, lane);
            wave_powers<float, H>(buf[wave], tw, lane);
            const float acc = wave_band<float>((const float*)buf[wave], fv, flo, fn, lane);
            if (lane < NB) ring[(int)((f0 + fr) & (RING - 1)) * RS + lane] = sqrtf(acc);
            wave_sync();  // the powers are read before the next frame's pass 0 writes
        }
        __syncthreads();  // the chunk's rows are complete
        // the samples whose eight frames are now complete; they reach back at
        // most DEC frames into the previous chunk, whose rows the ring still
        // holds (read before the next chunk's staging barrier, rewritten after it)
        if (tid < NB) {
            const int64_t done = f0 + nf;
            for (; m < a.M && DEC * m + TAPS <= done; ++m) {
                double E = 0.0;
#pragma unroll
                for (int t = 0; t < TAPS; ++t)
                    E += g[t] * (double)ring[(int)((DEC * m + t) & (RING - 1)) * RS + tid];
                cxy += dxs[m * NB] * E;
                sum_y += E;
                syy += E * E;
            }
        }
    }
    if (wave != 0) return;  // no workgroup barrier below
    double ti = 0.0, s = 0.0;
    if (lane < NB) {
        const double vx = a.vx[sig * RS + lane];
        s = a.sxx[sig * RS + lane];
        const double vy = fmax(syy - sum_y * sum_y / (double)a.M, 0.0);
        double r2 = 0.0;
        if (a.dead[sig * RS + lane] == 0 && vy > DEAD * syy) r2 = fmin(cxy * cxy / (vx * vy), 1.0);
        const double snr = 10.0 * log10(fmax(r2, TINY) / fmax(1.0 - r2, TINY));
        ti = (fmin(fmax(snr, -15.0), 15.0) + 15.0) / 30.0;
    }
    const double wa = lane < NB ? band_importance(lane) : 0.0;
    const double wb = lane < NB ? pow(s, a.p) : 0.0;
    const double total = wave_sum(s);
    const double na = wave_sum(wa * ti), da = wave_sum(wa);
    const double nb = wave_sum(wb * ti), db = wave_sum(wb);
    if (lane == 0) {
        a.out[2 * cell] = total == 0.0 ? nan : na / da;
        a.out[2 * cell + 1] = total == 0.0 ? nan : nb / db;
    }
}

}  // namespace ncm
}  // namespace cse

using namespace cse;

extern "C" int64_t cse_ncm_workspace_bytes(int64_t n_sig, int64_t len, int sr) {
    const int H = half_bins(sr);
    if (!H || !sizes_ok(n_sig, len)) return -1;
    return ncm::layout(n_sig, len, H).total;
}

extern "C" int64_t cse_ncm_scratch_bytes(int64_t n_cells, int64_t len, int sr) {
    if (!half_bins(sr) || n_cells < 0 || len < 0) return -1;
    return 0;
}

extern "C" int cse_ncm_prepare(const double* clean, int64_t n_sig, int64_t len, int sr,
                               void* workspace, cse_stream_t stream) {
    CSE_CHECK_PREPARE_ARGS("cse_ncm_prepare", clean, n_sig, len, sr, workspace);
    const int H = half_bins(sr);
    const seg::Bands* sup = seg::band_table(H);
    CSE_CHECK_ARG(sup != nullptr, "cse_ncm_prepare: filter support too wide");
    const ncm::Layout L = ncm::layout(n_sig, len, H);
    if (L.M < 2) return CSE_OK;  // no score: the cell kernel reads nothing of the workspace
    unsigned char* ws = (unsigned char*)workspace;
    double* env = (double*)(ws + L.env);
    double* dx = (double*)(ws + L.dx);
    double* vx = (double*)(ws + L.vx);
    double* sxx = (double*)(ws + L.sxx);
    int* dead = (int*)(ws + L.dead);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((L.J + ncm::PNW - 1) / ncm::PNW), (unsigned)n_sig);
    if (H == 512)
        hipLaunchKernelGGL(ncm::ncm_frames_kernel<512>, grid, dim3(ncm::PNT), 0, st, clean, len, L.J,
                           *sup, env);
    else
        hipLaunchKernelGGL(ncm::ncm_frames_kernel<256>, grid, dim3(ncm::PNT), 0, st, clean, len, L.J,
                           *sup, env);
    hipLaunchKernelGGL(ncm::ncm_stats_kernel, dim3((unsigned)n_sig), dim3(64), 0, st,
                       (const double*)env, L.J, L.M, dx, vx, sxx, dead);
    CSE_CHECK_LAUNCH("cse_ncm_prepare");
    return CSE_OK;
}

extern "C" int cse_ncm_cells(const float* y, const int64_t* y_offset, const int32_t* lag,
                             const int32_t* sig_of, int64_t n_cells, int64_t n_sig, int64_t len,
                             int sr, int clip, const void* workspace, void* scratch,
                             double bif_power, double* ncm_out, cse_stream_t stream) {
    (void)scratch;
    CSE_CHECK_CELLS_ARGS("cse_ncm_cells", y && y_offset && sig_of && workspace && ncm_out, n_cells,
                         n_sig, len, sr);
    const int H = half_bins(sr);
    CSE_CHECK_ARG(std::isfinite(bif_power) && bif_power >= 0.0,
                  "cse_ncm_cells: bif_power=%g (finite, >= 0)", bif_power);
    if (n_cells == 0) return CSE_OK;
    const seg::Bands* sup = seg::band_table(H);
    CSE_CHECK_ARG(sup != nullptr, "cse_ncm_cells: filter support too wide");
    const ncm::Layout L = ncm::layout(n_sig, len, H);
    const unsigned char* ws = (const unsigned char*)workspace;
    ncm::CellArgs a;
    a.bands = *sup;
    a.y = y;
    a.y_offset = y_offset;
    a.lag = lag;
    a.sig_of = sig_of;
    a.len = len;
    a.J = L.J;
    a.M = L.M;
    a.clip = clip;
    a.p = bif_power;
    a.dx = (const double*)(ws + L.dx);
    a.vx = (const double*)(ws + L.vx);
    a.sxx = (const double*)(ws + L.sxx);
    a.dead = (const int*)(ws + L.dead);
    a.out = ncm_out;
    hipStream_t st = (hipStream_t)stream;
    if (H == 512)
        hipLaunchKernelGGL(ncm::ncm_cells_kernel<512>, dim3((unsigned)n_cells), dim3(ncm::NT), 0, st,
                           a);
    else
        hipLaunchKernelGGL(ncm::ncm_cells_kernel<256>, dim3((unsigned)n_cells), dim3(ncm::NT), 0, st,
                           a);
    CSE_CHECK_LAUNCH("cse_ncm_cells");
    return CSE_OK;
}
