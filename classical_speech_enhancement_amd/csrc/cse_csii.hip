// Three-level coherence speech intelligibility index and I3
// (include/cse_csii.h) on device.
//
// The frames, the transform and the 25 critical-band sums are fwSegSNR's
// (cse_segfft.hpp; cse_segsnr.hip describes them): one workgroup per cell, one
// wave per frame.  What differs is the order of the frames.  The coherence of a
// level is a quotient of sums over all frames of that level, and a frame's
// value needs the finished quotient, so a level takes two passes over its
// frames and the levels are handled one after the other:
//
//   pass 1  every wave transforms its frames of the level (t = wave, wave + NW,
//           ... in the level's list), keeps the spectrum complex (wave_split)
//           and adds X conj(Y) and |Y|^2 for its R bins per lane in registers;
//           the NW partial sums are then added in wave order through LDS, one
//           bin per thread, and MSC and 1 - MSC go to LDS;
//   pass 2  the same frames again: the transform, MSC |Y|^2 and (1 - MSC) |Y|^2
//           side by side in the wave's buffer, two band sums over the filter
//           supports, the 25 logarithms, and the weighted sum over the bands as
//           an fp64 wave sum; each wave adds its frames' values in list order
//           and the NW sums are added in wave order.
//
// No sum depends on timing, so a call repeats to the bit.  The frames of a
// level are not consecutive, so the test signal is not staged in chunks as
// fwSegSNR and WSS stage it: each wave reads its frame's 480 (240) samples
// from global memory, where neighbouring frames meet in the caches.
//
// The clean side (cse_csii_prepare), fp64: one workgroup per signal sums S and
// the frame energies, classifies the frames and writes their indices ordered
// by level (a ballot scan per level keeps the frame order inside a level); one
// workgroup per (signal, level) then transforms the level's frames, stores
// X_j as f32 complex for pass 1 and adds |X_j|^2 into Pxx in the same fixed
// order.  The cell kernel never transforms x.
#include "cse_segfft.hpp"

#include "../../include/cse_csii.h"

namespace cse {
namespace csii {

using namespace seg;

constexpr int NL = 3;         // levels: high, mid, low
constexpr int PNT = 256;      // clean-side kernels: threads per workgroup
constexpr int PNW = PNT / 64;
constexpr float TINY = 7.8886090522101181e-31f;  // 2^-100

// the articulation-index weight of band i
__device__ __forceinline__ double band_importance(int i) {
    constexpr double A[NB] = {0.003, 0.003, 0.003, 0.007, 0.010, 0.016, 0.016, 0.017, 0.017,
                              0.022, 0.027, 0.028, 0.030, 0.032, 0.034, 0.035, 0.037, 0.036,
                              0.036, 0.033, 0.030, 0.029, 0.027, 0.026, 0.026};
    return A[i];
}

struct Layout {
    int64_t J;
    int64_t nl, order, lvl, pxx, spec, total;  // byte offsets
};

static Layout layout(int64_t n_sig, int64_t len, int H) {
    Layout L;
    L.J = frames_of(len, H / 16 * 15 / 4);
    L.nl = 0;                                      // int n_high, n_mid, n_low, 0 per signal
    L.order = up256(n_sig * 4 * 4);                // int [n_sig][J]: frames ordered by level
    L.lvl = L.order + up256(n_sig * L.J * 4);      // int [n_sig][J]: level of each frame
    L.pxx = L.lvl + up256(n_sig * L.J * 4);        // f32 [n_sig][NL][H]
    L.spec = L.pxx + up256(n_sig * NL * H * 4);    // f32 complex [n_sig][J][H]
    L.total = L.spec + up256(n_sig * L.J * H * 8);
    return L;
}

// ---------------------------------------------------------------------------
// clean side
// ---------------------------------------------------------------------------
template <int H>
__global__ void __launch_bounds__(PNT) csii_levels_kernel(const double* __restrict__ x,
                                                          int64_t len, int64_t J,
                                                          int* __restrict__ nl,
                                                          int* __restrict__ lvl,
                                                          int* __restrict__ order) {
    using C = Cfg<H>;
    __shared__ double red[PNT];
    __shared__ int wtot[PNW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t sig = blockIdx.x;
    const double* xs = x + sig * len;
    double acc = 0.0;
    for (int64_t i = tid; i < len; i += PNT) acc += xs[i] * xs[i];
    red[tid] = acc;
    __syncthreads();
    for (int s = PNT / 2; s >= 1; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const double S = red[0];
    const double b = S * (double)C::W;
    int* lv = lvl + sig * J;
    int* ord = order + sig * J;
    for (int64_t j = wave; j < J; j += PNW) {
        const double* xf = xs + j * C::HOP;
        double e = 0.0;
#pragma unroll
        for (int q = 0; q < (C::W + 63) / 64; ++q) {
            const int n = lane + 64 * q;
            if (n < C::W) e += xf[n] * xf[n];
        }
        e = wave_sum(e);
        const double a = e * (double)len;
        int code = NL;  // in no level
        if (S > 0.0) {
            if (a >= b) code = 0;
            else if (a >= 0.1 * b) code = 1;
            else if (a >= 0.001 * b) code = 2;
        }
        if (lane == 0) lv[j] = code;
    }
    __syncthreads();  // the codes are complete
    int base = 0;
    for (int L = 0; L < NL; ++L) {
        int running = 0;
        for (int64_t j0 = 0; j0 < J; j0 += PNT) {
            const int64_t j = j0 + tid;
            const bool in = j < J && lv[j] == L;
            const unsigned long long m = __ballot(in);
            if (lane == 0) wtot[wave] = __popcll(m);
            __syncthreads();
            int off = running, tot = 0;
#pragma unroll
            for (int w = 0; w < PNW; ++w) {
                if (w < wave) off += wtot[w];
                tot += wtot[w];
            }
            if (in) ord[base + off + __popcll(m & ((1ull << lane) - 1ull))] = (int)j;
            running += tot;
            __syncthreads();  // wtot is rewritten by the next chunk
        }
        if (tid == 0) nl[4 * sig + L] = running;
        base += running;
    }
    if (tid == 0) nl[4 * sig + NL] = 0;
}

template <int H>
__global__ void __launch_bounds__(PNT) csii_clean_kernel(const double* __restrict__ x, int64_t len,
                                                         int64_t J, const int* __restrict__ nl,
                                                         const int* __restrict__ order,
                                                         cx<float>* __restrict__ spec,
                                                         float* __restrict__ pxx) {
    using C = Cfg<H>;
    __shared__ cx<double> buf[PNW][C::BUF];
    __shared__ double wnd[C::W];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int L = blockIdx.x;
    const int64_t sig = blockIdx.y;
    int base = 0;
    for (int l = 0; l < L; ++l) base += nl[4 * sig + l];
    const int n = nl[4 * sig + L];
    const int* ord = order + sig * J + base;
    for (int i = tid; i < C::W; i += PNT) {  // hann_fill, written out (see there)
        double s, c;
        sincospi(2.0 * (double)(i + 1) / (double)(C::W + 1), &s, &c);
        wnd[i] = 0.5 * (1.0 - c);
    }
    __syncthreads();
    Twiddles<double, H> tw;
    tw.init(lane);
    double p[C::R];
#pragma unroll
    for (int r = 0; r < C::R; ++r) p[r] = 0.0;
    for (int t = wave; t < n; t += PNW) {
        const int64_t j = ord[t];
        const double* xs = x + sig * len + j * C::HOP;
        cx<double> v[C::R];
#pragma unroll
        for (int q = 0; q < C::R; ++q) {
            v[q] = {0.0, 0.0};
            if (q < C::NIN) {
                const int i = lane + 64 * q;
                if (i < C::W / 2) v[q] = {xs[2 * i] * wnd[2 * i], xs[2 * i + 1] * wnd[2 * i + 1]};
            }
        }
        wave_fft<double, H>(buf[wave], v, tw, lane);
        cx<double> f[C::R];
        wave_split<double, H>(buf[wave], tw, lane, f);
        cx<float>* out = spec + (sig * J + j) * H;
#pragma unroll
        for (int r = 0; r < C::R; ++r) {
            p[r] += f[r].x * f[r].x + f[r].y * f[r].y;
            out[lane + 64 * r] = {(float)f[r].x, (float)f[r].y};
        }
        wave_sync();  // the spectrum is read before the next frame's pass 0 writes
    }
    double* pw = (double*)buf[wave];  // this wave's share of Pxx, H doubles
#pragma unroll
    for (int r = 0; r < C::R; ++r) pw[lane + 64 * r] = p[r];
    __syncthreads();
    for (int k = tid; k < H; k += PNT) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < PNW; ++w) s += ((const double*)buf[w])[k];
        pxx[(sig * NL + L) * H + k] = (float)s;
    }
}

// ---------------------------------------------------------------------------
// cells
// ---------------------------------------------------------------------------
struct CellArgs {
    const float* y;
    const int64_t* y_offset;
    const int32_t* lag;
    const int32_t* sig_of;
    int64_t len, J;
    int clip;
    Bands bands;
    const int* nl;
    const int* order;
    const float* pxx;
    const cx<float>* spec;
    double* csii;
};

// the windowed frame at sample fs of the cell's test signal, as pass 0's inputs
template <int H>
__device__ __forceinline__ void load_frame(cx<float> (&v)[Cfg<H>::R], const float* yc, int64_t fs,
                                           int64_t len, int lag, bool clip, const float* wnd,
                                           int lane) {
    using C = Cfg<H>;
#pragma unroll
    for (int q = 0; q < C::R; ++q) {
        v[q] = {0.0f, 0.0f};
        if (q < C::NIN) {
            const int n = lane + 64 * q;
            if (n < C::W / 2) {
                const float2 ww = *(const float2*)&wnd[2 * n];
                v[q] = {cell_sample(yc, fs + 2 * n, len, lag, clip) * ww.x,
                        cell_sample(yc, fs + 2 * n + 1, len, lag, clip) * ww.y};
            }
        }
    }
}

// Two waves per SIMD: pass 1 keeps a level's Pxy and Pyy (24 registers at
// H = 512) beside the transform's 16 values and 30 twiddles, and the compiler
// takes 226 (154) registers for it; bounded to 128 it spilled.
template <int H>
__global__ void __launch_bounds__(NT, 2) csii_cells_kernel(CellArgs a) {
    using C = Cfg<H>;
    static_assert(2 * C::BUF >= 2 * H, "two spectra of H floats in a wave's buffer");
    __shared__ cx<float> buf[NW][C::BUF];
    __shared__ __attribute__((aligned(8))) float wnd[C::W];
    __shared__ float fv[NB * FWP];
    __shared__ int flo[32], fn[32];
    __shared__ float msc[H], omm[H];  // MSC_L and 1 - MSC_L
    __shared__ double red[NW];
    __shared__ double score[NL];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t cell = blockIdx.x;
    const double nan = quiet_nan();
    if (a.J < 1) {  // uniform over the grid
        if (tid < 4) a.csii[4 * cell + tid] = nan;
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
    __syncthreads();
    // the band weight of lanes i and i + 32 (i < 25), and the weights' sum
    const int band = lane & 31;
    const double wgt = lane < NB ? band_importance(lane) : 0.0;
    const double wsum = wave_sum(wgt);
    int base = 0;
#pragma unroll 1
    for (int L = 0; L < NL; ++L) {
        const int n = a.nl[4 * sig + L];
        const int* ord = a.order + sig * a.J + base;
        base += n;
        if (n == 0) {  // uniform over the workgroup
            if (tid == 0) score[L] = nan;
            continue;
        }
        // pass 1: the cross spectrum and the test signal's power over the level
        cx<float> pxy[C::R];
        float pyy[C::R];
#pragma unroll
        for (int r = 0; r < C::R; ++r) {
            pxy[r] = {0.0f, 0.0f};
            pyy[r] = 0.0f;
        }
        for (int t = wave; t < n; t += NW) {
            const int64_t j = ord[t];
            cx<float> v[C::R];
            load_frame<H>(v, yc, j * C::HOP, a.len, lag, clip, wnd, lane);
            wave_fft<float, H>(buf[wave], v, tw, lane);
            cx<float> f[C::R];
            wave_split<float, H>(buf[wave], tw, lane, f);
            // the clean spectrum of the lane's bins
            const cx<float>* xs = a.spec + (sig * a.J + j) * H;
#pragma unroll
            for (int r = 0; r < C::R; ++r) {
                const cx<float> xk = xs[lane + 64 * r];
                // X conj(Y)
                pxy[r].x += xk.x * f[r].x + xk.y * f[r].y;
                pxy[r].y += xk.y * f[r].x - xk.x * f[r].y;
                pyy[r] += f[r].x * f[r].x + f[r].y * f[r].y;
            }
            wave_sync();  // the spectrum is read before the next frame's pass 0 writes
        }
        // the NW partial sums, added in wave order, one bin per thread
#pragma unroll
        for (int r = 0; r < C::R; ++r) buf[wave][lane + 64 * r] = pxy[r];
        __syncthreads();
        cx<float> sxy = {0.0f, 0.0f};
        if (tid < H) {
#pragma unroll
            for (int w = 0; w < NW; ++w) sxy = sxy + buf[w][tid];
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < C::R; ++r) ((float*)buf[wave])[lane + 64 * r] = pyy[r];
        __syncthreads();
        if (tid < H) {
            float syy = 0.0f;
#pragma unroll
            for (int w = 0; w < NW; ++w) syy += ((const float*)buf[w])[tid];
            // the quotient in fp64: the product of two f32 powers cannot underflow there
            const double den = (double)a.pxx[(sig * NL + L) * H + tid] * (double)syy;
            const double num = (double)sxy.x * (double)sxy.x + (double)sxy.y * (double)sxy.y;
            const double m = den == 0.0 ? 0.0 : fmin(num / den, 1.0);
            msc[tid] = (float)m;
            omm[tid] = (float)(1.0 - m);
        }
        __syncthreads();  // MSC is complete, and the partial sums are read
        // pass 2: the frame values
        double acc = 0.0;
        for (int t = wave; t < n; t += NW) {
            const int64_t j = ord[t];
            cx<float> v[C::R];
            load_frame<H>(v, yc, j * C::HOP, a.len, lag, clip, wnd, lane);
            wave_fft<float, H>(buf[wave], v, tw, lane);
            cx<float> f[C::R];
            wave_split<float, H>(buf[wave], tw, lane, f);
            wave_sync();
            float* m = (float*)buf[wave];
#pragma unroll
            for (int r = 0; r < C::R; ++r) {
                const int k = lane + 64 * r;
                const float pw = f[r].x * f[r].x + f[r].y * f[r].y;
                m[k] = msc[k] * pw;
                m[H + k] = omm[k] * pw;
            }
            wave_sync();
            const float num = wave_band<float>(m, fv, flo, fn, lane);
            const float den = wave_band<float>(m + H, fv, flo, fn, lane);
            const float q = num / fmaxf(den, TINY);
            const float sdr = fminf(fmaxf(10.0f * log10f(fmaxf(q, TINY)), -15.0f), 15.0f);
            const float T = (sdr + 15.0f) / 30.0f;
            // lanes 32.. mirror the bands; they carry weight 0
            const double c = wave_sum(band < NB ? wgt * (double)T : 0.0) / wsum;
            acc += c;
            wave_sync();  // the products are read before the next frame's pass 0 writes
        }
        if (lane == 0) red[wave] = acc;
        __syncthreads();
        if (tid == 0) {
            double total = 0.0;
#pragma unroll
            for (int w = 0; w < NW; ++w) total += red[w];
            score[L] = total / (double)n;
        }
        __syncthreads();  // red and the buffers are rewritten by the next level
    }
    if (tid == 0) {
        double* o = a.csii + 4 * cell;
        o[0] = score[0];
        o[1] = score[1];
        o[2] = score[2];
        // NaN when the mid or the low level is empty
        o[3] = 1.0 / (1.0 + exp(-(-3.47 + 1.84 * score[2] + 9.99 * score[1])));
    }
}

}  // namespace csii
}  // namespace cse

using namespace cse;

extern "C" int64_t cse_csii_workspace_bytes(int64_t n_sig, int64_t len, int sr) {
    const int H = half_bins(sr);
    if (!H || !sizes_ok(n_sig, len)) return -1;
    return csii::layout(n_sig, len, H).total;
}

extern "C" int64_t cse_csii_scratch_bytes(int64_t n_cells, int64_t len, int sr) {
    if (!half_bins(sr) || n_cells < 0 || len < 0) return -1;
    return 0;
}

extern "C" int cse_csii_prepare(const double* clean, int64_t n_sig, int64_t len, int sr,
                                void* workspace, cse_stream_t stream) {
    CSE_CHECK_PREPARE_ARGS("cse_csii_prepare", clean, n_sig, len, sr, workspace);
    const int H = half_bins(sr);
    const csii::Layout L = csii::layout(n_sig, len, H);
    unsigned char* ws = (unsigned char*)workspace;
    int* nl = (int*)(ws + L.nl);
    int* order = (int*)(ws + L.order);
    int* lvl = (int*)(ws + L.lvl);
    float* pxx = (float*)(ws + L.pxx);
    seg::cx<float>* spec = (seg::cx<float>*)(ws + L.spec);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(csii::NL, (unsigned)n_sig);
    if (H == 512) {
        hipLaunchKernelGGL(csii::csii_levels_kernel<512>, dim3((unsigned)n_sig), dim3(csii::PNT), 0,
                           st, clean, len, L.J, nl, lvl, order);
        hipLaunchKernelGGL(csii::csii_clean_kernel<512>, grid, dim3(csii::PNT), 0, st, clean, len,
                           L.J, (const int*)nl, (const int*)order, spec, pxx);
    } else {
        hipLaunchKernelGGL(csii::csii_levels_kernel<256>, dim3((unsigned)n_sig), dim3(csii::PNT), 0,
                           st, clean, len, L.J, nl, lvl, order);
        hipLaunchKernelGGL(csii::csii_clean_kernel<256>, grid, dim3(csii::PNT), 0, st, clean, len,
                           L.J, (const int*)nl, (const int*)order, spec, pxx);
    }
    CSE_CHECK_LAUNCH("cse_csii_prepare");
    return CSE_OK;
}

extern "C" int cse_csii_cells(const float* y, const int64_t* y_offset, const int32_t* lag,
                              const int32_t* sig_of, int64_t n_cells, int64_t n_sig, int64_t len,
                              int sr, int clip, const void* workspace, void* scratch,
                              double* csii_out, cse_stream_t stream) {
    (void)scratch;
    CSE_CHECK_CELLS_ARGS("cse_csii_cells", y && y_offset && sig_of && workspace && csii_out,
                         n_cells, n_sig, len, sr);
    if (n_cells == 0) return CSE_OK;
    const int H = half_bins(sr);
    const seg::Bands* sup = seg::band_table(H);
    CSE_CHECK_ARG(sup != nullptr, "cse_csii_cells: filter support too wide");
    const csii::Layout L = csii::layout(n_sig, len, H);
    const unsigned char* ws = (const unsigned char*)workspace;
    csii::CellArgs a;
    a.bands = *sup;
    a.y = y;
    a.y_offset = y_offset;
    a.lag = lag;
    a.sig_of = sig_of;
    a.len = len;
    a.J = L.J;
    a.clip = clip;
    a.nl = (const int*)(ws + L.nl);
    a.order = (const int*)(ws + L.order);
    a.pxx = (const float*)(ws + L.pxx);
    a.spec = (const seg::cx<float>*)(ws + L.spec);
    a.csii = csii_out;
    hipStream_t st = (hipStream_t)stream;
    if (H == 512)
        hipLaunchKernelGGL(csii::csii_cells_kernel<512>, dim3((unsigned)n_cells), dim3(csii::NT), 0,
                           st, a);
    else
        hipLaunchKernelGGL(csii::csii_cells_kernel<256>, dim3((unsigned)n_cells), dim3(csii::NT), 0,
                           st, a);
    CSE_CHECK_LAUNCH("cse_csii_cells");
    return CSE_OK;
}
