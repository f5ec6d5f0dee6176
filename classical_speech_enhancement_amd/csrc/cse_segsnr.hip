// Segmental SNR and frequency-weighted segmental SNR (include/cse_segsnr.h) on
// device.
//
// One workgroup per cell, one wave per frame.  The frames overlap by 75 %, so
// the cell's test signal (shifted by its lag, clipped) and the f32 clean
// samples are staged in LDS a chunk of FCH frames at a time; the last
// W - hop samples of a chunk are carried over inside LDS, so each sample
// comes from memory once per cell.  (Fetching the next chunk into registers
// under the transforms was tried: 34 spilled VGPRs, 11.3 against 7.4 ms.)
//
// The NFFT-point transform of the real, zero-padded windowed frame f is an
// H-point complex transform (H = NFFT / 2) of z[n] = f[2n] + i f[2n+1] plus the
// real-FFT split.  z has W / 2 non-zero entries (240 of 512).  The H-point
// transform is a Stockham autosort FFT with H / 64 values per lane: three
// radix-8 passes at H = 512, four radix-4 passes at H = 256, exchanged through
// a padded per-wave LDS buffer; a lane's twiddles do not depend on the frame
// and stay in registers.  The first pass reads the staged samples directly
// (its upper inputs are the zero padding: constants to the compiler).
//
// Band product: the 25 filter rows have 7 to 29 non-zero entries (357 of
// 12,800); a band is summed over its support by two lanes, half each.
//
// What is uniform over a frame's wave in fp64 (the logarithm of segSNR, the
// divisions) waits in LDS and runs once per chunk, one frame per lane.
//
// The clean side (cse_segsnr_prepare) runs the same frame code in fp64 and
// leaves per frame a 224-byte record: ce[25], Wt[25], sum Wt, the silent flag
// (f32) and s (f64).  The cell kernel never transforms x.
//
// The frame code itself (transform, magnitudes, band sums, filter table) is in
// cse_segfft.hpp, shared with cse_wss.hip, cse_csii.hip and cse_ncm.hip; the
// window, the cell samples, the frame count and the entry points' checks are
// in cse_cells.hpp, shared with cse_lpc.hip as well.
#include "cse_segfft.hpp"

#include "../../include/cse_segsnr.h"

namespace cse {
namespace seg {

constexpr int REC = 56;       // f32 words per frame record
constexpr int R_SUMW = 50, R_SILENT = 51, R_S = 52;
constexpr int PNT = 256;      // clean-side kernel: threads per workgroup
constexpr int PNW = PNT / 64;
constexpr double EPS = 2.220446049250313e-16;  // 2^-52
constexpr double LO = -10.0, HI = 35.0;

// ---------------------------------------------------------------------------
// clean side
// ---------------------------------------------------------------------------
struct Layout {
    int64_t J;
    int64_t filt, ja, x32, rec, total;  // byte offsets
};

static Layout layout(int64_t n_sig, int64_t len, int H) {
    Layout L;
    L.J = frames_of(len, H / 16 * 15 / 4);
    L.filt = 0;  // int lo[32], int n[32], float vals[NB][FW]
    L.ja = up256(64 * 4 + NB * FW * 4);
    L.x32 = L.ja + up256(n_sig * 4);
    L.rec = L.x32 + up256(n_sig * len * 4);
    L.total = L.rec + up256(n_sig * L.J * REC * 4);
    return L;
}

__global__ void __launch_bounds__(1024) segsnr_filter_kernel(Bands b, int H, int* flo, int* fn,
                                                             float* fv) {
    const int t = threadIdx.x;
    if (t < 32) {
        flo[t] = t < NB ? b.lo[t] : 0;
        fn[t] = t < NB ? b.n[t] : 0;
    }
    for (int e = t; e < NB * FW; e += 1024) {
        const int i = e / FW, c = e % FW;
        fv[e] = c < b.n[i] ? (float)filter_entry(i, b.lo[i] + c, H) : 0.0f;
    }
}

__global__ void __launch_bounds__(256) segsnr_x32_kernel(const double* __restrict__ x, int64_t n,
                                                         float* __restrict__ x32) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) x32[i] = (float)x[i];
}

template <int H>
__global__ void __launch_bounds__(PNT) segsnr_clean_kernel(const double* __restrict__ x,
                                                           int64_t len, int64_t J, Bands bands,
                                                           float* __restrict__ rec) {
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
    if (tid < 32) {
        flo[tid] = tid < NB ? bands.lo[tid] : 0;
        fn[tid] = tid < NB ? bands.n[tid] : 0;
    }
    for (int e = tid; e < NB * FW; e += PNT) {
        const int i = e / FW, c = e % FW;
        fv[i * FWP + c] = c < bands.n[i] ? filter_entry(i, bands.lo[i] + c, H) : 0.0;
    }
    __syncthreads();
    const int64_t f = (int64_t)blockIdx.x * PNW + wave;
    if (f >= J) return;  // wave-uniform; no workgroup barrier below
    const int64_t sig = blockIdx.y;
    const double* xs = x + sig * len + f * C::HOP;
    float* r = rec + (sig * J + f) * REC;
    Twiddles<double, H> tw;
    tw.init(lane);
    cx<double> v[C::R];
    double sacc = 0.0;
    bool nz = false;
#pragma unroll
    for (int q = 0; q < C::R; ++q) {
        v[q] = {0.0, 0.0};
        if (q < C::NIN) {
            const int n = lane + 64 * q;
            if (n < C::W / 2) {
                const double a = xs[2 * n], b = xs[2 * n + 1];
                nz = nz || a != 0.0 || b != 0.0;
                v[q] = {a * wnd[2 * n], b * wnd[2 * n + 1]};
                sacc += v[q].x * v[q].x + v[q].y * v[q].y;
            }
        }
    }
    const bool silent = __ballot(nz) == 0;
    if (silent) {
        if (lane < REC) r[lane] = lane == R_SILENT ? 1.0f : 0.0f;
        return;
    }
    const double s = wave_sum(sacc);
    wave_fft<double, H>(buf[wave], v, tw, lane);
    const double sum = wave_sum(wave_magnitudes<double, H>(buf[wave], tw, lane));
    const double ce = wave_band<double>((const double*)buf[wave], fv, flo, fn, lane) / (sum + EPS);
    const double wt = pow(ce, 0.2);
    const double sumw = wave_sum(lane < NB ? wt : 0.0);
    if (lane < NB) {
        r[lane] = (float)ce;
        r[NB + lane] = (float)wt;
    }
    if (lane == 0) {
        r[R_SUMW] = (float)sumw;
        r[R_SILENT] = 0.0f;
        *(double*)(r + R_S) = s;
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
    const int* flo;
    const int* fn;
    const float* fv;
    const int* ja;
    const float* x32;
    const float* rec;
    double* seg;
    double* fw;
};

template <int H>
__global__ void __launch_bounds__(NT, 4) segsnr_cells_kernel(CellArgs a) {
    using C = Cfg<H>;
    __shared__ cx<float> buf[NW][C::BUF];
    __shared__ __attribute__((aligned(8))) float sy[C::SPAN];
    __shared__ __attribute__((aligned(8))) float sx[C::SPAN];
    __shared__ __attribute__((aligned(8))) float wnd[C::W];
    __shared__ float fv[NB * FWP];
    __shared__ int flo[32], fn[32];
    // per frame of the chunk: e (-1: silent frame) and the weighted band sum.
    // The fp64 logarithm and divisions of a frame are uniform over its wave;
    // they run once per chunk instead, one frame per lane of wave 0
    __shared__ double fe[FCH], fnum[FCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t cell = blockIdx.x;
    const int64_t sig = a.sig_of[cell];
    const int lag = a.lag ? a.lag[cell] : 0;
    const float* yc = a.y + a.y_offset[cell];
    const float* xc = a.x32 + sig * a.len;
    const bool clip = a.clip != 0, want_fw = a.fw != nullptr;
    hann_fill(wnd, C::W, tid, NT);
    if (tid < 32) {
        flo[tid] = a.flo[tid];
        fn[tid] = a.fn[tid];
    }
    for (int e = tid; e < NB * FW; e += NT) fv[e / FW * FWP + e % FW] = a.fv[e];
    Twiddles<float, H> tw;
    tw.init(lane);
    double seg_acc = 0.0, fw_acc = 0.0;  // thread t < FCH: the sums of frames t, t + FCH, ...
    for (int64_t f0 = 0; f0 < a.J; f0 += FCH) {
        const int nf = (int)((a.J - f0) < FCH ? (a.J - f0) : FCH);
        const int span = (nf - 1) * C::HOP + C::W;
        const int64_t base = f0 * C::HOP;
        int start = 0;
        if (f0 > 0) {  // the previous chunk was a full one: keep its last W - hop samples
            float cy = 0.0f, cxv = 0.0f;
            if (tid < C::CARRY) {
                cy = sy[FCH * C::HOP + tid];
                cxv = sx[FCH * C::HOP + tid];
            }
            __syncthreads();
            if (tid < C::CARRY) {
                sy[tid] = cy;
                sx[tid] = cxv;
            }
            start = C::CARRY;
        }
        for (int i = start + tid; i < span; i += NT) {
            sy[i] = cell_sample(yc, base + i, a.len, lag, clip);
            sx[i] = xc[base + i];
        }
        __syncthreads();
        for (int fr = wave; fr < nf; fr += NW) {
            const float* r = a.rec + (sig * a.J + f0 + fr) * REC;
            if (r[R_SILENT] != 0.0f) {  // wave-uniform
                if (lane == 0) fe[fr] = -1.0;
                continue;
            }
            const int fs = fr * C::HOP;
            cx<float> v[C::R];
            double eacc = 0.0;
#pragma unroll
            for (int q = 0; q < C::R; ++q) {
                v[q] = {0.0f, 0.0f};
                if (q < C::NIN) {
                    const int n = lane + 64 * q;
                    if (n < C::W / 2) {
                        const float2 yy = *(const float2*)&sy[fs + 2 * n];
                        const float2 xx = *(const float2*)&sx[fs + 2 * n];
                        const float2 ww = *(const float2*)&wnd[2 * n];
                        v[q] = {yy.x * ww.x, yy.y * ww.y};
                        // (x - y) w: one rounding of the difference, not two of the
                        // products it would cancel (frames near the 35 dB clamp)
                        const float d0 = (xx.x - yy.x) * ww.x, d1 = (xx.y - yy.y) * ww.y;
                        eacc += (double)(d0 * d0) + (double)(d1 * d1);
                    }
                }
            }
            const double e = wave_sum(eacc);
            if (lane == 0) fe[fr] = e;
            if (!want_fw) continue;
            wave_fft<float, H>(buf[wave], v, tw, lane);
            const double sum = wave_sum((double)wave_magnitudes<float, H>(buf[wave], tw, lane));
            const float acc = wave_band<float>((const float*)buf[wave], fv, flo, fn, lane);
            double num = 0.0;
            if (lane < NB) {
                const float pe = acc / (float)(sum + EPS);
                const float ce = r[lane], wt = r[NB + lane];
                const float dd = ce - pe;
                const float err = fmaxf(dd * dd, (float)EPS);
                const float snr = ce > 0.0f ? 10.0f * log10f(ce * ce / err) : 0.0f;
                num = (double)(wt * snr);
            }
            num = wave_sum(num);
            if (lane == 0) fnum[fr] = num;
            wave_sync();  // the magnitudes are read before the next frame's pass 0 writes
        }
        __syncthreads();
        // the frame values of the chunk (read before the next chunk's barrier,
        // written after it)
        if (tid < nf) {
            const double e = fe[tid];
            if (e >= 0.0) {
                const float* r = a.rec + (sig * a.J + f0 + tid) * REC;
                const double s = *(const double*)(r + R_S);
                const double sv = 10.0 * log10(s / (e + EPS) + EPS);
                seg_acc += fmin(fmax(sv, LO), HI);
                if (want_fw) {
                    const double fv_ = fnum[tid] / ((double)r[R_SUMW] + EPS);
                    fw_acc += fmin(fmax(fv_, LO), HI);
                }
            }
        }
    }
    if (wave != 0) return;  // no workgroup barrier below
    const double s0 = wave_sum(seg_acc), s1 = wave_sum(fw_acc);
    if (tid == 0) {
        const int ja = a.ja[sig];
        if (a.seg) a.seg[cell] = ja > 0 ? s0 / (double)ja : quiet_nan();
        if (a.fw) a.fw[cell] = ja > 0 ? s1 / (double)ja : quiet_nan();
    }
}

}  // namespace seg
}  // namespace cse

using namespace cse;

extern "C" int64_t cse_segsnr_workspace_bytes(int64_t n_sig, int64_t len, int sr) {
    const int H = half_bins(sr);
    if (!H || n_sig < 0 || len < 0) return -1;
    return seg::layout(n_sig, len, H).total;
}

extern "C" int64_t cse_segsnr_scratch_bytes(int64_t n_cells, int64_t len, int sr) {
    if (!half_bins(sr) || n_cells < 0 || len < 0) return -1;
    return 0;  // the cell kernel keeps its intermediates in LDS and registers
}

extern "C" int cse_segsnr_prepare(const double* clean, int64_t n_sig, int64_t len, int sr,
                                  void* workspace, cse_stream_t stream) {
    CSE_CHECK_PREPARE_ARGS("cse_segsnr_prepare", clean, n_sig, len, sr, workspace);
    const int H = half_bins(sr);
    seg::Bands bands;
    CSE_CHECK_ARG(seg::band_supports(H, &bands), "cse_segsnr_prepare: filter support too wide");
    const seg::Layout L = seg::layout(n_sig, len, H);
    unsigned char* ws = (unsigned char*)workspace;
    int* flo = (int*)(ws + L.filt);
    int* fn = flo + 32;
    float* fv = (float*)(fn + 32);
    int* ja = (int*)(ws + L.ja);
    float* x32 = (float*)(ws + L.x32);
    float* rec = (float*)(ws + L.rec);
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = n_sig * len;
    CSE_CHECK_ARG((n + 255) / 256 <= 0x7fffffffLL, "cse_segsnr_prepare: n_sig * len too large");
    hipLaunchKernelGGL(seg::segsnr_filter_kernel, dim3(1), dim3(1024), 0, st, bands, H, flo, fn, fv);
    hipLaunchKernelGGL(seg::segsnr_x32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                       clean, n, x32);
    if (L.J > 0) {
        const dim3 grid((unsigned)((L.J + seg::PNW - 1) / seg::PNW), (unsigned)n_sig);
        if (H == 512)
            hipLaunchKernelGGL(seg::segsnr_clean_kernel<512>, grid, dim3(seg::PNT), 0, st, clean,
                               len, L.J, bands, rec);
        else
            hipLaunchKernelGGL(seg::segsnr_clean_kernel<256>, grid, dim3(seg::PNT), 0, st, clean,
                               len, L.J, bands, rec);
    }
    hipLaunchKernelGGL((count_active_kernel<float, seg::REC, seg::R_SILENT, false>),
                       dim3((unsigned)n_sig), dim3(256), 0, st, (const float*)rec, L.J, ja);
    CSE_CHECK_LAUNCH("cse_segsnr_prepare");
    return CSE_OK;
}

extern "C" int cse_segsnr_cells(const float* y, const int64_t* y_offset, const int32_t* lag,
                                const int32_t* sig_of, int64_t n_cells, int64_t n_sig, int64_t len,
                                int sr, int clip, const void* workspace, void* scratch,
                                double* segsnr, double* fwsegsnr, cse_stream_t stream) {
    (void)scratch;
    CSE_CHECK_CELLS_ARGS("cse_segsnr_cells",
                         y && y_offset && sig_of && workspace && (segsnr || fwsegsnr), n_cells,
                         n_sig, len, sr);
    if (n_cells == 0) return CSE_OK;
    const int H = half_bins(sr);
    const seg::Layout L = seg::layout(n_sig, len, H);
    const unsigned char* ws = (const unsigned char*)workspace;
    seg::CellArgs a;
    a.y = y;
    a.y_offset = y_offset;
    a.lag = lag;
    a.sig_of = sig_of;
    a.len = len;
    a.J = L.J;
    a.clip = clip;
    a.flo = (const int*)(ws + L.filt);
    a.fn = a.flo + 32;
    a.fv = (const float*)(a.fn + 32);
    a.ja = (const int*)(ws + L.ja);
    a.x32 = (const float*)(ws + L.x32);
    a.rec = (const float*)(ws + L.rec);
    a.seg = segsnr;
    a.fw = fwsegsnr;
    hipStream_t st = (hipStream_t)stream;
    if (H == 512)
        hipLaunchKernelGGL(seg::segsnr_cells_kernel<512>, dim3((unsigned)n_cells), dim3(seg::NT), 0,
                           st, a);
    else
        hipLaunchKernelGGL(seg::segsnr_cells_kernel<256>, dim3((unsigned)n_cells), dim3(seg::NT), 0,
                           st, a);
    CSE_CHECK_LAUNCH("cse_segsnr_cells");
    return CSE_OK;
}
