// Weighted spectral slope distance (include/cse_wss.h) on device.
//
// The frames, the transform and the 25 critical-band sums are fwSegSNR's
// (cse_segfft.hpp; cse_segsnr.hip describes them): one workgroup per cell, one
// wave per frame, the cell's test signal staged in LDS a chunk of FCH
// overlapping frames at a time.  WSS needs no clean samples, so only y is
// staged, and it takes the band sums of the power spectrum as it is, where
// fwSegSNR normalises the magnitudes.
//
// After the band sums lane i < 25 of a frame's wave holds E_i.  The slopes come
// from the neighbouring lane, and the nearest-peak rule needs no walk: with
// the rising steps (s_i > 0) of the 24 slopes as one ballot mask, a rising band
// finds the end of its run with a count of trailing ones above it, any other
// band the start of its run with a count of leading zeros below it, and P_i
// is one lane read.  The frame's two weighted sums over the 24 slopes are
// wave sums in fp64; their quotient is uniform over the wave and waits in LDS
// to run once per chunk, one frame per lane, like fwSegSNR's.
//
// Trimmed mean: a frame's value is kept as f32, in LDS while J <= NSEL, in the
// caller's scratch beyond.  The values are >= 0, so their bit patterns order
// like the values and trimmed_mean (cse_cells.hpp) applies: four passes of an
// 8-bit histogram find the n95-th smallest value t, and the sum of the n95
// smallest is the sum of the values below t plus the missing count times t.
// Silent frames hold +inf and are never reached.
//
// The clean side (cse_wss_prepare) runs the same frame code in fp64 and leaves
// per frame a 208-byte record: E_x[25], Wx[24] and the silent flag (f32).  The
// cell kernel never transforms x.
#include "cse_segfft.hpp"

#include "../../include/cse_wss.h"

namespace cse {
namespace wss {

using namespace seg;

constexpr int NS = NB - 1;    // slopes
constexpr int REC = 52;       // f32 words per frame record
constexpr int R_W = NB, R_SILENT = NB + NS;
constexpr int PNT = 256;      // clean-side kernel: threads per workgroup
constexpr int PNW = PNT / 64;
constexpr double E_FLOOR = 1e-10;

// E_i of the band sum e_i.  The product is rounded on its own: contracted into
// the slope's subtraction (fma(-10, log, E_next)) it leaves the product's
// rounding error as the slope between two bands at the floor, whose sign then
// decides the peak search where the header has a tie.
__device__ __forceinline__ float band_db(float e) {
#pragma clang fp contract(off)
    return 10.0f * log10f(fmaxf(e, (float)E_FLOOR));
}
__device__ __forceinline__ double band_db(double e) {
#pragma clang fp contract(off)
    return 10.0 * log10(fmax(e, E_FLOOR));
}

// Lane i < 25 of a wave holds E_i (lanes 32.. may mirror them; the others are
// ignored).  Returns W_i = Wmax_i Wloc_i and the slope s_i in lanes i < 24;
// what the other lanes get is finite index arithmetic on lanes < 32 and
// carries no meaning.  All 64 lanes call.
template <typename T>
__device__ __forceinline__ T slope_weight(T E, int lane, T& slope) {
    const int band = lane & 31;
    T mx = band < NB ? E : (T)-__builtin_inf();
#pragma unroll
    for (int o = 16; o >= 1; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
    slope = __shfl_down(E, 1, 64) - E;
    const bool rising = lane < NS && slope > (T)0;
    const unsigned mask = (unsigned)__ballot(rising);  // bit i: s_i > 0, i < 24; the rest 0
    int p;
    if (rising) {
        // the run of rising steps from i ends at the first clear bit n > i
        // (bit 24 is clear): P_i = E_{n-1}
        p = band + __ffs((int)~(mask >> band)) - 2;
    } else {
        // the run of other steps from i starts above the highest set bit n < i
        // (none: n = -1): P_i = E_{n+1}
        const unsigned below = mask & ((1u << band) - 1u);
        p = below ? 32 - __clz((int)below) : 0;
    }
    const T P = __shfl(E, p, 64);
    return ((T)20 / ((T)20 + (mx - E))) * ((T)1 / ((T)1 + (P - E)));
}

// ---------------------------------------------------------------------------
// clean side
// ---------------------------------------------------------------------------
struct Layout {
    int64_t J;
    int64_t ja, rec, total;  // byte offsets
};

static Layout layout(int64_t n_sig, int64_t len, int H) {
    Layout L;
    L.J = frames_of(len, H / 16 * 15 / 4);
    L.ja = 0;  // int ja, n95 per signal
    L.rec = up256(n_sig * 2 * 4);
    L.total = L.rec + up256(n_sig * L.J * REC * 4);
    return L;
}

template <int H>
__global__ void __launch_bounds__(PNT) wss_clean_kernel(const double* __restrict__ x, int64_t len,
                                                        int64_t J, Bands bands,
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
    stage_filters<double>(bands, H, fv, flo, fn, tid, PNT);
    __syncthreads();
    const int64_t f = (int64_t)blockIdx.x * PNW + wave;
    if (f >= J) return;  // wave-uniform; no workgroup barrier below
    const int64_t sig = blockIdx.y;
    const double* xs = x + sig * len + f * C::HOP;
    float* r = rec + (sig * J + f) * REC;
    Twiddles<double, H> tw;
    tw.init(lane);
    cx<double> v[C::R];
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
            }
        }
    }
    if (__ballot(nz) == 0) {  // silent
        if (lane < REC) r[lane] = lane == R_SILENT ? 1.0f : 0.0f;
        return;
    }
    wave_fft<double, H>(buf[wave], v, tw, lane);
    wave_powers<double, H>(buf[wave], tw, lane);
    const double E = band_db(wave_band<double>((const double*)buf[wave], fv, flo, fn, lane));
    double slope;
    const double wgt = slope_weight<double>(E, lane, slope);
    if (lane < NB) r[lane] = (float)E;
    if (lane < NS) r[R_W + lane] = (float)wgt;
    if (lane >= R_SILENT && lane < REC) r[lane] = 0.0f;
}

// ---------------------------------------------------------------------------
// cells
// ---------------------------------------------------------------------------
struct CellArgs {
    const float* y;
    const int64_t* y_offset;
    const int32_t* lag;
    const int32_t* sig_of;
    int64_t len, J, vstride;  // vstride: f32 values per cell in scratch
    int clip;
    Bands bands;
    const int* ja;
    const float* rec;
    float* scratch;
    double* wss;
};

template <int H>
__global__ void __launch_bounds__(NT, 4) wss_cells_kernel(CellArgs a) {
    using C = Cfg<H>;
    __shared__ cx<float> buf[NW][C::BUF];
    __shared__ __attribute__((aligned(8))) float sy[C::SPAN];
    __shared__ __attribute__((aligned(8))) float wnd[C::W];
    __shared__ float fv[NB * FWP];
    __shared__ int flo[32], fn[32];
    __shared__ float sv[NSEL];
    // per frame of the chunk: the two weighted sums (fnum -1: silent frame);
    // their fp64 quotient is uniform over the frame's wave and runs once per
    // chunk instead, one frame per lane of wave 0
    __shared__ double fnum[FCH], fden[FCH];
    __shared__ int silent[FCH];
    __shared__ __attribute__((aligned(16))) unsigned hist[256];
    __shared__ unsigned sh[2];
    __shared__ double red[NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t cell = blockIdx.x;
    const int64_t sig = a.sig_of[cell];
    const int ja = a.ja[2 * sig], n95 = a.ja[2 * sig + 1];
    if (a.J < 1 || ja == 0) {  // uniform over the workgroup
        if (tid == 0) a.wss[cell] = quiet_nan();
        return;
    }
    const int lag = a.lag ? a.lag[cell] : 0;
    const float* yc = a.y + a.y_offset[cell];
    const bool clip = a.clip != 0;
    float* vals = a.J <= NSEL ? sv : a.scratch + cell * a.vstride;
    hann_fill(wnd, C::W, tid, NT);
    stage_filters<float>(a.bands, H, fv, flo, fn, tid, NT);
    Twiddles<float, H> tw;
    tw.init(lane);
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
        for (int i = start + tid; i < span; i += NT) sy[i] = cell_sample(yc, base + i, a.len, lag, clip);
        // the chunk's silent flags in one load
        if (tid < nf) silent[tid] = a.rec[(sig * a.J + f0 + tid) * REC + R_SILENT] != 0.0f ? 1 : 0;
        __syncthreads();
        for (int fr = wave; fr < nf; fr += NW) {
            if (silent[fr]) {  // wave-uniform
                if (lane == 0) fnum[fr] = -1.0;
                continue;
            }
            // the clean frame's record: lane i holds E_x[i], E_x[i + 1] and Wx[i]
            // (loaded under the transform)
            const float* r = a.rec + (sig * a.J + f0 + fr) * REC;
            const int bi = lane < NS ? lane : 0;
            const float ex0 = r[bi], ex1 = r[bi + 1], wx = r[R_W + bi];
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
            const float E = band_db(wave_band<float>((const float*)buf[wave], fv, flo, fn, lane));
            float slope;
            const float wy = slope_weight<float>(E, lane, slope);
            double num = 0.0, den = 0.0;
            if (lane < NS) {
                const float wt = 0.5f * (wx + wy);
                const float dd = (ex1 - ex0) - slope;
                num = (double)(wt * (dd * dd));
                den = (double)wt;
            }
            num = wave_sum(num);
            den = wave_sum(den);
            if (lane == 0) {
                fnum[fr] = num;
                fden[fr] = den;
            }
            wave_sync();  // the powers are read before the next frame's pass 0 writes
        }
        __syncthreads();
        // the frame values of the chunk (read before the next chunk's barrier,
        // written after it)
        if (tid < nf) {
            const double num = fnum[tid];
            vals[f0 + tid] = num >= 0.0 ? (float)(num / fden[tid]) : __uint_as_float(0x7f800000u);
        }
    }
    __syncthreads();  // the values are complete
    const double m = trimmed_mean<NT>(vals, a.J, (unsigned)n95, hist, sh, red, tid);
    if (tid == 0) a.wss[cell] = m;
}

}  // namespace wss
}  // namespace cse

using namespace cse;

extern "C" int64_t cse_wss_workspace_bytes(int64_t n_sig, int64_t len, int sr) {
    const int H = half_bins(sr);
    if (!H || n_sig < 0 || len < 0) return -1;
    return wss::layout(n_sig, len, H).total;
}

extern "C" int64_t cse_wss_scratch_bytes(int64_t n_cells, int64_t len, int sr) {
    const int H = half_bins(sr);
    if (!H || n_cells < 0 || len < 0) return -1;
    return n_cells * value_stride(wss::layout(1, len, H).J) * 4;
}

extern "C" int cse_wss_prepare(const double* clean, int64_t n_sig, int64_t len, int sr,
                               void* workspace, cse_stream_t stream) {
    CSE_CHECK_PREPARE_ARGS("cse_wss_prepare", clean, n_sig, len, sr, workspace);
    const int H = half_bins(sr);
    const seg::Bands* sup = seg::band_table(H);
    CSE_CHECK_ARG(sup != nullptr, "cse_wss_prepare: filter support too wide");
    const seg::Bands bands = *sup;
    const wss::Layout L = wss::layout(n_sig, len, H);
    unsigned char* ws = (unsigned char*)workspace;
    int* ja = (int*)(ws + L.ja);
    float* rec = (float*)(ws + L.rec);
    hipStream_t st = (hipStream_t)stream;
    if (L.J > 0) {
        CSE_CHECK_ARG((L.J + wss::PNW - 1) / wss::PNW <= 0x7fffffffLL,
                      "cse_wss_prepare: len too large");
        const dim3 grid((unsigned)((L.J + wss::PNW - 1) / wss::PNW), (unsigned)n_sig);
        if (H == 512)
            hipLaunchKernelGGL(wss::wss_clean_kernel<512>, grid, dim3(wss::PNT), 0, st, clean, len,
                               L.J, bands, rec);
        else
            hipLaunchKernelGGL(wss::wss_clean_kernel<256>, grid, dim3(wss::PNT), 0, st, clean, len,
                               L.J, bands, rec);
    }
    hipLaunchKernelGGL((count_active_kernel<float, wss::REC, wss::R_SILENT, true>),
                       dim3((unsigned)n_sig), dim3(256), 0, st, (const float*)rec, L.J, ja);
    CSE_CHECK_LAUNCH("cse_wss_prepare");
    return CSE_OK;
}

extern "C" int cse_wss_cells(const float* y, const int64_t* y_offset, const int32_t* lag,
                             const int32_t* sig_of, int64_t n_cells, int64_t n_sig, int64_t len,
                             int sr, int clip, const void* workspace, void* scratch, double* wss_out,
                             cse_stream_t stream) {
    CSE_CHECK_CELLS_ARGS("cse_wss_cells", y && y_offset && sig_of && workspace && wss_out, n_cells,
                         n_sig, len, sr);
    if (n_cells == 0) return CSE_OK;
    const int H = half_bins(sr);
    const wss::Layout L = wss::layout(n_sig, len, H);
    const int64_t vstride = value_stride(L.J);
    CSE_CHECK_ARG(vstride == 0 || scratch,
                  "cse_wss_cells: %lld frames need scratch (cse_wss_scratch_bytes)", (long long)L.J);
    const unsigned char* ws = (const unsigned char*)workspace;
    const seg::Bands* sup = seg::band_table(H);
    CSE_CHECK_ARG(sup != nullptr, "cse_wss_cells: filter support too wide");
    wss::CellArgs a;
    a.bands = *sup;
    a.y = y;
    a.y_offset = y_offset;
    a.lag = lag;
    a.sig_of = sig_of;
    a.len = len;
    a.J = L.J;
    a.vstride = vstride;
    a.clip = clip;
    a.ja = (const int*)(ws + L.ja);
    a.rec = (const float*)(ws + L.rec);
    a.scratch = (float*)scratch;
    a.wss = wss_out;
    hipStream_t st = (hipStream_t)stream;
    if (H == 512)
        hipLaunchKernelGGL(wss::wss_cells_kernel<512>, dim3((unsigned)n_cells), dim3(wss::NT), 0,
                           st, a);
    else
        hipLaunchKernelGGL(wss::wss_cells_kernel<256>, dim3((unsigned)n_cells), dim3(wss::NT), 0,
                           st, a);
    CSE_CHECK_LAUNCH("cse_wss_cells");
    return CSE_OK;
}
