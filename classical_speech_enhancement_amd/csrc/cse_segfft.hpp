// The frame transform of the critical-band scores: what cse_segsnr.hip
// (fwSegSNR), cse_wss.hip (WSS) and cse_csii.hip (CSII) share.  All take the
// 30-ms frames of include/cse_segsnr.h, one wave per frame: the NFFT-point transform of the
// zero-padded windowed frame and the 25 critical-band sums over the filter
// supports.  The comments at the head of cse_segsnr.hip describe the scheme.
// What is not about the transform (window, cell samples, counts, checks) is in
// cse_cells.hpp.
#ifndef CSE_SEGFFT_HPP_
#define CSE_SEGFFT_HPP_

#include "cse_cells.hpp"

namespace cse {
namespace seg {

constexpr int NB = 25;        // critical bands
constexpr int FW = 32;        // room per filter row (widest support: 29)
constexpr int FWP = FW + 1;   // row stride of the LDS copy: the lanes of a band product read
                              // one row each, and a stride of 32 words is two banks for all
constexpr int NT = 512;       // cell kernels: threads per workgroup
constexpr int NW = NT / 64;
constexpr int FCH = 16;       // frames per staged chunk

struct Bands {  // support of each filter row: [lo, lo + n)
    int lo[NB];
    int n[NB];
};

template <int H>
struct Cfg {
    static constexpr int W = H / 16 * 15;        // 480 / 240
    static constexpr int HOP = W / 4;
    static constexpr int R = H == 512 ? 8 : 4;   // radix; also the values per lane (H / 64)
    static constexpr int P = H == 512 ? 3 : 4;   // passes
    static constexpr int NIN = (W / 2 + 63) / 64;  // non-zero inputs per lane in pass 0
    static constexpr int BUF = H + H / 8;        // padded complex entries per wave
    static constexpr int SPAN = (FCH - 1) * HOP + W;
    static constexpr int CARRY = W - HOP;
    static_assert(H == 512 || H == 256, "H is 512 (16 kHz) or 256 (8 kHz)");
    static_assert(CARRY <= NT, "one carried sample per thread");
};

template <typename T>
struct cx {
    T x, y;
};
template <typename T>
__device__ __forceinline__ cx<T> operator+(cx<T> a, cx<T> b) { return {a.x + b.x, a.y + b.y}; }
template <typename T>
__device__ __forceinline__ cx<T> operator-(cx<T> a, cx<T> b) { return {a.x - b.x, a.y - b.y}; }
template <typename T>
__device__ __forceinline__ cx<T> operator*(cx<T> a, cx<T> b) {
    return {a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x};
}
template <typename T>
__device__ __forceinline__ cx<T> mul_mi(cx<T> a) { return {a.y, -a.x}; }  // -i a

// forward DFT (e^{-2 pi i nk/R}) in registers, natural order in and out
template <typename T>
__device__ __forceinline__ void dft4(cx<T>& a0, cx<T>& a1, cx<T>& a2, cx<T>& a3) {
    const cx<T> b0 = a0 + a2, b2 = a0 - a2, b1 = a1 + a3, b3 = mul_mi(a1 - a3);
    a0 = b0 + b1;
    a2 = b0 - b1;
    a1 = b2 + b3;
    a3 = b2 - b3;
}

template <typename T>
__device__ __forceinline__ void dft(cx<T> (&v)[4]) { dft4(v[0], v[1], v[2], v[3]); }

template <typename T>
__device__ __forceinline__ void dft(cx<T> (&v)[8]) {
    constexpr T r2 = (T)0.70710678118654752440;
    // even outputs: DFT4 of v[n] + v[n+4]; odd: DFT4 of W8^n (v[n] - v[n+4])
    cx<T> e0 = v[0] + v[4], e1 = v[1] + v[5], e2 = v[2] + v[6], e3 = v[3] + v[7];
    cx<T> d0 = v[0] - v[4], c1 = v[1] - v[5], d2 = mul_mi(v[2] - v[6]), c3 = v[3] - v[7];
    cx<T> d1 = {r2 * (c1.x + c1.y), r2 * (c1.y - c1.x)};    // c1 (1 - i) / sqrt 2
    cx<T> d3 = {r2 * (c3.y - c3.x), -r2 * (c3.x + c3.y)};   // c3 (-1 - i) / sqrt 2
    dft4(e0, e1, e2, e3);
    dft4(d0, d1, d2, d3);
    v[0] = e0;
    v[2] = e1;
    v[4] = e2;
    v[6] = e3;
    v[1] = d0;
    v[3] = d1;
    v[5] = d2;
    v[7] = d3;
}

__device__ __forceinline__ int pad(int i) { return i + (i >> 3); }

// the per-lane constants of the transform: the twiddles of passes 1.. and of
// the real-FFT split for the lane's bins k = lane + 64 r
template <typename T, int H>
struct Twiddles {
    using C = Cfg<H>;
    cx<T> tw[C::P - 1][C::R - 1];
    cx<T> st0;  // e^{-2 pi i lane / NFFT}; bin lane + 64 r takes st0 e^{-pi i 64 r / H}
    __device__ __forceinline__ void init(int lane) {
        int ns = C::R;
#pragma unroll
        for (int p = 1; p < C::P; ++p) {
            const int k = lane % ns;
#pragma unroll
            for (int r = 1; r < C::R; ++r) {
                double s, c;
                sincospi(-2.0 * (double)(k * r) / (double)(ns * C::R), &s, &c);
                tw[p - 1][r - 1] = {(T)c, (T)s};
            }
            ns *= C::R;
        }
        double s, c;
        sincospi(-(double)lane / (double)H, &s, &c);
        st0 = {(T)c, (T)s};
    }
    // e^{-pi i 64 r / H}: sixteenths of a half turn, two per step at H = 256
    static __device__ __forceinline__ cx<T> step(int r) {
        constexpr T c1 = (T)0.92387953251128675613, s1 = (T)0.38268343236508977173;
        constexpr T r2 = (T)0.70710678118654752440;
        switch (r * (512 / H)) {
            case 0: return {(T)1, (T)0};
            case 1: return {c1, -s1};
            case 2: return {r2, -r2};
            case 3: return {s1, -c1};
            case 4: return {(T)0, (T)-1};
            case 5: return {-s1, -c1};
            case 6: return {-r2, -r2};
            default: return {-c1, -s1};  // 7
        }
    }
};

// H-point forward transform of one wave: v = the inputs z[lane + 64 r] of pass
// 0; the result is left in buf (padded index), natural order.
template <typename T, int H>
__device__ __forceinline__ void wave_fft(cx<T>* buf, cx<T> (&v)[Cfg<H>::R],
                                         const Twiddles<T, H>& tw, int lane) {
    using C = Cfg<H>;
    dft(v);
#pragma unroll
    for (int r = 0; r < C::R; ++r) buf[pad(lane * C::R + r)] = v[r];
    wave_sync();
    int ns = C::R;
#pragma unroll
    for (int p = 1; p < C::P; ++p) {
#pragma unroll
        for (int r = 0; r < C::R; ++r) v[r] = buf[pad(lane + 64 * r)];
        wave_sync();
#pragma unroll
        for (int r = 1; r < C::R; ++r) v[r] = v[r] * tw.tw[p - 1][r - 1];
        dft(v);
        const int j0 = (lane / ns) * ns * C::R + lane % ns;
#pragma unroll
        for (int r = 0; r < C::R; ++r) buf[pad(j0 + r * ns)] = v[r];
        wave_sync();
        ns *= C::R;
    }
}

// |FFT_NFFT(f)[k]| for the lane's bins k = lane + 64 r from the H-point
// transform in buf (the real-FFT split); the magnitudes then replace buf's
// head as a plain T[H] array.  Returns the lane's share of their sum.
template <typename T, int H>
__device__ __forceinline__ T wave_magnitudes(cx<T>* buf, const Twiddles<T, H>& tw, int lane) {
    using C = Cfg<H>;
    T mag[C::R];
    T sum = (T)0;
#pragma unroll
    for (int r = 0; r < C::R; ++r) {
        const int k = lane + 64 * r;
        const cx<T> a = buf[pad(k)];
        cx<T> b = buf[pad((H - k) & (H - 1))];
        b.y = -b.y;
        const cx<T> e = a + b, d = mul_mi(a - b);       // 2 E[k], 2 O[k]
        const cx<T> f = e + tw.st0 * (Twiddles<T, H>::step(r) * d);
        mag[r] = (T)0.5 * sqrt(f.x * f.x + f.y * f.y);
        sum += mag[r];
    }
    wave_sync();
    T* m = (T*)buf;
#pragma unroll
    for (int r = 0; r < C::R; ++r) m[lane + 64 * r] = mag[r];
    wave_sync();
    return sum;
}

// |FFT_NFFT(f)[k]|^2 likewise: the powers replace buf's head as a plain T[H] array
template <typename T, int H>
__device__ __forceinline__ void wave_powers(cx<T>* buf, const Twiddles<T, H>& tw, int lane) {
    using C = Cfg<H>;
    T pw[C::R];
#pragma unroll
    for (int r = 0; r < C::R; ++r) {
        const int k = lane + 64 * r;
        const cx<T> a = buf[pad(k)];
        cx<T> b = buf[pad((H - k) & (H - 1))];
        b.y = -b.y;
        const cx<T> e = a + b, d = mul_mi(a - b);       // 2 E[k], 2 O[k]
        const cx<T> f = e + tw.st0 * (Twiddles<T, H>::step(r) * d);
        pw[r] = (T)0.25 * (f.x * f.x + f.y * f.y);
    }
    wave_sync();
    T* m = (T*)buf;
#pragma unroll
    for (int r = 0; r < C::R; ++r) m[lane + 64 * r] = pw[r];
    wave_sync();
}

// FFT_NFFT(f)[k] itself for the lane's bins k = lane + 64 r, kept complex in
// registers (cse_csii.hip's cross spectrum).  buf is only read: the caller
// orders its next write to buf after this with wave_sync.
template <typename T, int H>
__device__ __forceinline__ void wave_split(const cx<T>* buf, const Twiddles<T, H>& tw, int lane,
                                           cx<T> (&f)[Cfg<H>::R]) {
    using C = Cfg<H>;
#pragma unroll
    for (int r = 0; r < C::R; ++r) {
        const int k = lane + 64 * r;
        const cx<T> a = buf[pad(k)];
        cx<T> b = buf[pad((H - k) & (H - 1))];
        b.y = -b.y;
        const cx<T> e = a + b, d = mul_mi(a - b);       // 2 E[k], 2 O[k]
        const cx<T> g = e + tw.st0 * (Twiddles<T, H>::step(r) * d);
        f[r] = {(T)0.5 * g.x, (T)0.5 * g.y};
    }
}

// the band's filter row times the magnitudes: lanes l and l + 32 sum half of
// the support of band l each (l < 25); both end up with the whole sum
template <typename T>
__device__ __forceinline__ T wave_band(const T* m, const T* fv, const int* flo, const int* fn,
                                       int lane) {
    const int band = lane & 31, half = lane >> 5;
    T acc = (T)0;
    if (band < NB) {
        const int n = fn[band], lo = flo[band], mid = (n + 1) >> 1;
        const int t0 = half ? mid : 0, t1 = half ? n : mid;
        for (int t = t0; t < t1; ++t) acc += fv[band * FWP + t] * m[lo + t];
    }
    acc += __shfl_xor(acc, 32, 64);
    return acc;
}

// F[i][k] of include/cse_segsnr.h, before the floor (fp64, numpy's operation order)
__host__ __device__ inline double filter_entry(int i, int k, int H) {
    const double cent[NB] = {50.0,    120.0,   190.0,   260.0,   330.0,   400.0,   470.0,
                             540.0,   617.372, 703.378, 798.717, 904.128, 1020.38, 1148.30,
                             1288.72, 1442.54, 1610.70, 1794.16, 1993.93, 2211.08, 2446.71,
                             2701.97, 2978.04, 3276.17, 3597.63};
    const double band[NB] = {70.0,    70.0,    70.0,    70.0,    70.0,    70.0,    70.0,
                             77.3724, 86.0056, 95.3398, 105.411, 116.256, 127.914, 140.423,
                             153.823, 168.154, 183.457, 199.776, 217.153, 235.631, 255.255,
                             276.072, 298.126, 321.465, 346.136};
    // cent / (sr/2) H with H / (sr/2) = 512 / 8000 = 256 / 4000 at both rates
    const double nyq = H == 512 ? 8000.0 : 4000.0;
    const double f0 = floor(cent[i] / nyq * (double)H);
    const double bw = band[i] / nyq * (double)H;
    const double q = ((double)k - f0) / bw;
    return exp(-11.0 * (q * q) + log(band[0]) - log(band[i]));
}

// the supports of the filter rows (the entries above the floor), on the host
static inline bool band_supports(int H, Bands* b) {
    const double floor_v = exp(-30.0 / (2.0 * 2.303));
    for (int i = 0; i < NB; ++i) {
        int lo = -1, hi = -1;
        for (int k = 0; k < H; ++k)
            if (filter_entry(i, k, H) > floor_v) {
                if (lo < 0) lo = k;
                hi = k;
            }
        if (lo < 0 || hi - lo + 1 > FW) return false;
        b->lo[i] = lo;
        b->n[i] = hi - lo + 1;  // lo + n <= H by construction
    }
    return true;
}

// the supports of a rate, made once (12,800 exponentials on the host); NULL
// when a row is wider than its room
static inline const Bands* band_table(int H) {
    struct Table {
        Bands b;
        bool ok;
        explicit Table(int h) { ok = band_supports(h, &b); }
    };
    static const Table t512(512), t256(256);
    const Table& t = H == 512 ? t512 : t256;
    return t.ok ? &t.b : nullptr;
}

// the filter rows over their supports, and the supports, into LDS (fv:
// NB * FWP entries, flo and fn: 32), by nt threads
template <typename T>
__device__ __forceinline__ void stage_filters(const Bands& bands, int H, T* fv, int* flo, int* fn,
                                              int tid, int nt) {
    if (tid < 32) {
        flo[tid] = tid < NB ? bands.lo[tid] : 0;
        fn[tid] = tid < NB ? bands.n[tid] : 0;
    }
    for (int e = tid; e < NB * FW; e += nt) {
        const int i = e / FW, c = e % FW;
        fv[i * FWP + c] = c < bands.n[i] ? (T)filter_entry(i, bands.lo[i] + c, H) : (T)0;
    }
}

}  // namespace seg
}  // namespace cse

#endif  // CSE_SEGFFT_HPP_
