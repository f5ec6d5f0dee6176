// What the score families of the form "clean side + cells" share around their
// frame code (cse_segsnr.hip, cse_lpc.hip, cse_wss.hip, cse_csii.hip,
// cse_ncm.hip): the 30-ms frames of include/cse_segsnr.h, their window, a
// cell's test signal, the count of non-silent frames, the trimmed mean over a
// cell's frame values, and the argument checks of the entry points.
#ifndef CSE_CELLS_HPP_
#define CSE_CELLS_HPP_

#include "cse_wave.hpp"

namespace cse {

constexpr int NSEL = 1536;  // frames whose values a cell kernel keeps in LDS

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
static inline int64_t up256(int64_t v) { return (v + 255) & ~(int64_t)255; }

// half the transform length of a rate's frames; 0: the rate is not supported
static inline int half_bins(int sr) { return sr == 16000 ? 512 : (sr == 8000 ? 256 : 0); }

// frames of 4 hops in len samples, the header's len // hop - 4
static inline int64_t frames_of(int64_t len, int hop) {
    const int64_t J = len / hop - 4;
    return J < 0 ? 0 : J;
}

// the sizes the entry points accept (the grid's y dimension; 32-bit frame indices)
static inline bool sizes_ok(int64_t n_sig, int64_t len) {
    return n_sig >= 0 && n_sig <= 65535 && len >= 0 && len < ((int64_t)1 << 36);
}

// f32 values per cell and score in scratch (0: the cell kernel keeps them in LDS)
static inline int64_t value_stride(int64_t J) { return J <= NSEL ? 0 : (J + 63) & ~(int64_t)63; }

// The checks every *_prepare and *_cells entry point starts with, in their
// order; fn is the entry point's name as a string literal.
#define CSE_CHECK_PREPARE_ARGS(fn, clean, n_sig, len, sr, workspace)                            \
    CSE_CHECK_ARG(::cse::half_bins(sr) != 0, fn ": sr=%d not supported (16000, 8000)", sr);     \
    CSE_CHECK_ARG((clean) && (workspace), fn ": NULL argument");                                \
    CSE_CHECK_ARG((n_sig) >= 1 && (len) >= 1 && ::cse::sizes_ok(n_sig, len),                    \
                  fn ": n_sig=%lld (1-65535) len=%lld", (long long)(n_sig), (long long)(len))

#define CSE_CHECK_CELLS_ARGS(fn, pointers, n_cells, n_sig, len, sr)                             \
    CSE_CHECK_ARG(::cse::half_bins(sr) != 0, fn ": sr=%d not supported (16000, 8000)", sr);     \
    CSE_CHECK_ARG(pointers, fn ": NULL argument");                                              \
    CSE_CHECK_ARG((n_cells) >= 0 && (n_cells) <= 0x7fffffffLL && (n_sig) >= 1 && (len) >= 1 &&  \
                      ::cse::sizes_ok(n_sig, len),                                              \
                  fn ": n_cells=%lld n_sig=%lld len=%lld", (long long)(n_cells),                \
                  (long long)(n_sig), (long long)(len))

// ---------------------------------------------------------------------------
// device side
// ---------------------------------------------------------------------------
__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// The frame window w[i] = 0.5 (1 - cos(2 pi (i + 1) / (W + 1))), by nt threads.
// The fp64 frame kernels of the clean side keep this loop written out: inlined
// from here, their H = 512 instances allocate two of its registers the other
// way round, and their instruction streams are kept as they were.
template <typename T>
__device__ __forceinline__ void hann_fill(T* wnd, int W, int tid, int nt) {
    for (int i = tid; i < W; i += nt) {
        double s, c;
        sincospi(2.0 * (double)(i + 1) / (double)(W + 1), &s, &c);
        wnd[i] = (T)(0.5 * (1.0 - c));
    }
}

// sample n of a cell's test signal: y shifted by the alignment lag, zero
// outside [0, len), clipped (cse_stoi.hip's cell_sample)
__device__ __forceinline__ float cell_sample(const float* y, int64_t n, int64_t len, int lag,
                                             bool clip) {
    const int64_t s = n - lag;
    if (n < 0 || n >= len || s < 0 || s >= len) return 0.0f;
    float v = y[s];
    if (clip) v = fminf(fmaxf(v, -1.0f), 1.0f);
    return v;
}

// Non-silent frames of each signal, one workgroup of 256 per signal: a frame's
// record is REC values of T and its silent flag sits at FLAG.  ja[sig] gets
// the count; with N95, ja[2 sig] the count and ja[2 sig + 1] the number of
// frames the trimmed mean keeps, round(0.95 count).
template <typename T, int REC, int FLAG, bool N95>
__global__ void __launch_bounds__(256) count_active_kernel(const T* __restrict__ rec, int64_t J,
                                                           int* __restrict__ ja) {
    __shared__ int red[256];
    const int64_t sig = blockIdx.x;
    int n = 0;
    for (int64_t f = threadIdx.x; f < J; f += 256)
        n += rec[(sig * J + f) * REC + FLAG] == (T)0 ? 1 : 0;
    red[threadIdx.x] = n;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (N95) {
            ja[2 * sig] = red[0];
            ja[2 * sig + 1] = (int)((19 * (int64_t)red[0] + 10) / 20);
        } else {
            ja[sig] = red[0];
        }
    }
}

// Mean of the k smallest of v[0..n) (all >= 0 or +inf, at least k finite), by
// a whole workgroup of NT threads; the result is valid in thread 0.  The
// values' bit patterns order like the values: four passes of an 8-bit
// histogram (radix select) find the k-th smallest value t, and the sum of the
// k smallest is the sum of the values below t plus the missing count times t,
// the same as sorting whatever the ties.  hist: 256 entries, sh: 2, red:
// NT / 64; all three are free again on return.  SUM is the wave sum.
template <int NT, double (*SUM)(double) = wave_sum>
__device__ double trimmed_mean(const float* v, int64_t n, unsigned k, unsigned* hist, unsigned* sh,
                               double* red, int tid) {
    constexpr int NW = NT / 64;
    static_assert(NT >= 256 && (NW & (NW - 1)) == 0, "a thread per bin, a pairwise tree of waves");
    const int lane = tid & 63, wave = tid >> 6;
    unsigned prefix = 0, mask = 0, need = k;
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (NT == 256 || tid < 256) hist[tid] = 0;
        __syncthreads();
        for (int64_t i = tid; i < n; i += NT) {
            const unsigned b = __float_as_uint(v[i]);
            if ((b & mask) == prefix) atomicAdd(&hist[(b >> shift) & 255], 1u);
        }
        __syncthreads();
        if (wave == 0) {  // the bin that holds the need-th smallest of the matching values
            const unsigned h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2],
                           h3 = hist[4 * lane + 3];
            const unsigned s = h0 + h1 + h2 + h3;
            unsigned inc = s;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned t = __shfl_up(inc, o, 64);
                if (lane >= o) inc += t;
            }
            const unsigned long long m = __ballot(inc >= need);
            if (m != 0 && lane == __ffsll((long long)m) - 1) {
                unsigned cum = inc - s;
                int d = 3;
                if (cum + h0 >= need) d = 0;
                else if (cum + h0 + h1 >= need) { d = 1; cum += h0; }
                else if (cum + h0 + h1 + h2 >= need) { d = 2; cum += h0 + h1; }
                else cum += h0 + h1 + h2;
                sh[0] = (unsigned)(4 * lane + d);
                sh[1] = need - cum;
            }
        }
        __syncthreads();
        prefix |= sh[0] << shift;
        mask |= 255u << shift;
        need = sh[1];
        __syncthreads();  // sh and hist are rewritten by the next pass
    }
    double acc = 0.0;
    for (int64_t i = tid; i < n; i += NT) {
        const float f = v[i];
        if (__float_as_uint(f) < prefix) acc += (double)f;
    }
    acc = SUM(acc);
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    double part[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) part[w] = red[w];
#pragma unroll
    for (int s = 1; s < NW; s *= 2)
#pragma unroll
        for (int w = 0; w < NW; w += 2 * s) part[w] += part[w + s];
    const double total = part[0] + (double)need * (double)__uint_as_float(prefix);
    __syncthreads();  // red is reused by the next call
    return total / (double)k;
}

}  // namespace cse

#endif  // CSE_CELLS_HPP_
