// Log-likelihood ratio and LPC cepstrum distance (include/cse_lpc.h) on device.
//
// One workgroup of four waves per cell, CH frames at a time, in two phases.
//
// Autocorrelation (the cost: (P + 1) W multiply-adds per frame, and the 75 %
// frame overlap cannot be shared because the window moves with the frame): one
// wave per frame.  The wave stages the windowed frame once in LDS, followed by
// P zeros so that no lag needs a bound check.  Lane l then owns the SPL
// consecutive samples from SPL l: it reads f[SPL l .. SPL l + SPL + P) into
// registers once and accumulates all P + 1 lags from them.  The staged frame
// carries one unused slot after every SPL samples, so the lanes' first reads
// lie SPL + 1 doubles apart (72 B / 40 B: 32 lanes on 32 distinct even banks).
// Reduction over the lanes: per lag a sum over each row of 16 lanes by DPP,
// lane k of a row keeps lag k, then two shuffles add the four rows for all
// lags at once.  R of the chunk's frames waits in LDS.  A frame's sample loads
// are unconditional and issued together, and the chunk's silent flags are read
// once: with a bound-check branch per load and a flag read per frame the launch
// took 7.7 instead of 4.9 ms.  (Fetching the next frame's samples into
// registers under the current frame was tried: 195 VGPRs, 6.3 ms.)
//
// Levinson-Durbin, the quadratic form and the cepstrum recursion are about 1e3
// dependent operations per frame: one lane per frame runs them on register
// arrays (every loop unrolled), CH frames after each chunk's autocorrelations.
// The form A T(R_x) A^T is sum_k m_k R_x[k] rho[k] with rho the autocorrelation
// of A's coefficients: P + 1 terms.
//
// Trimmed mean: a frame's two values are kept as f32, in LDS while J <= NSEL,
// in the caller's scratch beyond.  Both are >= 0, so their bit patterns order
// like the values: four passes of an 8-bit histogram (radix select) find the
// n95-th smallest value t, and the sum of the n95 smallest is the sum of the
// values below t plus the missing count times t, the same as sorting whatever
// the ties.  Silent frames hold +inf and are never reached.
//
// The clean side (cse_lpc_prepare) runs the same two phases on x and leaves per
// frame a record of 2P + 3 doubles: silent flag, R_x[0..P], A_x T(R_x) A_x^T,
// c_x[1..P].
#include "cse_cells.hpp"

#include "../../include/cse_lpc.h"

namespace cse {
namespace lpc {

constexpr int NT = 256;       // threads per workgroup
constexpr int NW = NT / 64;
constexpr int CH = 128;       // frames per chunk
constexpr double K10 = 4.342944819032518;  // 10 / ln 10

template <int SR>
struct Cfg {
    static_assert(SR == 16000 || SR == 8000, "16 kHz or 8 kHz");
    static constexpr int W = SR == 16000 ? 480 : 240;
    static constexpr int HOP = W / 4;
    static constexpr int P = SR == 16000 ? 16 : 10;
    static constexpr int SPL = SR == 16000 ? 8 : 4;   // samples per lane
    static constexpr int NL = W / SPL;                // lanes with samples (60)
    static constexpr int NV = SPL + P;                // values such a lane reads
    static constexpr int FB = (W + P - 1) + (W + P - 1) / SPL + 1;  // staged doubles per wave
    static constexpr int RS = P + 1;                  // odd: a lane per row reads without conflicts
    static constexpr int REC = 2 * P + 3;             // doubles per clean frame record
    static constexpr int R_R = 1, R_DEN = P + 2, R_C = P + 3;  // record offsets (0: silent flag)
    static_assert(NL <= 64 && W % SPL == 0 && RS % 2 == 1, "lane split");
    static_assert(SPL * (NL - 1) + NV <= W + P, "a lane's reads stay inside the padded frame");
};

template <class C>
__device__ __forceinline__ int pidx(int i) { return i + i / C::SPL; }

// The windowed frame src(i) w[i], i < W, staged in fb; its autocorrelation
// R[0..P] written to Rrow.  Returns whether any sample is non-zero.  Called by
// a whole wave; fb's P entries after the frame are zero.
template <class C, class Src>
__device__ __forceinline__ bool frame_autocorr(double* fb, const double* wnd, Src src, int lane,
                                               double* Rrow) {
    constexpr int NQ = (C::W + 63) / 64;
    double smp[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {  // every load before the first use
        const int i = lane + 64 * q;
        smp[q] = i < C::W ? src(i) : 0.0;
    }
    bool nz = false;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int i = lane + 64 * q;
        nz = nz || smp[q] != 0.0;
        if (i < C::W) fb[pidx<C>(i)] = smp[q] * wnd[i];
    }
    wave_sync();
    double acc[C::P + 1];
#pragma unroll
    for (int k = 0; k <= C::P; ++k) acc[k] = 0.0;
    if (lane < C::NL) {
        double f[C::NV];
        const double* mine = fb + (C::SPL + 1) * lane;
#pragma unroll
        for (int m = 0; m < C::NV; ++m) f[m] = mine[m + m / C::SPL];
#pragma unroll
        for (int s = 0; s < C::SPL; ++s)
#pragma unroll
            for (int k = 0; k <= C::P; ++k) acc[k] = fma(f[s], f[s + k], acc[k]);
    }
    double m0 = 0.0, m1 = 0.0;  // lane k of a row: lag k (m0), lag 16 + k (m1)
#pragma unroll
    for (int k = 0; k <= C::P; ++k) {
        const double v = row_sum(acc[k]);
        if ((lane & 15) == (k & 15)) {
            if (k < 16) m0 = v; else m1 = v;
        }
    }
    m0 += __shfl_xor(m0, 16, 64);
    m0 += __shfl_xor(m0, 32, 64);
    if (lane < (C::P + 1 < 16 ? C::P + 1 : 16)) Rrow[lane] = m0;
    if (C::P + 1 > 16) {
        m1 += __shfl_xor(m1, 16, 64);
        m1 += __shfl_xor(m1, 32, 64);
        if (lane < C::P + 1 - 16) Rrow[16 + lane] = m1;
    }
    wave_sync();  // fb is read before the next frame's samples replace it
    return __ballot(nz) != 0;
}

// Levinson-Durbin with the header's guard: A[0] = 1, orders from the stop on 0
template <int P>
__device__ __forceinline__ void levinson(const double (&R)[P + 1], double (&A)[P + 1]) {
    A[0] = 1.0;
#pragma unroll
    for (int j = 1; j <= P; ++j) A[j] = 0.0;
    double E = R[0];
    bool go = true;
#pragma unroll
    for (int i = 1; i <= P; ++i) {
        double s = R[i];
#pragma unroll
        for (int j = 1; j < i; ++j) s = fma(A[j], R[i - j], s);
        const double k = -s / E;
        go = go && E > 0.0 && fabs(k) < 1.0;
        if (go) {
#pragma unroll
            for (int j = 1; 2 * j < i; ++j) {
                const double a = A[j], b = A[i - j];
                A[j] = fma(k, b, a);
                A[i - j] = fma(k, a, b);
            }
            if (i % 2 == 0) A[i / 2] = fma(k, A[i / 2], A[i / 2]);
            A[i] = k;
            E = (1.0 - k * k) * E;
        }
    }
}

// A T(R) A^T = R[0] rho[0] + 2 sum_{k > 0} R[k] rho[k], rho[k] = sum_j A[j] A[j + k]
template <int P, class RxT>
__device__ __forceinline__ double quad_form(RxT Rx, const double (&A)[P + 1]) {
    double q = 0.0;
#pragma unroll
    for (int k = P; k >= 0; --k) {
        double rho = 0.0;
#pragma unroll
        for (int j = 0; j + k <= P; ++j) rho = fma(A[j], A[j + k], rho);
        q = fma(k ? 2.0 * Rx[k] : Rx[k], rho, q);
    }
    return q;
}

// c[1..P] of the predictor A (c[0] unused)
template <int P>
__device__ __forceinline__ void cepstrum(const double (&A)[P + 1], double (&c)[P + 1]) {
    c[0] = 0.0;
    c[1] = -A[1];
#pragma unroll
    for (int n = 2; n <= P; ++n) {
        double s = 0.0;
#pragma unroll
        for (int k = 1; k < n; ++k) s = fma((double)k * c[k], A[n - k], s);
        c[n] = -(A[n] + s / (double)n);
    }
}

// ---------------------------------------------------------------------------
// clean side
// ---------------------------------------------------------------------------
struct Layout {
    int64_t J;
    int64_t ja, rec, total;  // byte offsets
};

static Layout layout(int64_t n_sig, int64_t len, int sr) {
    const int hop = sr == 16000 ? 120 : 60, rec = sr == 16000 ? Cfg<16000>::REC : Cfg<8000>::REC;
    Layout L;
    L.J = frames_of(len, hop);
    L.ja = 0;  // int ja, n95 per signal
    L.rec = up256(n_sig * 2 * 4);
    L.total = L.rec + up256(n_sig * L.J * rec * 8);
    return L;
}

template <class C>
__device__ __forceinline__ void init_frames(double* wnd, double (*fb)[C::FB], int tid) {
    hann_fill(wnd, C::W, tid, NT);
    for (int e = tid; e < NW * C::P; e += NT) fb[e / C::P][pidx<C>(C::W + e % C::P)] = 0.0;
}

template <class C>
__global__ void __launch_bounds__(NT) lpc_clean_kernel(const double* __restrict__ x, int64_t len,
                                                       int64_t J, double* __restrict__ rec) {
    __shared__ double wnd[C::W];
    __shared__ double fb[NW][C::FB];
    __shared__ double Rb[CH][C::RS];
    __shared__ int silent[CH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t sig = blockIdx.y, f0 = (int64_t)blockIdx.x * CH;
    const int nf = (int)((J - f0) < CH ? (J - f0) : CH);
    init_frames<C>(wnd, fb, tid);
    __syncthreads();
    for (int fr = wave; fr < nf; fr += NW) {
        const double* xs = x + sig * len + (f0 + fr) * C::HOP;
        const bool nz = frame_autocorr<C>(fb[wave], wnd, [&](int i) { return xs[i]; }, lane, Rb[fr]);
        if (lane == 0) silent[fr] = nz ? 0 : 1;
    }
    __syncthreads();
    if (tid >= nf) return;
    double* r = rec + (sig * J + f0 + tid) * C::REC;
    if (silent[tid]) {
        r[0] = 1.0;
        for (int e = 1; e < C::REC; ++e) r[e] = 0.0;
        return;
    }
    double R[C::P + 1], A[C::P + 1], c[C::P + 1];
#pragma unroll
    for (int k = 0; k <= C::P; ++k) R[k] = Rb[tid][k];
    levinson<C::P>(R, A);
    cepstrum<C::P>(A, c);
    r[0] = 0.0;
#pragma unroll
    for (int k = 0; k <= C::P; ++k) r[C::R_R + k] = R[k];
    r[C::R_DEN] = quad_form<C::P>(R, A);
#pragma unroll
    for (int n = 1; n <= C::P; ++n) r[C::R_C + n - 1] = c[n];
}

// ---------------------------------------------------------------------------
// cells
// ---------------------------------------------------------------------------
struct CellArgs {
    const float* y;
    const int64_t* y_offset;
    const int32_t* lag;
    const int32_t* sig_of;
    int64_t len, J, vstride;  // vstride: f32 values per cell and score in scratch
    int clip;
    const int* ja;
    const double* rec;
    float* scratch;
    double* llr;
    double* cep;
};

// cell_sample (cse_cells.hpp) with an unconditional load instead of its early
// return, so that a frame's loads are issued together (see the head comment)
__device__ __forceinline__ float cell_sample_unbranched(const float* y, int64_t n, int64_t len,
                                                        int lag, bool clip) {
    const int64_t s = n - lag;
    const bool ok = n >= 0 && n < len && s >= 0 && s < len;
    float v = y[ok ? s : 0];  // an unconditional load: a frame's loads are issued together
    if (clip) v = fminf(fmaxf(v, -1.0f), 1.0f);
    return ok ? v : 0.0f;
}

template <class C>
__global__ void __launch_bounds__(NT) lpc_cells_kernel(CellArgs a) {
    __shared__ double wnd[C::W];
    __shared__ double fb[NW][C::FB];
    __shared__ double Rb[CH][C::RS];
    __shared__ float sv[2][NSEL];
    __shared__ int silent[CH];
    __shared__ __attribute__((aligned(16))) unsigned hist[256];
    __shared__ unsigned sh[2];
    __shared__ double red[NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t cell = blockIdx.x;
    const int64_t sig = a.sig_of[cell];
    const int ja = a.ja[2 * sig], n95 = a.ja[2 * sig + 1];
    if (a.J < 1 || ja == 0) {  // uniform over the workgroup
        if (tid == 0) {
            if (a.llr) a.llr[cell] = quiet_nan();
            if (a.cep) a.cep[cell] = quiet_nan();
        }
        return;
    }
    const int lag = a.lag ? a.lag[cell] : 0;
    const float* yc = a.y + a.y_offset[cell];
    const bool clip = a.clip != 0, want_llr = a.llr != nullptr, want_cep = a.cep != nullptr;
    const bool in_lds = a.J <= NSEL;
    float* vl = in_lds ? sv[0] : a.scratch + cell * 2 * a.vstride;
    float* vc = in_lds ? sv[1] : a.scratch + (cell * 2 + 1) * a.vstride;
    init_frames<C>(wnd, fb, tid);
    __syncthreads();
    for (int64_t f0 = 0; f0 < a.J; f0 += CH) {
        const int nf = (int)((a.J - f0) < CH ? (a.J - f0) : CH);
        // the chunk's silent flags in one load (read per frame they would put a
        // memory latency in front of every frame)
        if (tid < nf) silent[tid] = a.rec[(sig * a.J + f0 + tid) * C::REC] != 0.0 ? 1 : 0;
        __syncthreads();
        for (int fr = wave; fr < nf; fr += NW) {
            if (silent[fr]) continue;  // wave-uniform
            const int64_t base = (f0 + fr) * C::HOP;
            frame_autocorr<C>(
                fb[wave], wnd,
                [&](int i) {
                    return (double)cell_sample_unbranched(yc, base + i, a.len, lag, clip);
                },
                lane, Rb[fr]);
        }
        __syncthreads();
        if (tid < nf) {
            const double* r = a.rec + (sig * a.J + f0 + tid) * C::REC;
            float fl = __uint_as_float(0x7f800000u), fc = fl;  // +inf: a silent frame
            if (!silent[tid]) {
                double R[C::P + 1], A[C::P + 1];
#pragma unroll
                for (int k = 0; k <= C::P; ++k) R[k] = Rb[tid][k];
                levinson<C::P>(R, A);
                fl = fc = 0.0f;
                if (want_llr) {
                    const double ratio = quad_form<C::P>(r + C::R_R, A) / r[C::R_DEN];
                    double v = (ratio > 0.0 && ratio < __builtin_inf()) ? log(ratio) : 2.0;
                    if (!(v > 0.0)) v = 0.0;
                    fl = (float)fmin(v, 2.0);
                }
                if (want_cep) {
                    double c[C::P + 1];
                    cepstrum<C::P>(A, c);
                    double d = 0.0;
#pragma unroll
                    for (int n = 1; n <= C::P; ++n) {
                        const double e = r[C::R_C + n - 1] - c[n];
                        d = fma(e, e, d);
                    }
                    double v = K10 * sqrt(2.0 * d);
                    if (!(v < 10.0)) v = 10.0;  // also a value that is not finite
                    fc = (float)v;
                }
            }
            vl[f0 + tid] = fl;
            vc[f0 + tid] = fc;
        }
        __syncthreads();  // Rb is rewritten by the next chunk; the values are complete
    }
    if (want_llr) {
        const double m =
            trimmed_mean<NT, wave_sum_shfl>(vl, a.J, (unsigned)n95, hist, sh, red, tid);
        if (tid == 0) a.llr[cell] = m;
    }
    if (want_cep) {
        const double m =
            trimmed_mean<NT, wave_sum_shfl>(vc, a.J, (unsigned)n95, hist, sh, red, tid);
        if (tid == 0) a.cep[cell] = m;
    }
}

}  // namespace lpc
}  // namespace cse

using namespace cse;

extern "C" int64_t cse_lpc_workspace_bytes(int64_t n_sig, int64_t len, int sr) {
    if (!half_bins(sr) || n_sig < 0 || len < 0) return -1;
    return lpc::layout(n_sig, len, sr).total;
}

extern "C" int64_t cse_lpc_scratch_bytes(int64_t n_cells, int64_t len, int sr) {
    if (!half_bins(sr) || n_cells < 0 || len < 0) return -1;
    return n_cells * 2 * value_stride(lpc::layout(1, len, sr).J) * 4;
}

extern "C" int cse_lpc_prepare(const double* clean, int64_t n_sig, int64_t len, int sr,
                               void* workspace, cse_stream_t stream) {
    CSE_CHECK_PREPARE_ARGS("cse_lpc_prepare", clean, n_sig, len, sr, workspace);
    const lpc::Layout L = lpc::layout(n_sig, len, sr);
    unsigned char* ws = (unsigned char*)workspace;
    int* ja = (int*)(ws + L.ja);
    double* rec = (double*)(ws + L.rec);
    hipStream_t st = (hipStream_t)stream;
    if (L.J > 0) {
        const dim3 grid((unsigned)((L.J + lpc::CH - 1) / lpc::CH), (unsigned)n_sig);
        if (sr == 16000)
            hipLaunchKernelGGL(lpc::lpc_clean_kernel<lpc::Cfg<16000>>, grid, dim3(lpc::NT), 0, st,
                               clean, len, L.J, rec);
        else
            hipLaunchKernelGGL(lpc::lpc_clean_kernel<lpc::Cfg<8000>>, grid, dim3(lpc::NT), 0, st,
                               clean, len, L.J, rec);
    }
    if (sr == 16000)
        hipLaunchKernelGGL((count_active_kernel<double, lpc::Cfg<16000>::REC, 0, true>),
                           dim3((unsigned)n_sig), dim3(256), 0, st, (const double*)rec, L.J, ja);
    else
        hipLaunchKernelGGL((count_active_kernel<double, lpc::Cfg<8000>::REC, 0, true>),
                           dim3((unsigned)n_sig), dim3(256), 0, st, (const double*)rec, L.J, ja);
    CSE_CHECK_LAUNCH("cse_lpc_prepare");
    return CSE_OK;
}

extern "C" int cse_lpc_cells(const float* y, const int64_t* y_offset, const int32_t* lag,
                             const int32_t* sig_of, int64_t n_cells, int64_t n_sig, int64_t len,
                             int sr, int clip, const void* workspace, void* scratch, double* llr,
                             double* cep, cse_stream_t stream) {
    CSE_CHECK_CELLS_ARGS("cse_lpc_cells", y && y_offset && sig_of && workspace && (llr || cep),
                         n_cells, n_sig, len, sr);
    if (n_cells == 0) return CSE_OK;
    const lpc::Layout L = lpc::layout(n_sig, len, sr);
    const int64_t vstride = value_stride(L.J);
    CSE_CHECK_ARG(vstride == 0 || scratch,
                  "cse_lpc_cells: %lld frames need scratch (cse_lpc_scratch_bytes)", (long long)L.J);
    const unsigned char* ws = (const unsigned char*)workspace;
    lpc::CellArgs a;
    a.y = y;
    a.y_offset = y_offset;
    a.lag = lag;
    a.sig_of = sig_of;
    a.len = len;
    a.J = L.J;
    a.vstride = vstride;
    a.clip = clip;
    a.ja = (const int*)(ws + L.ja);
    a.rec = (const double*)(ws + L.rec);
    a.scratch = (float*)scratch;
    a.llr = llr;
    a.cep = cep;
    hipStream_t st = (hipStream_t)stream;
    if (sr == 16000)
        hipLaunchKernelGGL(lpc::lpc_cells_kernel<lpc::Cfg<16000>>, dim3((unsigned)n_cells),
                           dim3(lpc::NT), 0, st, a);
    else
        hipLaunchKernelGGL(lpc::lpc_cells_kernel<lpc::Cfg<8000>>, dim3((unsigned)n_cells),
                           dim3(lpc::NT), 0, st, a);
    CSE_CHECK_LAUNCH("cse_lpc_cells");
    return CSE_OK;
}
