// The online enhancer (include/cse_online.h): the offline path, frame by frame,
// for S signals that advance in lockstep.
//
// One workgroup per signal; a push of k frames loops over them inside the
// kernel, because every stage of frame t reads what frame t - 1 left (the
// tracker, the mu recursion, the decision-directed state, the overlap ring).
// The work of one frame is the same code whatever k is, and all state a frame
// reads is either in the block (global memory, read and written per frame) or
// in LDS regions that are loaded from the block at the start of a push and
// stored at its end without an operation on them: the outputs cannot depend on
// how the frames are split over pushes.
//
//   analysis   radix-2 DIT FFT in LDS, fp64, the order of cse_stft's radix-2
//              form (window product into bit-reversed order, log2 n passes)
//   tracker    the per-bin device functions of cse_mcra.hip / cse_spp.hip
//   gain       gen_gain (cse_enhance_generic.hip): gain_bin<1024, ALGO>
//   synthesis  gen_irfft_ola (cse_enhance_generic.hip)
// are included, not restated.  The frames, the prime and the finish of one
// stream are device functions (on_frames, on_prime, on_finish) that the pool of
// cse_online_pool.hip runs on its slots as the kernels here run them on the
// streams of a batch.
#define CSE_ENHANCE_DEVICE_ONLY 1
#define CSE_GENERIC_DEVICE_ONLY 1
#define CSE_MCRA_DEVICE_ONLY 1
#define CSE_SPP_DEVICE_ONLY 1
#include "cse_enhance_generic.hip"
#include "cse_mcra.hip"
#include "cse_spp.hip"

#include "../../include/cse_online.h"

namespace cse {

// the state block of one signal, in bytes (cse_online.h, STATE)
struct OnState {
    int64_t tail, trk, mu, rr, ring, total;
    __host__ __device__ OnState(int N) {
        const int64_t B = N / 2 + 1;
        tail = 0;                  // f64 [N] (n_fft - hop used)
        trk = tail + 8 * (int64_t)N;  // f64 [5][B]
        mu = trk + 40 * B;         // f64 [B]
        rr = mu + 8 * B;           // f32 [B]
        ring = rr + 4 * B;         // f32 [N]
        total = (ring + 4 * (int64_t)N + 255) & ~(int64_t)255;
    }
};

// LDS: the generic kernel's regions (GenLds), then the analysis in fp64
struct OnLds {
    int re, im, twr, twi, win, P, total;
    __host__ __device__ OnLds(int N) {
        const int M = N / 2, B = M + 1;
        int o = GenLds(N).total;
        auto take = [&](int bytes) {
            const int at = o;
            o = (o + bytes + 15) & ~15;
            return at;
        };
        re = take(8 * N);
        im = take(8 * N);
        twr = take(8 * M);
        twi = take(8 * M);
        win = take(8 * N);
        P = take(8 * B);
        total = o;
    }
};

struct OnArgs {
    int N, log2n, hop, k;
    int64_t t0;            // frames pushed before this call
    unsigned char* state;
    const double* x;       // [S][k hop]
    float* y;              // [S][k hop]
    float* n_out;          // [S][k][B] or null
    cse_cell_t cell;       // algo and param[8] (gen_cell_param)
    McraK mk;
    SppK sk;
    int L, K;              // mcra window_frames, spp init_frames
    double eps, mu;
    float inv_eps;
};

__device__ __forceinline__ double on_smooth(double mu, double s, double c, double x) {
#pragma clang fp contract(off)
    return mu * s + c * x;  // cse_noise_finish's step: two products, one sum
}

// frame j of this push: window, transform, P into LDS.  Ends on a barrier.
__device__ __forceinline__ void on_analysis(const OnArgs& a, const OnLds& Lo, unsigned char* smem,
                                            const double* tail, const double* xs, int j) {
    const int N = a.N, M = N / 2, B = M + 1, log2n = a.log2n;
    const int tid = threadIdx.x;
    double* re = (double*)(smem + Lo.re);
    double* im = (double*)(smem + Lo.im);
    const double* twr = (const double*)(smem + Lo.twr);
    const double* twi = (const double*)(smem + Lo.twi);
    const double* win = (const double*)(smem + Lo.win);
    double* Pd = (double*)(smem + Lo.P);
    const int nt = N - a.hop;  // samples the tail holds
    __syncthreads();           // the previous frame's readers of re / im / P
    for (int n = tid; n < N; n += GEN_NT) {
        const int i = j * a.hop + n;  // < k hop + nt
        const double v = i < nt ? tail[i] : xs[i - nt];
        const int r = (int)(__brev((unsigned)n) >> (32 - log2n));
        re[r] = v * win[n];
        im[r] = 0.0;
    }
    __syncthreads();
    for (int st = 1; st <= log2n; ++st) {
        const int half = 1 << (st - 1);
        for (int b = tid; b < M; b += GEN_NT) {
            const int grp = b >> (st - 1);
            const int jj = b & (half - 1);
            const int i0 = grp * (half << 1) + jj;
            const int i1 = i0 + half;
            const int tw = jj << (log2n - st);
            const double wr = twr[tw], wi = twi[tw];
            const double br = re[i1] * wr - im[i1] * wi;
            const double bi = re[i1] * wi + im[i1] * wr;
            const double ar = re[i0], ai = im[i0];
            re[i0] = ar + br;
            im[i0] = ai + bi;
            re[i1] = ar - br;
            im[i1] = ai - bi;
        }
        __syncthreads();
    }
    for (int b = tid; b < B; b += GEN_NT) {
        const double r = re[b];
        double i = im[b];
        if (b == 0 || b == M) i = 0.0;
        im[b] = i;
        Pd[b] = r * r + i * i;
    }
    __syncthreads();
}

// The frames [a.t0, a.t0 + a.k) of one stream, by one workgroup: sb is the
// stream's state block, xs / ys its k hop samples in and out, ns its [k][B]
// rows or null.  Of `a` it reads N, log2n, hop, k, t0 and the parameters, not
// state, x, y or n_out: the lockstep kernel and the pool's (cse_online_pool.hip)
// find a stream's pointers in their own ways.
template <int ALGO, int METHOD>
__device__ __forceinline__ void on_frames(const OnArgs& a, unsigned char* smem, unsigned char* sb,
                                          const double* xs, float* ys, float* ns) {
    const int N = a.N, M = N / 2, B = M + 1, hop = a.hop, k = a.k;
    const int tid = threadIdx.x;
    const GenLds Ly(N);
    const OnLds Lo(N);
    const OnState Os(N);
    double* tail = (double*)(sb + Os.tail);
    double* trk = (double*)(sb + Os.trk);
    double* smu = (double*)(sb + Os.mu);
    float* rr_g = (float*)(sb + Os.rr);
    float* ring_g = (float*)(sb + Os.ring);

    const double* wsq = (const double*)(smem + Ly.wsq);
    float* sr = (float*)(smem + Ly.sr);
    float* si = (float*)(smem + Ly.si);
    float* rr = (float*)(smem + Ly.rr);
    float* ring = (float*)(smem + Ly.ring);
    const double* re = (const double*)(smem + Lo.re);
    const double* im = (const double*)(smem + Lo.im);
    double* twr = (double*)(smem + Lo.twr);
    double* twi = (double*)(smem + Lo.twi);
    double* win = (double*)(smem + Lo.win);
    const double* Pd = (const double*)(smem + Lo.P);
    const CellParam prm = gen_cell_param<ALGO>(&a.cell);
    const int log2m = a.log2n - 1;

    gen_tables(Ly, smem);
    for (int j = tid; j < M; j += GEN_NT) {
        double sn, c;
        sincospi(-2.0 * (double)j / (double)N, &sn, &c);
        twr[j] = c;
        twi[j] = sn;
    }
    for (int n = tid; n < N; n += GEN_NT) {
        win[n] = 0.5 - 0.5 * cospi(2.0 * (double)n / (double)N);
        ring[n] = ring_g[n];
    }
    for (int b = tid; b < B; b += GEN_NT) rr[b] = rr_g[b];
    // (on_analysis begins with a barrier)

    if (METHOD == CSE_NOISE_SPP && a.t0 == 0) {
        // lam = the sequential mean of P over the first K frames (k >= K: the host checks)
        for (int j = 0; j < a.K; ++j) {
            on_analysis(a, Lo, smem, tail, xs, j);
            for (int b = tid; b < B; b += GEN_NT) trk[b] = j == 0 ? Pd[b] : trk[b] + Pd[b];
        }
        for (int b = tid; b < B; b += GEN_NT) {
            trk[b] = trk[b] / (double)a.K;
            trk[B + b] = a.sk.prior_h1;
        }
    }

    const double c_mu = 1.0 - a.mu;
    for (int j = 0; j < k; ++j) {
        const int64_t tg = a.t0 + j;
        on_analysis(a, Lo, smem, tail, xs, j);
        const float alpha_t = tg == 0 ? 0.0f : prm.p0;
        for (int b = tid; b < B; b += GEN_NT) {
            // ---- the tracker's step: nread = N[tg]
            double nread;
            if (METHOD == CSE_NOISE_MCRA) {
                const int m = b == 0 ? 1 : b - 1, q = b == B - 1 ? B - 2 : b + 1;
                const McraRow r{Pd[m], Pd[b], Pd[q]};
                const double sf = mcra_sf(r);
                McraState s;
                double ci;
                if (tg == 0) {
#pragma clang fp contract(off)
                    s.S = sf;
                    s.Smin = s.Stmp = s.S;
                    s.p = 0.0;
                    s.lam = r.c;
                    nread = s.lam;
                    ci = s.S > a.mk.delta * s.Smin ? a.mk.c_p : 0.0;
                } else {
                    s.S = trk[b];
                    s.Smin = trk[B + b];
                    s.Stmp = trk[2 * B + b];
                    s.p = trk[3 * B + b];
                    s.lam = trk[4 * B + b];
                    nread = s.lam;
                    ci = mcra_presence(s, a.mk, sf, tg % a.L == 0);
                }
                mcra_track(s, a.mk, ci, r.c);
                trk[b] = s.S;
                trk[B + b] = s.Smin;
                trk[2 * B + b] = s.Stmp;
                trk[3 * B + b] = s.p;
                trk[4 * B + b] = s.lam;
            } else {
                double lam = trk[b], pm = trk[B + b];
                nread = spp_frame(lam, pm, a.sk, Pd[b]);
                trk[b] = lam;
                trk[B + b] = pm;
            }
            const float n32 = (float)fmax(nread, a.eps);
            if (ns) ns[(int64_t)j * B + b] = n32;
            // ---- cse_noise_finish's row
            const double xn = (double)n32;
            const double sm = tg == 0 ? xn : on_smooth(a.mu, smu[b], c_mu, xn);
            smu[b] = sm;
            const float nv = ALGO == CSE_ALGO_SS ? (float)sm : 1.0f / fmaxf((float)sm, a.inv_eps);
            // ---- gain, S = Y s
            float2 yv = make_float2((float)re[b], (float)im[b]);
            float st = rr[b], g;
            const float s = gen_gain<ALGO>(yv, nv, st, alpha_t, prm, g);
            rr[b] = st;
            float vr = yv.x * s, vi = yv.y * s;
            if (b == 0 || b == M) vi = 0.0f;  // irfft ignores these imaginary parts
            sr[b] = vr;
            si[b] = vi;
        }
        __syncthreads();
        gen_irfft_ola(Ly, smem, log2m, tg * hop);
        // ---- padded samples [tg hop, (tg + 1) hop) are final
        for (int i = tid; i < hop; i += GEN_NT) {
            const int64_t q = tg * hop + i;
            const int ri = (int)(q % N);
            const float v = ring[ri];
            ring[ri] = 0.0f;
            const int64_t tlo = q - N + 1 <= 0 ? 0 : (q - N + 1 + hop - 1) / hop;
            double wss = 0.0;
            for (int64_t t = tlo; t <= tg; ++t) wss += wsq[q - t * hop];
            ys[(int64_t)j * hop + i] = wss > 2.2250738585072014e-308 ? (float)((double)v / wss) : v;
        }
    }
    __syncthreads();
    // ---- what the next push reads: the ring, the decision-directed state, the input tail
    for (int n = tid; n < N; n += GEN_NT) ring_g[n] = ring[n];
    for (int b = tid; b < B; b += GEN_NT) rr_g[b] = rr[b];
    const int nt = N - hop;
    constexpr int TU = (2048 - 2048 / 8 + GEN_NT - 1) / GEN_NT;  // 7
    double keep[TU];
#pragma unroll
    for (int u = 0; u < TU; ++u) {
        const int i = tid + GEN_NT * u;
        const int64_t src = (int64_t)i + (int64_t)k * hop;
        keep[u] = i < nt ? (src < nt ? tail[src] : xs[src - nt]) : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < TU; ++u) {
        const int i = tid + GEN_NT * u;
        if (i < nt) tail[i] = keep[u];
    }
}

// (CSE_ONLINE_DEVICE_ONLY: the device functions and host checks only, no
// kernel and no entry point, for cse_online_pool.hip)
#ifndef CSE_ONLINE_DEVICE_ONLY
template <int ALGO, int METHOD>
__global__ void __launch_bounds__(GEN_NT) online_push_kernel(OnArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int64_t sig = blockIdx.x;
    const int64_t B = a.N / 2 + 1;
    on_frames<ALGO, METHOD>(a, smem, a.state + sig * OnState(a.N).total,
                            a.x + sig * (int64_t)a.k * a.hop, a.y + sig * (int64_t)a.k * a.hop,
                            a.n_out ? a.n_out + sig * (int64_t)a.k * B : nullptr);
}
#endif  // !CSE_ONLINE_DEVICE_ONLY

// one stream's block sb: all state zero, then the input tail xh [N - hop]
__device__ __forceinline__ void on_prime(unsigned char* sb, int N, int hop, const double* xh) {
    const OnState Os(N);
    uint32_t* w = (uint32_t*)sb;
    const int nt = N - hop;
    // the words past the tail, then the tail (disjoint: no barrier)
    for (int64_t i = Os.trk / 4 + threadIdx.x; i < Os.total / 4; i += GEN_NT) w[i] = 0u;
    double* tail = (double*)(sb + Os.tail);
    for (int i = threadIdx.x; i < N; i += GEN_NT) tail[i] = i < nt ? xh[i] : 0.0;
}

#ifndef CSE_ONLINE_DEVICE_ONLY
__global__ void __launch_bounds__(GEN_NT) online_prime_kernel(unsigned char* state, int N, int hop,
                                                              const double* x_head) {
    on_prime(state + (int64_t)blockIdx.x * OnState(N).total, N, hop,
             x_head + (int64_t)blockIdx.x * (N - hop));
}
#endif  // !CSE_ONLINE_DEVICE_ONLY

// the last n_fft - hop samples of one stream's ring (block sb, T frames run):
// padded [T hop, (T - 1) hop + n_fft) -> out [N - hop]; wsq: LDS, f64 [N]
__device__ __forceinline__ void on_finish(const unsigned char* sb, int N, int hop, int64_t T,
                                          float* out, double* wsq) {
    const float* ring = (const float*)(sb + OnState(N).ring);
    for (int n = threadIdx.x; n < N; n += GEN_NT) {
        const double w = 0.5 - 0.5 * cospi(2.0 * (double)n / (double)N);
        wsq[n] = w * w;
    }
    __syncthreads();
    const int nt = N - hop;
    for (int i = threadIdx.x; i < nt; i += GEN_NT) {
        const int64_t q = T * hop + i;
        const float v = ring[q % N];
        const int64_t tlo = q - N + 1 <= 0 ? 0 : (q - N + 1 + hop - 1) / hop;
        double wss = 0.0;
        for (int64_t t = tlo; t <= T - 1; ++t) wss += wsq[q - t * hop];
        out[i] = wss > 2.2250738585072014e-308 ? (float)((double)v / wss) : v;
    }
}

#ifndef CSE_ONLINE_DEVICE_ONLY
__global__ void __launch_bounds__(GEN_NT) online_finish_kernel(const unsigned char* state, int N,
                                                               int hop, int64_t T, float* y_tail) {
    __shared__ double wsq[2048];
    on_finish(state + (int64_t)blockIdx.x * OnState(N).total, N, hop, T,
              y_tail + (int64_t)blockIdx.x * (N - hop), wsq);
}
#endif  // !CSE_ONLINE_DEVICE_ONLY

static bool online_shape_ok(int n_fft) {
    return n_fft >= 128 && n_fft <= 2048 && (n_fft & (n_fft - 1)) == 0;
}

// the configuration checks of cse_online_init, under the caller's name (the
// pool, cse_online_pool.hip, includes this file with CSE_ONLINE_DEVICE_ONLY)
static int online_check_config(const char* name, const cse_online_config_t* cfg) {
    CSE_CHECK_ARG(online_shape_ok(cfg->n_fft), "%s: n_fft=%d (a power of two in [128, 2048])", name,
                  cfg->n_fft);
    CSE_CHECK_ARG(cfg->hop == cfg->n_fft / 8 || cfg->hop == cfg->n_fft / 4 ||
                      cfg->hop == cfg->n_fft / 2,
                  "%s: hop=%d (n_fft/8, n_fft/4 or n_fft/2 of n_fft=%d)", name, cfg->hop,
                  cfg->n_fft);
    CSE_CHECK_ARG(cfg->algo >= CSE_ALGO_SS && cfg->algo <= CSE_ALGO_OMLSA, "%s: algo=%d unknown",
                  name, cfg->algo);
    switch (cfg->noise_method) {
        case CSE_NOISE_MCRA:
            if (mcra_check_params(name, &cfg->mcra) != CSE_OK) return CSE_EINVAL;
            break;
        case CSE_NOISE_SPP:
            if (spp_check_params(name, &cfg->spp) != CSE_OK) return CSE_EINVAL;
            break;
        case CSE_NOISE_PERCENTILE:
        case CSE_NOISE_MIN_TRACKING:
        case CSE_NOISE_TRUE:
            CSE_CHECK_ARG(false, "%s: noise method %d needs the whole clip (mcra or spp only)",
                          name, cfg->noise_method);
        case 5:
        case 6:
            CSE_CHECK_ARG(false, "%s: noise method %d (minstat, imcra) keeps state of another "
                          "size with coupled bins: not streamed (mcra or spp only)", name,
                          cfg->noise_method);
        default:
            CSE_CHECK_ARG(false, "%s: noise method %d unknown (mcra or spp only)", name,
                          cfg->noise_method);
    }
    CSE_CHECK_ARG(cfg->eps > 0.0, "%s: eps=%g not > 0", name, cfg->eps);
    CSE_CHECK_ARG(cfg->mu == cfg->mu, "%s: mu is NaN", name);
    return CSE_OK;
}

// the arguments a frame reads besides the launch's own (k, t0, the pointers)
static void online_fill_args(OnArgs& a, int n_fft, int hop, int algo, int noise_method,
                             const float* param, const cse_mcra_params_t* mcra,
                             const cse_spp_params_t* spp, double eps, double mu) {
    a.N = n_fft;
    a.log2n = __builtin_ctz((unsigned)n_fft);
    a.hop = hop;
    a.cell = cse_cell_t{};
    a.cell.algo = algo;
    a.cell.hop = hop;
    for (int i = 0; i < 8; ++i) a.cell.param[i] = param[i];
    a.mk = mcra_constants(mcra);
    a.sk = noise_method == CSE_NOISE_SPP ? spp_constants(spp) : SppK{};
    a.L = mcra->window_frames;
    a.K = spp->init_frames;
    a.eps = eps;
    a.mu = mu;
    a.inv_eps = (float)eps;
}

#ifndef CSE_ONLINE_DEVICE_ONLY
template <int ALGO>
static const void* push_fn(int method) {
    return method == CSE_NOISE_MCRA ? (const void*)online_push_kernel<ALGO, CSE_NOISE_MCRA>
                                    : (const void*)online_push_kernel<ALGO, CSE_NOISE_SPP>;
}
#endif  // !CSE_ONLINE_DEVICE_ONLY

}  // namespace cse

#ifndef CSE_ONLINE_DEVICE_ONLY

using namespace cse;

extern "C" int64_t cse_online_state_bytes(int n_fft, int64_t n_streams) {
    if (!online_shape_ok(n_fft) || n_streams < 0) return -1;
    return OnState(n_fft).total * n_streams;
}

extern "C" int cse_online_init(cse_online_t* h, const cse_online_config_t* cfg, int64_t n_streams,
                               void* state) {
    const char* name = "cse_online_init";
    CSE_CHECK_ARG(h && cfg, "%s: NULL handle or configuration", name);
    CSE_CHECK_ARG(n_streams >= 0 && n_streams < (1ll << 31), "%s: n_streams=%lld", name,
                  (long long)n_streams);
    CSE_CHECK_ARG(state || n_streams == 0, "%s: NULL state", name);
    if (online_check_config(name, cfg) != CSE_OK) return CSE_EINVAL;
    h->cfg = *cfg;
    h->cfg.mu = fmin(fmax(cfg->mu, 0.0), 0.9999);
    h->n_streams = n_streams;
    h->state = state;
    h->frames = 0;
    h->primed = 0;
    h->reserved = 0;
    return CSE_OK;
}

extern "C" int cse_online_prime(cse_online_t* h, const double* x_head, cse_stream_t stream) {
    const char* name = "cse_online_prime";
    CSE_CHECK_ARG(h && x_head, "%s: NULL handle or x_head", name);
    CSE_CHECK_ARG(online_shape_ok(h->cfg.n_fft), "%s: handle not initialised", name);
    h->frames = 0;
    h->primed = 1;
    if (h->n_streams == 0) return CSE_OK;
    hipLaunchKernelGGL(online_prime_kernel, dim3((unsigned)h->n_streams), dim3(GEN_NT), 0,
                       (hipStream_t)stream, (unsigned char*)h->state, h->cfg.n_fft, h->cfg.hop,
                       x_head);
    CSE_CHECK_LAUNCH(name);
    return CSE_OK;
}

extern "C" int cse_online_push(cse_online_t* h, const double* x, int k, float* y, float* n_out,
                               cse_stream_t stream) {
    const char* name = "cse_online_push";
    CSE_CHECK_ARG(h && x && y, "%s: NULL handle, x or y", name);
    CSE_CHECK_ARG(online_shape_ok(h->cfg.n_fft), "%s: handle not initialised", name);
    CSE_CHECK_ARG(k >= 0, "%s: k=%d", name, k);
    CSE_CHECK_ARG(h->primed == 1, "%s: not primed, or finished (cse_online_prime first)", name);
    const cse_online_config_t& c = h->cfg;
    if (k == 0 || h->n_streams == 0) return CSE_OK;
    CSE_CHECK_ARG(c.noise_method != CSE_NOISE_SPP || h->frames > 0 || k >= c.spp.init_frames,
                  "%s: k=%d < init_frames=%d on spp's first push", name, k, c.spp.init_frames);
    CSE_CHECK_ARG((int64_t)k * c.hop < (1ll << 30) && h->frames + k < (1ll << 40),
                  "%s: k=%d too many frames", name, k);
    OnArgs a;
    online_fill_args(a, c.n_fft, c.hop, c.algo, c.noise_method, c.param, &c.mcra, &c.spp, c.eps,
                     c.mu);
    a.k = k;
    a.t0 = h->frames;
    a.state = (unsigned char*)h->state;
    a.x = x;
    a.y = y;
    a.n_out = n_out;
    const void* fn = nullptr;
    switch (c.algo) {
        case CSE_ALGO_SS: fn = push_fn<CSE_ALGO_SS>(c.noise_method); break;
        case CSE_ALGO_WIENER: fn = push_fn<CSE_ALGO_WIENER>(c.noise_method); break;
        case CSE_ALGO_MMSE: fn = push_fn<CSE_ALGO_MMSE>(c.noise_method); break;
        default: fn = push_fn<CSE_ALGO_OMLSA>(c.noise_method); break;
    }
    const int bytes = OnLds(c.n_fft).total;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) {
        ::cse::set_error("%s: cannot reserve %d bytes of LDS", name, bytes);
        return CSE_ELAUNCH;
    }
    void* args[] = {&a};
    if (hipLaunchKernel(fn, dim3((unsigned)h->n_streams), dim3(GEN_NT), args, bytes,
                        (hipStream_t)stream) != hipSuccess) {
        ::cse::set_error("%s: launch failed", name);
        return CSE_ELAUNCH;
    }
    CSE_CHECK_LAUNCH(name);
    h->frames += k;
    return CSE_OK;
}

extern "C" int cse_online_finish(cse_online_t* h, float* y_tail, cse_stream_t stream) {
    const char* name = "cse_online_finish";
    CSE_CHECK_ARG(h && y_tail, "%s: NULL handle or y_tail", name);
    CSE_CHECK_ARG(online_shape_ok(h->cfg.n_fft), "%s: handle not initialised", name);
    CSE_CHECK_ARG(h->primed == 1, "%s: not primed, or finished already", name);
    h->primed = 0;
    if (h->n_streams == 0) return CSE_OK;
    hipLaunchKernelGGL(online_finish_kernel, dim3((unsigned)h->n_streams), dim3(GEN_NT), 0,
                       (hipStream_t)stream, (const unsigned char*)h->state, h->cfg.n_fft,
                       h->cfg.hop, h->frames, y_tail);
    CSE_CHECK_LAUNCH(name);
    return CSE_OK;
}
#endif  // !CSE_ONLINE_DEVICE_ONLY
