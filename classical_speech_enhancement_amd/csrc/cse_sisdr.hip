// SI-SDR, SI-SIR and SI-SAR (include/cse_sisdr.h) on the device.
//
// Six inner products per cell over the whole clip, three of them against
// samples every cell of a signal shares: a bandwidth kernel.  Per sample it
// moves 4 B of y (f32, read once, from HBM) and 16 B of s and v (f64, shared by
// every cell of the signal: from L2 / Infinity Cache), and spends one
// conversion, the clip and four fp64 operations (three v_fma_f64, one add).
//
// One workgroup of four waves per cell.  The samples are taken in chunks of
// four at n = 4 k, whatever the addresses: the 16-byte loads are declared with
// the alignment the data has (4 B for y, whose address moves with y_offset -
// lag; 8 B for s and v), which gfx950 serves as one global_load_dwordx4 each.
// So the split of the samples over lanes and accumulators depends on len and
// lag alone, not on where the buffers lie.  Only chunks that lie inside the
// cell's valid range [max(0, lag), min(len, len + lag)) are loaded whole; the
// at most three samples on either side of them go one to a lane.  Outside that
// range y is zero and adds nothing to any sum, so nothing is read there.
//
// A lane owns the chunks j = tid + NT i and rotates them over U accumulator
// sets: U chunks' loads (80 B each) are issued before the first is used, and
// the U x 4 fp64 chains are independent.  Reduction, fixed in shape: the
// lane's sets ((0 + 1) + (2 + 3)), a butterfly over the wave, LDS across the
// four waves, summed in order by thread 0, which then runs the header's chain
// with contraction off.
//
// cse_sisdr_prepare is the same loop over pairs of samples, one workgroup of
// 1024 threads per signal: v = noisy - s stored as f64, and ss, vv, sv, S, V.
#include "cse_common.hpp"

#include <mutex>

#include "../../include/cse_sisdr.h"

namespace cse {
namespace sisdr {

constexpr int NT = 256;    // threads per cell workgroup
constexpr int NW = NT / 64;
constexpr int U = 4;       // chunks in flight per lane, one accumulator set each
constexpr int PT = 1024;   // threads per prepare workgroup
constexpr int PW = PT / 64;
constexpr int HDR_BYTES = 64;   // int64: zero_mean, with_noise, n_sig, len
constexpr int SUM_STRIDE = 8;   // doubles per signal: ss, vv, sv, S, V

// 16-byte accesses at the alignment the data has
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
typedef double d2u __attribute__((ext_vector_type(2), aligned(8)));

struct Layout {
    int64_t lenp, sums, v, total;
};

static Layout layout(int64_t n_sig, int64_t len, int with_noise) {
    Layout L;
    L.lenp = (len + 1) & ~(int64_t)1;  // v rows start on 16 bytes
    L.sums = HDR_BYTES;
    L.v = (L.sums + n_sig * SUM_STRIDE * 8 + 255) & ~(int64_t)255;
    L.total = L.v + (with_noise ? n_sig * L.lenp * 8 : 0);
    return L;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// K sums over the workgroup's NWV waves: every lane's a[] in, the totals in
// thread 0's a[] out.  Fixed shape: butterfly in the wave, then the waves in order.
template <int K, int NWV>
__device__ __forceinline__ void block_sum(double (&a)[K], double (*red)[K], int tid) {
#pragma unroll
    for (int k = 0; k < K; ++k) a[k] = wave_sum(a[k]);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) red[tid >> 6][k] = a[k];
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            double t = red[0][k];
            for (int w = 1; w < NWV; ++w) t += red[w][k];
            a[k] = t;
        }
    }
}

// <a,b> - (A * B) / len: one multiplication, one division, one subtraction
__device__ __forceinline__ double centred(double ab, double A, double B, double dlen) {
#pragma clang fp contract(off)
    const double p = A * B;
    const double q = p / dlen;
    return ab - q;
}

// ---------------------------------------------------------------------------
// prepare: v and the per-signal sums
// ---------------------------------------------------------------------------
struct PrepAcc {
    double ss, vv, sv, s1, v1;
};

template <bool HAS_V>
__device__ __forceinline__ void prep_add(PrepAcc& A, double s, double v) {
    A.ss = fma(s, s, A.ss);
    A.s1 += s;
    if (HAS_V) {
        A.vv = fma(v, v, A.vv);
        A.sv = fma(s, v, A.sv);
        A.v1 += v;
    }
}

template <bool HAS_V>
__global__ void __launch_bounds__(PT) sisdr_prepare_kernel(const double* clean, const double* noisy,
                                                           int64_t n_sig, int64_t len, int64_t lenp,
                                                           int zero_mean, int64_t* hdr, double* sums,
                                                           double* vout) {
    __shared__ double red[PW][5];
    const int tid = threadIdx.x;
    const int64_t g = blockIdx.x;
    if (g == 0 && tid == 0) {
        hdr[0] = zero_mean ? 1 : 0;
        hdr[1] = HAS_V ? 1 : 0;
        hdr[2] = n_sig;
        hdr[3] = len;
    }
    const double* s = clean + g * len;
    const double* z = HAS_V ? noisy + g * len : nullptr;
    double* v = HAS_V ? vout + g * lenp : nullptr;
    PrepAcc acc[2] = {};
    const int64_t npair = len >> 1;
    for (int64_t j = tid; j < npair; j += 2 * PT) {
        const int64_t j1 = j + PT;
        const bool two = j1 < npair;
        const d2u sa = *(const d2u*)(s + 2 * j);
        const d2u sb = two ? *(const d2u*)(s + 2 * j1) : d2u{0.0, 0.0};
        d2u va = {0.0, 0.0}, vb = {0.0, 0.0};
        if (HAS_V) {
            const d2u za = *(const d2u*)(z + 2 * j);
            const d2u zb = two ? *(const d2u*)(z + 2 * j1) : d2u{0.0, 0.0};
            va = za - sa;
            vb = zb - sb;
            *(d2u*)(v + 2 * j) = va;
            if (two) *(d2u*)(v + 2 * j1) = vb;
        }
        prep_add<HAS_V>(acc[0], sa.x, va.x);
        prep_add<HAS_V>(acc[0], sa.y, va.y);
        if (two) {
            prep_add<HAS_V>(acc[1], sb.x, vb.x);
            prep_add<HAS_V>(acc[1], sb.y, vb.y);
        }
    }
    if (tid == 0 && (len & 1)) {  // the odd sample out
        const double sl = s[len - 1];
        double vl = 0.0;
        if (HAS_V) {
            vl = z[len - 1] - sl;
            v[len - 1] = vl;
        }
        prep_add<HAS_V>(acc[0], sl, vl);
    }
    double t[5] = {acc[0].ss + acc[1].ss, acc[0].vv + acc[1].vv, acc[0].sv + acc[1].sv,
                   acc[0].s1 + acc[1].s1, acc[0].v1 + acc[1].v1};
    block_sum<5, PW>(t, red, tid);
    if (tid == 0) {
        const double dlen = (double)len;
        double ss = t[0], vv = t[1], sv = t[2];
        if (zero_mean) {
            ss = centred(ss, t[3], t[3], dlen);
            vv = centred(vv, t[4], t[4], dlen);
            sv = centred(sv, t[3], t[4], dlen);
        }
        double* o = sums + g * SUM_STRIDE;
        o[0] = ss;
        o[1] = vv;
        o[2] = sv;
        o[3] = t[3];
        o[4] = t[4];
        o[5] = o[6] = o[7] = 0.0;
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
    int64_t n_sig, len, lenp;
    int clip;
    const double* clean;
    const int64_t* hdr;
    const double* sums;
    const double* v;
    double *sisdr, *sisir, *sisar;
};

struct Acc {
    double ys, yv, yy, y1;
};

template <bool HAS_V>
__device__ __forceinline__ void cell_add(Acc& A, float yf, double s, double v, bool clip) {
    if (clip) yf = fminf(fmaxf(yf, -1.0f), 1.0f);
    const double y = (double)yf;
    A.ys = fma(y, s, A.ys);
    if (HAS_V) A.yv = fma(y, v, A.yv);
    A.yy = fma(y, y, A.yy);
    A.y1 += y;
}

template <bool HAS_V>
__device__ __forceinline__ void chunk_add(Acc& A, f4u y, d2u s0, d2u s1, d2u v0, d2u v1, bool clip) {
    cell_add<HAS_V>(A, y.x, s0.x, v0.x, clip);
    cell_add<HAS_V>(A, y.y, s0.y, v0.y, clip);
    cell_add<HAS_V>(A, y.z, s1.x, v1.x, clip);
    cell_add<HAS_V>(A, y.w, s1.y, v1.y, clip);
}

// the header's chain, every operation rounded on its own
__device__ __forceinline__ void finish(double ys, double yv, double yy, double ss, double vv,
                                       double sv, bool has_v, double& sdr, double& sir,
                                       double& sar) {
#pragma clang fp contract(off)
    const double a = ys / ss;
    const double et = a * ys;
    const double d = yy - et;
    const double r2 = d > 0.0 ? d : 0.0;
    sdr = 10.0 * log10(et / r2);
    if (has_v) {
        const double av = a * sv;
        const double rv = yv - av;
        const double rr = rv * rv;
        const double ei = vv == 0.0 ? 0.0 : rr / vv;
        const double e = r2 - ei;
        const double ea = e > 0.0 ? e : 0.0;
        sir = 10.0 * log10(et / ei);
        sar = 10.0 * log10(et / ea);
    }
}

template <bool HAS_V>
__global__ void __launch_bounds__(NT) sisdr_cells_kernel(CellArgs a) {
    __shared__ double red[NW][4];
    const int tid = threadIdx.x;
    const int64_t cell = blockIdx.x;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const int64_t sig = a.sig_of[cell];
    // a workspace prepared for other sizes, or a signal that is not there: NaN
    if (a.hdr[2] != a.n_sig || a.hdr[3] != a.len || sig < 0 || sig >= a.n_sig) {
        if (tid == 0) {
            if (a.sisdr) a.sisdr[cell] = nan;
            if (a.sisir) a.sisir[cell] = nan;
            if (a.sisar) a.sisar[cell] = nan;
        }
        return;
    }
    const bool zero_mean = a.hdr[0] != 0;
    // interference asked for from a workspace without it (only when the host no
    // longer remembers the workspace): v reads s, and NaN is written below
    const bool noise = HAS_V && a.hdr[1] != 0;
    const bool clip = a.clip != 0;
    const int64_t lag = a.lag ? a.lag[cell] : 0;
    const int64_t len = a.len;
    const double* s = a.clean + sig * len;
    const double* v = noise ? a.v + sig * a.lenp : s;
    const float* y = a.y + a.y_offset[cell];  // the test sample at n is y[n - lag]
    const int64_t lo = lag > 0 ? (lag < len ? lag : len) : 0;
    int64_t hi = lag < 0 ? len + lag : len;
    if (hi < lo) hi = lo;
    const int64_t k0 = (lo + 3) >> 2, k1 = hi >> 2;
    const int64_t nck = k1 > k0 ? k1 - k0 : 0;

    Acc acc[U] = {};
    int64_t j = tid;
    for (; j + (U - 1) * NT < nck; j += U * NT) {
        f4u yy[U];
        d2u s0[U], s1[U], v0[U], v1[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {  // every load before the first use
            const int64_t n = 4 * (k0 + j + u * NT);
            yy[u] = *(const f4u*)(y + (n - lag));
            s0[u] = *(const d2u*)(s + n);
            s1[u] = *(const d2u*)(s + n + 2);
            if (HAS_V) {
                v0[u] = *(const d2u*)(v + n);
                v1[u] = *(const d2u*)(v + n + 2);
            } else {
                v0[u] = v1[u] = d2u{0.0, 0.0};
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) chunk_add<HAS_V>(acc[u], yy[u], s0[u], s1[u], v0[u], v1[u], clip);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {  // the last, incomplete round
        const int64_t jj = j + u * NT;
        if (jj < nck) {
            const int64_t n = 4 * (k0 + jj);
            const f4u yq = *(const f4u*)(y + (n - lag));
            const d2u sa = *(const d2u*)(s + n), sb = *(const d2u*)(s + n + 2);
            d2u va = {0.0, 0.0}, vb = {0.0, 0.0};
            if (HAS_V) {
                va = *(const d2u*)(v + n);
                vb = *(const d2u*)(v + n + 2);
            }
            chunk_add<HAS_V>(acc[u], yq, sa, sb, va, vb, clip);
        }
    }
    {   // the samples before the first and after the last whole chunk, one to a lane
        const int64_t he = 4 * k0 < hi ? 4 * k0 : hi;   // head: [lo, he)
        const int64_t ts = 4 * k1 > he ? 4 * k1 : he;   // tail: [ts, hi)
        const int64_t n = tid < 3 ? lo + tid : ts + (tid - 3);
        const bool mine = tid < 3 ? n < he : (tid < 6 && n < hi);
        if (mine) cell_add<HAS_V>(acc[0], y[n - lag], s[n], HAS_V ? v[n] : 0.0, clip);
    }
    double t[4] = {(acc[0].ys + acc[1].ys) + (acc[2].ys + acc[3].ys),
                   (acc[0].yv + acc[1].yv) + (acc[2].yv + acc[3].yv),
                   (acc[0].yy + acc[1].yy) + (acc[2].yy + acc[3].yy),
                   (acc[0].y1 + acc[1].y1) + (acc[2].y1 + acc[3].y1)};
    static_assert(U == 4, "the lane's sets are added as ((0 + 1) + (2 + 3))");
    block_sum<4, NW>(t, red, tid);
    if (tid == 0) {
        const double* sm = a.sums + sig * SUM_STRIDE;
        double ys = t[0], yv = t[1], yy = t[2];
        if (zero_mean) {
            const double dlen = (double)len;
            ys = centred(ys, t[3], sm[3], dlen);
            yv = centred(yv, t[3], sm[4], dlen);
            yy = centred(yy, t[3], t[3], dlen);
        }
        double sdr = nan, sir = nan, sar = nan;
        finish(ys, yv, yy, sm[0], sm[1], sm[2], noise, sdr, sir, sar);
        if (a.sisdr) a.sisdr[cell] = sdr;
        if (a.sisir) a.sisir[cell] = sir;
        if (a.sisar) a.sisar[cell] = sar;
    }
}

// which of the workspaces prepared last hold interference (host side, fixed size)
struct Seen {
    const void* ws;
    int64_t n_sig, len;
    int with_noise;
};
static Seen seen[CSE_SISDR_REMEMBERED];
static unsigned seen_next = 0;
static std::mutex seen_mu;

static void remember(const void* ws, int64_t n_sig, int64_t len, int with_noise) {
    std::lock_guard<std::mutex> lock(seen_mu);
    Seen* e = nullptr;
    for (Seen& q : seen)
        if (q.ws == ws) e = &q;
    if (!e) e = &seen[seen_next++ % CSE_SISDR_REMEMBERED];
    *e = Seen{ws, n_sig, len, with_noise};
}

static bool recall(const void* ws, Seen* out) {
    std::lock_guard<std::mutex> lock(seen_mu);
    for (const Seen& q : seen)
        if (q.ws == ws) {
            *out = q;
            return true;
        }
    return false;
}

static bool counts_ok(int64_t n_sig, int64_t len) {
    return n_sig >= 0 && n_sig <= 0x7fffffffLL && len >= 1 && len < ((int64_t)1 << 36);
}

}  // namespace sisdr
}  // namespace cse

using namespace cse;

extern "C" int64_t cse_sisdr_workspace_bytes(int64_t n_sig, int64_t len, int with_noise) {
    if (n_sig < 0 || len < 0) return -1;
    return sisdr::layout(n_sig, len, with_noise).total;
}

extern "C" int64_t cse_sisdr_scratch_bytes(int64_t n_cells, int64_t len) {
    if (n_cells < 0 || len < 0) return -1;
    return 0;
}

extern "C" int cse_sisdr_prepare(const double* clean, const double* noisy, int64_t n_sig,
                                 int64_t len, int zero_mean, void* workspace,
                                 cse_stream_t stream) {
    CSE_CHECK_ARG(clean && workspace, "cse_sisdr_prepare: NULL argument");
    CSE_CHECK_ARG(sisdr::counts_ok(n_sig, len), "cse_sisdr_prepare: n_sig=%lld len=%lld",
                  (long long)n_sig, (long long)len);
    if (n_sig == 0) return CSE_OK;
    const sisdr::Layout L = sisdr::layout(n_sig, len, noisy != nullptr);
    unsigned char* ws = (unsigned char*)workspace;
    int64_t* hdr = (int64_t*)ws;
    double* sums = (double*)(ws + L.sums);
    double* v = (double*)(ws + L.v);
    hipStream_t st = (hipStream_t)stream;
    if (noisy)
        hipLaunchKernelGGL(sisdr::sisdr_prepare_kernel<true>, dim3((unsigned)n_sig), dim3(sisdr::PT),
                           0, st, clean, noisy, n_sig, len, L.lenp, zero_mean, hdr, sums, v);
    else
        hipLaunchKernelGGL(sisdr::sisdr_prepare_kernel<false>, dim3((unsigned)n_sig),
                           dim3(sisdr::PT), 0, st, clean, noisy, n_sig, len, L.lenp, zero_mean, hdr,
                           sums, v);
    CSE_CHECK_LAUNCH("cse_sisdr_prepare");
    sisdr::remember(workspace, n_sig, len, noisy != nullptr);
    return CSE_OK;
}

extern "C" int cse_sisdr_cells(const float* y, const int64_t* y_offset, const int32_t* lag,
                               const int32_t* sig_of, int64_t n_cells, int64_t n_sig, int64_t len,
                               int clip, const double* clean, const void* workspace, void* scratch,
                               double* sisdr_out, double* sisir, double* sisar,
                               cse_stream_t stream) {
    (void)scratch;
    CSE_CHECK_ARG(y && y_offset && sig_of && clean && workspace, "cse_sisdr_cells: NULL argument");
    CSE_CHECK_ARG((sisir != nullptr) == (sisar != nullptr),
                  "cse_sisdr_cells: sisir and sisar go together (both or neither NULL)");
    CSE_CHECK_ARG(sisdr_out || sisir, "cse_sisdr_cells: no output");
    CSE_CHECK_ARG(n_cells >= 0 && n_cells <= 0x7fffffffLL && sisdr::counts_ok(n_sig, len),
                  "cse_sisdr_cells: n_cells=%lld n_sig=%lld len=%lld", (long long)n_cells,
                  (long long)n_sig, (long long)len);
    if (n_cells == 0 || n_sig == 0) return CSE_OK;
    sisdr::Seen e;
    int with_noise = 1;  // a workspace no longer remembered: the device decides
    if (sisdr::recall(workspace, &e)) {
        CSE_CHECK_ARG(e.n_sig == n_sig && e.len == len,
                      "cse_sisdr_cells: workspace prepared for n_sig=%lld len=%lld, not %lld, %lld",
                      (long long)e.n_sig, (long long)e.len, (long long)n_sig, (long long)len);
        with_noise = e.with_noise;
    }
    CSE_CHECK_ARG(!sisir || with_noise,
                  "cse_sisdr_cells: sisir / sisar requested, but cse_sisdr_prepare had no noisy");
    const sisdr::Layout L = sisdr::layout(n_sig, len, with_noise);
    const unsigned char* ws = (const unsigned char*)workspace;
    sisdr::CellArgs a;
    a.y = y;
    a.y_offset = y_offset;
    a.lag = lag;
    a.sig_of = sig_of;
    a.n_sig = n_sig;
    a.len = len;
    a.lenp = L.lenp;
    a.clip = clip;
    a.clean = clean;
    a.hdr = (const int64_t*)ws;
    a.sums = (const double*)(ws + L.sums);
    a.v = (const double*)(ws + L.v);
    a.sisdr = sisdr_out;
    a.sisir = sisir;
    a.sisar = sisar;
    hipStream_t st = (hipStream_t)stream;
    if (sisir)
        hipLaunchKernelGGL(sisdr::sisdr_cells_kernel<true>, dim3((unsigned)n_cells), dim3(sisdr::NT),
                           0, st, a);
    else
        hipLaunchKernelGGL(sisdr::sisdr_cells_kernel<false>, dim3((unsigned)n_cells),
                           dim3(sisdr::NT), 0, st, a);
    CSE_CHECK_LAUNCH("cse_sisdr_cells");
    return CSE_OK;
}
