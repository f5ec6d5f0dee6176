// The pool of online streams (include/cse_online_pool.h): cse_online.hip's
// frames on slots that open, advance and close one by one.
//
// A slot is a header followed by the state block of cse_online.h.  What the
// lockstep push passes as kernel arguments for the whole batch (the cell
// parameters, the tracker's constants, mu) a slot keeps in its header, written
// once by cse_pool_open; what a step adds per item (slot, k, t0, where the
// item's samples begin) comes from a work list the step copies to the device.
// Both are read at addresses that are uniform over the workgroup, before the
// kernel's first store, so they are scalar loads into the SGPRs that hold the
// lockstep kernel's arguments.  The frames themselves are on_frames of
// cse_online.hip, included and not restated.
#define CSE_ONLINE_DEVICE_ONLY 1
#include "cse_online.hip"

#include "../../include/cse_online_pool.h"

namespace cse {

struct PoolHdr {  // the head of a slot's block
    cse_cell_t cell;
    McraK mk;
    SppK sk;
    int L, K;
    double mu;
    float inv_eps;
    int reserved;
};
static_assert(sizeof(PoolHdr) <= CSE_POOL_HEADER_BYTES, "the header's bytes");
static_assert(sizeof(PoolHdr) % 4 == 0, "written as 32-bit words");

struct PoolWork {  // one item of a step
    int32_t slot, k;
    int64_t t0;   // the slot's frames before this step
    int64_t off;  // frames of the items listed before this one
};
constexpr int POOL_COPY = 1024;  // records per host-to-device copy

struct PoolArgs {
    int N, log2n, hop;
    double eps;
    unsigned char* state;
    const PoolWork* work;
    const double* x;
    float* y;
    float* n_out;
};

__host__ __device__ inline int64_t pool_stride(int N) {
    return CSE_POOL_HEADER_BYTES + OnState(N).total;
}

template <int ALGO, int METHOD>
__global__ void __launch_bounds__(GEN_NT) pool_step_kernel(PoolArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const PoolWork w = p.work[blockIdx.x];
    unsigned char* slot = p.state + w.slot * pool_stride(p.N);
    const PoolHdr* __restrict__ h = (const PoolHdr*)slot;
    OnArgs a;
    a.N = p.N;
    a.log2n = p.log2n;
    a.hop = p.hop;
    a.k = w.k;
    a.t0 = w.t0;
    a.cell = h->cell;
    a.mk = h->mk;
    a.sk = h->sk;
    a.L = h->L;
    a.K = h->K;
    a.eps = p.eps;
    a.mu = h->mu;
    a.inv_eps = h->inv_eps;
    const int64_t B = p.N / 2 + 1;
    on_frames<ALGO, METHOD>(a, smem, slot + CSE_POOL_HEADER_BYTES, p.x + w.off * p.hop,
                            p.y + w.off * p.hop, p.n_out ? p.n_out + w.off * B : nullptr);
}

// the slot's state as cse_online_prime leaves it, and its header
__global__ void __launch_bounds__(GEN_NT) pool_open_kernel(unsigned char* slot, int N, int hop,
                                                           const double* x_head, PoolHdr hdr) {
    on_prime(slot + CSE_POOL_HEADER_BYTES, N, hop, x_head);
    const uint32_t* src = (const uint32_t*)&hdr;
    uint32_t* dst = (uint32_t*)slot;
    for (int i = threadIdx.x; i < CSE_POOL_HEADER_BYTES / 4; i += GEN_NT)
        dst[i] = i < (int)(sizeof(PoolHdr) / 4) ? src[i] : 0u;
}

__global__ void __launch_bounds__(GEN_NT) pool_close_kernel(const unsigned char* slot, int N,
                                                            int hop, int64_t T, float* y_tail) {
    __shared__ double wsq[2048];
    on_finish(slot + CSE_POOL_HEADER_BYTES, N, hop, T, y_tail, wsq);
}

template <int ALGO>
static const void* pool_fn(int method) {
    return method == CSE_NOISE_MCRA ? (const void*)pool_step_kernel<ALGO, CSE_NOISE_MCRA>
                                    : (const void*)pool_step_kernel<ALGO, CSE_NOISE_SPP>;
}

static bool pool_ready(const cse_pool_t* h) { return online_shape_ok(h->cfg.n_fft); }

}  // namespace cse

using namespace cse;

extern "C" int64_t cse_pool_state_bytes(int n_fft, int64_t capacity) {
    if (!online_shape_ok(n_fft) || capacity < 0) return -1;
    return pool_stride(n_fft) * capacity;
}

extern "C" int64_t cse_pool_work_bytes(int64_t capacity) {
    if (capacity < 0) return -1;
    return (capacity * (int64_t)sizeof(PoolWork) + 255) & ~(int64_t)255;
}

extern "C" int cse_pool_init(cse_pool_t* h, const cse_online_config_t* cfg, int64_t capacity,
                             void* state, void* work, cse_pool_slot_t* slots) {
    const char* name = "cse_pool_init";
    CSE_CHECK_ARG(h && cfg, "%s: NULL handle or configuration", name);
    CSE_CHECK_ARG(capacity >= 0 && capacity < (1ll << 31), "%s: capacity=%lld", name,
                  (long long)capacity);
    CSE_CHECK_ARG((state && work && slots) || capacity == 0, "%s: NULL state, work or slots", name);
    if (online_check_config(name, cfg) != CSE_OK) return CSE_EINVAL;
    h->cfg = *cfg;
    h->cfg.mu = fmin(fmax(cfg->mu, 0.0), 0.9999);
    h->capacity = capacity;
    h->state = state;
    h->work = work;
    h->slots = slots;
    for (int64_t s = 0; s < capacity; ++s) slots[s] = cse_pool_slot_t{0, 0, 0};
    return CSE_OK;
}

extern "C" int cse_pool_open(cse_pool_t* h, int64_t slot, const cse_pool_params_t* prm,
                             const double* x_head, cse_stream_t stream) {
    const char* name = "cse_pool_open";
    CSE_CHECK_ARG(h && x_head, "%s: NULL handle or x_head", name);
    CSE_CHECK_ARG(pool_ready(h), "%s: handle not initialised", name);
    CSE_CHECK_ARG(slot >= 0 && slot < h->capacity, "%s: slot=%lld outside [0, %lld)", name,
                  (long long)slot, (long long)h->capacity);
    CSE_CHECK_ARG(h->slots[slot].open == 0, "%s: slot=%lld is open", name, (long long)slot);
    const cse_online_config_t& c = h->cfg;
    const float* param = prm ? prm->param : c.param;
    const cse_mcra_params_t* mcra = prm ? &prm->mcra : &c.mcra;
    const cse_spp_params_t* spp = prm ? &prm->spp : &c.spp;
    const double mu_in = prm ? prm->mu : c.mu;
    if (c.noise_method == CSE_NOISE_MCRA) {
        if (mcra_check_params(name, mcra) != CSE_OK) return CSE_EINVAL;
    } else {
        if (spp_check_params(name, spp) != CSE_OK) return CSE_EINVAL;
    }
    CSE_CHECK_ARG(mu_in == mu_in, "%s: mu is NaN", name);
    OnArgs a;
    online_fill_args(a, c.n_fft, c.hop, c.algo, c.noise_method, param, mcra, spp, c.eps,
                     fmin(fmax(mu_in, 0.0), 0.9999));
    PoolHdr hdr;
    hdr.cell = a.cell;
    hdr.mk = a.mk;
    hdr.sk = a.sk;
    hdr.L = a.L;
    hdr.K = a.K;
    hdr.mu = a.mu;
    hdr.inv_eps = a.inv_eps;
    hdr.reserved = 0;
    hipLaunchKernelGGL(pool_open_kernel, dim3(1), dim3(GEN_NT), 0, (hipStream_t)stream,
                       (unsigned char*)h->state + slot * pool_stride(c.n_fft), c.n_fft, c.hop,
                       x_head, hdr);
    CSE_CHECK_LAUNCH(name);
    h->slots[slot].frames = 0;
    h->slots[slot].open = 1;
    h->slots[slot].first_frames = c.noise_method == CSE_NOISE_SPP ? spp->init_frames : 1;
    return CSE_OK;
}

extern "C" int cse_pool_step(cse_pool_t* h, const cse_pool_item_t* items, int n, const double* x,
                             float* y, float* n_out, cse_stream_t stream) {
    const char* name = "cse_pool_step";
    CSE_CHECK_ARG(h && items && x && y, "%s: NULL handle, items, x or y", name);
    CSE_CHECK_ARG(pool_ready(h), "%s: handle not initialised", name);
    CSE_CHECK_ARG(n >= 0, "%s: n=%d", name, n);
    if (n == 0) return CSE_OK;
    const cse_online_config_t& c = h->cfg;
    cse_pool_slot_t* slots = h->slots;
    // every refusal first; a listed slot is marked open == 2 until the list is through
    int64_t total = 0;
    int seen = 0, rc = CSE_OK;
    for (; seen < n && rc == CSE_OK; ++seen) {
        const int64_t s = items[seen].slot;
        const int k = items[seen].k;
        rc = CSE_EINVAL;
        if (s < 0 || s >= h->capacity)
            set_error("%s: item %d: slot=%lld outside [0, %lld)", name, seen, (long long)s,
                      (long long)h->capacity);
        else if (slots[s].open == 2)
            set_error("%s: item %d: slot=%lld listed twice", name, seen, (long long)s);
        else if (slots[s].open != 1)
            set_error("%s: item %d: slot=%lld is not open", name, seen, (long long)s);
        else if (k < 1)
            set_error("%s: item %d: k=%d < 1", name, seen, k);
        else if (slots[s].frames == 0 && k < slots[s].first_frames)
            set_error("%s: item %d: k=%d < init_frames=%d on an spp slot's first step", name, seen,
                      k, slots[s].first_frames);
        else if ((total + k) * c.hop >= (1ll << 30) || slots[s].frames + k >= (1ll << 40))
            set_error("%s: item %d: k=%d too many frames", name, seen, k);
        else {
            rc = CSE_OK;
            slots[s].open = 2;
            total += k;
        }
    }
    if (rc != CSE_OK) --seen;  // the refused item was not marked
    for (int i = 0; i < seen; ++i) slots[items[i].slot].open = 1;
    if (rc != CSE_OK) return rc;

    // the list: pageable host memory, which hipMemcpyAsync has read when it returns
    PoolWork rec[POOL_COPY];
    int64_t off = 0;
    for (int i0 = 0; i0 < n; i0 += POOL_COPY) {
        const int m = n - i0 < POOL_COPY ? n - i0 : POOL_COPY;
        for (int i = 0; i < m; ++i) {
            const cse_pool_item_t& it = items[i0 + i];
            rec[i] = PoolWork{it.slot, it.k, slots[it.slot].frames, off};
            off += it.k;
        }
        if (hipMemcpyAsync((PoolWork*)h->work + i0, rec, (size_t)m * sizeof(PoolWork),
                           hipMemcpyHostToDevice, (hipStream_t)stream) != hipSuccess) {
            set_error("%s: the work list's copy failed", name);
            return CSE_ELAUNCH;
        }
    }
    PoolArgs p;
    p.N = c.n_fft;
    p.log2n = __builtin_ctz((unsigned)c.n_fft);
    p.hop = c.hop;
    p.eps = c.eps;
    p.state = (unsigned char*)h->state;
    p.work = (const PoolWork*)h->work;
    p.x = x;
    p.y = y;
    p.n_out = n_out;
    const void* fn = nullptr;
    switch (c.algo) {
        case CSE_ALGO_SS: fn = pool_fn<CSE_ALGO_SS>(c.noise_method); break;
        case CSE_ALGO_WIENER: fn = pool_fn<CSE_ALGO_WIENER>(c.noise_method); break;
        case CSE_ALGO_MMSE: fn = pool_fn<CSE_ALGO_MMSE>(c.noise_method); break;
        default: fn = pool_fn<CSE_ALGO_OMLSA>(c.noise_method); break;
    }
    const int bytes = OnLds(c.n_fft).total;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) {
        set_error("%s: cannot reserve %d bytes of LDS", name, bytes);
        return CSE_ELAUNCH;
    }
    void* args[] = {&p};
    if (hipLaunchKernel(fn, dim3((unsigned)n), dim3(GEN_NT), args, bytes, (hipStream_t)stream) !=
        hipSuccess) {
        set_error("%s: launch failed", name);
        return CSE_ELAUNCH;
    }
    CSE_CHECK_LAUNCH(name);
    for (int i = 0; i < n; ++i) slots[items[i].slot].frames += items[i].k;
    return CSE_OK;
}

extern "C" int cse_pool_close(cse_pool_t* h, int64_t slot, float* y_tail, cse_stream_t stream) {
    const char* name = "cse_pool_close";
    CSE_CHECK_ARG(h && y_tail, "%s: NULL handle or y_tail", name);
    CSE_CHECK_ARG(pool_ready(h), "%s: handle not initialised", name);
    CSE_CHECK_ARG(slot >= 0 && slot < h->capacity, "%s: slot=%lld outside [0, %lld)", name,
                  (long long)slot, (long long)h->capacity);
    CSE_CHECK_ARG(h->slots[slot].open == 1, "%s: slot=%lld is not open", name, (long long)slot);
    hipLaunchKernelGGL(pool_close_kernel, dim3(1), dim3(GEN_NT), 0, (hipStream_t)stream,
                       (const unsigned char*)h->state + slot * pool_stride(h->cfg.n_fft),
                       h->cfg.n_fft, h->cfg.hop, h->slots[slot].frames, y_tail);
    CSE_CHECK_LAUNCH(name);
    h->slots[slot].open = 0;
    return CSE_OK;
}

extern "C" int cse_pool_drop(cse_pool_t* h, int64_t slot) {
    const char* name = "cse_pool_drop";
    CSE_CHECK_ARG(h, "%s: NULL handle", name);
    CSE_CHECK_ARG(pool_ready(h), "%s: handle not initialised", name);
    CSE_CHECK_ARG(slot >= 0 && slot < h->capacity, "%s: slot=%lld outside [0, %lld)", name,
                  (long long)slot, (long long)h->capacity);
    CSE_CHECK_ARG(h->slots[slot].open == 1, "%s: slot=%lld is not open", name, (long long)slot);
    h->slots[slot].open = 0;
    return CSE_OK;
}
