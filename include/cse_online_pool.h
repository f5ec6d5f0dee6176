/*
 * cse_online_pool.h — a pool of online streams on one state block: streams
 * open and close one at a time, every stream has parameter values and a frame
 * counter of its own, and one launch advances every stream that has frames
 * pending, each by its own number of frames.  What a stream computes is
 * cse_online.h's: FRAMING, PER FRAME, EMISSION, LATENCY and EQUALITY WITH
 * OFFLINE hold per slot word for word, with t counted from the slot's open.
 * Same conventions as cse_online.h: caller-owned memory, asynchronous on
 * `stream`, CSE_OK or a negative code and a cse_last_error message.
 *
 * FIXED PER POOL: n_fft, hop, algo, noise_method and eps of the
 * cse_online_config_t given to cse_pool_init (they select the kernel
 * instantiation, its LDS and block size; cse_online_init's rules and
 * refusals).  PER SLOT: cse_pool_params_t (param[8], mu, the tracker's
 * parameter struct with mcra.window_frames and spp.init_frames), the frame
 * counter, and whether the slot is open.  cfg's own param, mu, mcra and spp
 * are the values of a slot opened with prm == NULL.
 *
 * MEMORY.  state: cse_pool_state_bytes(n_fft, capacity) bytes of device
 * memory, work: cse_pool_work_bytes(capacity) bytes of device memory, both
 * 256-byte aligned; slots: a host array [capacity] of cse_pool_slot_t.  All
 * three are the caller's and stay valid while the handle is used; the library
 * allocates nothing.  cse_pool_t is plain data; the calls on one handle are
 * made from one thread at a time, in stream order.
 *
 * THE SLOT'S DEVICE BLOCK is a header of CSE_POOL_HEADER_BYTES followed by the
 * block of cse_online.h (STATE), unchanged: slot s begins at
 * s (CSE_POOL_HEADER_BYTES + cse_online_state_bytes(n_fft, 1)).  The header
 * holds what a lockstep push carries as kernel arguments: the cse_cell_t
 * parameters, the tracker's derived constants with window_frames and
 * init_frames, mu clipped to [0, 0.9999] and (float) eps.  cse_pool_open
 * writes it, from a record passed by value to its kernel: no host-to-device
 * copy.  A step reads it with loads that are uniform over the workgroup.
 *
 * cse_pool_state_bytes / cse_pool_work_bytes: the sizes; -1 for an
 *   unsupported n_fft or capacity < 0, 0 for capacity 0.
 * cse_pool_init: checks cfg as cse_online_init does (same cases, under this
 *   call's name), fills the handle and marks every slot free.  No device work.
 *   CSE_EINVAL also for capacity < 0 or >= 2^31 and for a NULL state, work or
 *   slots with capacity > 0.
 * cse_pool_open: slot becomes open with frame counter 0.  prm NULL: cfg's
 *   values.  x_head [n_fft - hop] f64 on the device is xp[0, n_fft - hop) of
 *   the stream (cse_online_prime's).  One workgroup zeroes the slot's state,
 *   loads the input tail and writes the header.  CSE_EINVAL before any launch
 *   for: a NULL handle or x_head; a slot outside [0, capacity); a slot that is
 *   open; tracker parameters their own entry point refuses; mu NaN.
 * cse_pool_step: n items {slot, k}, a host array.  x f64 is the
 *   concatenation, in list order, of each item's next k hop samples of its
 *   xp; y f32 has the same layout (each item's padded samples
 *   [t0 hop, (t0 + k) hop), t0 the slot's frame counter); n_out, if not NULL,
 *   holds each item's [k][B] rows in the same order.  The library writes one
 *   record {slot, k, t0, frames before this item in the list} per item into
 *   `work` (hipMemcpyAsync on `stream` from a host array that the call owns,
 *   1,024 records per copy, so one copy up to 1,024 items), launches one
 *   workgroup per item, and advances each listed slot's counter by its k.
 *   CSE_EINVAL before the copy and any launch, with all bookkeeping untouched,
 *   for: a NULL handle, items, x or y; n < 0; a slot outside [0, capacity); a
 *   slot that is not open; a slot listed twice (two workgroups on one block
 *   would race); k < 1; k < the slot's init_frames on an spp slot's first
 *   step; the list's frames times hop >= 2^30 or a slot's counter >= 2^40
 *   (cse_online_push's limits).  n == 0 launches nothing and returns CSE_OK.
 * cse_pool_close: y_tail [n_fft - hop] f32 on the device receives the slot's
 *   padded samples [T hop, (T - 1) hop + n_fft), T the slot's frame counter,
 *   as cse_online_finish emits them; the slot is free afterwards.  CSE_EINVAL
 *   for a NULL handle or y_tail, a slot outside [0, capacity), a free slot.
 * cse_pool_drop: host only; the slot is free again and nothing is emitted
 *   (the next cse_pool_open overwrites all of its state).  CSE_EINVAL for a
 *   NULL handle, a slot outside [0, capacity), a free slot.
 */
#ifndef CSE_ONLINE_POOL_H_
#define CSE_ONLINE_POOL_H_

#include "cse_online.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CSE_POOL_HEADER_BYTES 256

typedef struct cse_pool_params {
    float param[8];         /* as cse_cell_t.param */
    double mu;              /* noise smoothing (mmse, omlsa); 0 = none */
    cse_mcra_params_t mcra; /* read for CSE_NOISE_MCRA */
    cse_spp_params_t spp;   /* read for CSE_NOISE_SPP */
} cse_pool_params_t;        /* 128 bytes */

typedef struct cse_pool_item {
    int32_t slot;
    int32_t k; /* frames this step runs on the slot, >= 1 */
} cse_pool_item_t; /* 8 bytes; a host array */

typedef struct cse_pool_slot {
    int64_t frames;       /* frames run since the slot's open */
    int32_t open;         /* 1 between cse_pool_open and cse_pool_close / cse_pool_drop */
    int32_t first_frames; /* frames the first step must carry (spp: init_frames) */
} cse_pool_slot_t;        /* 16 bytes; host bookkeeping, the library's to write */

typedef struct cse_pool {
    cse_online_config_t cfg;
    int64_t capacity;
    void* state;            /* device, cse_pool_state_bytes */
    void* work;             /* device, cse_pool_work_bytes */
    cse_pool_slot_t* slots; /* host [capacity] */
} cse_pool_t;               /* 184 bytes */

int64_t cse_pool_state_bytes(int n_fft, int64_t capacity);
int64_t cse_pool_work_bytes(int64_t capacity);
int cse_pool_init(cse_pool_t* h, const cse_online_config_t* cfg, int64_t capacity, void* state,
                  void* work, cse_pool_slot_t* slots);
int cse_pool_open(cse_pool_t* h, int64_t slot, const cse_pool_params_t* prm,
                  const double* x_head, cse_stream_t stream);
int cse_pool_step(cse_pool_t* h, const cse_pool_item_t* items, int n, const double* x, float* y,
                  float* n_out, cse_stream_t stream);
int cse_pool_close(cse_pool_t* h, int64_t slot, float* y_tail, cse_stream_t stream);
int cse_pool_drop(cse_pool_t* h, int64_t slot);

#ifdef __cplusplus
}
#endif

#endif /* CSE_ONLINE_POOL_H_ */
