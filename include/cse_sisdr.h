/*
 * cse_sisdr.h — scale-invariant signal-to-distortion ratio (SI-SDR) and its
 * two parts, the scale-invariant signal-to-interference ratio (SI-SIR) and
 * signal-to-artifact ratio (SI-SAR), on the device, next to the entry points of
 * cse_lpc.h and cse_segsnr.h (same conventions: caller-owned device memory,
 * asynchronous on `stream`, CSE_OK or a negative code and a cse_last_error
 * message, no allocation in the library, all argument checks before any device
 * work).
 *
 * Le Roux, Wisdom, Erdogan & Hershey ("SDR - half-baked or well done?", ICASSP
 * 2019) define SI-SDR as the ratio of the projection of the test signal on the
 * clean signal to everything else, which makes it blind to the level of the
 * test signal (a cell that returns 0.7 clean scores +inf, not 10.5 dB).  The
 * sweep knows the interference exactly (noisy - clean), so the "everything
 * else" splits, as in Vincent, Gribonval & Fevotte (IEEE TASLP 14(4), 2006),
 * into the part that is still that interference and the rest, the artifacts.
 * The reference scores none of these, so this header is the specification.
 *
 * Inputs, per signal g, any rate, any len >= 1:
 *   s[n]  the clean signal, f64, length len.
 *   v[n] = noisy[n] - s[n], the interference: one fp64 subtraction.  noisy may
 *         be NULL: then there is no interference and only SI-SDR is defined.
 *   y[n]  the cell's test signal exactly as cse_stoi_cells defines it: f32 at
 *         y + y_offset[c], y[n - lag], zero outside [0, len), clipped to
 *         [-1, 1] when clip, then widened to f64.
 *
 * Sums, all in fp64 over n in [0, len); every product is an fp64 product of the
 * widened samples (it may be fused with the addition that follows it), and the
 * order of summation is free:
 *   per signal (cse_sisdr_prepare):  ss = <s,s>, vv = <v,v>, sv = <s,v>;
 *   per cell:                        ys = <y,s>, yv = <y,v>, yy = <y,y>.
 * With zero_mean != 0 also S = sum s, V = sum v per signal and Y = sum y per
 * cell, and each of the six sums above is replaced by its centred form
 *   <a,b> - (A * B) / len
 * taken as one multiplication, one division by (double)len and one
 * subtraction, in that order, each rounded on its own.
 *
 * Then, each line one chain of individually rounded fp64 operations as
 * written (no fused multiply-add), max(x, 0) being x when x > 0 and 0
 * otherwise:
 *   a  = ys / ss
 *   et = a * ys                           |projection of y on s|^2
 *   r2 = max(yy - et, 0)                  |y - a s|^2
 *   rv = yv - a * sv                      <y - a s, v>
 *   ei = (vv == 0) ? 0 : rv * rv / vv     interference part of the residual
 *   ea = max(r2 - ei, 0)                  artifact part
 *   sisdr = 10 log10(et / r2)
 *   sisir = 10 log10(et / ei)
 *   sisar = 10 log10(et / ea)
 * Without interference (noisy == NULL) only the first three lines and sisdr
 * exist.
 *
 * Otherwise plain IEEE semantics, with no further guards: 0/0 = NaN,
 * x/0 = +inf, log10(0) = -inf.  So ss == 0 or yy == 0 gives NaN for all
 * three; a cell with no interference left (ei == 0 < et) has sisir = +inf and
 * sisar = sisdr; y = g s with g != 0, where the sums are exact, gives +inf;
 * y orthogonal to s gives sisdr = -inf.  By construction
 *   10^(-sisdr/10) = 10^(-sisir/10) + 10^(-sisar/10)
 * wherever all three are finite.
 *
 * The unprocessed noisy input: y = s + v has a = 1 + sv/ss; its SI-SAR is
 * finite but carries no meaning (it is the part of (1 - a) s orthogonal to v,
 * not an artifact of any processing), so the results layer reports SI-SDR for
 * the noisy input and no sisar_noisy.
 *
 * Determinism: a cell's three values depend on its own inputs only (its
 * samples, lag, clip, and its signal's sums).  Scored alone or at any position
 * in a launch of any n_cells it returns the same bits: no floating-point
 * atomics, and the shape of the reduction is fixed by len and lag alone.
 *
 * cse_sisdr_workspace_bytes: bytes of the per-batch workspace (with_noise != 0:
 *   room for v as f64); -1 on a negative count.
 * cse_sisdr_prepare: once per batch of n_sig equal-length signals (clean and
 *   noisy: [n_sig][len] f64; noisy NULL: no interference): v and the sums.  The
 *   workspace then holds zero_mean, whether there is interference, the
 *   per-signal sums and, with interference, v as f64.  The library remembers,
 *   on the host, which of the workspaces it prepared last (CSE_SISDR_REMEMBERED
 *   of them) hold interference; that is how cse_sisdr_cells refuses sisir /
 *   sisar without it before any device work.  For a workspace it no longer
 *   remembers the device decides: such a cell's sisir and sisar are NaN.
 * cse_sisdr_scratch_bytes: bytes of per-launch scratch: 0 (the cell kernel
 *   keeps everything on chip; `scratch` may be NULL); -1 on a negative count.
 * cse_sisdr_cells: y, y_offset, lag (NULL = 0), sig_of as in cse_stoi_cells;
 *   clean is the array prepare was given.  sisdr[c], sisir[c], sisar[c] = the
 *   scores of cell c.  sisir and sisar may be NULL, both or neither; they must
 *   be NULL when prepare had no noisy.  sisdr may be NULL only if the other two
 *   are not.  n_cells == 0 or n_sig == 0 launches nothing.  CSE_EINVAL for NULL
 *   required pointers, negative counts, len < 1, or sisir / sisar requested
 *   without interference.
 */
#ifndef CSE_SISDR_H_
#define CSE_SISDR_H_

#include "cse.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CSE_SISDR_REMEMBERED 256

int64_t cse_sisdr_workspace_bytes(int64_t n_sig, int64_t len, int with_noise);
int cse_sisdr_prepare(const double* clean, const double* noisy, int64_t n_sig, int64_t len,
                      int zero_mean, void* workspace, cse_stream_t stream);
int64_t cse_sisdr_scratch_bytes(int64_t n_cells, int64_t len);
int cse_sisdr_cells(const float* y, const int64_t* y_offset, const int32_t* lag,
                    const int32_t* sig_of, int64_t n_cells, int64_t n_sig, int64_t len, int clip,
                    const double* clean, const void* workspace, void* scratch, double* sisdr,
                    double* sisir, double* sisar, cse_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* CSE_SISDR_H_ */
