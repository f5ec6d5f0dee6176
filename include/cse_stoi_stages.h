/*
 * cse_stoi_stages.h — where the stages of STOI's clean side lie in a prepared
 * workspace (include/cse.h: cse_stoi_prepare; include/cse_estoi.h:
 * cse_estoi_prepare), for tests and tools that read them back.  A header of
 * its own like every later addition to libcse.so: the code of cse.h is part
 * of the enhance kernels' pinned source digest.
 *
 * cse_stoi_layout is host only: nothing is launched.  extended != 0 describes
 * a workspace of extended STOI.  out takes CSE_STOI_LAYOUT_N values, in this
 * order:
 *   byte offsets  coef64 (f64 [5][128], 16 kHz only), meta (i32 [n_sig][META]:
 *                 K, M, J, ok, nblk), x10 (f64 [n_sig][n10]), en (f64 [n_sig][F]),
 *                 kf (i32 [n_sig][F]), btab (i32 [n_sig][NBLK][BT]: D, j0, nf,
 *                 p[MAXD], sa[FB + 1], sb[FB + 1]), xtob (f64 [n_sig][Mmax][16]),
 *                 xstat (f64 [n_sig][Jmax][16][4]: norm, mean, 1 / (norm of the
 *                 mean-removed + eps), 0), hgen (f64, the generic filter, other
 *                 rates only), xcol (f64 [n_sig][Jmax][30][2]; -1 unless
 *                 extended), total (the workspace size)
 *   sizes         n10, F, Mmax, Jmax, NBLK
 *   constants     BT, META, MAXD, FB
 *   and           ntap, the taps of the generic filter at hgen (0 at 16 kHz)
 * Rows >= M of a signal, column 15 of xtob and xstat, and table entries past
 * D / nf / nblk are unspecified.  Returns -1, with a cse_last_error message,
 * for the arguments cse_stoi_workspace_bytes_sr refuses and for
 * n_out < CSE_STOI_LAYOUT_N.
 */
#ifndef CSE_STOI_STAGES_H_
#define CSE_STOI_STAGES_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CSE_STOI_LAYOUT_N 21
int cse_stoi_layout(int64_t n_sig, int64_t len, int sr, int extended, int64_t* out, int n_out);

#ifdef __cplusplus
}
#endif

#endif /* CSE_STOI_STAGES_H_ */
