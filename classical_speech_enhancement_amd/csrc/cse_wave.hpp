// Wave-level primitives of the score kernels: ordering of a wave's LDS
// accesses and fp64 sums over its lanes without LDS traffic.  Included by
// cse_cells.hpp (and through it cse_segfft.hpp) and cse_lpc.hip.
// cse_minstat.hip keeps a wave_sum of its own: its row steps are mov_dpp with
// bound_ctrl, which saves the zeroed target that update_dpp takes here, on a
// serial chain where that shows; cse_stoi.hip, cse_sisdr.hip and
// cse_logerr.hip keep theirs too (a butterfly with another summation order).
#ifndef CSE_WAVE_HPP_
#define CSE_WAVE_HPP_

#include "cse_common.hpp"

namespace cse {

// ordering of LDS accesses among the lanes of one wave (the LDS executes a
// wave's DS instructions in issue order: a compiler-level barrier suffices)
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int CTRL>
__device__ __forceinline__ double dpp_add(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, false);
    return v + __hiloint2double(hi, lo);
}

// sum over each row of 16 lanes, all 64 active; every lane gets its row's sum
// (quad swaps, then the half-row and row mirrors)
__device__ __forceinline__ double row_sum(double v) {
    v = dpp_add<0xB1>(v);   // quad_perm [1, 0, 3, 2]
    v = dpp_add<0x4E>(v);   // quad_perm [2, 3, 0, 1]
    v = dpp_add<0x141>(v);  // row_half_mirror
    v = dpp_add<0x140>(v);  // row_mirror
    return v;
}

__device__ __forceinline__ double row_sum_of(double v, int lane) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane),
                            __builtin_amdgcn_readlane(__double2loint(v), lane));
}

// Sum over the 64 lanes of a wave, all active; every lane gets the result.
// The four row sums by v_readlane: no LDS traffic, where __shfl_xor costs two
// ds_bpermute per step for a double.
__device__ __forceinline__ double wave_sum(double v) {
    v = row_sum(v);
    return (row_sum_of(v, 0) + row_sum_of(v, 16)) + (row_sum_of(v, 32) + row_sum_of(v, 48));
}

// The same sum with the rows added by two butterfly shuffles: (r0 + r16) +
// (r32 + r48) in every lane, so the bits are wave_sum's.  cse_lpc.hip uses
// this form (beside the shuffles of its autocorrelation); everything else
// uses wave_sum.
__device__ __forceinline__ double wave_sum_shfl(double v) {
    v = row_sum(v);
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}

}  // namespace cse

#endif  // CSE_WAVE_HPP_
