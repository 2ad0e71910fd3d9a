// lse_double.h -- the log-sum-exp step of the log-domain lattices in DOUBLES (ctc_long.hip: the CTC loss beyond the wave lattice;
// ctc_segment.hip through lattice.h: the segment posteriors), ONCE.
#pragma once
#include "common.h"

namespace {

constexpr double LOG2E_D = 1.4426950408889634;
constexpr double LN2_D = 0.6931471805599453;
constexpr double NEG_INF_D = -(double)INFINITY;

// log2(2^a + 2^b [+ 2^c]) of lattice values in DOUBLES.  The values carry the whole utterance (|log2| up to 1e5 over 4000
// frames, where an fp32 ulp is 8e-3); the step's own part -- log2 of a sum in [1, 3] of powers 2^(x - max) <= 1 -- is taken
// with the raw fp32 instructions, as ctc_lattice_kernel's lse3_2 does: it is below 1.585 and comes back to within 1.5e-7, so
// a frame adds at most 1e-7 (in natural-log units) to a state, against the 1.2e-6 per frame that the fp32 emissions
// themselves are allowed, and the error is common to the states of a frame to first order (alpha + beta - log Z cancels it).
// The library's double exp2 / log2 here cost four times the frame time.  Branch-free: an all -inf input gives -inf.
__device__ __forceinline__ double lse_tail(double m, float sum) {
    return m + (double)__builtin_amdgcn_logf(sum);  // (sum == 0 only where m stands in for -inf: log2(0) = -inf)
}
__device__ __forceinline__ double lse2_long(double a, double b) {
    const double mx = fmax(a, b);
    const double m = mx == NEG_INF_D ? 0.0 : mx;
    return lse_tail(m, __builtin_amdgcn_exp2f((float)(a - m)) + __builtin_amdgcn_exp2f((float)(b - m)));
}
__device__ __forceinline__ double lse3_long(double a, double b, double c) {
    const double mx = fmax(a, fmax(b, c));
    const double m = mx == NEG_INF_D ? 0.0 : mx;
    return lse_tail(m, __builtin_amdgcn_exp2f((float)(a - m)) + __builtin_amdgcn_exp2f((float)(b - m)) +
                           __builtin_amdgcn_exp2f((float)(c - m)));
}

}  // namespace
