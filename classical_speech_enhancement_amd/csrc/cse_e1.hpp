// The exponential integral E1(v) = int_v^inf exp(-t) / t dt in fp64, for
// cse_imcra.hip (include/cse_imcra.h): v in [DBL_MIN, inf), relative error
// 3.2e-15 against mpmath on a log grid 1e-300 .. 700 (tools/gen_e1.py, which
// computes the tables below; the header's bound is 1e-13).
//
//   v < 1:   E1 = -(log v + gamma) + v A(v), A the power series, 17 terms
//   v >= 1:  E1 = exp(-v) w h(w), w = 1 / v, h(w) = v exp(v) E1(v): a polynomial
//            of 22 terms in x on w in [0, 1/4] and another on [1/4, 1], x in
//            [-1, 1] over the interval (Chebyshev interpolants in powers of x)
//            (one continued fraction for all of v >= 1 would need about 65
//            terms at v = 1, each a division)
//
// Both ranges are evaluated for every lane and one is selected: the lengths
// are fixed, there is no loop that depends on v and no branch.  The two tables
// of v >= 1 are selected per coefficient, so one polynomial is evaluated, by
// Horner's rule: the kernel is bound by the instructions a lone wave issues,
// not by the depth of this chain (Estrin's scheme, 5 dependent steps for 21,
// was measured 2 % slower; the Clenshaw recurrence on the Chebyshev
// coefficients costs two operations a term).
// exp(-v) is an argument: the caller has it already (the header's p).  It is 0
// above 745, and so is the result.
#ifndef CSE_E1_HPP_
#define CSE_E1_HPP_

#include <math.h>

#if defined(__HIPCC__)
#define CSE_E1_FN __host__ __device__ inline
#else
#define CSE_E1_FN inline
#endif

namespace cse {

constexpr int E1_NA = 17, E1_NC = 22;
// (-1)^k / ((k + 1) (k + 1)!)
constexpr double E1_A[E1_NA] = {
    1.0, -0.25, 0.05555555555555555,
    -0.010416666666666666, 0.0016666666666666668, -0.0002314814814814815,
    2.834467120181406e-05, -3.1001984126984127e-06, 3.0619243582206544e-07,
    -2.755731922398589e-08, 2.27746439867652e-09, -1.7397297489890083e-10,
    1.2353110643708935e-11, -8.193389712664089e-13, 5.0981091545465446e-14,
    -2.9871733327421158e-15, 1.6537983849091297e-16,
};
// h on w in [0, 1/4] in powers of x = 8 w - 1
constexpr double E1_LO[E1_NC] = {
    0.8982371140279957, -0.08413402625195116, 0.013618587371441594,
    -0.002924527776028665, 0.000753038643404985, -0.00022070913434590653,
    7.137986785019903e-05, -2.4960777443526394e-05, 9.306374846412745e-06,
    -3.66055994458505e-06, 1.5005816602993519e-06, -6.418753370880593e-07,
    3.037783461006505e-07, -1.4116800119767527e-07, 3.1009386280519465e-08,
    -1.188433344661462e-08, 4.807307742638637e-08, -2.680693764259844e-08,
    -1.7516015015644236e-08, 1.0370433083101574e-08, 7.590115848414773e-09,
    -4.333997118286989e-09,
};
// h on w in [1/4, 1] in powers of x = (8 w - 5) / 3
constexpr double E1_HI[E1_NC] = {
    0.6839807604790853, -0.10700998634737262, 0.024557244273056604,
    -0.006733165717135658, 0.002055327824675905, -0.0006752252637980559,
    0.00023418543348323646, -8.471115853895918e-05, 3.169739337994008e-05,
    -1.2196879404240793e-05, 4.803460020929566e-06, -1.931117634054129e-06,
    7.95745857881501e-07, -3.309675546578763e-07, 1.2916976335526266e-07,
    -5.477351463643987e-08, 3.5970712479736875e-08, -1.595825693855869e-08,
    -2.1598147351337004e-09, 1.088043575210975e-09, 3.3734874258382277e-09,
    -1.5453481883549762e-09,
};

// E1(v) for v >= DBL_MIN; emv = exp(-v)
CSE_E1_FN double e1(double v, double emv) {
    // v < 1 (evaluated at min(v, 1), so that the other lanes stay finite)
    const double vs = fmin(v, 1.0);
    double a = E1_A[E1_NA - 1];
#pragma unroll
    for (int k = E1_NA - 2; k >= 0; --k) a = fma(a, vs, E1_A[k]);
    const double small = fma(vs, a, -(log(vs) + 0.5772156649015329));
    // v >= 1 (evaluated at max(v, 1))
    const double w = 1.0 / fmax(v, 1.0);
    const bool lo = w < 0.25;
    const double x = lo ? fma(8.0, w, -1.0) : fma(8.0, w, -5.0) * (1.0 / 3.0);
    double h = lo ? E1_LO[E1_NC - 1] : E1_HI[E1_NC - 1];
#pragma unroll
    for (int k = E1_NC - 2; k >= 0; --k) h = fma(h, x, lo ? E1_LO[k] : E1_HI[k]);
    return v < 1.0 ? small : emv * (w * h);
}

}  // namespace cse

#endif  // CSE_E1_HPP_
