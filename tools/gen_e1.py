"""The tables of csrc/cse_e1.hpp (the fp64 exponential integral E1 of the
IMCRA tracker), computed with mpmath at 50 digits and printed as C++
initialisers, with the largest relative error of the tables evaluated in fp64,
in the header's way, against mpmath's E1 on a log grid.

  v < 1:   E1(v) = -(log v + gamma) + v A(v),  A(v) = sum_k a_k v^k,
           a_k = (-1)^k / ((k + 1) (k + 1)!), the power series, NA terms
  v >= 1:  E1(v) = exp(-v) w h(w),  w = 1 / v,  h(w) = v exp(v) E1(v): the
           Chebyshev interpolant of NC terms on w in [0, 1/4] and another on
           [1/4, 1], each rewritten in powers of x (x in [-1, 1] over the
           interval): their Chebyshev coefficients fall by 4 to 5 a term,
           faster than those of T_j grow, so the power form loses nothing

All three are evaluated by Horner's rule: one multiply-add a term, against
the Clenshaw recurrence's two.

    python tools/gen_e1.py            # prints the tables and the error
"""

import math

import mpmath as mp
import numpy as np

NA, NC = 17, 22
SPLIT = 0.25


def h(w):
    if w == 0:
        return mp.mpf(1)
    v = 1 / mp.mpf(w)
    return v * mp.exp(v) * mp.e1(v)


def cheb(f, a, b, n):
    """Chebyshev coefficients c_0 .. c_{n-1} of f on [a, b] (c_0 halved), mpf."""
    xs = [mp.cos(mp.pi * (k + mp.mpf(0.5)) / n) for k in range(n)]
    fs = [f((a + b) / 2 + (b - a) / 2 * x) for x in xs]
    c = [2 * mp.fsum(fs[k] * mp.cos(mp.pi * j * (k + mp.mpf(0.5)) / n) for k in range(n)) / n
         for j in range(n)]
    c[0] /= 2
    return c


def powers(c):
    """sum_j c_j T_j(x) as coefficients of x^k, fp64."""
    n = len(c)
    T = [[mp.mpf(1)], [mp.mpf(0), mp.mpf(1)]]
    for _ in range(2, n):
        up = [mp.mpf(0)] + [2 * x for x in T[-1]]
        T.append([x - y for x, y in zip(up, T[-2] + [mp.mpf(0)] * (len(up) - len(T[-2])))])
    out = [mp.mpf(0)] * n
    for j in range(n):
        for k, t in enumerate(T[j]):
            out[k] += c[j] * t
    return [float(x) for x in out]


def tables():
    a = [float(mp.mpf((-1) ** k) / ((k + 1) * mp.factorial(k + 1))) for k in range(NA)]
    return (a, powers(cheb(h, mp.mpf(0), mp.mpf(SPLIT), NC)),
            powers(cheb(h, mp.mpf(SPLIT), mp.mpf(1), NC)))


def horner(c, y):
    s = 0.0
    for ck in c[::-1]:
        s = s * y + ck
    return s


def e1(v, a, lo, hi):
    """The header's evaluation, in Python floats (fp64, no FMA)."""
    if v < 1.0:
        return -(math.log(v) + 0.5772156649015329) + v * horner(a, v)
    w = 1.0 / v
    c, x = (lo, 8.0 * w - 1.0) if w < SPLIT else (hi, (8.0 * w - 5.0) / 3.0)
    return math.exp(-v) * (w * horner(c, x))


def main():
    mp.mp.dps = 50
    a, lo, hi = tables()
    for name, t in (("E1_A", a), ("E1_LO", lo), ("E1_HI", hi)):
        print(f"constexpr double {name}[{len(t)}] = {{")
        for i in range(0, len(t), 3):
            print("    " + ", ".join(repr(x) for x in t[i:i + 3]) + ",")
        print("};")
    worst = 0.0
    for v in np.concatenate([np.logspace(-300, 0, 3001), np.logspace(0, math.log10(700), 6001),
                             np.nextafter(1.0, [0.0, 2.0]), np.nextafter(4.0, [0.0, 8.0])]):
        ref = mp.e1(mp.mpf(float(v)))
        worst = max(worst, float(abs((mp.mpf(e1(float(v), a, lo, hi)) - ref) / ref)))
    print(f"// largest relative error against mpmath: {worst:.2e}")


if __name__ == "__main__":
    main()
