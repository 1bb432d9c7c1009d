// griffinlim_project.hpp — the projection step of the Griffin-Lim iteration for one bin: the ONE function every kernel that
// forms the iterate calls (the update kernel of griffinlim.hip; the projecting frame load of tools/ablation), so that all of them
// produce the same bits:
//
//   A = R - m Rprev,   X = M A / (|A| + 1e-16)
//
// Every rounded operation is written out (fmaf, one product, one sum, sqrt, two quotients, two products) under
// `fp contract(off)`: the compiler is left no choice of its own.  The operations and what each costs:
//   a_c  = fmaf(-m, p_c, r_c)                 one rounding of the exact r_c - m p_c (no cancellation of rounded terms)
//   e    = exponent of max(|a_re|, |a_im|);  s_c = ldexp(a_c, -e)       exact: the larger |s_c| lies in [0.5, 1).  The smaller one
//                                             may fall below 2^-126 and lose bits there: at most 2^-150 absolute of a quotient <= 2
//   t    = s_im s_im,  n2 = fmaf(s_re, s_re, t),  n = sqrt(n2)          n = |s| within 2 u, no overflow or underflow for finite A
//   d    = n + ldexp(1e-16, -e)               the scaled 1e-16 is exact unless it is below 2^-126, where n >= 0.5 absorbs it
//   q_c  = s_c / d,   x_c = M q_c
// so x_c carries 5 u of its own value from the function and 2 u M |A| / (|A| + 1e-16) from the rounding of A
// (tests/griffinlim_rules.py: update_bound).  A = 0 gives s = 0, q = 0 and X = 0 exactly.
#pragma once
#include "fft_core.hpp"

namespace tac {

constexpr float GL_EPS = 1e-16f;

// prev == false: A = R (the first step, and momentum 0)
__device__ __forceinline__ cf gl_project(cf r, cf p, float m, float mag, bool prev) {
#pragma clang fp contract(off)
    const float ar = prev ? __builtin_fmaf(-m, p.x, r.x) : r.x;
    const float ai = prev ? __builtin_fmaf(-m, p.y, r.y) : r.y;
    const float big = __builtin_fmaxf(__builtin_fabsf(ar), __builtin_fabsf(ai));
    const int e = __builtin_amdgcn_frexp_expf(big);            // big = f 2^e, f in [0.5, 1); 0 for big == 0
    const float sr = __builtin_ldexpf(ar, -e), si = __builtin_ldexpf(ai, -e);
    const float t = si * si;
    const float n = __builtin_sqrtf(__builtin_fmaf(sr, sr, t));
    const float d = n + __builtin_ldexpf(GL_EPS, -e);
    const float qr = sr / d, qi = si / d;
    return mkc(mag * qr, mag * qi);
}

}  // namespace tac
