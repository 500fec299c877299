// Defective-pixel correction in: the definition of risp_raw_defect (include/risp.h states it; tests/defect_reference.py restates it
// in numpy).
//
//     S(y,x): the decoded raw sample of the frame as stored, indices outside the frame reflected without repeating the edge
//     pairs, in this order:  H  S(y,x-2), S(y,x+2)      V  S(y-2,x), S(y+2,x)      D  S(y-2,x-2), S(y+2,x+2)      A  S(y-2,x+2), S(y+2,x-2)
//     mx, mn = maximum and minimum of the eight;   T(v) = threshold + ((v * slope) >> 8)
//     hot  p > mx + T(mx);   dead  p + T(mn) < mn;   listed  the pixel's bit of the defect map
//     a hot, dead or listed pixel becomes (a + b + 1) >> 1 of the pair with the smallest |a - b|, the first such pair in the order
//     above; every other pixel passes
//
// All in unsigned 32-bit arithmetic.  Nothing wraps there - the largest terms are 65535 + 65535 + (65535 * 255 >> 8) and
// 65535 + 65535 + 1 - but mx + T(mx), p + T(mn) and a + b + 1 pass 2^16: a form that keeps these sums in packed 16-bit lanes
// (v_pk_add_u16) is wrong, at (65535, 255) it corrects pixels of a full-range frame that the definition leaves alone.  The maxima,
// minima and differences alone would fit 16 bits.
//
// The dynamic test is switched off by a threshold no sum can reach (NO_THRESHOLD with slope 0): mx + 2^31 and p + 2^31 stay below
// 2^32 and above every sample, so neither comparison holds and the kernels need no second form.
#pragma once
#include "risp_common.h"

namespace risp_defect {

constexpr unsigned NO_THRESHOLD = 0x80000000u;

__device__ __forceinline__ unsigned umax(unsigned a, unsigned b) { return a > b ? a : b; }
__device__ __forceinline__ unsigned umin(unsigned a, unsigned b) { return a < b ? a : b; }

// the sample at p with the pairs h, v, d, a around it; `listed`: its bit of the defect map
__device__ __forceinline__ unsigned correct(unsigned p, unsigned h0, unsigned h1, unsigned v0, unsigned v1, unsigned d0, unsigned d1,
                                            unsigned a0, unsigned a1, bool listed, unsigned threshold, unsigned slope) {
    const unsigned mx = umax(umax(umax(h0, h1), umax(v0, v1)), umax(umax(d0, d1), umax(a0, a1)));
    const unsigned mn = umin(umin(umin(h0, h1), umin(v0, v1)), umin(umin(d0, d1), umin(a0, a1)));
    // (a sample is below 2^16 and the slope below 2^8: the 24-bit multiply is exact and issues at full rate, the 32-bit one at a quarter)
    const bool hot = p > mx + threshold + (__umul24(mx, slope) >> 8);
    const bool dead = p + threshold + (__umul24(mn, slope) >> 8) < mn;
    unsigned best = umax(h0, h1) - umin(h0, h1), sum = h0 + h1;
    unsigned diff = umax(v0, v1) - umin(v0, v1);
    if (diff < best) best = diff, sum = v0 + v1;
    diff = umax(d0, d1) - umin(d0, d1);
    if (diff < best) best = diff, sum = d0 + d1;
    diff = umax(a0, a1) - umin(a0, a1);
    if (diff < best) sum = a0 + a1;
    return hot || dead || listed ? (sum + 1u) >> 1 : p;
}

}  // namespace risp_defect
