// Temporal noise reduction in: the definition of risp_raw_temporal (include/risp.h states it; tests/temporal_reference.py restates it
// in numpy int64).
//
//     c: the current frame, p: the state (the previous filtered frame), both in the sample domain the route demosaics
//     the window: the full 5 x 5 around (y,x), all colours; indices outside the frame reflected without repeating the edge
//     A  = sum over the window of (c - p)        signed, |A| <= 25 * 65535
//     B  = sum over the window of p
//     Bs = max(B - 25 * black_level, 0)
//     lo = 25 * threshold + ((Bs * slope) >> 8)
//     e  = min(max(|A| - lo, 0), 65535)
//     k  = min(strength + ((e * ramp) >> 8), 256)
//     out(y,x) = (p(y,x) * (256 - k) + c(y,x) * k + 128) >> 8
//
// Every intermediate fits unsigned 32 bits: Bs < 2^21 and slope < 2^8, e and ramp < 2^16, p, c < 2^16 and k <= 2^8 - so every product
// is one of two factors below 2^24 whose result stays below 2^32, which the 24-bit multiply gives exactly at full rate (the 32-bit
// one issues at a quarter).  With k == 256 the blend is (c * 256 + 128) >> 8 == c.
#pragma once
#include "risp_common.h"

namespace risp_temporal {

struct Params {
    unsigned strength;          // 0 .. 256, Q8
    unsigned thr25;             // 25 * threshold
    unsigned slope;             // 0 .. 255, Q8
    unsigned ramp;              // 0 .. 65535, Q8 per code of summed excess
    unsigned black25;           // 25 * black_level
};

// the sample c over the state p, A and B the window sums around it
__device__ __forceinline__ unsigned blend(unsigned c, unsigned p, int A, unsigned B, const Params &q) {
    const unsigned bs = B > q.black25 ? B - q.black25 : 0u;
    const unsigned lo = q.thr25 + (__umul24(bs, q.slope) >> 8);
    const unsigned mag = (unsigned)(A < 0 ? -A : A);
    unsigned e = mag > lo ? mag - lo : 0u;
    e = e < 65535u ? e : 65535u;
    unsigned k = q.strength + (__umul24(e, q.ramp) >> 8);
    k = k < 256u ? k : 256u;
    return (__umul24(p, 256u - k) + __umul24(c, k) + 128u) >> 8;
}

}  // namespace risp_temporal
