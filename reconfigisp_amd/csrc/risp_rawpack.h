// MIPI-packed RAW10 / RAW12 in: the definition risp_raw_unpack and the fused loads of risp_serve_packed /
// risp_serve_classical_packed share (include/risp.h states it; tests/raw_packed_reference.py restates it in numpy).
//
//     RAW10: pixels 4g .. 4g+3 of a row live in bytes 5g .. 5g+4:  P[4g+k] = byte[5g+k] << 2 | (byte[5g+4] >> 2k & 3)
//     RAW12: pixels 2g, 2g+1 live in bytes 3g .. 3g+2:             P[2g]   = byte[3g]   << 4 | (byte[3g+2] & 15)
//                                                                  P[2g+1] = byte[3g+1] << 4 | (byte[3g+2] >> 4)
//
// An image is H rows of `stride` bytes, stride >= W * bits / 8; the bytes behind the first W * bits / 8 of a row are padding and
// are never read.  A row may start at any byte: the loads below are 4-, 2- and 1-byte copies that the compiler may issue at
// any address, and each covers bytes of the groups it decodes and nothing else - the last group of the last row ends where the
// buffer ends.
#pragma once
#include "risp_common.h"

namespace risp_rawpack {

// the rules on the format every packed entry point shares; `name` is the entry point's, for the message
inline int rawpack_check(const char *name, int bits, int W, int stride) {
    RISP_CHECK_ARG(bits == 10 || bits == 12, "%s: bits %d (10: RAW10, 12: RAW12)", name, bits);
    RISP_CHECK_ARG(W >= 4 && W % 4 == 0, "%s: W %d (a multiple of 4: a row is whole groups)", name, W);
    RISP_CHECK_ARG((long long)stride >= (long long)W * bits / 8, "%s: stride %d below the %lld bytes of a row of W=%d %d-bit samples",
                   name, stride, (long long)W * bits / 8, W, bits);
    return 0;
}

__device__ __forceinline__ unsigned ldb4(const uint8_t *p) {
    unsigned v;
    __builtin_memcpy(&v, p, 4);
    return v;
}
__device__ __forceinline__ unsigned ldb2(const uint8_t *p) {
    unsigned short v;
    __builtin_memcpy(&v, p, 2);
    return v;
}

// the four pixels of RAW10 group `hi` = bytes 0 .. 3, `lo` = byte 4
__device__ __forceinline__ ushort4 raw10_group(unsigned hi, unsigned lo) {
    return ushort4{(unsigned short)((hi & 255u) << 2 | (lo & 3u)), (unsigned short)((hi >> 8 & 255u) << 2 | (lo >> 2 & 3u)),
                   (unsigned short)((hi >> 16 & 255u) << 2 | (lo >> 4 & 3u)), (unsigned short)((hi >> 24) << 2 | (lo >> 6 & 3u))};
}
// the two pixels of a RAW12 group from its bytes b0, b1, b2
__device__ __forceinline__ ushort2 raw12_group(unsigned b0, unsigned b1, unsigned b2) {
    return ushort2{(unsigned short)(b0 << 4 | (b2 & 15u)), (unsigned short)(b1 << 4 | b2 >> 4)};
}

// pixels x .. x + 3 of a packed row, x % 4 == 0: one 5-byte group, or two 3-byte groups
template <int BITS>
__device__ __forceinline__ ushort4 ld4(const uint8_t *row, int x) {
    if constexpr (BITS == 10) {
        const uint8_t *b = row + (size_t)(x >> 2) * 5;
        return raw10_group(ldb4(b), b[4]);
    } else {
        const uint8_t *b = row + (size_t)(x >> 2) * 6;
        const unsigned d = ldb4(b), e = ldb2(b + 4);
        const ushort2 p = raw12_group(d & 255u, d >> 8 & 255u, d >> 16 & 255u), q = raw12_group(d >> 24, e & 255u, e >> 8);
        return ushort4{p.x, p.y, q.x, q.y};
    }
}

// pixels x, x + 1, x even: half a RAW10 group (its bytes k, k + 1 and 4, k = x % 4), or one RAW12 group
template <int BITS>
__device__ __forceinline__ ushort2 ld2(const uint8_t *row, int x) {
    if constexpr (BITS == 10) {
        const uint8_t *b = row + (size_t)(x >> 2) * 5;
        const int k = x & 2;
        const unsigned hi = ldb2(b + k), lo = (unsigned)b[4] >> (2 * k);
        return ushort2{(unsigned short)((hi & 255u) << 2 | (lo & 3u)), (unsigned short)((hi >> 8) << 2 | (lo >> 2 & 3u))};
    } else {
        const uint8_t *b = row + (size_t)(x >> 1) * 3;
        const unsigned hi = ldb2(b);
        return raw12_group(hi & 255u, hi >> 8, b[2]);
    }
}

}  // namespace risp_rawpack
