// Where a sensor sample is: what the raw-domain pre-passes (risp_shade.hip, risp_defect.hip, risp_stats.hip, risp_temporal.hip)
// share in front of their own arithmetic.  Frames are rows of uint16 (bits 16) or MIPI-packed RAW10 / RAW12 (bits 10 / 12, whose
// layout risp_rawpack.h owns), `stride` bytes apart; every load here takes a byte pointer to the row.
//
//     BITS 16, WIDE:   base and stride 8-byte aligned - a group of four is one 8-byte load, a pair one 4-byte load
//     BITS 16, !WIDE:  2-byte aligned - single samples
//     BITS 10 / 12:    the byte form of risp_rawpack.h, any base and any stride (WIDE is false)
//
// No load leaves the row: a window at the row's end is filled from the group itself (load_row).  The serving kernels have loads
// of their own (risp_serve_patch.h: mirrored and phase-aware).
#pragma once
#include <type_traits>

#include "risp_common.h"
#include "risp_rawpack.h"

namespace risp_rawframe {

// the rules on the frames every pre-pass that takes all three formats shares; `name` is the entry point's, for the message
inline int frame_check(const char *name, const void *raw, int bits, int W, int stride) {
    RISP_CHECK_ARG(bits == 16 || bits == 10 || bits == 12, "%s: bits %d (16: uint16 rows, 10: RAW10, 12: RAW12)", name, bits);
    if (bits != 16) return risp_rawpack::rawpack_check(name, bits, W, stride);
    RISP_CHECK_ARG(W >= 4 && W % 4 == 0, "%s: W %d (a multiple of 4)", name, W);
    RISP_CHECK_ARG(stride % 2 == 0 && (long long)stride >= 2LL * W && reinterpret_cast<uintptr_t>(raw) % 2 == 0,
                   "%s: stride %d (even, at least the %lld bytes of a row of W=%d) and raw %p (2-byte aligned)", name, stride, 2LL * W,
                   W, raw);
    return 0;
}

// the groups of four go out as one 8-byte store each
inline int out_check(const char *name, const void *out) {
    RISP_CHECK_ARG(reinterpret_cast<uintptr_t>(out) % 8 == 0, "%s: out %p must be 8-byte aligned", name, out);
    return 0;
}

// workgroups of 256 for `items` work items that the kernels walk with a grid stride
inline dim3 capped_grid(size_t items) {
    const size_t blocks = (items + 255) / 256;
    return dim3((unsigned)(blocks > 65536 ? 65536 : blocks));
}

// whether uint16 rows take the WIDE form
inline bool wide16(const void *raw, int stride) { return reinterpret_cast<uintptr_t>(raw) % 8 == 0 && stride % 8 == 0; }

// calls f(std::integral_constant<int, BITS>, std::bool_constant<WIDE>) for the form the frames take (bits as frame_check passed it)
template <class F>
inline void dispatch(int bits, const void *raw, int stride, F &&f) {
    if (bits == 10) f(std::integral_constant<int, 10>{}, std::false_type{});
    else if (bits == 12) f(std::integral_constant<int, 12>{}, std::false_type{});
    else if (wide16(raw, stride)) f(std::integral_constant<int, 16>{}, std::true_type{});
    else f(std::integral_constant<int, 16>{}, std::false_type{});
}

// pixels x .. x + 3 of a row, x % 4 == 0
template <int BITS, bool WIDE>
__device__ __forceinline__ ushort4 ld4(const uint8_t *row, int x) {
    if constexpr (BITS != 16) {
        return risp_rawpack::ld4<BITS>(row, x);
    } else if constexpr (WIDE) {
        return *reinterpret_cast<const ushort4 *>(reinterpret_cast<const unsigned short *>(row) + x);
    } else {
        const unsigned short *p = reinterpret_cast<const unsigned short *>(row) + x;
        return ushort4{p[0], p[1], p[2], p[3]};
    }
}

// pixels x, x + 1 of a row, x even
template <int BITS, bool WIDE>
__device__ __forceinline__ ushort2 ld2(const uint8_t *row, int x) {
    if constexpr (BITS != 16) {
        return risp_rawpack::ld2<BITS>(row, x);
    } else if constexpr (WIDE) {
        return *reinterpret_cast<const ushort2 *>(reinterpret_cast<const unsigned short *>(row) + x);
    } else {
        const unsigned short *p = reinterpret_cast<const unsigned short *>(row) + x;
        return ushort2{p[0], p[1]};
    }
}

struct Row {
    unsigned v[8];              // columns x-2 .. x+5
};

// The window of the group x .. x+3 (x % 4 == 0): the group and the pairs left and right of it.  `left`: x == 0, `right`:
// x + 4 == W.  Reflection without the repeated edge keeps a column's parity, and the columns behind a row's end are those of the
// group itself: columns -2, -1 are columns 2, 1 and columns W, W+1 are W-2, W-3 - elements 2 and 1 of the group in both cases,
// W == 4 included.  So a border thread drops a pair load and selects.  REFLECT false: the caller never reads a pair outside the
// row, and it is 0 (risp_stats.hip: the select cost its kernel time, NOTES.md).  The outside pair is written inside each select's
// arm on purpose: named once in front of them it cost raw_defect_kernel<12, ..> 2 us of 33 on a full frame.
template <int BITS, bool WIDE, bool REFLECT = true>
__device__ __forceinline__ Row load_row(const uint8_t *row, int x, bool left, bool right) {
    const ushort4 c = ld4<BITS, WIDE>(row, x);
    const ushort2 l = left ? (REFLECT ? ushort2{c.z, c.y} : ushort2{0, 0}) : ld2<BITS, WIDE>(row, x - 2);
    const ushort2 r = right ? (REFLECT ? ushort2{c.z, c.y} : ushort2{0, 0}) : ld2<BITS, WIDE>(row, x + 4);
    return Row{{l.x, l.y, c.x, c.y, c.z, c.w, r.x, r.y}};
}

// Row y of a frame of H rows, reflected without the repeated edge: -2 -> 2, H+1 -> H-3.  Two rows beyond either end stay inside
// for every H >= 3; the index is clamped behind the reflection all the same.
__device__ __forceinline__ int reflect_row(int y, int H) {
    y = y < 0 ? -y : (y >= H ? 2 * (H - 1) - y : y);
    return y < 0 ? 0 : (y > H - 1 ? H - 1 : y);
}

}  // namespace risp_rawframe
