// Lens-shading correction in: the definition risp_raw_shade and the fused load of risp_serve_classical_shaded share (include/risp.h
// states it; tests/lens_shading_reference.py restates it in numpy).
//
//     gains (GH,GW,4) uint16, Q12; node (i,j) at sensor pixel (i << k, j << k); plane c = 2 * (y & 1) + (x & 1)
//     g  = bilinear interpolation of the four nodes around (y,x), weights in 1 / cell, rounded once: (.. + (1 << (2k-1))) >> 2k
//     s' = min((max(s - black, 0) * g + 2048) >> 12, 65535)
//
// All in unsigned 32-bit arithmetic: the sums reach 2^16 * 65535 + 2^15 and 65535 * 65535 + 2048, above 2^31 and below 2^32.
// The interpolation is exact until its one shift, so the order is free: the code here goes down first - a row's fy is the same
// for every sample of it, and a node column serves a whole cell - and then across per sample.  A row touches two planes only,
// 2 * (y & 1) and the one behind it: one aligned dword of a node.
//
// Plain 32-bit multiplies: a form with 24-bit multiplies (every factor is below 2^24) and the horizontal step rewritten as
// (l << k) + fx * r - fx * l was measured slower in the serving kernel, by 7 to 24 % of the launch.
#pragma once
#include "risp_common.h"

namespace risp_shade {

// the rules on the map every shading entry point shares; `name` is the entry point's, for the message
inline int shade_check(const char *name, const uint16_t *gains, int cell_log2, int GH, int GW, int black_level, int H, int W) {
    RISP_CHECK_ARG(gains, "%s: null argument", name);
    RISP_CHECK_ARG(cell_log2 >= 2 && cell_log2 <= 8, "%s: cell_log2 %d outside 2 .. 8", name, cell_log2);
    RISP_CHECK_ARG(H >= 1 && W >= 1 && GH == ((H - 1) >> cell_log2) + 2 && GW == ((W - 1) >> cell_log2) + 2,
                   "%s: a %d x %d map for H=%d W=%d cell_log2=%d, it must be %d x %d", name, GH, GW, H, W, cell_log2,
                   H >= 1 ? ((H - 1) >> cell_log2) + 2 : 0, W >= 1 ? ((W - 1) >> cell_log2) + 2 : 0);
    RISP_CHECK_ARG(reinterpret_cast<uintptr_t>(gains) % 8 == 0, "%s: gains %p must be 8-byte aligned", name, (const void *)gains);
    RISP_CHECK_ARG(black_level >= 0 && black_level <= 65535, "%s: black_level %d outside 0 .. 65535", name, black_level);
    return 0;
}

// sensor row y of a map: where its two planes start in the node rows above and below it, and its weights.  node(j): the two
// planes at node column j interpolated down the cell, x = the even column's plane, y = the odd column's
struct MapRow {
    const uint16_t *top, *bot;
    unsigned wt, wb;            // cell - fy, fy

    __device__ __forceinline__ MapRow(const uint16_t *gains, int GW, int k, int y) {
        top = gains + ((size_t)(y >> k) * GW) * 4 + 2 * (y & 1);
        bot = top + (size_t)GW * 4;
        wb = (unsigned)y & ((1u << k) - 1u);
        wt = (1u << k) - wb;
    }
    __device__ __forceinline__ uint2 node(int j) const {
        const unsigned a = *reinterpret_cast<const unsigned *>(top + 4 * (size_t)j);
        const unsigned b = *reinterpret_cast<const unsigned *>(bot + 4 * (size_t)j);
        return uint2{wt * (a & 0xFFFFu) + wb * (b & 0xFFFFu), wt * (a >> 16) + wb * (b >> 16)};
    }
};

// a cell of a row: the interpolated node columns left (l) and right (r) of it
struct Cell {
    uint2 l, r;

    // the Q12 gain fx pixels into the cell, in the even (ODD 0) or the odd column's plane
    template <int ODD>
    __device__ __forceinline__ unsigned gain(unsigned fx, int k) const {
        const unsigned a = ODD ? l.y : l.x, b = ODD ? r.y : r.x;
        return (((1u << k) - fx) * a + fx * b + (1u << (2 * k - 1))) >> (2 * k);
    }
};

// pixels into its cell of sensor column x
__device__ __forceinline__ unsigned cell_fx(int x, int k) { return (unsigned)x & ((1u << k) - 1u); }

// the shaded sample
__device__ __forceinline__ unsigned shade(unsigned s, unsigned black, unsigned g) {
    const unsigned d = s > black ? s - black : 0u;
    const unsigned v = (d * g + 2048u) >> 12;
    return v < 65535u ? v : 65535u;
}

}  // namespace risp_shade
