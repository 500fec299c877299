// YUV 4:2:0 (NV12) from 8-bit codes: the integer definition risp_bgr8_to_nv12 and the fused NV12 stores of risp_serve_nv12 /
// risp_serve_classical_nv12 share (include/risp.h states it; tests/nv12_reference.py restates it in numpy).
//
//     Y(y,x) = (cy0*R + cy1*G + cy2*B + cy3) >> 8                      per pixel
//     Rm     = (R00 + R01 + R10 + R11 + 2) >> 2   (Gm, Bm likewise)    per 2 x 2 quad: the rounded mean of the CODES
//     U(j,i) = (cu0*Rm + cu1*Gm + cu2*Bm + cu3) >> 8,  V likewise
//
// An image is (3H/2, W) bytes: H rows of Y, then H/2 rows of U V U V ...  The offsets carry the rounding constant and the
// plane offset, and nv12_check admits a matrix only when every sum lies in 0 .. 65535 for all codes: no clamp, no signed shift.
#pragma once
#include "risp_common.h"

namespace risp_nv12 {

struct Coef {
    int k[12];                  // cy[4], cu[4], cv[4]: kR, kG, kB, offset
};

// for each row: |k| <= 256, offset + 255 * (sum of positive k) <= 65535, offset + 255 * (sum of negative k) >= 0
inline int nv12_check(const char *name, const int32_t *coef, Coef &out) {
    RISP_CHECK_ARG(coef, "%s: null argument", name);
    static const char *const rows[3] = {"cy", "cu", "cv"};
    for (int r = 0; r < 3; ++r) {
        const int32_t *k = coef + 4 * r;
        long long pos = 0, neg = 0;
        for (int c = 0; c < 3; ++c) {
            RISP_CHECK_ARG(k[c] >= -256 && k[c] <= 256, "%s: matrix row %s (%d, %d, %d, %d): coefficient %d outside -256 .. 256", name,
                           rows[r], k[0], k[1], k[2], k[3], k[c]);
            (k[c] > 0 ? pos : neg) += k[c];
        }
        RISP_CHECK_ARG((long long)k[3] + 255 * pos <= 65535 && (long long)k[3] + 255 * neg >= 0,
                       "%s: matrix row %s (%d, %d, %d, %d) leaves 0 .. 65535 for some codes", name, rows[r], k[0], k[1], k[2], k[3]);
    }
    for (int i = 0; i < 12; ++i) out.k[i] = coef[i];
    return 0;
}

// one row of the matrix on three codes (the sum is in 0 .. 65535 by nv12_check)
__device__ __forceinline__ unsigned nv12_dot(const int *k, unsigned r, unsigned g, unsigned b) {
    return (unsigned)(k[0] * (int)r + k[1] * (int)g + k[2] * (int)b + k[3]) >> 8;
}

// the U and V bytes of one quad from the sums of its four codes per channel: U | V << 8
__device__ __forceinline__ unsigned nv12_uv(const Coef &m, unsigned sr, unsigned sg, unsigned sb) {
    const unsigned rm = (sr + 2) >> 2, gm = (sg + 2) >> 2, bm = (sb + 2) >> 2;
    return nv12_dot(m.k + 4, rm, gm, bm) | nv12_dot(m.k + 8, rm, gm, bm) << 8;
}

// A thread's 2 x 4 patch of codes at (py, px) of the mirrored image -> two Y dwords and one UV dword of the un-mirrored image
// `img` (3H/2, W).  flip bit 0: the four Y bytes of a row go to column W-4-px in reverse order and the two quads swap places
// in the UV dword at byte column W-4-px; bit 1: rows py, py+1 go to H-1-py, H-2-py and the chroma row is (H-2-py)/2.  H even
// and W % 4 == 0 keep quads on quads and every store a dword
__device__ __forceinline__ void nv12_store_patch(uint8_t *img, const Coef &m, const unsigned (&r)[2][4], const unsigned (&g)[2][4],
                                                 const unsigned (&b)[2][4], int H, int W, int py, int px, int flip) {
    const bool fx = flip & 1, fy = flip & 2;
    const int col = fx ? W - 4 - px : px;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        unsigned y[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) y[c] = nv12_dot(m.k, r[p][c], g[p][c], b[p][c]);
        const unsigned fwd = y[0] | y[1] << 8 | y[2] << 16 | y[3] << 24, rev = y[3] | y[2] << 8 | y[1] << 16 | y[0] << 24;
        *reinterpret_cast<unsigned *>(img + (size_t)(fy ? H - 1 - py - p : py + p) * W + col) = fx ? rev : fwd;
    }
    const unsigned q0 = nv12_uv(m, r[0][0] + r[0][1] + r[1][0] + r[1][1], g[0][0] + g[0][1] + g[1][0] + g[1][1],
                                b[0][0] + b[0][1] + b[1][0] + b[1][1]);
    const unsigned q1 = nv12_uv(m, r[0][2] + r[0][3] + r[1][2] + r[1][3], g[0][2] + g[0][3] + g[1][2] + g[1][3],
                                b[0][2] + b[0][3] + b[1][2] + b[1][3]);
    *reinterpret_cast<unsigned *>(img + (size_t)(H + ((fy ? H - 2 - py : py) >> 1)) * W + col) = fx ? (q1 | q0 << 16) : (q0 | q1 << 16);
}

}  // namespace risp_nv12
