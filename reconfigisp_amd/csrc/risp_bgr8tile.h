// Packed 8-bit images in and out of a 64-column tile: what the output-stage launches (risp_resize.hip, risp_sharpen.hip,
// risp_warp.hip, risp_nv12.hip) share around their own phases.  An image is (N,H,W,3) bytes and starts at ANY byte address, so
// neither a row nor the buffer is dword aligned; an NV12 image is (N,3H/2,W) bytes (risp_nv12.h has the conversion).
//
//     stage_box     a source box -> LDS in aligned dwords, Box::at(y, x) undoes the per-row shift
//     store_dword   one dword of a packed tile row: whole where aligned and inside the row, bytes otherwise; store_tile: a tile
//     unpack4       twelve bytes of a row -> four pixels' R, G, B
//     nv12_patch    a 2 x 4 patch of codes -> two Y dwords and two UV halves; nv12_store_patch_at stores them, dwords or bytes
//     sizes_ok, row_tiles, apart_check   the host-side checks the entry points share
#pragma once
#include "risp_common.h"
#include "risp_nv12.h"

namespace risp_bgr8tile {

using namespace risp_nv12;

constexpr int TW = 64, ROWB = TW * 3, ROWD = ROWB / 4;     // a tile row: columns, bytes, dwords (a wave owns one row at a time)

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// A staged box: rows by0 .. and columns bx0 .. of one image in LDS, `pitch` bytes per box row.  Box row r was read from the
// 4-byte aligned address at or below its first byte, so it begins (a0 + r * rw3) & 3 bytes into its LDS row
struct Box {
    const uint8_t *box;
    int by0, bx0, pitch, a0, rw3;
    // the bytes of pixel (y, x) of the image, inside the box
    __device__ __forceinline__ const uint8_t *at(int y, int x) const {
        const int r = y - by0;
        return box + r * pitch + ((a0 + r * rw3) & 3) + (x - bx0) * 3;
    }
};

// Rows by0 .. by1 and columns bx0 .. bx1 of one image of img (N,H,W,3), `first_byte` the address of the box's first, go to `lds`,
// a dword per thread (256) and step: lanes read consecutive aligned dwords, and a dword that is not wholly inside img - at most
// the first and the last of the whole buffer - is put together from guarded byte loads.  The pitch: a multiple of 4, at least the
// box row's bytes + 3 (up to 3 bytes lie in front of a row's first); PITCH where the caller knows it at compile time, else 0 and
// `pitch`.  How the pitch and `first_byte` reach the loop is measured, not taste (NOTES.md): a constant in `pitch` cost
// risp_bgr8_sharpen 8 %, the address made here from the image's index cost the bilinear risp_bgr8_warp 8 %.  The caller's barrier follows.
template <int PITCH = 0>
__device__ __forceinline__ Box stage_box(const uint8_t *__restrict__ img, int N, int H, int W, const uint8_t *first_byte, int by0, int by1,
                                         int bx0, int bx1, unsigned *lds, int tid, int pitch = PITCH) {
    if (PITCH) pitch = PITCH;
    const int brows = by1 - by0 + 1, bbytes = (bx1 - bx0 + 1) * 3, pd = pitch / 4;
    const uintptr_t lo = reinterpret_cast<uintptr_t>(img);
    const uintptr_t first = reinterpret_cast<uintptr_t>(first_byte);
    const long long total = (long long)N * H * W * 3;
    for (int t = tid; t < brows * pd; t += 256) {
        const int r = t / pd, d = t - r * pd;
        const uintptr_t begin = first + (size_t)r * W * 3, a = (begin & ~(uintptr_t)3) + (size_t)d * 4;
        if (a >= begin + bbytes) continue;                          // a dword behind the row's last byte: never read
        const long long off = (long long)(a - lo);                  // from img's first byte: -3 at the least
        unsigned v = 0;
        if (off >= 0 && off + 4 <= total) {
            v = *reinterpret_cast<const unsigned *>(img + off);
        } else {
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (off + b >= 0 && off + b < total) v |= (unsigned)img[off + b] << (8 * b);
        }
        lds[t] = v;
    }
    return Box{reinterpret_cast<const uint8_t *>(lds), by0, bx0, pitch, (int)(first & 3), (W * 3) & 3};
}

// The store policy of a packed row: dword `v` belongs at p, `at` bytes into a tile row of `valid` bytes.  Whole where p is
// 4-byte aligned and the dword inside the row, byte by byte otherwise
__device__ __forceinline__ void store_dword(uint8_t *p, unsigned v, int at, int valid) {
    if (at + 4 <= valid && reinterpret_cast<uintptr_t>(p) % 4 == 0) {
        *reinterpret_cast<unsigned *>(p) = v;
    } else {
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if (at + b < valid) p[b] = (uint8_t)(v >> (8 * b));
    }
}

// a tile of rows x ROWD dwords in LDS -> `cols` pixels of `rows` rows, `pitch` bytes apart, dst the first row's first byte
__device__ __forceinline__ void store_tile(uint8_t *dst, size_t pitch, const unsigned *tile, int rows, int cols, int tid) {
    const int valid = cols * 3;
    for (int t = tid; t < rows * ROWD; t += 256) {
        const int i = t / ROWD, d = t - i * ROWD;
        if (d * 4 < valid) store_dword(dst + i * pitch + d * 4, tile[t], d * 4, valid);
    }
}

// three dwords of a row, from a pixel's first byte on -> four pixels; rgb_in: the first byte of a pixel is R, else B
__device__ __forceinline__ void unpack4(unsigned d0, unsigned d1, unsigned d2, int rgb_in, unsigned (&r)[4], unsigned (&g)[4],
                                        unsigned (&b)[4]) {
    const unsigned c0[4] = {d0 & 255u, d0 >> 24, d1 >> 16 & 255u, d2 >> 8 & 255u};         // first byte of each pixel
    const unsigned c2[4] = {d0 >> 16 & 255u, d1 >> 8 & 255u, d2 & 255u, d2 >> 24};         // third byte
    g[0] = d0 >> 8 & 255u, g[1] = d1 & 255u, g[2] = d1 >> 24, g[3] = d2 >> 16 & 255u;
#pragma unroll
    for (int c = 0; c < 4; ++c) r[c] = rgb_in ? c0[c] : c2[c], b[c] = rgb_in ? c2[c] : c0[c];
}

// a 2 x 4 patch of codes -> the Y dword of each row and U | V << 8 of each of its two quads
__device__ __forceinline__ void nv12_patch(const Coef &m, const unsigned (&r)[2][4], const unsigned (&g)[2][4],
                                           const unsigned (&b)[2][4], unsigned (&y)[2], unsigned (&uv)[2]) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
        y[a] = nv12_dot(m.k, r[a][0], g[a][0], b[a][0]) | nv12_dot(m.k, r[a][1], g[a][1], b[a][1]) << 8 |
               nv12_dot(m.k, r[a][2], g[a][2], b[a][2]) << 16 | nv12_dot(m.k, r[a][3], g[a][3], b[a][3]) << 24;
#pragma unroll
    for (int h = 0; h < 2; ++h)
        uv[h] = nv12_uv(m, r[0][2 * h] + r[0][2 * h + 1] + r[1][2 * h] + r[1][2 * h + 1],
                        g[0][2 * h] + g[0][2 * h + 1] + g[1][2 * h] + g[1][2 * h + 1],
                        b[0][2 * h] + b[0][2 * h + 1] + b[1][2 * h] + b[1][2 * h + 1]);
}

// ... stored: py the patch's first Y byte, pc its first chroma byte, rows `pitch` bytes apart.  `wide`: every patch of the image
// is whole and its dwords aligned - three dword stores; otherwise the narrow form for the `quads` (1 or 2) quads inside the
// tile: bytes, or with PAIRS byte pairs where the image is 2-byte aligned (risp_bgr8_resize: bytes cost it 0.3 us of 26, NOTES.md)
template <bool PAIRS = false>
__device__ __forceinline__ void nv12_store_patch_at(uint8_t *py, uint8_t *pc, size_t pitch, bool wide, int quads, const unsigned (&y)[2],
                                                    const unsigned (&uv)[2]) {
    const unsigned c = uv[0] | uv[1] << 16;
    if (wide) {
        *reinterpret_cast<unsigned *>(py) = y[0];
        *reinterpret_cast<unsigned *>(py + pitch) = y[1];
        *reinterpret_cast<unsigned *>(pc) = c;
    } else {
        auto put = [](uint8_t *p, unsigned v) {
            if constexpr (PAIRS) *reinterpret_cast<unsigned short *>(p) = (unsigned short)v;
            else *p = (uint8_t)v;
        };
        for (int k = 0; k < 2 * quads; k += PAIRS ? 2 : 1)
            put(py + k, y[0] >> (8 * k)), put(py + pitch + k, y[1] >> (8 * k)), put(pc + k, c >> (8 * k));
    }
}

// ---- host side: the checks of the entry points that are the same in substance (each entry point words its own shape message)
inline bool sizes_ok(int lim, int N, int a, int b, int c = 1, int d = 1) {
    return N >= 1 && N <= 65535 && a >= 1 && a <= lim && b >= 1 && b <= lim && c >= 1 && c <= lim && d >= 1 && d <= lim;
}

// gy: the tiles of `tile` rows over `rows` output rows, `dim` the name of that argument; a grid has at most 65535 of them
inline int row_tiles(const char *name, const char *dim, int rows, int tile, unsigned &gy) {
    gy = (unsigned)((rows + tile - 1) / tile);
    RISP_CHECK_ARG(gy <= 65535, "%s: %u row tiles for %s=%d, at most 65535", name, gy, dim, rows);
    return 0;
}

// a tile reads `what` ("rows", "pixels") of img that other tiles write when out lies on it
inline int apart_check(const char *name, const uint8_t *img, size_t in_bytes, const uint8_t *out, size_t out_bytes, const char *what) {
    RISP_CHECK_ARG(out + out_bytes <= img || img + in_bytes <= out, "%s: out overlaps img: a tile reads %s other tiles write", name, what);
    return 0;
}

}  // namespace risp_bgr8tile
