// Lens-shading correction of (N,H,W) sensor frames into (N,H,W) uint16, one launch: the definition of risp_shade.h.  The front of
// every serving route that has no fused shading load (risp_serve_classical_shaded has one).  The frames come as uint16 rows or
// MIPI-packed RAW10 / RAW12 (risp_rawpack.h), so packed frames are decoded and shaded in this one pass: bits / 8 bytes read and
// 2 written per pixel, plus the map, which is small and stays in cache.
//
// A thread owns up to 16 pixels of one row, in groups of four: a group starts at a multiple of 4 and a cell is at least 4 wide, so
// a group lies in one cell.  The row's two planes of the node columns left and right of the group are interpolated down the cell
// once and kept while the groups stay in that cell (at cell >= 16 for the whole chunk); moving one cell on, the right column
// becomes the left.  Per sample: two multiplies, an add and a shift for the gain, then the product.
#include "risp_common.h"
#include "risp_rawpack.h"
#include "risp_shade.h"

namespace {

using namespace risp_shade;

constexpr int CHUNK = 16;       // pixels per thread

// BITS 16: rows of uint16 (WIDE: base and stride 8-byte aligned, a group is one load); 10 / 12: the byte form of risp_rawpack.h
template <int BITS, bool WIDE>
__global__ __launch_bounds__(256) void raw_shade_kernel(const uint8_t *__restrict__ raw, uint16_t *__restrict__ out,
                                                        const uint16_t *__restrict__ gains, size_t chunks, int H, int W, int stride,
                                                        int per_row, int k, int GW, unsigned black) {
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < chunks; t += (size_t)gridDim.x * blockDim.x) {
        const size_t line = t / per_row;                // n * H + y
        const int x0 = (int)(t - line * per_row) * CHUNK, y = (int)(line % (size_t)H);
        const uint8_t *row = raw + line * (size_t)stride;
        ushort4 *dst = reinterpret_cast<ushort4 *>(out + line * (size_t)W + x0);         // W % 4 == 0, out 8-byte aligned
        const int groups = (W - x0 < CHUNK ? W - x0 : CHUNK) / 4;
        const MapRow map(gains, GW, k, y);
        int jc = x0 >> k;
        Cell nd{map.node(jc), map.node(jc + 1)};
        for (int g = 0; g < groups; ++g) {
            const int x = x0 + 4 * g, j = x >> k;
            if (j != jc) {                              // the next cell: j == jc + 1
                nd = Cell{nd.r, map.node(j + 1)};
                jc = j;
            }
            ushort4 s;
            if constexpr (BITS != 16) {
                s = risp_rawpack::ld4<BITS>(row, x);
            } else if constexpr (WIDE) {
                s = *reinterpret_cast<const ushort4 *>(row + 2 * (size_t)x);
            } else {
                const unsigned short *p = reinterpret_cast<const unsigned short *>(row) + x;
                s = ushort4{p[0], p[1], p[2], p[3]};
            }
            const unsigned fx = cell_fx(x, k);
            dst[g] = ushort4{(unsigned short)shade(s.x, black, nd.gain<0>(fx, k)), (unsigned short)shade(s.y, black, nd.gain<1>(fx + 1, k)),
                             (unsigned short)shade(s.z, black, nd.gain<0>(fx + 2, k)), (unsigned short)shade(s.w, black, nd.gain<1>(fx + 3, k))};
        }
    }
}

}  // namespace

extern "C" int risp_raw_shade(const void *raw, int bits, int stride, uint16_t *out, const uint16_t *gains, int cell_log2, int GH,
                              int GW, int black_level, int N, int H, int W, void *stream) {
    const char *name = "risp_raw_shade";
    RISP_CHECK_ARG(raw && out && gains, "%s: null argument", name);
    RISP_CHECK_ARG(N >= 1 && H >= 1, "%s: bad shape N=%d H=%d", name, N, H);
    RISP_CHECK_ARG(bits == 16 || bits == 10 || bits == 12, "%s: bits %d (16: uint16 rows, 10: RAW10, 12: RAW12)", name, bits);
    if (bits == 16) {
        RISP_CHECK_ARG(W >= 4 && W % 4 == 0, "%s: W %d (a multiple of 4)", name, W);
        RISP_CHECK_ARG(stride % 2 == 0 && (long long)stride >= 2LL * W && reinterpret_cast<uintptr_t>(raw) % 2 == 0,
                       "%s: stride %d (even, at least the %lld bytes of a row of W=%d) and raw %p (2-byte aligned)", name, stride, 2LL * W,
                       W, raw);
    } else if (int err = risp_rawpack::rawpack_check(name, bits, W, stride)) {
        return err;
    }
    if (int err = shade_check(name, gains, cell_log2, GH, GW, black_level, H, W)) return err;
    RISP_CHECK_ARG(reinterpret_cast<uintptr_t>(out) % 8 == 0, "%s: out %p must be 8-byte aligned", name, (void *)out);
    const int per_row = (W + CHUNK - 1) / CHUNK;
    const size_t chunks = (size_t)N * H * per_row, blocks = (chunks + 255) / 256;
    const dim3 grid((unsigned)(blocks > 65536 ? 65536 : blocks));
    hipStream_t s = (hipStream_t)stream;
    const uint8_t *src = static_cast<const uint8_t *>(raw);
    const unsigned black = (unsigned)black_level;
#define RISP_SHADE_LAUNCH(BITS, WIDE) \
    hipLaunchKernelGGL((raw_shade_kernel<BITS, WIDE>), grid, dim3(256), 0, s, src, out, gains, chunks, H, W, stride, per_row, cell_log2, GW, black)
    if (bits == 10) RISP_SHADE_LAUNCH(10, false);
    else if (bits == 12) RISP_SHADE_LAUNCH(12, false);
    else if (reinterpret_cast<uintptr_t>(raw) % 8 == 0 && stride % 8 == 0) RISP_SHADE_LAUNCH(16, true);
    else RISP_SHADE_LAUNCH(16, false);
#undef RISP_SHADE_LAUNCH
    RISP_LAUNCH_CHECK(name);
    return 0;
}
