// Lens-shading correction of (N,H,W) sensor frames into (N,H,W) uint16, one launch: the definition of risp_shade.h.  The front of
// every serving route that has no fused shading load (risp_serve_classical_shaded has one).  The frames come as uint16 rows or
// MIPI-packed RAW10 / RAW12 (risp_rawpack.h), so packed frames are decoded and shaded in this one pass: bits / 8 bytes read and
// 2 written per pixel, plus the map, which is small and stays in cache.  The loads and the format dispatch are risp_rawframe.h's.
//
// A thread owns up to 16 pixels of one row, in groups of four: a group starts at a multiple of 4 and a cell is at least 4 wide, so
// a group lies in one cell.  The row's two planes of the node columns left and right of the group are interpolated down the cell
// once and kept while the groups stay in that cell (at cell >= 16 for the whole chunk); moving one cell on, the right column
// becomes the left.  Per sample: two multiplies, an add and a shift for the gain, then the product.
#include "risp_common.h"
#include "risp_rawframe.h"
#include "risp_shade.h"

namespace {

using namespace risp_rawframe;
using namespace risp_shade;

constexpr int CHUNK = 16;       // pixels per thread

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
            const ushort4 s = ld4<BITS, WIDE>(row, x);
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
    if (int err = frame_check(name, raw, bits, W, stride)) return err;
    if (int err = shade_check(name, gains, cell_log2, GH, GW, black_level, H, W)) return err;
    if (int err = out_check(name, out)) return err;
    const int per_row = (W + CHUNK - 1) / CHUNK;
    const size_t chunks = (size_t)N * H * per_row;
    const uint8_t *src = static_cast<const uint8_t *>(raw);
    dispatch(bits, raw, stride, [&](auto bits_c, auto wide_c) {
        hipLaunchKernelGGL((raw_shade_kernel<decltype(bits_c)::value, decltype(wide_c)::value>), capped_grid(chunks), dim3(256), 0,
                           (hipStream_t)stream, src, out, gains, chunks, H, W, stride, per_row, cell_log2, GW, (unsigned)black_level);
    });
    RISP_LAUNCH_CHECK(name);
    return 0;
}
