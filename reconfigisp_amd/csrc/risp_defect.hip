// Defective-pixel correction of (N,H,W) sensor frames into (N,H,W) uint16, one launch: the definition of risp_defect.h.  The
// pre-pass in front of every serving route: the frames come as uint16 rows or MIPI-packed RAW10 / RAW12 (risp_rawpack.h) and are
// decoded on the way, and with a gain map each corrected sample is shaded as risp_raw_shade shades it (risp_shade.h) - decode,
// correction and shading cost bits / 8 bytes read and 2 written per pixel, once.
//
// A thread owns a group of four columns x .. x+3 (x % 4 == 0) and walks down ROWS rows.  It keeps columns x-2 .. x+5 of the last
// five rows in registers: per new row the group itself (one ld4) and the pairs left and right of it (two ld2), so a sample is
// fetched from cache (ROWS + 4) / ROWS times per thread that needs it instead of 3.  The ring is indexed by the unrolled loop
// counter alone: every slot is a register, nothing lives in scratch.  Only rows y-2, y, y+2 enter row y; rows y-1 and y+1 wait
// for their turn.
//
// Borders.  The window, its reflected columns at a row's end and the reflected row index are risp_rawframe.h's (load_row,
// reflect_row): no load ever leaves the frame.  Rows below the frame's last are neither loaded nor stored.
#include "risp_common.h"
#include "risp_defect.h"
#include "risp_rawframe.h"
#include "risp_shade.h"

namespace {

using namespace risp_rawframe;
using namespace risp_shade;

#ifndef RISP_DEFECT_ROWS
#define RISP_DEFECT_ROWS 8      // (make EXTRA=-DRISP_DEFECT_ROWS=4 | 16: the ablation builds of tools/bench_serve_defect_rows.py)
#endif
constexpr int ROWS = RISP_DEFECT_ROWS;          // rows per thread

// pixel I of the group in row `mid`, rows `top` and `bot` two above and below
template <int I>
__device__ __forceinline__ unsigned pixel(const Row &top, const Row &mid, const Row &bot, unsigned listed, unsigned threshold,
                                          unsigned slope) {
    return risp_defect::correct(mid.v[I + 2], mid.v[I], mid.v[I + 4], top.v[I + 2], bot.v[I + 2], top.v[I], bot.v[I + 4], top.v[I + 4],
                                bot.v[I], (listed >> I) & 1u, threshold, slope);
}

template <int BITS, bool WIDE, bool SHADE>
__global__ __launch_bounds__(256) void raw_defect_kernel(const uint8_t *__restrict__ raw, uint16_t *__restrict__ out,
                                                         const unsigned *__restrict__ defects, const uint16_t *__restrict__ gains,
                                                         size_t items, int H, int W, int stride, int per_row, int strips, int words,
                                                         unsigned threshold, unsigned slope, int k, int GW, unsigned black) {
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < items; t += (size_t)gridDim.x * blockDim.x) {
        const size_t band = t / per_row;                // n * strips + strip
        const int x = (int)(t - band * per_row) * 4, y0 = (int)(band % (size_t)strips) * ROWS;
        const size_t n = band / (size_t)strips;
        const uint8_t *img = raw + n * (size_t)H * (size_t)stride;
        const bool left = x == 0, right = x + 4 == W;
        Row win[5];
#pragma unroll
        for (int r = 0; r < ROWS + 4; ++r) {
            const int y = y0 + r - 4;                   // the row this step completes, once r >= 4
            if (r >= 4 && y >= H) break;
            const int yy = reflect_row(y + 2, H);       // the row this step loads: y0-2 .. y0+ROWS+1, at most H+1
            win[r % 5] = load_row<BITS, WIDE>(img + (size_t)yy * (size_t)stride, x, left, right);
            if (r < 4) continue;
            const Row &top = win[(r - 4) % 5], &mid = win[(r - 2) % 5], &bot = win[r % 5];
            // the map: one word per 32 pixels of a row, the group's four bits lie in one word
            const unsigned listed = defects ? defects[(size_t)y * words + (x >> 5)] >> (x & 31) : 0u;
            unsigned o0 = pixel<0>(top, mid, bot, listed, threshold, slope), o1 = pixel<1>(top, mid, bot, listed, threshold, slope);
            unsigned o2 = pixel<2>(top, mid, bot, listed, threshold, slope), o3 = pixel<3>(top, mid, bot, listed, threshold, slope);
            if constexpr (SHADE) {                      // a group lies in one cell: cells are at least 4 wide
                const MapRow map(gains, GW, k, y);
                const int j = x >> k;
                const Cell nd{map.node(j), map.node(j + 1)};
                const unsigned fx = cell_fx(x, k);
                o0 = shade(o0, black, nd.gain<0>(fx, k)), o1 = shade(o1, black, nd.gain<1>(fx + 1, k));
                o2 = shade(o2, black, nd.gain<0>(fx + 2, k)), o3 = shade(o3, black, nd.gain<1>(fx + 3, k));
            }
            *reinterpret_cast<ushort4 *>(out + (n * (size_t)H + y) * (size_t)W + x) =      // W % 4 == 0, out 8-byte aligned
                ushort4{(unsigned short)o0, (unsigned short)o1, (unsigned short)o2, (unsigned short)o3};
        }
    }
}

}  // namespace

extern "C" int risp_raw_defect(const void *raw, int bits, int stride, uint16_t *out, int threshold, int slope, const uint32_t *defects,
                               const uint16_t *gains, int cell_log2, int GH, int GW, int black_level, int N, int H, int W,
                               void *stream) {
    const char *name = "risp_raw_defect";
    RISP_CHECK_ARG(raw && out, "%s: null argument", name);
    RISP_CHECK_ARG(N >= 1 && H >= 3, "%s: bad shape N=%d H=%d (at least 3 rows: a reflected row stays inside the frame)", name, N, H);
    if (int err = frame_check(name, raw, bits, W, stride)) return err;
    RISP_CHECK_ARG(threshold >= -1 && threshold <= 65535, "%s: threshold %d outside 0 .. 65535 (-1: no dynamic test)", name, threshold);
    RISP_CHECK_ARG(slope >= 0 && slope <= 255, "%s: slope %d outside 0 .. 255", name, slope);
    RISP_CHECK_ARG(threshold >= 0 || defects, "%s: neither a threshold nor a defect map: nothing to correct", name);
    RISP_CHECK_ARG(reinterpret_cast<uintptr_t>(defects) % 4 == 0, "%s: defects %p must be 4-byte aligned", name, (const void *)defects);
    if (gains) {
        if (int err = shade_check(name, gains, cell_log2, GH, GW, black_level, H, W)) return err;
    } else {
        RISP_CHECK_ARG(cell_log2 == 0 && GH == 0 && GW == 0 && black_level == 0,
                       "%s: without gains cell_log2 %d, GH %d, GW %d and black_level %d must be 0", name, cell_log2, GH, GW, black_level);
    }
    if (int err = out_check(name, out)) return err;
    const int per_row = W / 4, strips = (H + ROWS - 1) / ROWS, words = (W + 31) / 32;
    const size_t items = (size_t)N * strips * per_row;
    const uint8_t *src = static_cast<const uint8_t *>(raw);
    const unsigned thr = threshold < 0 ? risp_defect::NO_THRESHOLD : (unsigned)threshold, slp = threshold < 0 ? 0u : (unsigned)slope;
    dispatch(bits, raw, stride, [&](auto bits_c, auto wide_c) {
        auto launch = [&](auto shade_c) {
            hipLaunchKernelGGL((raw_defect_kernel<decltype(bits_c)::value, decltype(wide_c)::value, decltype(shade_c)::value>),
                               capped_grid(items), dim3(256), 0, (hipStream_t)stream, src, out, defects, gains, items, H, W, stride,
                               per_row, strips, words, thr, slp, cell_log2, GW, (unsigned)black_level);
        };
        if (gains) launch(std::true_type{});
        else launch(std::false_type{});
    });
    RISP_LAUNCH_CHECK(name);
    return 0;
}
