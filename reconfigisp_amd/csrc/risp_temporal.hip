// Temporal noise reduction of (N,H,W) uint16 frames against a state of the same shape, one launch and one copy: the definition of
// risp_temporal.h.  The pre-pass behind defect correction and lens shading and in front of every serving route: a recursive filter
// whose share of the new frame grows where the 5 x 5 neighbourhood says that something moved.  The launch reads the current frame
// and the state and writes `out` (6 bytes per pixel); a device-to-device copy of `out` into the state follows on the same stream
// (4 more) - the state cannot be written in place, other workgroups still read its halo, and two buffers alternated by the host
// would bake one direction into a captured graph.
//
// The shape of risp_defect.hip.  A thread owns a group of four columns x .. x+3 (x % 4 == 0) and walks down ROWS rows.  Per new row
// it loads columns x-2 .. x+5 of both frames - the group itself (one ld4) and the pairs left and right of it (two ld2) - and folds
// them at once into the horizontal 5-sums of c - p and of p for its four pixels; those sums and the group's own samples of the last
// five rows live in registers, indexed by the unrolled loop counter alone: nothing lives in scratch.  A pixel's window sums are the
// five rows' 5-sums added up.
//
// Borders as in risp_defect.hip, with risp_rawframe.h's load_row and reflect_row on uint16 rows 2 W bytes apart: no load ever leaves
// the frame, and rows below the frame's last are neither loaded nor stored.
#include "risp_common.h"
#include "risp_rawframe.h"
#include "risp_temporal.h"

namespace {

using namespace risp_rawframe;
using risp_temporal::Params;

#ifndef RISP_TEMPORAL_ROWS
#define RISP_TEMPORAL_ROWS 8
#endif
constexpr int ROWS = RISP_TEMPORAL_ROWS;        // rows per thread

// what a row leaves behind for the five steps it is part of a window: per pixel of the group the horizontal 5-sums and the samples
struct Sums {
    int a[4];                   // sum of c - p over columns i-2 .. i+2
    unsigned b[4];              // sum of p over the same
    unsigned cp[4];             // the group's own samples, c below p << 16
};

__device__ __forceinline__ Sums fold(const Row &c, const Row &p) {
    int d[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) d[j] = (int)c.v[j] - (int)p.v[j];
    Sums s;
    s.a[0] = d[0] + d[1] + d[2] + d[3] + d[4];
    s.b[0] = p.v[0] + p.v[1] + p.v[2] + p.v[3] + p.v[4];
#pragma unroll
    for (int i = 1; i < 4; ++i) {
        s.a[i] = s.a[i - 1] - d[i - 1] + d[i + 4];
        s.b[i] = s.b[i - 1] - p.v[i - 1] + p.v[i + 4];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) s.cp[i] = c.v[i + 2] | (p.v[i + 2] << 16);
    return s;
}

// WIDE: both frames are 8-byte aligned (the row pitch 2 W always is)
template <bool WIDE>
__global__ __launch_bounds__(256) void raw_temporal_kernel(const uint16_t *__restrict__ cur, const uint16_t *__restrict__ state,
                                                           uint16_t *__restrict__ out, size_t items, int H, int W, int per_row,
                                                           int strips, Params q) {
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < items; t += (size_t)gridDim.x * blockDim.x) {
        const size_t band = t / per_row;                // n * strips + strip
        const int x = (int)(t - band * per_row) * 4, y0 = (int)(band % (size_t)strips) * ROWS;
        const size_t n = band / (size_t)strips, img = n * (size_t)H * (size_t)W;
        const bool left = x == 0, right = x + 4 == W;
        Sums win[5];
#pragma unroll
        for (int r = 0; r < ROWS + 4; ++r) {
            const int y = y0 + r - 4;                   // the row this step completes, once r >= 4
            if (r >= 4 && y >= H) break;
            const int yy = reflect_row(y + 2, H);       // the row this step loads: y0-2 .. y0+ROWS+1, at most H+1
            const size_t at = img + (size_t)yy * (size_t)W;
            win[r % 5] = fold(load_row<16, WIDE>(reinterpret_cast<const uint8_t *>(cur + at), x, left, right),
                              load_row<16, WIDE>(reinterpret_cast<const uint8_t *>(state + at), x, left, right));
            if (r < 4) continue;
            const Sums &mid = win[(r - 2) % 5];         // row y itself
            unsigned o[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int A = win[0].a[i] + win[1].a[i] + win[2].a[i] + win[3].a[i] + win[4].a[i];
                const unsigned B = win[0].b[i] + win[1].b[i] + win[2].b[i] + win[3].b[i] + win[4].b[i];
                o[i] = risp_temporal::blend(mid.cp[i] & 0xFFFFu, mid.cp[i] >> 16, A, B, q);
            }
            *reinterpret_cast<ushort4 *>(out + img + (size_t)y * (size_t)W + x) =         // W % 4 == 0, out 8-byte aligned
                ushort4{(unsigned short)o[0], (unsigned short)o[1], (unsigned short)o[2], (unsigned short)o[3]};
        }
    }
}

}  // namespace

extern "C" int risp_raw_temporal(const uint16_t *cur, uint16_t *state, uint16_t *out, int prime, int strength, int threshold,
                                 int slope, int ramp, int black_level, int N, int H, int W, void *stream) {
    const char *name = "risp_raw_temporal";
    RISP_CHECK_ARG(cur && state && out, "%s: null argument", name);
    RISP_CHECK_ARG(N >= 1 && H >= 3, "%s: bad shape N=%d H=%d (at least 3 rows: a reflected row stays inside the frame)", name, N, H);
    RISP_CHECK_ARG(W >= 4 && W % 4 == 0, "%s: W %d (a multiple of 4)", name, W);
    RISP_CHECK_ARG(strength >= 0 && strength <= 256, "%s: strength %d outside 0 .. 256", name, strength);
    RISP_CHECK_ARG(threshold >= 0 && threshold <= 65535, "%s: threshold %d outside 0 .. 65535", name, threshold);
    RISP_CHECK_ARG(slope >= 0 && slope <= 255, "%s: slope %d outside 0 .. 255", name, slope);
    RISP_CHECK_ARG(ramp >= 0 && ramp <= 65535, "%s: ramp %d outside 0 .. 65535", name, ramp);
    RISP_CHECK_ARG(black_level >= 0 && black_level <= 65535, "%s: black_level %d outside 0 .. 65535", name, black_level);
    const uintptr_t c0 = reinterpret_cast<uintptr_t>(cur), s0 = reinterpret_cast<uintptr_t>(state), o0 = reinterpret_cast<uintptr_t>(out);
    RISP_CHECK_ARG(c0 % 2 == 0 && s0 % 2 == 0, "%s: cur %p and state %p must be 2-byte aligned", name, (const void *)cur, (void *)state);
    if (int err = out_check(name, out)) return err;
    const size_t bytes = (size_t)N * (size_t)H * (size_t)W * sizeof(uint16_t);
    RISP_CHECK_ARG((o0 + bytes <= c0 || c0 + bytes <= o0) && (o0 + bytes <= s0 || s0 + bytes <= o0),
                   "%s: out %p overlaps cur %p or state %p: a thread reads rows other threads write", name, (void *)out,
                   (const void *)cur, (void *)state);
    hipStream_t s = (hipStream_t)stream;
    if (prime) {                                        // the state is not read: out = cur, and the copy below makes state = cur
        if (hipMemcpyAsync(out, cur, bytes, hipMemcpyDeviceToDevice, s) != hipSuccess) {
            risp_set_error("%s: copy failed", name);
            return 2;
        }
    } else {
        const int per_row = W / 4, strips = (H + ROWS - 1) / ROWS;
        const size_t items = (size_t)N * strips * per_row;
        const dim3 grid = capped_grid(items);
        const Params q{(unsigned)strength, 25u * (unsigned)threshold, (unsigned)slope, (unsigned)ramp, 25u * (unsigned)black_level};
        if (c0 % 8 == 0 && s0 % 8 == 0)
            hipLaunchKernelGGL((raw_temporal_kernel<true>), grid, dim3(256), 0, s, cur, state, out, items, H, W, per_row, strips, q);
        else
            hipLaunchKernelGGL((raw_temporal_kernel<false>), grid, dim3(256), 0, s, cur, state, out, items, H, W, per_row, strips, q);
        RISP_LAUNCH_CHECK(name);
    }
#ifndef RISP_TEMPORAL_NO_COPY                           // (make EXTRA=-DRISP_TEMPORAL_NO_COPY: the launch alone, tools/bench_serve_temporal.py)
    if (hipMemcpyAsync(state, out, bytes, hipMemcpyDeviceToDevice, s) != hipSuccess) {
        risp_set_error("%s: copy failed", name);
        return 2;
    }
#endif
    return 0;
}
