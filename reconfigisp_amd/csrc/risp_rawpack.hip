// MIPI-packed RAW10 / RAW12 frames to (N,H,W) uint16, one sample per word: the definition of risp_rawpack.h.  The front of every
// serving route that has no fused packed load (risp_serve_packed and risp_serve_classical_packed have one): bits / 8 bytes read
// and 2 written per pixel, one launch.
//
// A thread owns up to 16 pixels of one row: four RAW10 groups (20 bytes) or eight RAW12 groups (24 bytes) in, four 8-byte
// stores out.  Wide form (packed base and stride 4-byte aligned): a full chunk is five or six dword loads - the chunk starts at
// a multiple of 20 / 24 bytes of an aligned row - and a row's last, shorter chunk takes the byte form.  Byte form (any base,
// any stride): the 4-, 2- and 1-byte copies of risp_rawpack.h per four pixels.  Neither reads a byte behind W * bits / 8 of a row.
#include "risp_common.h"
#include "risp_rawframe.h"
#include "risp_rawpack.h"

namespace {

using namespace risp_rawpack;

constexpr int CHUNK = 16;       // pixels per thread

template <int BITS, bool WIDE>
__global__ __launch_bounds__(256) void raw_unpack_kernel(const uint8_t *__restrict__ packed, uint16_t *__restrict__ out, size_t chunks,
                                                         int W, int stride, int per_row) {
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < chunks; t += (size_t)gridDim.x * blockDim.x) {
        const size_t line = t / per_row;                // n * H + y
        const int x0 = (int)(t - line * per_row) * CHUNK;
        const uint8_t *row = packed + line * (size_t)stride;
        ushort4 *dst = reinterpret_cast<ushort4 *>(out + line * (size_t)W + x0);         // W % 4 == 0, out 8-byte aligned
        const int groups = (W - x0 < CHUNK ? W - x0 : CHUNK) / 4;
        if (WIDE && groups == CHUNK / 4) {
            constexpr int DW = CHUNK * BITS / 32;       // 5 or 6
            const unsigned *src = reinterpret_cast<const unsigned *>(row + (size_t)x0 * BITS / 8);
            unsigned d[DW];
#pragma unroll
            for (int i = 0; i < DW; ++i) d[i] = src[i];
            auto byte = [&](int i) { return d[i >> 2] >> (8 * (i & 3)) & 255u; };
#pragma unroll
            for (int g = 0; g < CHUNK / 4; ++g) {
                if constexpr (BITS == 10) {
                    const int b = 5 * g;
                    dst[g] = raw10_group(byte(b) | byte(b + 1) << 8 | byte(b + 2) << 16 | byte(b + 3) << 24, byte(b + 4));
                } else {
                    const int b = 6 * g;
                    const ushort2 p = raw12_group(byte(b), byte(b + 1), byte(b + 2)), q = raw12_group(byte(b + 3), byte(b + 4), byte(b + 5));
                    dst[g] = ushort4{p.x, p.y, q.x, q.y};
                }
            }
        } else {
            for (int g = 0; g < groups; ++g) dst[g] = ld4<BITS>(row, x0 + 4 * g);
        }
    }
}

}  // namespace

extern "C" int risp_raw_unpack(const uint8_t *packed, uint16_t *out, int bits, int N, int H, int W, int stride, void *stream) {
    const char *name = "risp_raw_unpack";
    RISP_CHECK_ARG(packed && out, "%s: null argument", name);
    RISP_CHECK_ARG(N >= 1 && H >= 1, "%s: bad shape N=%d H=%d", name, N, H);
    if (int err = rawpack_check(name, bits, W, stride)) return err;
    if (int err = risp_rawframe::out_check(name, out)) return err;
    const int per_row = (W + CHUNK - 1) / CHUNK;
    const size_t chunks = (size_t)N * H * per_row;
    const dim3 grid = risp_rawframe::capped_grid(chunks);
    hipStream_t s = (hipStream_t)stream;
    const bool wide = reinterpret_cast<uintptr_t>(packed) % 4 == 0 && stride % 4 == 0;
    if (bits == 10) {
        if (wide) hipLaunchKernelGGL((raw_unpack_kernel<10, true>), grid, dim3(256), 0, s, packed, out, chunks, W, stride, per_row);
        else hipLaunchKernelGGL((raw_unpack_kernel<10, false>), grid, dim3(256), 0, s, packed, out, chunks, W, stride, per_row);
    } else {
        if (wide) hipLaunchKernelGGL((raw_unpack_kernel<12, true>), grid, dim3(256), 0, s, packed, out, chunks, W, stride, per_row);
        else hipLaunchKernelGGL((raw_unpack_kernel<12, false>), grid, dim3(256), 0, s, packed, out, chunks, W, stride, per_row);
    }
    RISP_LAUNCH_CHECK(name);
    return 0;
}
