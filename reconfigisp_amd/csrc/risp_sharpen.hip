// Output sharpening in ONE launch: (N,H,W,3) packed bytes -> (N,H,W,3) packed bytes or (N,3H/2,W) NV12 of the sharpened codes.
// The edge-enhancement block of the serving path: an unsharp mask of an 8-bit luma with a binomial blur of radius 1 or 2
// (replicate border), soft coring, a Q8 gain and a limit, the same signed step added to B, G and R.  include/risp.h has the
// integer definition; tests/sharpen_reference.py restates it in numpy.
//
// A workgroup of 256 threads owns RISP_SHARPEN_TILE_W x RISP_SHARPEN_TILE_H = 64 x 16 pixels.
//   phase 0  the tile's source box - the tile widened by the radius, clamped into the image - goes to LDS (stage_box of
//            risp_bgr8tile.h, which owns the loads of an image that starts at any byte and every store below).
//   phase 1  the luma byte of every pixel of the (64 + 2R) x (16 + 2R) halo, its indices clamped into the image (they stay
//            inside the box by construction).
//   phase 2  the horizontal binomial sums of the 64 columns for the 16 + 2R halo rows, 16 bits each.
//   phase 3  a thread owns one column and four consecutive rows: 4 + 2R horizontal sums from LDS give its four blurs; detail,
//            coring, gain, limit, and the three clamped channels go to a 16 x 192 byte image of the tile in LDS.
//   phase 4  BGR: the tile is stored (store_tile).  NV12: a thread makes a 2 x 4 pixel patch - two Y dwords and one UV dword -
//            and stores dwords where W % 4 == 0 and out is 4-byte aligned, bytes otherwise.
// LDS: static, 11.2 KB (radius 2) or 10.1 KB (radius 1).  No scratch.
#include "risp_bgr8tile.h"

namespace {

using namespace risp_bgr8tile;

constexpr int TH = RISP_SHARPEN_TILE_H, PIX = TW * TH / 256;
static_assert(TW == RISP_SHARPEN_TILE_W && TH == 4 * PIX && PIX == 4, "a wave owns one 64-pixel row at a time, a thread four consecutive rows");

struct Par {
    int rgb_in, amount, thr256, limit;
};

template <int R, bool NV12>
__global__ __launch_bounds__(256) void sharpen_kernel(const uint8_t *__restrict__ img, uint8_t *__restrict__ out, const Coef m,
                                                      const Par par, int N, int H, int W) {
    constexpr int HW = TW + 2 * R, HH = TH + 2 * R;
    constexpr int PITCH = (HW * 3 + 3 + 3) & ~3, PD = PITCH / 4;    // up to 3 bytes in front of a box row's first, whole dwords
    __shared__ __align__(16) unsigned s_box[HH * PD];               // the source box
    __shared__ __align__(16) unsigned s_outd[TH * ROWD];            // the tile's sharpened bytes
    __shared__ unsigned short s_h[HH * TW];                         // horizontal binomial sums of luma
    __shared__ uint8_t s_l[HH * HW];                                // luma of the halo
    uint8_t *s_out = reinterpret_cast<uint8_t *>(s_outd);
    const int tid = threadIdx.x, j0 = blockIdx.x * TW, i0 = blockIdx.y * TH, n = blockIdx.z;
    const int cols = min(TW, W - j0), rows = min(TH, H - i0);

    // phase 0
    const int by0 = max(i0 - R, 0), by1 = min(i0 + rows - 1 + R, H - 1), bx0 = max(j0 - R, 0), bx1 = min(j0 + cols - 1 + R, W - 1);
    const Box box = stage_box<PITCH>(img, N, H, W, img + (((size_t)n * H + by0) * W + bx0) * 3, by0, by1, bx0, bx1, s_box, tid);
    __syncthreads();

    // phase 1: the clamped indices lie inside the box - its last row is the clamp of the halo's last row, its last column likewise
    for (int t = tid; t < HH * HW; t += 256) {
        const int r = t / HW, c = t - r * HW;
        const uint8_t *p = box.at(clampi(i0 - R + r, 0, H - 1), clampi(j0 - R + c, 0, W - 1));
        const unsigned c0 = p[0], g = p[1], c2 = p[2], rr = par.rgb_in ? c0 : c2, bb = par.rgb_in ? c2 : c0;
        s_l[t] = (uint8_t)((77u * rr + 150u * g + 29u * bb + 128u) >> 8);
    }
    __syncthreads();

    // phase 2
    for (int t = tid; t < HH * TW; t += 256) {
        const int r = t / TW, c = t - r * TW;
        const uint8_t *l = s_l + r * HW + c;
        s_h[t] = (unsigned short)(R == 2 ? l[0] + 4 * l[1] + 6 * l[2] + 4 * l[3] + l[4] : l[0] + 2 * l[1] + l[2]);
    }
    __syncthreads();

    // phase 3
    {
        const int px = tid & (TW - 1), pyb = (tid >> 6) * PIX;
        int v[PIX + 2 * R];
#pragma unroll
        for (int e = 0; e < PIX + 2 * R; ++e) v[e] = s_h[(pyb + e) * TW + px];
#pragma unroll
        for (int e = 0; e < PIX; ++e) {
            const int py = pyb + e;
            if (px >= cols || py >= rows) continue;
            const int S = R == 2 ? v[e] + 4 * v[e + 1] + 6 * v[e + 2] + 4 * v[e + 3] + v[e + 4] : 16 * (v[e] + 2 * v[e + 1] + v[e + 2]);
            const int D = 256 * (int)s_l[(py + R) * HW + px + R] - S;
            const unsigned A = (unsigned)max((D < 0 ? -D : D) - par.thr256, 0);
            const int E = (int)min((A * (unsigned)par.amount + 32768u) >> 16, (unsigned)par.limit), step = D < 0 ? -E : E;
            const uint8_t *p = box.at(i0 + py, j0 + px);
            uint8_t *dst = s_out + py * ROWB + px * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) dst[c] = (uint8_t)clampi((int)p[c] + step, 0, 255);
        }
    }
    __syncthreads();

    // phase 4
    if (!NV12) {
        store_tile(out + (((size_t)n * H + i0) * W + j0) * 3, (size_t)W * 3, s_outd, rows, cols, tid);
    } else {
        // H and W even: i0 and rows are even, a patch has two whole rows and one or two whole quads
        uint8_t *dst = out + (size_t)n * (H + H / 2) * W;
        const bool wide = W % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 4 == 0;     // every patch whole, its dwords aligned
        for (int t = tid; t < (rows / 2) * (TW / 4); t += 256) {
            const int p = t / (TW / 4), q = t - p * (TW / 4), col = q * 4;
            if (col >= cols) continue;
            unsigned r[2][4], g[2][4], b[2][4], y[2], uv[2];
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                const unsigned *src = s_outd + (2 * p + a) * ROWD + q * 3;
                unpack4(src[0], src[1], src[2], par.rgb_in, r[a], g[a], b[a]);
            }
            nv12_patch(m, r, g, b, y, uv);
            uint8_t *py = dst + (size_t)(i0 + 2 * p) * W + j0 + col, *pc = dst + (size_t)(H + i0 / 2 + p) * W + j0 + col;
            nv12_store_patch_at(py, pc, W, wide, col + 4 <= cols ? 2 : 1, y, uv);   // (a packed NV12 image starts at any byte too)
        }
    }
}

}  // namespace

extern "C" int risp_bgr8_sharpen(const uint8_t *img, uint8_t *out, const int32_t *coef, int rgb_in, int radius, int amount,
                                 int threshold, int limit, int N, int H, int W, void *stream) {
    const char *name = "risp_bgr8_sharpen";
    RISP_CHECK_ARG(img && out, "%s: null argument (img %p, out %p)", name, (const void *)img, (void *)out);
    RISP_CHECK_ARG(sizes_ok(1 << 24, N, H, W), "%s: bad shape N=%d H=%d W=%d (N <= 65535, sizes 1 .. 2^24)", name, N, H, W);
    RISP_CHECK_ARG(radius == 1 || radius == 2, "%s: radius %d: 1 (3 x 3 binomial blur) or 2 (5 x 5)", name, radius);
    RISP_CHECK_ARG(amount >= 0 && amount <= RISP_SHARPEN_MAX_AMOUNT, "%s: amount %d: 0 .. %d (Q8: 256 is 1.0)", name, amount,
                   RISP_SHARPEN_MAX_AMOUNT);
    RISP_CHECK_ARG(threshold >= 0 && threshold <= 255, "%s: threshold %d: 0 .. 255 codes", name, threshold);
    RISP_CHECK_ARG(limit >= 0 && limit <= 255, "%s: limit %d: 0 .. 255 codes", name, limit);
    unsigned gy;
    if (int err = row_tiles(name, "H", H, TH, gy)) return err;
    const size_t in_bytes = (size_t)N * H * W * 3, out_bytes = coef ? (size_t)N * (H + H / 2) * W : in_bytes;
    if (int err = apart_check(name, img, in_bytes, out, out_bytes, "pixels")) return err;
    Coef m = {};
    if (coef) {
        RISP_CHECK_ARG(H % 2 == 0 && W % 2 == 0, "%s: NV12 out needs H and W even, got %d x %d", name, H, W);
        if (int err = nv12_check(name, coef, m)) return err;
    }
    const Par par = {rgb_in ? 1 : 0, amount, 256 * threshold, limit};
    const dim3 grid((unsigned)((W + TW - 1) / TW), gy, (unsigned)N);
    hipStream_t s = (hipStream_t)stream;
    if (radius == 2) {
        if (coef) hipLaunchKernelGGL((sharpen_kernel<2, true>), grid, dim3(256), 0, s, img, out, m, par, N, H, W);
        else hipLaunchKernelGGL((sharpen_kernel<2, false>), grid, dim3(256), 0, s, img, out, m, par, N, H, W);
    } else {
        if (coef) hipLaunchKernelGGL((sharpen_kernel<1, true>), grid, dim3(256), 0, s, img, out, m, par, N, H, W);
        else hipLaunchKernelGGL((sharpen_kernel<1, false>), grid, dim3(256), 0, s, img, out, m, par, N, H, W);
    }
    RISP_LAUNCH_CHECK(name);
    return 0;
}
