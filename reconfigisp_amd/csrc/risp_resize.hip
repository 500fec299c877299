// A scaled, cropped output in ONE launch: (N,H,W,3) packed bytes -> (N,OH,OW,3) packed bytes or (N,3*OH/2,OW) NV12, resampled
// separably with the integer tap tables of include/risp.h (Q14 weights, rows summing to 16384; horizontal first, each pass
// rounded to a code).  The end of a serving call with out_size / out_window; tests/resize_reference.py restates it in numpy.
//
// A workgroup of 256 threads owns TW = 64 output columns x `rows` output rows.
//   phase 0  the tile's slices of both tables go to LDS (columns and rows past the image get zero weights).
//   phase 1  for the `need` source rows the tile's output rows touch, its 64 columns are resampled horizontally into LDS as
//            bytes: a thread makes one dword (4 of a row's 192 bytes) per step, its source bytes come from global memory
//            (neighbouring lanes read neighbouring and overlapping taps, which the vector cache serves).
//   phase 2  vertical sums from LDS, one dword per LDS row and tap.  BGR: a thread makes one dword of an output row and stores
//            it by the policy of a packed row (store_dword of risp_bgr8tile.h, which owns every store here).  NV12: a thread
//            makes a 2 x 4 pixel patch - two Y dwords and one UV dword - and stores dwords where OW % 4 == 0, byte pairs otherwise.
// LDS: span x 192 bytes of rows plus the table slices (at most 6.4 KB), dynamic, at most RISP_RESIZE_LDS_BYTES.  The span is the
// caller's, since only the caller has read ystart; every LDS row index is clamped into the rows phase 1 wrote and every source
// index into the image, so no table can make an access leave either.
#include "risp_bgr8tile.h"

namespace {

using namespace risp_bgr8tile;

static_assert(TW == RISP_RESIZE_TILE_W, "the tile of risp_bgr8tile.h");

struct Geo {
    int H, W, OH, OW, tx, ty, rows, span;
};

__host__ __device__ inline size_t resize_lds_bytes(int span, int rows, int tx, int ty) {
    return (size_t)span * ROWB + (size_t)(TW + rows) * 4 + ((size_t)TW * tx + (size_t)rows * ty) * 2;
}

// a Q14 sum -> a code: rounded, floored by the arithmetic shift, clamped
__device__ __forceinline__ unsigned q14_code(int s) { return (unsigned)clampi((s + 8192) >> 14, 0, 255); }

template <bool NV12>
__global__ __launch_bounds__(256) void resize_kernel(const uint8_t *__restrict__ img, uint8_t *__restrict__ out,
                                                     const int32_t *__restrict__ xstart, const int16_t *__restrict__ xweight,
                                                     const int32_t *__restrict__ ystart, const int16_t *__restrict__ yweight,
                                                     const Coef m, int rgb_in, const Geo g) {
    extern __shared__ __align__(16) uint8_t lds[];
    unsigned *s_h = reinterpret_cast<unsigned *>(lds);                                   // [span][ROWD] dwords of codes
    int *s_xs = reinterpret_cast<int *>(lds + (size_t)g.span * ROWB), *s_ys = s_xs + TW;   // [TW], [rows]
    short *s_wx = reinterpret_cast<short *>(s_ys + g.rows), *s_wy = s_wx + TW * g.tx;      // [TW][tx], [rows][ty]
    const int tid = threadIdx.x, j0 = blockIdx.x * TW, i0 = blockIdx.y * g.rows, n = blockIdx.z;
    const int cols = min(TW, g.OW - j0), rows = min(g.rows, g.OH - i0), tx = g.tx, ty = g.ty;

    // (a start of a right table lies in the image already; clamped here, no sum below can wrap whatever the table holds, and
    // the bytes of a wrong table are defined: those of the clamped one)
    for (int t = tid; t < TW; t += 256) s_xs[t] = clampi(xstart[min(j0 + t, g.OW - 1)], 0, g.W - 1);
    for (int t = tid; t < g.rows; t += 256) s_ys[t] = clampi(ystart[min(i0 + t, g.OH - 1)], 0, g.H - 1);
    for (int t = tid; t < TW * tx; t += 256) s_wx[t] = t / tx < cols ? xweight[(size_t)j0 * tx + t] : (short)0;
    for (int t = tid; t < g.rows * ty; t += 256) s_wy[t] = t / ty < rows ? yweight[(size_t)i0 * ty + t] : (short)0;
    __syncthreads();

    // the source rows of this tile, from its smallest start to its largest plus ty.  Starts are not monotone everywhere: a bicubic
    // enlargement drops the zero outer taps of an output that falls exactly on a sample.  (every lane reads the same LDS words)
    int y0 = s_ys[0], y1 = y0;
    for (int i = 1; i < rows; ++i) y0 = min(y0, s_ys[i]), y1 = max(y1, s_ys[i]);
    const int need = clampi(y1 + ty - y0, 1, g.span);
    const uint8_t *src = img + (size_t)n * g.H * g.W * 3;
    for (int t = tid; t < need * ROWD; t += 256) {
        const int r = t / ROWD, d = t - r * ROWD;
        const uint8_t *row = src + (size_t)clampi(y0 + r, 0, g.H - 1) * g.W * 3;
        unsigned pack = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int e = d * 4 + b, j = e / 3, c = e - j * 3, xs = s_xs[j];
            const short *w = s_wx + j * tx;
            int s = 0;
            for (int k = 0; k < tx; ++k) s += (int)w[k] * (int)row[clampi(xs + k, 0, g.W - 1) * 3 + c];
            pack |= q14_code(s) << (8 * b);
        }
        s_h[t] = pack;
    }
    __syncthreads();

    if (!NV12) {
        uint8_t *dst = out + ((size_t)n * g.OH * g.OW + j0) * 3;
        const int valid = cols * 3;
        for (int t = tid; t < rows * ROWD; t += 256) {
            const int i = t / ROWD, d = t - i * ROWD;
            if (d * 4 >= valid) continue;
            const int r0 = s_ys[i] - y0;
            const short *w = s_wy + i * ty;
            int s[4] = {0, 0, 0, 0};
            for (int k = 0; k < ty; ++k) {
                const unsigned v = s_h[clampi(r0 + k, 0, need - 1) * ROWD + d];
                const int wk = w[k];
                s[0] += wk * (int)(v & 255u), s[1] += wk * (int)(v >> 8 & 255u), s[2] += wk * (int)(v >> 16 & 255u),
                    s[3] += wk * (int)(v >> 24);
            }
            const unsigned pack = q14_code(s[0]) | q14_code(s[1]) << 8 | q14_code(s[2]) << 16 | q14_code(s[3]) << 24;
            store_dword(dst + (size_t)(i0 + i) * g.OW * 3 + d * 4, pack, d * 4, valid);
        }
    } else {
        // OH, OW, g.rows even: i0 and rows are even, a patch has two whole rows and one or two whole quads
        uint8_t *dst = out + (size_t)n * (g.OH + g.OH / 2) * g.OW;
        const bool wide = g.OW % 4 == 0;                    // with out 4-byte aligned: every patch is whole and its dwords aligned
        for (int t = tid; t < (rows / 2) * (TW / 4); t += 256) {
            const int p = t / (TW / 4), q = t - p * (TW / 4), col = q * 4;
            if (col >= cols) continue;
            unsigned R[2][4], G[2][4], B[2][4];
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                const int i = 2 * p + a, r0 = s_ys[i] - y0;
                const short *w = s_wy + i * ty;
                int s[12];
#pragma unroll
                for (int e = 0; e < 12; ++e) s[e] = 0;
                for (int k = 0; k < ty; ++k) {
                    const unsigned *v = s_h + clampi(r0 + k, 0, need - 1) * ROWD + q * 3;
                    const int wk = w[k];
#pragma unroll
                    for (int e = 0; e < 12; ++e) s[e] += wk * (int)(v[e >> 2] >> (8 * (e & 3)) & 255u);
                }
#pragma unroll
                for (int x = 0; x < 4; ++x) {
                    const unsigned first = q14_code(s[3 * x]), third = q14_code(s[3 * x + 2]);
                    G[a][x] = q14_code(s[3 * x + 1]);
                    R[a][x] = rgb_in ? first : third, B[a][x] = rgb_in ? third : first;
                }
            }
            unsigned y[2], uv[2];
            nv12_patch(m, R, G, B, y, uv);
            uint8_t *py = dst + (size_t)(i0 + 2 * p) * g.OW + j0 + col, *pc = dst + (size_t)(g.OH + i0 / 2 + p) * g.OW + j0 + col;
            nv12_store_patch_at<true>(py, pc, g.OW, wide, col + 4 <= cols ? 2 : 1, y, uv);   // OW even, out aligned: byte pairs
        }
    }
}

}  // namespace

extern "C" int risp_bgr8_resize(const uint8_t *img, uint8_t *out, const int32_t *xstart, const int16_t *xweight, int tx,
                                const int32_t *ystart, const int16_t *yweight, int ty, int tile_rows, int span, const int32_t *coef,
                                int rgb_in, int N, int H, int W, int OH, int OW, void *stream) {
    const char *name = "risp_bgr8_resize";
    RISP_CHECK_ARG(img && out && xstart && xweight && ystart && yweight, "%s: null argument", name);
    RISP_CHECK_ARG(sizes_ok(1 << 24, N, H, W, OH, OW), "%s: bad shape N=%d H=%d W=%d OH=%d OW=%d (N <= 65535, sizes 1 .. 2^24)", name, N,
                   H, W, OH, OW);
    RISP_CHECK_ARG(tx >= 1 && tx <= RISP_RESIZE_MAX_TAPS && ty >= 1 && ty <= RISP_RESIZE_MAX_TAPS,
                   "%s: %d x %d taps: at most RISP_RESIZE_MAX_TAPS = %d per axis (the largest served reductions are about 32:1 box, "
                   "16:1 triangle, 8:1 bicubic)",
                   name, ty, tx, RISP_RESIZE_MAX_TAPS);
    RISP_CHECK_ARG(tx <= W && ty <= H, "%s: %d x %d taps on a %d x %d image: T <= S on both axes", name, ty, tx, H, W);
    RISP_CHECK_ARG(tile_rows >= 1 && tile_rows <= 64 && span >= 1, "%s: tile_rows %d (1 .. 64), span %d (>= 1)", name, tile_rows, span);
    const size_t lds = resize_lds_bytes(span, tile_rows, tx, ty);
    RISP_CHECK_ARG(lds <= RISP_RESIZE_LDS_BYTES,
                   "%s: a span of %d source rows with %d tile rows needs %zu bytes of LDS, at most %d: take fewer tile rows", name, span,
                   tile_rows, lds, RISP_RESIZE_LDS_BYTES);
    const size_t in_bytes = (size_t)N * H * W * 3, out_bytes = coef ? (size_t)N * (OH + OH / 2) * OW : (size_t)N * OH * OW * 3;
    if (int err = apart_check(name, img, in_bytes, out, out_bytes, "rows")) return err;
    Coef m = {};
    if (coef) {
        RISP_CHECK_ARG(OH % 2 == 0 && OW % 2 == 0 && tile_rows % 2 == 0, "%s: NV12 out needs OH, OW and tile_rows even, got %d x %d, %d",
                       name, OH, OW, tile_rows);
        RISP_CHECK_ARG(reinterpret_cast<uintptr_t>(out) % 4 == 0, "%s: NV12 out must be 4-byte aligned", name);
        if (int err = nv12_check(name, coef, m)) return err;
    }
    const unsigned gy = (unsigned)((OH + tile_rows - 1) / tile_rows);
    RISP_CHECK_ARG(gy <= 65535, "%s: %u row tiles, at most 65535", name, gy);
    const Geo g = {H, W, OH, OW, tx, ty, tile_rows, span};
    const dim3 grid((unsigned)((OW + TW - 1) / TW), gy, (unsigned)N);
    hipStream_t s = (hipStream_t)stream;
    if (coef)
        hipLaunchKernelGGL(resize_kernel<true>, grid, dim3(256), lds, s, img, out, xstart, xweight, ystart, yweight, m, rgb_in ? 1 : 0, g);
    else
        hipLaunchKernelGGL(resize_kernel<false>, grid, dim3(256), lds, s, img, out, xstart, xweight, ystart, yweight, m, 0, g);
    RISP_LAUNCH_CHECK(name);
    return 0;
}
