// A geometry-corrected output in ONE launch: (N,H,W,3) packed bytes -> (N,WH,WW,3) packed bytes through a mesh of Q8 source
// coordinates (include/risp.h has the integer definition: bilinear patches of 1 << k output pixels, replicate border, bilinear
// or Q11 Catmull-Rom taps).  The LDC / GDC / dewarp block of the serving path; tests/warp_reference.py restates it in numpy.
//
// A workgroup of 256 threads owns RISP_WARP_TILE_W x RISP_WARP_TILE_H = 64 x 16 output pixels, a thread four of them (one per
// quarter of the tile's rows: a wave works on one output row at a time).
//   phase 0  bicubic: thread f makes row f of the Q11 weight table in LDS from the integer formula.  Every thread evaluates the
//            clamped Q8 coordinates of its four pixels from the four mesh nodes of their cell (64-bit products) and keeps them.
//   phase 1  the smallest and largest integer source row and column of the tile (LDS atomics), widened by the kernel's taps and
//            clamped into the image: the tile's source box.
//   phase 2  stage = 1 and the box fits: the box goes to LDS (stage_box of risp_bgr8tile.h, which owns the loads of an image that
//            starts at any byte and the store of phase 4).  Otherwise (stage = 0, or a strong reduction, a twisted cell, a
//            meaningless mesh) the tile samples global memory.  The decision is the same for every thread of the workgroup.
//   phase 3  the taps, from LDS bytes or global bytes - the same integer function -, into a 16 x 192 byte image of the tile in LDS.
//   phase 4  the tile is stored (store_tile).
// LDS: dynamic; 2048 bytes of weights, 16 of box corners, 3072 of output tile, then the box (stage = 1: RISP_WARP_LDS_BYTES in
// all, stage = 0 the fixed part only).  Every coordinate is clamped into the image before it is used, so no mesh can make an
// access leave img, and every LDS index derives from coordinates inside the box by construction.
#include "risp_bgr8tile.h"

namespace {

using namespace risp_bgr8tile;

constexpr int TH = RISP_WARP_TILE_H, PIX = TW * TH / 256;
constexpr int FIXED_LDS = 256 * 4 * 2 + 16 + TH * ROWB;
// what a stage = 1 launch asks for and a tile's box has to fit beside the fixed part.  RISP_WARP_AB_LDS: the ablation builds of
// profiles/serve_warp_lds.txt (make EXTRA=-DRISP_WARP_AB_LDS=16384), never the library's
#ifdef RISP_WARP_AB_LDS
constexpr int LDS_BYTES = RISP_WARP_AB_LDS;
#else
constexpr int LDS_BYTES = RISP_WARP_LDS_BYTES;
#endif
static_assert(TW == RISP_WARP_TILE_W && (TW * TH) % 256 == 0, "a wave owns one 64-pixel row of the tile at a time");
static_assert(FIXED_LDS % 4 == 0 && FIXED_LDS < LDS_BYTES && LDS_BYTES <= 65536, "the box begins on a dword");

struct Geo {
    int H, W, WH, WW, k, MW;
};

// row f of the Catmull-Rom table: Q11, the four weights sum to exactly 2048
__device__ __forceinline__ void cubic_row(int f, short *q) {
    const int f2 = f * f, f3 = f2 * f;
    const int n[4] = {-f3 + 512 * f2 - 65536 * f, 3 * f3 - 1280 * f2 + (1 << 25), -3 * f3 + 1024 * f2 + 65536 * f, f3 - 256 * f2};
    int v[4], best = 0, sum = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        v[t] = (n[t] + 8192) >> 14;
        sum += v[t];
    }
#pragma unroll
    for (int t = 1; t < 4; ++t)
        if (v[t] > v[best]) best = t;
#pragma unroll
    for (int t = 0; t < 4; ++t) q[t] = (short)(v[t] + (t == best ? 2048 - sum : 0));
}

// one component of the per-pixel coordinate: the bilinear patch in 64 bits, rounded, floored, clamped
__device__ __forceinline__ int patch_coord(int m00, int m01, int m10, int m11, int fx, int fy, int k, int S) {
    const long long cell = 1LL << k;
    const long long top = (cell - fx) * (long long)m00 + fx * (long long)m01;
    const long long bot = (cell - fx) * (long long)m10 + fx * (long long)m11;
    const long long u = ((cell - fy) * top + fy * bot + (1LL << (2 * k - 1))) >> (2 * k);
    const long long hi = (long long)(S - 1) << 8;
    return (int)(u < 0 ? 0 : (u > hi ? hi : u));
}

// the bytes of a pixel: from the staged Box or from img
struct ImgFetch {
    const uint8_t *src;
    int W;
    __device__ __forceinline__ const uint8_t *at(int y, int x) const { return src + ((size_t)y * W + x) * 3; }
};

template <typename Fetch>
__device__ __forceinline__ void sample_bilinear(const Fetch &f, int uy, int ux, int H, int W, uint8_t *dst) {
    const int y0 = uy >> 8, ty = uy & 255, y1 = min(y0 + 1, H - 1), x0 = ux >> 8, tx = ux & 255, x1 = min(x0 + 1, W - 1);
    const uint8_t *p00 = f.at(y0, x0), *p01 = f.at(y0, x1), *p10 = f.at(y1, x0), *p11 = f.at(y1, x1);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const unsigned top = (256 - tx) * p00[c] + tx * p01[c], bot = (256 - tx) * p10[c] + tx * p11[c];
        dst[c] = (uint8_t)(((256 - ty) * top + ty * bot + 32768u) >> 16);
    }
}

template <typename Fetch>
__device__ __forceinline__ void sample_bicubic(const Fetch &f, const short *q, int uy, int ux, int H, int W, uint8_t *dst) {
    const int y0 = uy >> 8, ty = uy & 255, x0 = ux >> 8, tx = ux & 255;
    int wx[4], wy[4], xs[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) wx[t] = q[tx * 4 + t], wy[t] = q[ty * 4 + t], xs[t] = clampi(x0 - 1 + t, 0, W - 1);
    int v[3] = {0, 0, 0};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int y = clampi(y0 - 1 + r, 0, H - 1);
        int h[3] = {0, 0, 0};
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const uint8_t *p = f.at(y, xs[t]);
#pragma unroll
            for (int c = 0; c < 3; ++c) h[c] += wx[t] * (int)p[c];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] += wy[r] * h[c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[c] = (uint8_t)clampi((v[c] + (1 << 21)) >> 22, 0, 255);
}

template <bool CUBIC>
__global__ __launch_bounds__(256) void warp_kernel(const uint8_t *__restrict__ img, uint8_t *__restrict__ out,
                                                   const int32_t *__restrict__ mesh, int stage, int N, const Geo g) {
    extern __shared__ __align__(16) uint8_t lds[];
    short *s_q = reinterpret_cast<short *>(lds);                        // [256][4] Q11 weights
    int *s_box = reinterpret_cast<int *>(lds + 2048);                   // smallest row, largest row, smallest column, largest column
    uint8_t *s_out = lds + 2048 + 16;                                   // [TH][ROWB] the tile's bytes
    unsigned *s_src = reinterpret_cast<unsigned *>(lds + FIXED_LDS);   // the staged box
    const int tid = threadIdx.x, j0 = blockIdx.x * TW, i0 = blockIdx.y * TH, n = blockIdx.z;
    const int cols = min(TW, g.WW - j0), rows = min(TH, g.WH - i0), k = g.k, H = g.H, W = g.W;

    if (CUBIC) cubic_row(tid, s_q + tid * 4);
    if (tid < 4) s_box[tid] = (tid & 1) ? 0 : 0x7fffffff;
    int uy[PIX], ux[PIX];
    const int px = tid & (TW - 1);
    const bool in_x = px < cols;
#pragma unroll
    for (int e = 0; e < PIX; ++e) {
        const int py = (tid >> 6) + e * (256 / TW);
        // (a pixel of a ragged tile outside the output takes the coordinate of the tile's last one: never sampled, reads stay inside mesh)
        const int y = i0 + min(py, rows - 1), x = j0 + min(px, cols - 1);
        const int i = y >> k, fy = y & ((1 << k) - 1), j = x >> k, fx = x & ((1 << k) - 1);
        const int2 *m = reinterpret_cast<const int2 *>(mesh) + (size_t)i * g.MW + j;
        const int2 m00 = m[0], m01 = m[1], m10 = m[g.MW], m11 = m[g.MW + 1];
        uy[e] = patch_coord(m00.x, m01.x, m10.x, m11.x, fx, fy, k, H);
        ux[e] = patch_coord(m00.y, m01.y, m10.y, m11.y, fx, fy, k, W);
    }
    __syncthreads();
    const uint8_t *src = img + (size_t)n * H * W * 3;
    bool staged = false;
    Box bf = {};
    if (stage) {                                                        // (the same in every thread)
        int y_lo = uy[0] >> 8, y_hi = y_lo, x_lo = ux[0] >> 8, x_hi = x_lo;
#pragma unroll
        for (int e = 1; e < PIX; ++e)
            y_lo = min(y_lo, uy[e] >> 8), y_hi = max(y_hi, uy[e] >> 8), x_lo = min(x_lo, ux[e] >> 8), x_hi = max(x_hi, ux[e] >> 8);
        atomicMin(&s_box[0], y_lo), atomicMax(&s_box[1], y_hi), atomicMin(&s_box[2], x_lo), atomicMax(&s_box[3], x_hi);
        __syncthreads();
        // the taps: bilinear rows y0 .. y0+1, bicubic y0-1 .. y0+2, every index clamped into the image
        const int by0 = max(s_box[0] - (CUBIC ? 1 : 0), 0), by1 = min(s_box[1] + (CUBIC ? 2 : 1), H - 1);
        const int bx0 = max(s_box[2] - (CUBIC ? 1 : 0), 0), bx1 = min(s_box[3] + (CUBIC ? 2 : 1), W - 1);
        const long long pitch = ((long long)(bx1 - bx0 + 1) * 3 + 3 + 3) & ~3LL;   // up to 3 bytes in front of the row's first, whole dwords
        staged = (by1 - by0 + 1) * pitch <= LDS_BYTES - FIXED_LDS;
        if (staged) {
            bf = stage_box(img, N, H, W, src + ((size_t)by0 * W + bx0) * 3, by0, by1, bx0, bx1, s_src, tid, (int)pitch);
            __syncthreads();
        }
    }
    const ImgFetch gf = {src, W};
#pragma unroll
    for (int e = 0; e < PIX; ++e) {
        const int py = (tid >> 6) + e * (256 / TW);
        if (!in_x || py >= rows) continue;
        uint8_t *dst = s_out + py * ROWB + px * 3;
        if (staged) {
            if (CUBIC) sample_bicubic(bf, s_q, uy[e], ux[e], H, W, dst);
            else sample_bilinear(bf, uy[e], ux[e], H, W, dst);
        } else {
            if (CUBIC) sample_bicubic(gf, s_q, uy[e], ux[e], H, W, dst);
            else sample_bilinear(gf, uy[e], ux[e], H, W, dst);
        }
    }
    __syncthreads();
    store_tile(out + (((size_t)n * g.WH + i0) * g.WW + j0) * 3, (size_t)g.WW * 3, reinterpret_cast<const unsigned *>(s_out), rows, cols,
               tid);
}

}  // namespace

extern "C" int risp_bgr8_warp(const uint8_t *img, uint8_t *out, const int32_t *mesh, int cell_log2, int MH, int MW, int kernel,
                              int stage, int N, int H, int W, int WH, int WW, void *stream) {
    const char *name = "risp_bgr8_warp";
    RISP_CHECK_ARG(img && out && mesh, "%s: null argument (img %p, out %p, mesh %p)", name, (const void *)img, (void *)out,
                   (const void *)mesh);
    RISP_CHECK_ARG(sizes_ok(1 << 23, N, H, W, WH, WW),
                   "%s: bad shape N=%d H=%d W=%d WH=%d WW=%d (N <= 65535, sizes 1 .. 2^23: a Q8 coordinate fits int32)", name, N, H, W,
                   WH, WW);
    RISP_CHECK_ARG(cell_log2 >= 2 && cell_log2 <= 8, "%s: cell_log2 %d: 2 .. 8 (cells of 4 .. 256 pixels)", name, cell_log2);
    const int mh = ((WH - 1) >> cell_log2) + 2, mw = ((WW - 1) >> cell_log2) + 2;
    RISP_CHECK_ARG(MH == mh && MW == mw, "%s: a %d x %d mesh for a %d x %d output with cell_log2 %d: exactly %d x %d nodes", name, MH,
                   MW, WH, WW, cell_log2, mh, mw);
    RISP_CHECK_ARG(kernel == 0 || kernel == 1, "%s: kernel %d: 0 (bilinear) or 1 (bicubic)", name, kernel);
    RISP_CHECK_ARG(stage == 0 || stage == 1, "%s: stage %d: 0 (sample global memory) or 1 (stage the source box in LDS)", name, stage);
    unsigned gy;
    if (int err = row_tiles(name, "WH", WH, TH, gy)) return err;
    if (int err = apart_check(name, img, (size_t)N * H * W * 3, out, (size_t)N * WH * WW * 3, "pixels")) return err;
    RISP_CHECK_ARG(reinterpret_cast<uintptr_t>(mesh) % 8 == 0, "%s: mesh %p must be 8-byte aligned", name, (const void *)mesh);
    const Geo g = {H, W, WH, WW, cell_log2, MW};
    const dim3 grid((unsigned)((WW + TW - 1) / TW), gy, (unsigned)N);
    const size_t lds = stage ? LDS_BYTES : FIXED_LDS;
    hipStream_t s = (hipStream_t)stream;
    if (kernel)
        hipLaunchKernelGGL(warp_kernel<true>, grid, dim3(256), lds, s, img, out, mesh, stage, N, g);
    else
        hipLaunchKernelGGL(warp_kernel<false>, grid, dim3(256), lds, s, img, out, mesh, stage, N, g);
    RISP_LAUNCH_CHECK(name);
    return 0;
}
