// Packed 8-bit images to YUV 4:2:0 (NV12): (N,H,W,3) bytes in B,G,R or R,G,B order -> (N,3H/2,W) bytes, the integer definition
// of risp_nv12.h.  The end of every serving route that has no fused NV12 store (risp_serve_nv12 and risp_serve_classical_nv12
// have one): 3 bytes read and 1.5 written per pixel, one launch.
//
// Vector form (W % 4 == 0, both buffers 4-byte aligned): a thread owns a 2 x 4 pixel patch - two chroma quads -, loads the three
// dwords of each of its two rows (the row offset is a multiple of 12 bytes) and stores one Y dword per row and one UV dword.
// Scalar form (any even W, any alignment): a thread owns one quad and moves bytes.  unpack4 is risp_bgr8tile.h's.
#include "risp_bgr8tile.h"

namespace {

using namespace risp_bgr8tile;

__global__ __launch_bounds__(256) void bgr8_to_nv12_vec_kernel(const uint8_t *__restrict__ img, uint8_t *__restrict__ out, const Coef m,
                                                               int rgb_in, size_t patches, int H, int w4) {
    const int W = w4 * 4, h2 = H / 2;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < patches; t += (size_t)gridDim.x * blockDim.x) {
        const size_t n = t / ((size_t)h2 * w4), i = t - n * ((size_t)h2 * w4);
        const int py = (int)(i / w4) * 2, px = (int)(i % w4) * 4;
        unsigned r[2][4], g[2][4], b[2][4];
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const unsigned *src = reinterpret_cast<const unsigned *>(img + (((size_t)n * H + py + p) * W + px) * 3);
            unpack4(src[0], src[1], src[2], rgb_in, r[p], g[p], b[p]);
        }
        nv12_store_patch(out + n * ((size_t)(H + h2) * W), m, r, g, b, H, W, py, px, 0);
    }
}

__global__ __launch_bounds__(256) void bgr8_to_nv12_any_kernel(const uint8_t *__restrict__ img, uint8_t *__restrict__ out, const Coef m,
                                                               int rgb_in, size_t quads, int H, int W) {
    const int h2 = H / 2, w2 = W / 2;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < quads; t += (size_t)gridDim.x * blockDim.x) {
        const size_t n = t / ((size_t)h2 * w2), i = t - n * ((size_t)h2 * w2);
        const int j = (int)(i / w2), q = (int)(i % w2);
        uint8_t *dst = out + n * ((size_t)(H + h2) * W);
        unsigned sr = 0, sg = 0, sb = 0;
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const uint8_t *px = img + (((size_t)n * H + 2 * j + p) * W + 2 * q + c) * 3;
                const unsigned r = px[rgb_in ? 0 : 2], g = px[1], b = px[rgb_in ? 2 : 0];
                dst[(size_t)(2 * j + p) * W + 2 * q + c] = (uint8_t)nv12_dot(m.k, r, g, b);
                sr += r, sg += g, sb += b;
            }
        const unsigned uv = nv12_uv(m, sr, sg, sb);
        dst[(size_t)(H + j) * W + 2 * q] = (uint8_t)(uv & 255u);
        dst[(size_t)(H + j) * W + 2 * q + 1] = (uint8_t)(uv >> 8);
    }
}

}  // namespace

extern "C" int risp_bgr8_to_nv12(const uint8_t *img, uint8_t *nv12, const int32_t coef[12], int rgb_in, int N, int H, int W,
                                 void *stream) {
    const char *name = "risp_bgr8_to_nv12";
    RISP_CHECK_ARG(img && nv12, "%s: null argument", name);
    RISP_CHECK_ARG(N >= 1 && H >= 2 && H % 2 == 0 && W >= 2 && W % 2 == 0, "%s: bad shape N=%d H=%d W=%d (H and W even)", name, N, H, W);
    Coef m;
    if (int err = nv12_check(name, coef, m)) return err;
    hipStream_t s = (hipStream_t)stream;
    const int rgb = rgb_in ? 1 : 0;
    if (W % 4 == 0 && reinterpret_cast<uintptr_t>(img) % 4 == 0 && reinterpret_cast<uintptr_t>(nv12) % 4 == 0) {
        const size_t patches = (size_t)N * (H / 2) * (W / 4), blocks = (patches + 255) / 256;
        hipLaunchKernelGGL(bgr8_to_nv12_vec_kernel, dim3((unsigned)(blocks > 65536 ? 65536 : blocks)), dim3(256), 0, s, img, nv12, m, rgb,
                           patches, H, W / 4);
    } else {
        const size_t quads = (size_t)N * (H / 2) * (W / 2), blocks = (quads + 255) / 256;
        hipLaunchKernelGGL(bgr8_to_nv12_any_kernel, dim3((unsigned)(blocks > 65536 ? 65536 : blocks)), dim3(256), 0, s, img, nv12, m, rgb,
                           quads, H, W);
    }
    RISP_LAUNCH_CHECK(name);
    return 0;
}
