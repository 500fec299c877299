// Overlapped tiling of a full frame (utils/util_path_restore.py:47-134) on the device.
// gather = whole2patch's crop; blend = patch2whole with the linear edge-ramp mask and the
// count-map normalisation, evaluated per output pixel in tile order (same fp32 operation
// order as the reference's sequential "+=" loop).
#include "risp_common.h"

namespace {

__device__ __forceinline__ float ramp(int i, int size, int e) {
    // create_patch_mask (:56-63): (i+1)/(e+1) on the first e and (size-i)/(e+1) on the last e entries
    if (i < e) return (float)(i + 1) / (float)(e + 1);
    if (i >= size - e) return (float)(size - i) / (float)(e + 1);
    return 1.f;
}

__global__ __launch_bounds__(256) void tile_gather_kernel(const float *__restrict__ img, float *__restrict__ patches,
                                                          const int32_t *__restrict__ pos, int C, int H, int W, int h,
                                                          int w) {
    const int t = blockIdx.z, c = blockIdx.y;
    const int py = pos[2 * t], px = pos[2 * t + 1];
    const float *src = img + (size_t)c * H * W;
    float *dst = patches + ((size_t)t * C + c) * h * w;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < h * w; i += gridDim.x * blockDim.x) {
        const int y = i / w, x = i - y * w;
        dst[i] = src[(size_t)(py + y) * W + px + x];
    }
}

// One workgroup = 256 pixels of BLEND_ROWS image rows.  The tiles that reach into that block are listed first (in tile order, by the whole
// workgroup: a ballot per 64 tiles; index and corner in LDS) - a pixel then walks that list instead of all T tiles (63 tiles of a
// 4000 x 3000 frame: 1-6 reach a block): same adds in the same order, 396 -> ~1/3 of the time per frame.
constexpr int BLEND_ROWS = 4;
__global__ __launch_bounds__(256) void tile_blend_kernel(const float *__restrict__ patches, float *__restrict__ img,
                                                         const int32_t *__restrict__ pos, int T, int C, int H, int W,
                                                         int h, int w, int eh, int ew) {
    constexpr int LIST = 256;                          // listed tiles kept in LDS; a longer list falls back to the full walk
    __shared__ int list[LIST], list_y[LIST], list_x[LIST];
    __shared__ int wave_n[4];
    const int X0 = blockIdx.x * blockDim.x, X = X0 + threadIdx.x, Y0 = blockIdx.y * BLEND_ROWS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int n_list = 0;
    bool listed = true;
    for (int t0 = 0; t0 < T && listed; t0 += 256) {     // (uniform: every thread sees the same counts)
        const int t = t0 + threadIdx.x;
        bool in = false;
        int ty = 0, tx = 0;
        if (t < T) {
            ty = pos[2 * t];
            tx = pos[2 * t + 1];
            in = Y0 + BLEND_ROWS - 1 >= ty && Y0 < ty + h && X0 + 255 >= tx && X0 < tx + w;
        }
        const unsigned long long m = __ballot(in);
        if (lane == 0) wave_n[wave] = __popcll(m);
        __syncthreads();
        int before = n_list;
        for (int k = 0; k < wave; ++k) before += wave_n[k];
        const int all = n_list + wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
        if (all > LIST) {
            listed = false;
        } else if (in) {
            const int at = before + __popcll(m & ((1ull << lane) - 1ull));
            list[at] = t;
            list_y[at] = ty;
            list_x[at] = tx;
        }
        n_list = all;
        __syncthreads();
    }
    if (X >= W) return;
    const int n = listed ? n_list : T;
    for (int Y = Y0; Y < Y0 + BLEND_ROWS && Y < H; ++Y) {
        float cnt = 0.f;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int i = 0; i < n; ++i) {
            const int t = listed ? list[i] : i;
            const int y = Y - (listed ? list_y[i] : pos[2 * t]), x = X - (listed ? list_x[i] : pos[2 * t + 1]);
            if (y < 0 || y >= h || x < 0 || x >= w) continue;
            const float m = fminf(ramp(y, h, eh), ramp(x, w, ew));
            cnt += m;
            const float *p = patches + ((size_t)t * C) * h * w + (size_t)y * w + x;
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (c < C) acc[c] += p[(size_t)c * h * w] * m;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (c < C) img[((size_t)c * H + Y) * W + X] = acc[c] / cnt;
    }
}

// ---------------------------------------------------------------- blend straight into packed bytes (risp_tile_blend_u8)
// tile_blend_kernel's sum followed by risp_quantise_u8[_flip]'s conversion, the fp32 frame never written.  The workgroup covers the
// same 4 rows x 256 pixels and lists its tiles the same way; a wave is one row of it and a thread owns FOUR adjacent pixels of that
// row: per listed tile one 16-byte load per channel (a wave reads 1 KiB of a tile row), and the 12 bytes of the four pixels leave as
// three dwords (a wave writes 768 contiguous bytes - the store of risp_serve.hip).  Per pixel and channel the expressions are
// tile_blend_kernel's in its order (m = min(ramp_y, ramp_x), cnt += m, acc += p * m, acc / cnt), then clip(v * 255) truncated: built
// with -ffp-contract=off the bytes are those of the two launches.

// clip(v * 255, 0, 255).astype(uint8): risp_serve.hip's u8(), the product in fp32, the conversion truncates
__device__ __forceinline__ unsigned blend_u8(float v) {
    float t = v * 255.f;
    t = t < 0.f ? 0.f : (t > 255.f ? 255.f : t);
    return (unsigned)(int)t;
}

// VEC: W % 4 == 0, w % 4 == 0, patches 16-byte and out 4-byte aligned (the host's part of the rule).  A tile whose x origin is a
// multiple of 4 then holds a thread's four pixels or none of them, at a 16-byte aligned address; any other tile - the origins live
// on the device, so the kernel looks, and the answer is the same for the whole workgroup - is read float by float.  !VEC: every
// geometry and alignment, floats read and bytes stored one at a time; same adds, same bytes.
// Coordinates are those of the blended image; only the store knows about the mirror: output pixel (Yo, Xo) = blended
// (fy ? H-1-Yo : Yo, fx ? W-1-Xo : Xo), so the four pixels X .. X+3 land at W-4-X in reverse order, still four pixels of one row.
template <int C, bool VEC>
__global__ __launch_bounds__(256) void tile_blend_u8_kernel(const float *__restrict__ patches, uint8_t *__restrict__ out,
                                                            const int32_t *__restrict__ pos, int T, int H, int W, int h, int w,
                                                            int eh, int ew, int reverse, int fx, int fy) {
    constexpr int LIST = 256;                          // as in tile_blend_kernel: a longer list falls back to the full walk
    __shared__ int list[LIST], list_y[LIST], list_x[LIST];
    __shared__ int wave_n[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int X0 = blockIdx.x * 256, Y0 = blockIdx.y * BLEND_ROWS;
    int n_list = 0;
    bool listed = true;
    for (int t0 = 0; t0 < T && listed; t0 += 256) {     // (uniform: every thread sees the same counts)
        const int t = t0 + threadIdx.x;
        bool in = false;
        int ty = 0, tx = 0;
        if (t < T) {
            ty = pos[2 * t];
            tx = pos[2 * t + 1];
            in = Y0 + BLEND_ROWS - 1 >= ty && Y0 < ty + h && X0 + 255 >= tx && X0 < tx + w;
        }
        const unsigned long long m = __ballot(in);
        if (lane == 0) wave_n[wave] = __popcll(m);
        __syncthreads();
        int before = n_list;
        for (int k = 0; k < wave; ++k) before += wave_n[k];
        const int all = n_list + wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
        if (all > LIST) {
            listed = false;
        } else if (in) {
            const int at = before + __popcll(m & ((1ull << lane) - 1ull));
            list[at] = t;
            list_y[at] = ty;
            list_x[at] = tx;
        }
        n_list = all;
        __syncthreads();
    }
    const int X = X0 + 4 * lane, Y = Y0 + wave;         // a wave is one row: everything that depends on Y alone is wave-uniform
    if (X >= W || Y >= H) return;
    const size_t plane = (size_t)h * w;
    float cnt[4] = {0.f, 0.f, 0.f, 0.f};
    float acc[C][4];
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[c][k] = 0.f;
    const int n = listed ? n_list : T;
    for (int i = 0; i < n; ++i) {
        const int t = listed ? list[i] : i;
        const int ty = listed ? list_y[i] : pos[2 * t], tx = listed ? list_x[i] : pos[2 * t + 1];
        const int y = Y - ty, x0 = X - tx;
        if (y < 0 || y >= h) continue;
        const float my = ramp(y, h, eh);
        const float *p = patches + (size_t)t * C * plane + (size_t)y * w;
        if (VEC && (tx & 3) == 0) {
            if (x0 < 0 || x0 >= w) continue;            // x0 % 4 == 0 and w % 4 == 0: four pixels of the tile or none
            float4 v[C];
#pragma unroll
            for (int c = 0; c < C; ++c) v[c] = *reinterpret_cast<const float4 *>(p + c * plane + x0);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float m = fminf(my, ramp(x0 + k, w, ew));
                cnt[k] += m;
#pragma unroll
                for (int c = 0; c < C; ++c) acc[c][k] += (k == 0 ? v[c].x : k == 1 ? v[c].y : k == 2 ? v[c].z : v[c].w) * m;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int x = x0 + k;
                if (x < 0 || x >= w) continue;          // (a pixel past W lies in no tile: tx + w <= W)
                const float m = fminf(my, ramp(x, w, ew));
                cnt[k] += m;
#pragma unroll
                for (int c = 0; c < C; ++c) acc[c][k] += p[c * plane + x] * m;
            }
        }
    }
    const int Yo = fy ? H - 1 - Y : Y;
    if (VEC) {
        unsigned q[C][4];                               // the bytes of the blended pixels X .. X+3, by blended channel
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
            for (int k = 0; k < 4; ++k) q[c][k] = blend_u8(acc[c][k] / cnt[k]);
        unsigned b[4][C];                               // byte c of output pixel j (value selects, not address selects)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const unsigned fwd = fx ? q[c][3 - j] : q[c][j], rev = fx ? q[C - 1 - c][3 - j] : q[C - 1 - c][j];
                b[j][c] = reverse ? rev : fwd;
            }
        unsigned *dst = reinterpret_cast<unsigned *>(out + ((size_t)Yo * W + (fx ? W - 4 - X : X)) * C);
        if (C == 1) {
            dst[0] = b[0][0] | b[1][0] << 8 | b[2][0] << 16 | b[3][0] << 24;
        } else {
            dst[0] = b[0][0] | b[0][1] << 8 | b[0][C - 1] << 16 | b[1][0] << 24;
            dst[1] = b[1][1] | b[1][C - 1] << 8 | b[2][0] << 16 | b[2][1] << 24;
            dst[2] = b[2][C - 1] | b[3][0] << 8 | b[3][1] << 16 | b[3][C - 1] << 24;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (X + k >= W) continue;
            uint8_t *dst = out + ((size_t)Yo * W + (fx ? W - 1 - X - k : X + k)) * C;
#pragma unroll
            for (int c = 0; c < C; ++c) dst[c] = (uint8_t)blend_u8((reverse ? acc[C - 1 - c][k] : acc[c][k]) / cnt[k]);
        }
    }
}

}  // namespace

extern "C" {

int risp_tile_gather(const float *img, float *patches, const int32_t *pos_dev, int T, int C, int H, int W, int h, int w,
                     void *stream) {
    RISP_CHECK_ARG(img && patches && pos_dev && T > 0 && T <= 65535 && C > 0 && C <= 65535 && h > 0 && w > 0 && h <= H && w <= W,
                   "risp_tile_gather: bad arguments");
    int bx = (h * w + 255) / 256;
    if (bx > 256) bx = 256;
    hipLaunchKernelGGL(tile_gather_kernel, dim3(bx, C, T), dim3(256), 0, (hipStream_t)stream, img, patches, pos_dev, C, H,
                       W, h, w);
    RISP_LAUNCH_CHECK("risp_tile_gather");
    return 0;
}

int risp_tile_blend(const float *patches, float *img, const int32_t *pos_dev, int T, int C, int H, int W, int h, int w,
                    int eh, int ew, void *stream) {
    RISP_CHECK_ARG(patches && img && pos_dev && T > 0 && C > 0 && C <= 4 && h > 0 && w > 0 && h <= H && w <= W && H <= 65535,
                   "risp_tile_blend: bad arguments (C must be <= 4)");
    RISP_CHECK_ARG(eh >= 0 && ew >= 0 && eh <= h / 2 && ew <= w / 2, "risp_tile_blend: edge larger than half a tile");
    hipLaunchKernelGGL(tile_blend_kernel, dim3((W + 255) / 256, (H + BLEND_ROWS - 1) / BLEND_ROWS), dim3(256), 0, (hipStream_t)stream, patches, img,
                       pos_dev, T, C, H, W, h, w, eh, ew);
    RISP_LAUNCH_CHECK("risp_tile_blend");
    return 0;
}

int risp_tile_blend_u8(const float *patches, uint8_t *out, const int32_t *pos_dev, int T, int C, int H, int W, int h, int w,
                       int eh, int ew, int reverse_channels, int flip, void *stream) {
    RISP_CHECK_ARG(patches && out && pos_dev, "risp_tile_blend_u8: null argument (patches %p, out %p, pos_dev %p)", (const void *)patches,
                   (const void *)out, (const void *)pos_dev);
    RISP_CHECK_ARG(T >= 1 && T <= 65535, "risp_tile_blend_u8: T %d outside 1 .. 65535", T);
    RISP_CHECK_ARG(C == 1 || C == 3, "risp_tile_blend_u8: C %d (1 or 3)", C);
    RISP_CHECK_ARG(H >= 1 && H <= 65535 && W >= 1, "risp_tile_blend_u8: frame H=%d W=%d (1 <= H <= 65535, W >= 1)", H, W);
    RISP_CHECK_ARG(h >= 1 && w >= 1 && h <= H && w <= W, "risp_tile_blend_u8: tile h=%d w=%d does not fit the frame H=%d W=%d", h, w, H,
                   W);
    RISP_CHECK_ARG(eh >= 0 && ew >= 0 && eh <= h / 2 && ew <= w / 2,
                   "risp_tile_blend_u8: edge eh=%d ew=%d larger than half a tile (h=%d w=%d)", eh, ew, h, w);
    RISP_CHECK_ARG(flip >= 0 && flip <= 3, "risp_tile_blend_u8: flip %d (bit 0 mirrors x, bit 1 mirrors y)", flip);
    const dim3 grid((W + 255) / 256, (H + BLEND_ROWS - 1) / BLEND_ROWS);
    hipStream_t s = (hipStream_t)stream;
    const int rev = reverse_channels ? 1 : 0, fx = flip & 1, fy = flip >> 1;
    const bool vec = W % 4 == 0 && w % 4 == 0 && reinterpret_cast<uintptr_t>(patches) % 16 == 0 && reinterpret_cast<uintptr_t>(out) % 4 == 0;
#define RISP_BLEND_U8(CH, V) \
    hipLaunchKernelGGL((tile_blend_u8_kernel<CH, V>), grid, dim3(256), 0, s, patches, out, pos_dev, T, H, W, h, w, eh, ew, rev, fx, fy)
    if (C == 1) {
        if (vec) RISP_BLEND_U8(1, true);
        else RISP_BLEND_U8(1, false);
    } else {
        if (vec) RISP_BLEND_U8(3, true);
        else RISP_BLEND_U8(3, false);
    }
#undef RISP_BLEND_U8
    RISP_LAUNCH_CHECK("risp_tile_blend_u8");
    return 0;
}

}  // extern "C"
