// DemosaicNet (demosaic index 04, tools_origin.py:289-308): the parts of the Gharbi et al. 2016 Bayer network that no
// convolution kernel of the library serves.  Build-defined OPSPEC: DESIGN.md section 2, include/risp.h "DemosaicNet", restated in
// float64 in tests/demosaicnet_reference.py.  The half-resolution body (pack_mosaic folded into conv1, conv2..15) runs on the
// convolution kernels (convnets.py); these four launches are the tail (gate, 1x1 64 -> 12, grouped 2x2 transposed conv) and the
// full-resolution head (3x3 6 -> 64, ReLU, 1x1 64 -> 3), forward and backward.
//
// All four are deterministic: no atomics, every sum in a fixed order, no dependence on the batch position.  A head thread owns
// a 2x2 quad of pixels: H and W are even, so the quad holds one site of each CFA phase and the masked-mosaic channel of every
// tap is a compile-time constant - the weights are wave-uniform (scalar loads) and the masked mosaic is never formed.
#include "risp_common.h"

namespace {

constexpr int QT = 16;              // head tile: 16 x 16 quads = 32 x 32 pixels, one quad per thread of a 256-thread block
constexpr int TP = 2 * QT;          // tile side in pixels
constexpr int FI = TP + 2;          // forward: staged side (1-pixel halo)
constexpr int RQ = QT + 2;          // backward: quads per side of the region where g_h is formed (tile + 2-pixel halo)
constexpr int RG = 2 * RQ;          // ... its side in pixels
constexpr int BI = RG + 2;          // backward: staged input side (region + 1-pixel halo)
constexpr int HC = 8;               // backward: hidden channels per LDS chunk
constexpr int HID = 64;

// RGGB: channel (0 R, 1 G, 2 B) of the site with row parity a and column parity b
__device__ __forceinline__ constexpr int cfa(int a, int b) { return a + b; }

// stage `planes` (N, ., H, W) planes of one image into an lds[planes][side][side] window whose origin is pixel (oy, ox); zero
// outside the image (the convolution's zero padding)
__device__ __forceinline__ void stage(float *lds, const float *x, const float *up, int side, int oy, int ox, int H, int W) {
    const size_t hw = (size_t)H * W;
    const int per = side * side;
    for (int i = threadIdx.x; i < 4 * per; i += blockDim.x) {
        const int p = i / per, r = (i - p * per) / side, c = i - p * per - r * side;
        const int gy = oy + r, gx = ox + c;
        float v = 0.f;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = p == 0 ? x[(size_t)gy * W + gx] : up[(p - 1) * hw + (size_t)gy * W + gx];
        lds[i] = v;
    }
}

// pre-activation of hidden channel h at the four pixels of a quad: win[p][4][4] = planes (mosaic, up R, G, B) around the quad
// (origin one pixel up-left of its first pixel).  Sum order: bias, mosaic taps (ky, kx), up channels (c, ky, kx).
__device__ __forceinline__ void hidden_quad(const float (&win)[4][4][4], const float *__restrict__ wp, float b, float (&acc)[4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int qy = q >> 1, qx = q & 1;
        float a = b;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx)
                a = __builtin_fmaf(wp[cfa((qy + ky + 1) & 1, (qx + kx + 1) & 1) * 9 + ky * 3 + kx], win[0][qy + ky][qx + kx], a);
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) a = __builtin_fmaf(wp[(3 + c) * 9 + ky * 3 + kx], win[1 + c][qy + ky][qx + kx], a);
        acc[q] = a;
    }
}

struct TailArgs {
    const float *filt, *mask, *w_rp, *b_rp, *w_up, *b_up, *g_up;
    float *up, *g_filt, *g_mask;
    int h2, w2, W;                  // half-resolution plane, full-resolution width
};

// one thread per half-resolution pixel: r = b_rp + W_rp (filt * mask) (k ascending), then the 2x2 block of each output channel
// c = b_up[c] + sum_j W_up[4c + j][dy][dx] r[4c + j] (j ascending)
__global__ __launch_bounds__(256) void dmnet_tail_fwd_kernel(TailArgs a) {
    const int hw = a.h2 * a.w2;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= hw) return;
    const size_t n = blockIdx.y;
    const float *f = a.filt + n * HID * hw + p, *m = a.mask + n * HID * hw + p;
    float r[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) r[j] = a.b_rp[j];
    for (int k = 0; k < HID; ++k) {
        const float g = f[(size_t)k * hw] * m[(size_t)k * hw];
#pragma unroll
        for (int j = 0; j < 12; ++j) r[j] = __builtin_fmaf(a.w_rp[j * HID + k], g, r[j]);
    }
    const int y = p / a.w2, x = p - y * a.w2;
    const size_t H = 2 * (size_t)a.h2, plane = H * a.W;
    float *o = a.up + n * 3 * plane + (size_t)(2 * y) * a.W + 2 * x;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            float v[2];
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                float s = a.b_up[c];
#pragma unroll
                for (int j = 0; j < 4; ++j) s = __builtin_fmaf(a.w_up[(4 * c + j) * 4 + dy * 2 + dx], r[4 * c + j], s);
                v[dx] = s;
            }
            *reinterpret_cast<float2 *>(o + c * plane + dy * a.W) = make_float2(v[0], v[1]);
        }
}

// g_r[4c + j] = sum_{dy,dx} W_up[4c + j][dy][dx] g_up[c](2y + dy, 2x + dx); g_prod[k] = sum_j W_rp[j][k] g_r[j]; the two halves
// of conv15's pre-activation: g_filt = g_prod * mask * [filt > 0], g_mask = g_prod * filt * [mask > 0]
__global__ __launch_bounds__(256) void dmnet_tail_bwd_kernel(TailArgs a) {
    const int hw = a.h2 * a.w2;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= hw) return;
    const size_t n = blockIdx.y;
    const int y = p / a.w2, x = p - y * a.w2;
    const size_t H = 2 * (size_t)a.h2, plane = H * a.W;
    const float *gu = a.g_up + n * 3 * plane + (size_t)(2 * y) * a.W + 2 * x;
    float gr[12];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float2 t = *reinterpret_cast<const float2 *>(gu + c * plane);
        const float2 b = *reinterpret_cast<const float2 *>(gu + c * plane + a.W);
        const float g4[4] = {t.x, t.y, b.x, b.y};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float s = 0.f;
#pragma unroll
            for (int t4 = 0; t4 < 4; ++t4) s = __builtin_fmaf(a.w_up[(4 * c + j) * 4 + t4], g4[t4], s);
            gr[4 * c + j] = s;
        }
    }
    const size_t off = n * HID * hw + p;
    for (int k = 0; k < HID; ++k) {
        float g = 0.f;
#pragma unroll
        for (int j = 0; j < 12; ++j) g = __builtin_fmaf(a.w_rp[j * HID + k], gr[j], g);
        const size_t i = off + (size_t)k * hw;
        const float fv = a.filt[i], mv = a.mask[i];
        a.g_filt[i] = fv > 0.f ? g * mv : 0.f;
        a.g_mask[i] = mv > 0.f ? g * fv : 0.f;
    }
}

struct HeadArgs {
    const float *x, *up, *w_post, *b_post, *w_out, *b_out, *g_y, *add;
    float *y, *g_up, *g_x;
    int H, W;
};

// forward: y = W_out relu(post_conv(cat(m3, up))) + b_out, the 64 hidden values of a pixel in registers only
__global__ __launch_bounds__(256) void dmnet_head_fwd_kernel(HeadArgs a) {
    __shared__ float lds[4 * FI * FI];
    const int H = a.H, W = a.W;
    const size_t n = blockIdx.z, hw = (size_t)H * W;
    const int y0 = blockIdx.y * TP, x0 = blockIdx.x * TP;
    stage(lds, a.x + n * hw, a.up + n * 3 * hw, FI, y0 - 1, x0 - 1, H, W);
    __syncthreads();
    const int tx = threadIdx.x % QT, ty = threadIdx.x / QT;
    const int py = y0 + 2 * ty, px = x0 + 2 * tx;
    if (py >= H || px >= W) return;                 // H, W even: a quad is inside or outside as a whole
    float win[4][4][4];
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) win[p][r][c] = lds[(p * FI + 2 * ty + r) * FI + 2 * tx + c];
    float out[3][4];
#pragma unroll
    for (int o = 0; o < 3; ++o)
#pragma unroll
        for (int q = 0; q < 4; ++q) out[o][q] = a.b_out[o];
    for (int h = 0; h < HID; ++h) {
        float acc[4];
        hidden_quad(win, a.w_post + h * 54, a.b_post[h], acc);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float v = fmaxf(acc[q], 0.f);
#pragma unroll
            for (int o = 0; o < 3; ++o) out[o][q] = __builtin_fmaf(a.w_out[o * HID + h], v, out[o][q]);
        }
    }
    float *yo = a.y + n * 3 * hw + (size_t)py * W + px;
#pragma unroll
    for (int o = 0; o < 3; ++o) {
        *reinterpret_cast<float2 *>(yo + o * hw) = make_float2(out[o][0], out[o][1]);
        *reinterpret_cast<float2 *>(yo + o * hw + W) = make_float2(out[o][2], out[o][3]);
    }
}

// backward: g_h = (W_out^T g_y) * [h > 0] is recomputed on the tile plus a halo, HC hidden channels at a time in LDS; then
// g_in[c](p) = sum_{h,ky,kx} W_post[h][c][ky][kx] g_h[h](p - (ky - 1, kx - 1)) for the three up channels and for the mosaic
// channel of p's own site (h ascending, taps (ky, kx)); g_x = add + that mosaic term
__global__ __launch_bounds__(256) void dmnet_head_bwd_kernel(HeadArgs a) {
    __shared__ float lin[4 * BI * BI];
    __shared__ float lgh[HC * RG * RG];
    const int H = a.H, W = a.W;
    const size_t n = blockIdx.z, hw = (size_t)H * W;
    const int y0 = blockIdx.y * TP, x0 = blockIdx.x * TP;
    stage(lin, a.x + n * hw, a.up + n * 3 * hw, BI, y0 - 3, x0 - 3, H, W);
    // the region quads of this thread (324 = 256 + 68): their g_y, zero outside the image (then g_h is zero there too)
    const float *gy = a.g_y + n * 3 * hw;
    float gyq[2][3][4];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int q = threadIdx.x + 256 * s;
        const int ry = q / RQ, rx = q - ry * RQ;
        const int gy0 = y0 - 2 + 2 * ry, gx0 = x0 - 2 + 2 * rx;
        const bool in = q < RQ * RQ && gy0 >= 0 && gy0 < H && gx0 >= 0 && gx0 < W;
#pragma unroll
        for (int o = 0; o < 3; ++o)
#pragma unroll
            for (int k = 0; k < 4; ++k)
                gyq[s][o][k] = in ? gy[o * hw + (size_t)(gy0 + (k >> 1)) * W + gx0 + (k & 1)] : 0.f;
    }
    const int tx = threadIdx.x % QT, ty = threadIdx.x / QT;
    float gu[3][4], gd[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        gd[q] = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) gu[c][q] = 0.f;
    }
    for (int h0 = 0; h0 < HID; h0 += HC) {
        __syncthreads();                            // staging done / the previous chunk consumed
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int q = threadIdx.x + 256 * s;
            if (q >= RQ * RQ) continue;
            const int ry = q / RQ, rx = q - ry * RQ;
            float win[4][4][4];
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int c = 0; c < 4; ++c) win[p][r][c] = lin[(p * BI + 2 * ry + r) * BI + 2 * rx + c];
            for (int hh = 0; hh < HC; ++hh) {
                const int h = h0 + hh;
                float acc[4];
                hidden_quad(win, a.w_post + h * 54, a.b_post[h], acc);
                const float w0 = a.w_out[h], w1 = a.w_out[HID + h], w2 = a.w_out[2 * HID + h];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float g = w0 * gyq[s][0][k];
                    g = __builtin_fmaf(w1, gyq[s][1][k], g);
                    g = __builtin_fmaf(w2, gyq[s][2][k], g);
                    lgh[(hh * RG + 2 * ry + (k >> 1)) * RG + 2 * rx + (k & 1)] = acc[k] > 0.f ? g : 0.f;
                }
            }
        }
        __syncthreads();
        for (int hh = 0; hh < HC; ++hh) {
            const int h = h0 + hh;
            float gw[4][4];                         // g_h around the quad: rows / columns -1 .. 2 of it
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) gw[r][c] = lgh[(hh * RG + 2 * ty + 1 + r) * RG + 2 * tx + 1 + c];
            const float *wp = a.w_post + h * 54;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int qy = q >> 1, qx = q & 1;
#pragma unroll
                for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx) {
                        const float g = gw[qy - ky + 2][qx - kx + 2];
                        gd[q] = __builtin_fmaf(wp[cfa(qy, qx) * 9 + ky * 3 + kx], g, gd[q]);
#pragma unroll
                        for (int c = 0; c < 3; ++c) gu[c][q] = __builtin_fmaf(wp[(3 + c) * 9 + ky * 3 + kx], g, gu[c][q]);
                    }
            }
        }
    }
    const int py = y0 + 2 * ty, px = x0 + 2 * tx;
    if (py >= H || px >= W) return;
    const size_t o = (size_t)py * W + px;
    float *gup = a.g_up + n * 3 * hw + o;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        *reinterpret_cast<float2 *>(gup + c * hw) = make_float2(gu[c][0], gu[c][1]);
        *reinterpret_cast<float2 *>(gup + c * hw + W) = make_float2(gu[c][2], gu[c][3]);
    }
    float d[4] = {gd[0], gd[1], gd[2], gd[3]};
    if (a.add) {
        const float *ad = a.add + n * hw + o;
        const float2 t = *reinterpret_cast<const float2 *>(ad), b = *reinterpret_cast<const float2 *>(ad + W);
        d[0] = t.x + gd[0]; d[1] = t.y + gd[1]; d[2] = b.x + gd[2]; d[3] = b.y + gd[3];
    }
    float *gx = a.g_x + n * hw + o;
    *reinterpret_cast<float2 *>(gx) = make_float2(d[0], d[1]);
    *reinterpret_cast<float2 *>(gx + W) = make_float2(d[2], d[3]);
}

// the limits of include/risp.h: 1 <= N <= 65535, H and W even and >= 4, a full-resolution plane below 2^31 bytes
bool dims_ok(int N, int H, int W) {
    return N > 0 && N <= 65535 && H >= 4 && W >= 4 && H % 2 == 0 && W % 2 == 0 && (long long)H * W * 4 < (1ll << 31);
}

bool aligned8(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

}  // namespace

extern "C" {

int risp_dmnet_tail_fwd(const float *filt, const float *mask, const float *w_rp, const float *b_rp, const float *w_up,
                        const float *b_up, float *up, int N, int H, int W, void *stream) {
    RISP_CHECK_ARG(filt && mask && w_rp && b_rp && w_up && b_up && up && dims_ok(N, H, W) && aligned8(up),
                   "risp_dmnet_tail_fwd: bad arguments (N=%d H=%d W=%d)", N, H, W);
    TailArgs a{};
    a.filt = filt; a.mask = mask; a.w_rp = w_rp; a.b_rp = b_rp; a.w_up = w_up; a.b_up = b_up; a.up = up;
    a.h2 = H / 2; a.w2 = W / 2; a.W = W;
    hipLaunchKernelGGL(dmnet_tail_fwd_kernel, dim3((a.h2 * a.w2 + 255) / 256, N), dim3(256), 0, (hipStream_t)stream, a);
    RISP_LAUNCH_CHECK("risp_dmnet_tail_fwd");
    return 0;
}

int risp_dmnet_tail_bwd(const float *g_up, const float *filt, const float *mask, const float *w_rp, const float *w_up,
                        float *g_filt, float *g_mask, int N, int H, int W, void *stream) {
    RISP_CHECK_ARG(g_up && filt && mask && w_rp && w_up && g_filt && g_mask && dims_ok(N, H, W) && aligned8(g_up),
                   "risp_dmnet_tail_bwd: bad arguments (N=%d H=%d W=%d)", N, H, W);
    TailArgs a{};
    a.g_up = g_up; a.filt = filt; a.mask = mask; a.w_rp = w_rp; a.w_up = w_up; a.g_filt = g_filt; a.g_mask = g_mask;
    a.h2 = H / 2; a.w2 = W / 2; a.W = W;
    hipLaunchKernelGGL(dmnet_tail_bwd_kernel, dim3((a.h2 * a.w2 + 255) / 256, N), dim3(256), 0, (hipStream_t)stream, a);
    RISP_LAUNCH_CHECK("risp_dmnet_tail_bwd");
    return 0;
}

int risp_dmnet_head_fwd(const float *x, const float *up, const float *w_post, const float *b_post, const float *w_out,
                        const float *b_out, float *y, int N, int H, int W, void *stream) {
    RISP_CHECK_ARG(x && up && w_post && b_post && w_out && b_out && y && dims_ok(N, H, W) && aligned8(y),
                   "risp_dmnet_head_fwd: bad arguments (N=%d H=%d W=%d)", N, H, W);
    HeadArgs a{};
    a.x = x; a.up = up; a.w_post = w_post; a.b_post = b_post; a.w_out = w_out; a.b_out = b_out; a.y = y; a.H = H; a.W = W;
    hipLaunchKernelGGL(dmnet_head_fwd_kernel, dim3((W + TP - 1) / TP, (H + TP - 1) / TP, N), dim3(256), 0, (hipStream_t)stream, a);
    RISP_LAUNCH_CHECK("risp_dmnet_head_fwd");
    return 0;
}

int risp_dmnet_head_bwd(const float *g_y, const float *x, const float *up, const float *w_post, const float *b_post,
                        const float *w_out, const float *add, float *g_up, float *g_x, int N, int H, int W, void *stream) {
    RISP_CHECK_ARG(g_y && x && up && w_post && b_post && w_out && g_up && g_x && dims_ok(N, H, W) && aligned8(g_up) &&
                       aligned8(g_x) && (!add || aligned8(add)),
                   "risp_dmnet_head_bwd: bad arguments (N=%d H=%d W=%d)", N, H, W);
    HeadArgs a{};
    a.g_y = g_y; a.x = x; a.up = up; a.w_post = w_post; a.b_post = b_post; a.w_out = w_out; a.add = add;
    a.g_up = g_up; a.g_x = g_x; a.H = H; a.W = W;
    hipLaunchKernelGGL(dmnet_head_bwd_kernel, dim3((W + TP - 1) / TP, (H + TP - 1) / TP, N), dim3(256), 0, (hipStream_t)stream, a);
    RISP_LAUNCH_CHECK("risp_dmnet_head_bwd");
    return 0;
}

}  // extern "C"
