// Serving path for the classical pipelines that hold ONE classical denoiser AND one or two automatic white balances
// (gray-world, white-world): the two launches that risp_serve_denoise.hip and risp_serve_scene.hip leave open between them.
//
//     risp_serve_denoise_stats      risp_serve_denoise_u8's tile pipeline through the denoiser and the Q stages behind it, reduced
//                                   per workgroup (sums or maxima of B, G, R) into the partial rows risp_serve_scene_finish takes:
//                                   the statistic of an image that lies BEHIND a denoiser
//     risp_serve_denoise_scene_u8   risp_serve_denoise_u8 with RISP_OP_GAIN3_Q8 (white-world's apply step) accepted among the
//                                   stages on either side of the denoiser; gray-world applies as RISP_OP_GAIN3
//
// A statistic in front of the denoiser needs no tile: risp_serve_scene_stats takes that prefix as it is.  Behind the denoiser a
// stencil needs finished neighbours, so the statistic takes the tile form: a workgroup owns a 64 x 32 pixel tile and works in two
// phases around one LDS image of 36 x 72 pixels (the tile and a ring of 2 rows / 4 columns, three fp32 planes, 31104 bytes):
//
//   phase 1  the 18 x 18 patches of 2 x 4 pixels that cover the image - demosaic and the P stages exactly as
//            serve_classical_kernel evaluates a patch - written to LDS in the 0..255 domain (the median stages the 8-bit codes).
//            Patches outside the image are skipped; after a barrier the ring positions outside the image copy the pixel at the
//            reflect-101 IMAGE coordinate from LDS (H >= 4, W >= 4 and a ring of 2: one reflection, and its source lies in the
//            same tile's image).
//   phase 2  after the barrier a thread denoises its own 2 x 4 patch row by row with the expression sequence of
//            bilateral4_kernel<1> / median3x4_kernel / fastnlm4_kernel<true>'s fast branch (risp_origin.hip), emits
//            q8(v) * (1 / 255) and runs the Q stages in registers.  The serving launch stores 12 bytes per row as serve_kernel
//            does.  The statistics launch stores no image: the thread's eight pixels are accumulated in row order, then
//            block_reduce3 of risp_serve_scene.hip (wavefront shuffles, one LDS step in wave order, no atomics) and one row of
//            four floats per workgroup.  A thread of a ragged tile that owns no pixel holds 0 for a sum and -inf for a maximum.
//
// The tile pipeline restates serve_denoise_kernel (risp_serve_denoise.hip) and the reduction restates risp_serve_scene.hip, as
// those files restated their sources: their instantiations stay as measured.  One kernel template serves both
// launches; STATS is a compile-time switch.  With -ffp-contract=off a pixel's value has the bits of the composed route, so a
// maximum - which has no order - gives the composed route's constants and bytes; a sum taken in this order gives constants
// that differ in their last bits, and given the constants the bytes are the composed route's.  Black level and Bayer phase as
// in risp_serve_u8_cfa: the phase is a mirror of addresses; coordinates, reflection, parity and the tile grid live in the
// mirrored (RGGB) image.
#include <math.h>

#include "risp_common.h"
#include "risp_ops.h"

namespace {

using namespace risp_ops;

// clip(v * 255, 0, 255).astype(uint8): the product in fp32, the conversion truncates (risp_quantise_u8)
__device__ __forceinline__ unsigned u8(float v) {
    float t = v * 255.f;
    t = t < 0.f ? 0.f : (t > 255.f ? 255.f : t);
    return (unsigned)(int)t;
}

// the 8-bit code of a value in the 0..255 domain (risp_origin.hip q8; v is never NaN here)
__device__ __forceinline__ float q8(float v) { return floorf(__builtin_amdgcn_fmed3f(v, 0.f, 255.f) + 0.5f); }

__device__ __forceinline__ float hable(float t) {
    const float A = 0.15f, B = 0.50f, C = 0.10f, D = 0.20f, E = 0.02f, F = 0.30f;
    return (t * (A * t + C * B) + D * E) / (t * (A * t + B) + D * F) - E / F;
}

struct DenoiseSceneArgs {
    const uint16_t *raw;        // (N,H,W) mosaic of the sensor
    uint8_t *out;               // (N,H,W,3); the serving launch
    float *partials;            // (N,G,4); the statistics launch
    float divisor;
    int n_pre, n_ops, N, H, W;  // stages 0 .. n_pre - 1 run in front of the denoiser, n_pre .. n_ops - 1 behind it
    int reverse;                // store R, G, B instead of B, G, R
    int black;                  // subtracted from every sample in integers, clamped at 0
    int flip;                   // RISP_CFA_*: bit 0 mirrors x, bit 1 mirrors y
    int stat;                   // RISP_SCENE_MEAN3 | RISP_SCENE_MAX3; the statistics launch
    const float *da, *db;       // bilateral: sigma_color, sigma_space (N); non-local means: decay (N), -
    int ops[RISP_MAX_CHAIN];
    const float *params[RISP_MAX_CHAIN];
};

// XCD-aware tile order, as in risp_serve.hip: XCD k works through the k-th contiguous eighth of the tile list
__device__ __forceinline__ void xcd_tile(int &bx, int &by, int &bz) {
    bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
    const unsigned total = gridDim.x * gridDim.y * gridDim.z;
    if ((total & 7u) == 0) {
        const unsigned lin = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
        const unsigned t = (lin & 7u) * (total >> 3) + (lin >> 3);
        bx = t % gridDim.x;
        by = (t / gridDim.x) % gridDim.y;
        bz = t / (gridDim.x * gridDim.y);
    }
}

constexpr int STX = 16, STY = 256 / STX, PXT = 4;      // threads across and down a workgroup: a 64 x 32 pixel tile
constexpr int TILE_W = STX * PXT, TILE_H = STY * 2;
constexpr int RING_Y = 2, RING_X = 4;                  // LDS rows above / columns left of the tile (whole patches)
constexpr int LW = TILE_W + 2 * RING_X, LH = TILE_H + 2 * RING_Y, LPLANE = LW * LH;   // 72 x 36 per plane
constexpr int PCOLS = LW / PXT, PROWS = LH / 2;        // 18 x 18 patches
constexpr int REACH = 2;                               // ring positions a denoiser may read (non-local means: 1 + 1)

// a tone curve on NPX pixels: tonemap_kernel's pixel expression with si = so = 255, p0 / p1 as tonemap_prepare_kernel forms them
template <bool FILMIC, int NPX>
__device__ __forceinline__ void tone_all(float p0, float p1, f3 *px) {
    auto curve = [&](float x) {
        float v = x * 255.f / 255.f;
        v = fmaxf(v, 0.f);
        if (FILMIC) v = hable(v * p0) * p1;
        else v = 1.f - __expf(-v * p0);
        return q8(v * 255.f) * (1.f / 255.f);
    };
#pragma unroll
    for (int i = 0; i < NPX; ++i) px[i] = {curve(px[i].b), curve(px[i].g), curve(px[i].r)};
}

// white-world apply on NPX pixels: tonemap_kernel<TM_GAIN>'s pixel expression with si = so = 255, the gains of
// risp_serve_scene_finish (risp_serve_scene.hip gain_q8_all)
template <int NPX>
__device__ __forceinline__ void gain_q8_all(float p0, float p1, float p2, f3 *px) {
#pragma unroll
    for (int i = 0; i < NPX; ++i) {
        float b = px[i].b * 255.f / 255.f, g = px[i].g * 255.f / 255.f, r = px[i].r * 255.f / 255.f;
        b *= p0; g *= p1; r *= p2;
        px[i] = {q8(b * 255.f) * (1.f / 255.f), q8(g * 255.f) * (1.f / 255.f), q8(r * 255.f) * (1.f / 255.f)};
    }
}

// sum or maximum of three values over the workgroup, in a fixed order: wavefront shuffles, then one LDS step in wave order
// (risp_serve_scene.hip block_reduce3).  Thread 0 receives the result.  Contains a barrier: every thread of the workgroup calls it
template <bool MAX>
__device__ __forceinline__ void block_reduce3(float (&v)[3], float *red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        float s = v[i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float t = __shfl_down(s, o, 64);
            s = MAX ? fmaxf(s, t) : s + t;
        }
        if (lane == 0) red[i * 4 + wave] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float *q = red + i * 4;
            v[i] = MAX ? fmaxf(fmaxf(fmaxf(q[0], q[1]), q[2]), q[3]) : ((q[0] + q[1]) + q[2]) + q[3];
        }
    }
}

// stages k0 .. k1 - 1 on NPX pixels in registers: the two tone curves and the white-world apply here (their per-image
// constants are cheap enough to form in every thread; a scene stage's block is the (N,4) constants of
// risp_serve_scene_finish), the rest in risp_ops.h
template <int NPX, bool WBQ>
__device__ __forceinline__ void run_stages(const DenoiseSceneArgs &a, int k0, int k1, int n, f3 *px) {
    for (int k = k0; k < k1; ++k) {
        const int op = a.ops[k];
        const float *p = a.params[k];
        if (op == RISP_OP_TONE_CRYSIS) {               // p (N,1): lum_adapted
            tone_all<false, NPX>(0.5f / (p[n] + 0.05f), 0.f, px);
        } else if (op == RISP_OP_TONE_FILMIC) {        // p (N,2): white_point, exposure_bias
            tone_all<true, NPX>(p[2 * n + 1], 1.f / hable(fmaxf(p[2 * n], 0.01f) * 11.2f), px);
        } else if (op == RISP_OP_GAIN3_Q8) {
            gain_q8_all<NPX>(p[4 * n], p[4 * n + 1], p[4 * n + 2], px);
        } else {
            apply_op<NPX, WBQ>(op, p, n, px);
        }
    }
}

// KIND: RISP_DEMOSAIC_*, DEN: RISP_DENOISE_*.  Every coordinate is one of the mirrored image, which is RGGB; only row_at /
// ld2 / ld4 and the store know where the samples really are.  STATS: no image is stored; the values behind the last stage are
// reduced over the workgroup's tile and one row of four floats goes to partials[(n * G + tile) * 4 ..]
template <int KIND, int DEN, bool WBQ, bool STATS>
__global__ __launch_bounds__(256) void serve_denoise_scene_kernel(const DenoiseSceneArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[3 * LPLANE];
    const int H = a.H, W = a.W;
    int bxi, byi, bzi;
    xcd_tile(bxi, byi, bzi);
    const int n = bzi, x0 = bxi * TILE_W, y0 = byi * TILE_H;
    const uint16_t *bay = a.raw + (size_t)n * H * W;
    const float div = a.divisor;
    const int black = a.black, flip = a.flip;
    auto row_at = [&](int y) { return bay + (size_t)(flip & 2 ? H - 1 - y : y) * W; };
    auto ld2 = [&](const uint16_t *row, int x) {       // samples x, x + 1 of the mirrored row (x even)
        const bool fx = flip & 1;
        const ushort2 v = *reinterpret_cast<const ushort2 *>(row + (fx ? W - 2 - x : x));
        return fx ? ushort2{v.y, v.x} : v;
    };
    auto ld4 = [&](const uint16_t *row, int x) {       // x .. x + 3 (x % 4 == 0)
        const bool fx = flip & 1;
        const ushort4 v = *reinterpret_cast<const ushort4 *>(row + (fx ? W - 4 - x : x));
        return fx ? ushort4{v.w, v.z, v.y, v.x} : v;
    };
    auto smp = [&](unsigned short s) { return (float)((int)s > black ? (int)s - black : 0); };

    // ---- phase 1: demosaic and the stages in front of the denoiser for every patch of the LDS image that lies in the image
#pragma unroll 1
    for (int t = threadIdx.x; t < PROWS * PCOLS; t += 256) {
        const int pr = t / PCOLS, pc = t - pr * PCOLS;
        const int px = x0 - RING_X + pc * PXT, py = y0 - RING_Y + pr * 2;
        if (px < 0 || px >= W || py < 0 || py >= H) continue;      // W % 4 == 0, H % 2 == 0: a patch is in or out as a whole
        f3 pix[2][PXT];
        if constexpr (KIND == RISP_DEMOSAIC_NEAREST) {
            // no stencil: the patch's own two quads, in the [0,1] domain (serve_kernel's branch)
            const ushort4 r0 = ld4(row_at(py), px), r1 = ld4(row_at(py + 1), px);
            const float R0 = smp(r0.x) / div, G10 = smp(r0.y) / div, R1 = smp(r0.z) / div, G11 = smp(r0.w) / div;
            const float G20 = smp(r1.x) / div, B0 = smp(r1.y) / div, G21 = smp(r1.z) / div, B1 = smp(r1.w) / div;
            pix[0][0] = pix[0][1] = {B0, G10, R0};
            pix[0][2] = pix[0][3] = {B1, G11, R1};
            pix[1][0] = pix[1][1] = {B0, G20, R0};
            pix[1][2] = pix[1][3] = {B1, G21, R1};
        } else {
            // m[r][c]: mosaic row py - 2 + r, column px - 2 + c in the 0..255 domain, reflect-101 over radius 2 - the loads and
            // border rules of serve_classical_kernel.  Bilinear needs the inner ring alone: rows 1 .. 4
            constexpr bool LAP = KIND == RISP_DEMOSAIC_LAPLACIAN;
            constexpr int R0 = LAP ? 0 : 1, R1 = LAP ? 6 : 5;
            const bool left = px > 0, right = px + 4 < W;
            const int xl = left ? px - 2 : 0, xr = right ? px + 4 : px;
            float m[6][8];
#pragma unroll
            for (int r = R0; r < R1; ++r) {
                int y = py - 2 + r;
                y = y < 0 ? -y : (y >= H ? 2 * H - 2 - y : y);
                const uint16_t *row = row_at(y);
                const ushort2 l = ld2(row, xl), e = ld2(row, xr);
                const ushort4 c = ld4(row, px);
                const unsigned short s[8] = {left ? l.x : c.z, left ? l.y : c.y, c.x, c.y, c.z, c.w, right ? e.x : c.z, right ? e.y : c.y};
#pragma unroll
                for (int k = 0; k < 8; ++k) m[r][k] = (smp(s[k]) / div) * 255.f;       // risp_raw_crop_cfa's expression, x 255 on load
            }
#pragma unroll
            for (int p = 0; p < 2; ++p)
#pragma unroll
                for (int i = 0; i < PXT; ++i) {
                    // origin_demosaic_kernel's expressions; py is even and px a multiple of 4: the site is known at compile time
                    auto s = [&](int dy, int dx) { return m[2 + p + dy][2 + i + dx]; };
                    const float c = s(0, 0);
                    const float cross = s(-1, 0) + s(1, 0) + s(0, -1) + s(0, 1);
                    const float diag = s(-1, -1) + s(-1, 1) + s(1, -1) + s(1, 1);
                    const float hor = s(0, -1) + s(0, 1), ver = s(-1, 0) + s(1, 0);
                    float g_rb, rb_hor, rb_ver, rb_diag;
                    if constexpr (LAP) {
                        const float fh = s(0, -2) + s(0, 2), fv = s(-2, 0) + s(2, 0), far = fh + fv;
                        g_rb = (4.f * c + 2.f * cross - far) / 8.f;
                        rb_hor = (5.f * c + 4.f * hor - diag - fh + 0.5f * fv) / 8.f;
                        rb_ver = (5.f * c + 4.f * ver - diag - fv + 0.5f * fh) / 8.f;
                        rb_diag = (6.f * c + 2.f * diag - 1.5f * far) / 8.f;
                    } else {
                        g_rb = cross / 4.f;
                        rb_hor = hor / 2.f;
                        rb_ver = ver / 2.f;
                        rb_diag = diag / 4.f;
                    }
                    const bool er = p == 0, ec = (i & 1) == 0;      // R at (even,even), B at (odd,odd)
                    float R_, G_, B_;
                    if (er && ec) { R_ = c; G_ = g_rb; B_ = rb_diag; }
                    else if (er && !ec) { G_ = c; R_ = rb_hor; B_ = rb_ver; }
                    else if (!er && ec) { G_ = c; R_ = rb_ver; B_ = rb_hor; }
                    else { B_ = c; G_ = g_rb; R_ = rb_diag; }
                    const float inv255 = 1.f / 255.f;
                    pix[p][i] = {q8(B_) * inv255, q8(G_) * inv255, q8(R_) * inv255};
                }
        }
        run_stages<2 * PXT, WBQ>(a, 0, a.n_pre, n, &pix[0][0]);
        // the denoisers' domain: value x in_scale (255); the median works on the 8-bit codes
        auto conv = [&](float v) { v *= 255.f; return DEN == RISP_DENOISE_MEDIAN ? q8(v) : v; };
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            float *dst = lds + (pr * 2 + p) * LW + pc * PXT;
            *reinterpret_cast<float4 *>(dst) = make_float4(conv(pix[p][0].b), conv(pix[p][1].b), conv(pix[p][2].b), conv(pix[p][3].b));
            *reinterpret_cast<float4 *>(dst + LPLANE) = make_float4(conv(pix[p][0].g), conv(pix[p][1].g), conv(pix[p][2].g), conv(pix[p][3].g));
            *reinterpret_cast<float4 *>(dst + 2 * LPLANE) = make_float4(conv(pix[p][0].r), conv(pix[p][1].r), conv(pix[p][2].r), conv(pix[p][3].r));
        }
    }
    __syncthreads();

    // ---- ring positions outside the image: the pixel at the reflect-101 image coordinate.  Only tiles on the image border have
    // any (a workgroup-uniform condition: the barrier inside is reached by all or by none)
    if (y0 == 0 || x0 == 0 || y0 + TILE_H + REACH > H || x0 + TILE_W + REACH > W) {
        for (int idx = threadIdx.x; idx < LPLANE; idx += 256) {
            const int r = idx / LW, c = idx - r * LW;
            const int gy = y0 - RING_Y + r, gx = x0 - RING_X + c;
            if (gy < -REACH || gy >= H + REACH || gx < -REACH || gx >= W + REACH) continue;
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) continue;
            const int sy = gy < 0 ? -gy : (gy >= H ? 2 * H - 2 - gy : gy), sx = gx < 0 ? -gx : (gx >= W ? 2 * W - 2 - gx : gx);
            const int src = (sy - y0 + RING_Y) * LW + sx - x0 + RING_X;
            lds[idx] = lds[src];
            lds[idx + LPLANE] = lds[src + LPLANE];
            lds[idx + 2 * LPLANE] = lds[src + 2 * LPLANE];
        }
        __syncthreads();
    }

    // ---- phase 2: the thread's own patch, a row of 4 pixels at a time
    const int lx = (int)(threadIdx.x % STX) * PXT, ly = (int)(threadIdx.x / STX) * 2;
    const int px = x0 + lx, py = y0 + ly;
    const bool live = px < W && py < H;
    if (!STATS && !live) return;                        // (the statistics launch keeps its idle threads for the workgroup reduction)
    // a thread that owns no pixel holds the identity: 0 for a sum, -inf for a maximum (behind WbManual or WbQuadratic every
    // value of an image can be negative)
    const bool smax = STATS && a.stat == RISP_SCENE_MAX3;
    float acc[3];
    acc[0] = acc[1] = acc[2] = smax ? -INFINITY : 0.f;
#pragma unroll 1
    for (int p = 0; p < (live ? 2 : 0); ++p) {
        f3 o[PXT];
        const float inv255 = 1.f / 255.f;
        if constexpr (DEN == RISP_DENOISE_BILATERAL) {
            // bilateral4_kernel<1>, every image at radius 1
            const float sig_s = a.db[n], sig_c = a.da[n];
            const float ks = -1.f / (2.f * sig_s * sig_s), kc = -1.f / (2.f * sig_c * sig_c);
            const float ks2 = ks * 1.4426950408889634f, kc2 = kc * 1.4426950408889634f;
#pragma unroll
            for (int i = 0; i < PXT; ++i) {
                const float *ctr = lds + (ly + p + RING_Y) * LW + lx + RING_X + i;
                const float cb = ctr[0], cg = ctr[LPLANE], cr = ctr[2 * LPLANE];
                float nb = 0.f, ng = 0.f, nr = 0.f, den = 0.f;
                auto tap = [&](int dy, int dx) {
                    const float *q = ctr + dy * LW + dx;
                    const float qb = q[0], qg = q[LPLANE], qr = q[2 * LPLANE];
                    if (dy == 0 && dx == 0) {
                        nb += qb; ng += qg; nr += qr; den += 1.f;
                        return;
                    }
                    const float dist = fabsf(qb - cb) + fabsf(qg - cg) + fabsf(qr - cr);
                    const float wgt = __builtin_amdgcn_exp2f(__builtin_fmaf(dist * dist, kc2, (float)(dy * dy + dx * dx) * ks2));
                    nb = __builtin_fmaf(wgt, qb, nb); ng = __builtin_fmaf(wgt, qg, ng); nr = __builtin_fmaf(wgt, qr, nr); den += wgt;
                };
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                    for (int dx = -1; dx <= 1; ++dx) tap(dy, dx);
                const float rden = 1.f / den;
                o[i] = {q8(nb * rden) * inv255, q8(ng * rden) * inv255, q8(nr * rden) * inv255};
            }
        } else if constexpr (DEN == RISP_DENOISE_MEDIAN) {
            // median3x4_kernel: the six window columns sorted once, a pixel's median from three of them
            float res[3][PXT];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float *top = lds + c * LPLANE + (ly + p + RING_Y - 1) * LW + lx + RING_X - 1;   // image columns px-1 .. px+4
                float lo[6], md[6], hi[6];
#pragma unroll
                for (int j = 0; j < 6; ++j) {
                    const float u = top[j], v = top[LW + j], w = top[2 * LW + j];
                    lo[j] = fminf(fminf(u, v), w);
                    hi[j] = fmaxf(fmaxf(u, v), w);
                    md[j] = __builtin_amdgcn_fmed3f(u, v, w);
                }
#pragma unroll
                for (int i = 0; i < PXT; ++i) {
                    const float u = fmaxf(fmaxf(lo[i], lo[i + 1]), lo[i + 2]);
                    const float v = __builtin_amdgcn_fmed3f(md[i], md[i + 1], md[i + 2]);
                    const float w = fminf(fminf(hi[i], hi[i + 1]), hi[i + 2]);
                    res[c][i] = __builtin_amdgcn_fmed3f(u, v, w) * inv255;
                }
            }
#pragma unroll
            for (int i = 0; i < PXT; ++i) o[i] = {res[0][i], res[1][i], res[2][i]};
        } else {
            // fastnlm4_kernel<true>, block 3 and search 3.  v[row][col][ch]: image rows py+p-2 .. py+p+2, columns px-2 .. px+5
            const float dec = a.da[n];
            const float scale = -1.f / (3.f * (float)(3 * 3) * dec * dec);
            float v[5][8][3];
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int rr = 0; rr < 5; ++rr) {
                    const float *row = lds + c * LPLANE + (ly + p + rr) * LW + lx;
                    const float2 l2 = *reinterpret_cast<const float2 *>(row + 2), e2 = *reinterpret_cast<const float2 *>(row + 8);
                    const float4 d = *reinterpret_cast<const float4 *>(row + 4);
                    v[rr][0][c] = l2.x; v[rr][1][c] = l2.y; v[rr][2][c] = d.x; v[rr][3][c] = d.y;
                    v[rr][4][c] = d.z; v[rr][5][c] = d.w; v[rr][6][c] = e2.x; v[rr][7][c] = e2.y;
                }
            float nb[4] = {0.f, 0.f, 0.f, 0.f}, ng[4] = {0.f, 0.f, 0.f, 0.f}, nr[4] = {0.f, 0.f, 0.f, 0.f}, den[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int sy = -1; sy <= 1; ++sy)
#pragma unroll
                for (int sx = -1; sx <= 1; ++sx) {
                    float e[3][6];                         // q = (py + p + qy, px + qx), qy = -1..1, qx = -1..4
#pragma unroll
                    for (int qy = 0; qy < 3; ++qy)
#pragma unroll
                        for (int qx = 0; qx < 6; ++qx) {
                            const float d0 = v[qy + 1 + sy][qx + 1 + sx][0] - v[qy + 1][qx + 1][0];
                            const float d1 = v[qy + 1 + sy][qx + 1 + sx][1] - v[qy + 1][qx + 1][1];
                            const float d2c = v[qy + 1 + sy][qx + 1 + sx][2] - v[qy + 1][qx + 1][2];
                            e[qy][qx] = d0 * d0 + d1 * d1 + d2c * d2c;
                        }
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        float d2 = 0.f;
#pragma unroll
                        for (int oy = 0; oy < 3; ++oy)
#pragma unroll
                            for (int ox = 0; ox < 3; ++ox) d2 += e[oy][i + ox];
                        const float wgt = __expf(d2 * scale);
                        nb[i] += wgt * v[2 + sy][i + 2 + sx][0];
                        ng[i] += wgt * v[2 + sy][i + 2 + sx][1];
                        nr[i] += wgt * v[2 + sy][i + 2 + sx][2];
                        den[i] += wgt;
                    }
                }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float rden = 1.f / den[i];
                o[i] = {q8(nb[i] * rden) * inv255, q8(ng[i] * rden) * inv255, q8(nr[i] * rden) * inv255};
            }
        }

        run_stages<PXT, WBQ>(a, a.n_pre, a.n_ops, n, o);

        if constexpr (STATS) {
            // the row's four pixels in order: with the loop over p the thread's eight pixels in row order
#pragma unroll
            for (int i = 0; i < PXT; ++i) {
                if (smax) { acc[0] = fmaxf(acc[0], o[i].b); acc[1] = fmaxf(acc[1], o[i].g); acc[2] = fmaxf(acc[2], o[i].r); }
                else { acc[0] += o[i].b; acc[1] += o[i].g; acc[2] += o[i].r; }
            }
            continue;
        }
        // the result alone: 4 pixels x 3 bytes of a row are three dwords (the row offset is a multiple of 12 bytes).  Mirrored
        // along x the four pixels land at W-4-px in reverse order (the bytes of a pixel keep theirs)
        unsigned b[PXT][3];
#pragma unroll
        for (int c = 0; c < PXT; ++c) {
            const f3 v = o[c], m = o[PXT - 1 - c];
            const bool fx = flip & 1;
            const unsigned vb = u8(fx ? m.b : v.b), vg = u8(fx ? m.g : v.g), vr = u8(fx ? m.r : v.r);
            b[c][0] = a.reverse ? vr : vb;
            b[c][1] = vg;
            b[c][2] = a.reverse ? vb : vr;
        }
        unsigned *dst = reinterpret_cast<unsigned *>(
            a.out + (((size_t)n * H + (flip & 2 ? H - 1 - py - p : py + p)) * W + (flip & 1 ? W - 4 - px : px)) * 3);
        dst[0] = b[0][0] | b[0][1] << 8 | b[0][2] << 16 | b[1][0] << 24;
        dst[1] = b[1][1] | b[1][2] << 8 | b[2][0] << 16 | b[2][1] << 24;
        dst[2] = b[2][2] | b[3][0] << 8 | b[3][1] << 16 | b[3][2] << 24;
    }

    if constexpr (STATS) {
        __shared__ float red[12];
        if (smax) block_reduce3<true>(acc, red);           // (a.stat is workgroup-uniform: all threads take the same branch)
        else block_reduce3<false>(acc, red);
        if (threadIdx.x == 0) {                         // the logical tile after the remap: the order of the partials is the image's
            const size_t tile = (size_t)byi * gridDim.x + bxi;
            *reinterpret_cast<float4 *>(a.partials + ((size_t)n * gridDim.x * gridDim.y + tile) * 4) = float4{acc[0], acc[1], acc[2], 0.f};
        }
    }
}

template <int KIND, int DEN, bool STATS>
void launch_form(bool wbq, dim3 grid, hipStream_t s, const DenoiseSceneArgs &a) {
    if (wbq) hipLaunchKernelGGL((serve_denoise_scene_kernel<KIND, DEN, true, STATS>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((serve_denoise_scene_kernel<KIND, DEN, false, STATS>), grid, dim3(256), 0, s, a);
}

template <int KIND, bool STATS>
void launch_kind(int denoise, bool wbq, dim3 grid, hipStream_t s, const DenoiseSceneArgs &a) {
    if (denoise == RISP_DENOISE_BILATERAL) launch_form<KIND, RISP_DENOISE_BILATERAL, STATS>(wbq, grid, s, a);
    else if (denoise == RISP_DENOISE_MEDIAN) launch_form<KIND, RISP_DENOISE_MEDIAN, STATS>(wbq, grid, s, a);
    else launch_form<KIND, RISP_DENOISE_FASTNLM, STATS>(wbq, grid, s, a);
}

template <bool STATS>
void launch(int demosaic, int denoise, bool wbq, dim3 grid, hipStream_t s, const DenoiseSceneArgs &a) {
    if (demosaic == RISP_DEMOSAIC_LAPLACIAN) launch_kind<RISP_DEMOSAIC_LAPLACIAN, STATS>(denoise, wbq, grid, s, a);
    else if (demosaic == RISP_DEMOSAIC_BILINEAR) launch_kind<RISP_DEMOSAIC_BILINEAR, STATS>(denoise, wbq, grid, s, a);
    else launch_kind<RISP_DEMOSAIC_NEAREST, STATS>(denoise, wbq, grid, s, a);
}

// the tile grid: that of risp_serve_scene_stats, so G = risp_serve_scene_groups(H, W) rows per image
dim3 tile_grid(int N, int H, int W) { return dim3((W + TILE_W - 1) / TILE_W, (H + TILE_H - 1) / TILE_H, N); }

// the rules both launches share; fills a (but for out / partials / stat / reverse)
int denoise_scene_args(const char *name, const uint16_t *raw, float divisor, int demosaic, int n_pre, const int *pre_ops,
                       const float *const *pre_params, int denoise, int window, int search, const float *den_a, const float *den_b,
                       int n_post, const int *post_ops, const float *const *post_params, int N, int H, int W, int black_level, int cfa,
                       DenoiseSceneArgs &a, bool &wbq) {
    RISP_CHECK_ARG(raw, "%s: null argument (raw)", name);
    RISP_CHECK_ARG(divisor > 0.f, "%s: divisor %g", name, (double)divisor);
    RISP_CHECK_ARG(demosaic >= RISP_DEMOSAIC_NEAREST && demosaic <= RISP_DEMOSAIC_LAPLACIAN,
                   "%s: demosaic %d (RISP_DEMOSAIC_NEAREST 0, BILINEAR 1, LAPLACIAN 2)", name, demosaic);
    RISP_CHECK_ARG(denoise >= RISP_DENOISE_BILATERAL && denoise <= RISP_DENOISE_FASTNLM,
                   "%s: denoiser %d (RISP_DENOISE_BILATERAL 0, MEDIAN 1, FASTNLM 2)", name, denoise);
    if (denoise == RISP_DENOISE_BILATERAL) {
        RISP_CHECK_ARG(window == 3, "%s: bilateral window %d (only 3 is served here)", name, window);
        RISP_CHECK_ARG(den_a && den_b, "%s: the bilateral has no sigma_color / sigma_space parameter block", name);
    } else if (denoise == RISP_DENOISE_MEDIAN) {
        RISP_CHECK_ARG(window == 3, "%s: median size %d (only 3 is served here)", name, window);
    } else {
        RISP_CHECK_ARG(window == 3 && search == 3, "%s: non-local means block %d search %d (only 3 and 3 are served here)", name,
                       window, search);
        RISP_CHECK_ARG(den_a, "%s: non-local means has no decay parameter block", name);
    }
    RISP_CHECK_ARG(cfa >= 0 && cfa <= 3, "%s: cfa %d (RISP_CFA_RGGB 0, GRBG 1, GBRG 2, BGGR 3)", name, cfa);
    RISP_CHECK_ARG(black_level >= 0 && black_level <= 65535, "%s: black_level %d outside 0 .. 65535", name, black_level);
    RISP_CHECK_ARG(n_pre >= 0 && n_post >= 0 && n_pre <= RISP_MAX_CHAIN && n_post <= RISP_MAX_CHAIN && n_pre + n_post <= RISP_MAX_CHAIN,
                   "%s: bad op list: %d + %d stages (at most %d in all)", name, n_pre, n_post, RISP_MAX_CHAIN);
    RISP_CHECK_ARG((n_pre == 0 || (pre_ops && pre_params)) && (n_post == 0 || (post_ops && post_params)), "%s: bad op list: null",
                   name);
    RISP_CHECK_ARG(N >= 1 && N <= 65535 && H >= 4 && H % 2 == 0 && W >= 4 && W % 4 == 0,
                   "%s: bad shape N=%d H=%d W=%d (H even and >= 4, W a multiple of 4)", name, N, H, W);
    RISP_CHECK_ARG(reinterpret_cast<uintptr_t>(raw) % 8 == 0, "%s: raw must be 8-byte aligned", name);
    a.raw = raw;
    a.out = nullptr;
    a.partials = nullptr;
    a.divisor = divisor;
    a.n_pre = n_pre;
    a.n_ops = n_pre + n_post;
    a.N = N;
    a.H = H;
    a.W = W;
    a.reverse = 0;
    a.black = black_level;
    a.flip = cfa;
    a.stat = 0;
    a.da = den_a;
    a.db = den_b;
    wbq = false;
    for (int k = 0; k < RISP_MAX_CHAIN; ++k) {
        a.ops[k] = RISP_OP_SKIP;
        a.params[k] = nullptr;
    }
    for (int k = 0; k < n_pre + n_post; ++k) {
        const int op = k < n_pre ? pre_ops[k] : post_ops[k - n_pre];
        const float *p = k < n_pre ? pre_params[k] : post_params[k - n_pre];
        const bool scene = op == RISP_OP_GAIN3_Q8;
        RISP_CHECK_ARG(op != RISP_OP_TONE_REINHARD, "%s: op %d (RISP_OP_TONE_REINHARD) is not served beside a denoiser", name, op);
        RISP_CHECK_ARG(op == RISP_OP_SKIP || (op >= RISP_OP_WB_MANUAL && op <= RISP_OP_TONE_FILMIC) || scene, "%s: op %d not allowed",
                       name, op);
        RISP_CHECK_ARG(!scene || p, "%s: stage %d (op %d) needs the constants of risp_serve_scene_finish", name, k, op);
        RISP_CHECK_ARG(!scene || reinterpret_cast<uintptr_t>(p) % 16 == 0, "%s: the constants of stage %d must be 16-byte aligned", name,
                       k);
        RISP_CHECK_ARG(op == RISP_OP_SKIP || p, "%s: stage %d has no parameter block", name, k);
        a.ops[k] = op;
        a.params[k] = op == RISP_OP_SKIP ? nullptr : p;
        wbq |= op == RISP_OP_WB_QUADRATIC;
    }
    return 0;
}

}  // namespace

extern "C" int risp_serve_denoise_stats(const uint16_t *raw, float divisor, int demosaic, int n_pre, const int *pre_ops,
                                        const float *const *pre_params, int denoise, int window, int search, const float *den_a,
                                        const float *den_b, int n_post, const int *post_ops, const float *const *post_params, int stat,
                                        float *partials, int N, int H, int W, int black_level, int cfa, void *stream) {
    const char *name = "risp_serve_denoise_stats";
    DenoiseSceneArgs a;
    bool wbq;
    if (int e = denoise_scene_args(name, raw, divisor, demosaic, n_pre, pre_ops, pre_params, denoise, window, search, den_a, den_b, n_post,
                                   post_ops, post_params, N, H, W, black_level, cfa, a, wbq))
        return e;
    RISP_CHECK_ARG(stat != RISP_SCENE_LOGLUM, "%s: stat %d (RISP_SCENE_LOGLUM) is not served behind a denoiser", name, stat);
    RISP_CHECK_ARG(stat == RISP_SCENE_MEAN3 || stat == RISP_SCENE_MAX3, "%s: stat %d (RISP_SCENE_MEAN3 0, MAX3 1)", name, stat);
    RISP_CHECK_ARG(partials, "%s: null argument (partials)", name);
    RISP_CHECK_ARG(reinterpret_cast<uintptr_t>(partials) % 16 == 0, "%s: partials must be 16-byte aligned", name);
    a.partials = partials;
    a.stat = stat;
    launch<true>(demosaic, denoise, wbq, tile_grid(N, H, W), (hipStream_t)stream, a);
    RISP_LAUNCH_CHECK("risp_serve_denoise_stats");
    return 0;
}

extern "C" int risp_serve_denoise_scene_u8(const uint16_t *raw, float divisor, int demosaic, int n_pre, const int *pre_ops,
                                           const float *const *pre_params, int denoise, int window, int search, const float *den_a,
                                           const float *den_b, int n_post, const int *post_ops, const float *const *post_params,
                                           uint8_t *out, int reverse_channels, int N, int H, int W, int black_level, int cfa,
                                           void *stream) {
    const char *name = "risp_serve_denoise_scene_u8";
    DenoiseSceneArgs a;
    bool wbq;
    if (int e = denoise_scene_args(name, raw, divisor, demosaic, n_pre, pre_ops, pre_params, denoise, window, search, den_a, den_b, n_post,
                                   post_ops, post_params, N, H, W, black_level, cfa, a, wbq))
        return e;
    RISP_CHECK_ARG(out, "%s: null argument (out)", name);
    RISP_CHECK_ARG(reinterpret_cast<uintptr_t>(out) % 4 == 0, "%s: out must be 4-byte aligned", name);
    a.out = out;
    a.reverse = reverse_channels ? 1 : 0;
    launch<false>(demosaic, denoise, wbq, tile_grid(N, H, W), (hipStream_t)stream, a);
    RISP_LAUNCH_CHECK("risp_serve_denoise_scene_u8");
    return 0;
}
