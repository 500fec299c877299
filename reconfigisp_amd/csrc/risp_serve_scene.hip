// Serving path for pipelines with a scene-adaptive stage: gray-world, white-world, Reinhard.  Each needs one whole-image
// quantity first - three sums, three maxima, one sum of logarithms - and every value that feeds it is a pure function of a
// 6 x 8 mosaic neighbourhood.  So the 2-byte mosaic is read twice instead of fp32 planes being written once:
//
//     risp_serve_scene_stats    the pixel pipeline of risp_serve_classical_u8 up to the scene stage, reduced per workgroup
//     risp_serve_scene_finish   the partials of an image, added in double precision, become its per-image constants
//     risp_serve_scene_u8       risp_serve_classical_u8 with two more stages that take those constants
//
// The patch loader, the two demosaics and the stage loop restate serve_classical_kernel (risp_serve_classical.hip), as that
// file restated risp_origin.hip: its six instantiations stay as measured.  One kernel template serves both the
// statistics and the serving launch; STATS is a compile-time switch.  With -ffp-contract=off a pixel's value in front of the
// scene stage has the bits of the composed route, so a maximum - which has no order - gives the composed route's constants
// and bytes; a sum taken in another order gives constants that differ in their last bits.
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

struct SceneArgs {
    const uint16_t *raw;        // (N,H,W) mosaic of the sensor
    uint8_t *out;               // (N,H,W,3); the serving launch
    float *partials;            // (N,G,4); the statistics launch
    float divisor;
    int n_ops, N, H, W;
    int reverse;                // store R, G, B instead of B, G, R
    int black;                  // subtracted from every sample in integers, clamped at 0
    int flip;                   // RISP_CFA_*: bit 0 mirrors x, bit 1 mirrors y
    int stat;                   // RISP_SCENE_*
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

// a tone curve on the patch: tonemap_kernel's pixel expression with si = so = 255, p0 / p1 as tonemap_prepare_kernel forms them
template <bool FILMIC>
__device__ __forceinline__ void tone_all(float p0, float p1, f3 *px) {
    auto curve = [&](float x) {
        float v = x * 255.f / 255.f;
        v = fmaxf(v, 0.f);
        if (FILMIC) v = hable(v * p0) * p1;
        else v = 1.f - __expf(-v * p0);
        return q8(v * 255.f) * (1.f / 255.f);
    };
#pragma unroll
    for (int i = 0; i < 2 * PXT; ++i) px[i] = {curve(px[i].b), curve(px[i].g), curve(px[i].r)};
}

// white-world apply: tonemap_kernel<TM_GAIN>'s pixel expression with si = so = 255, the gains of risp_serve_scene_finish
__device__ __forceinline__ void gain_q8_all(float p0, float p1, float p2, f3 *px) {
#pragma unroll
    for (int i = 0; i < 2 * PXT; ++i) {
        float b = px[i].b * 255.f / 255.f, g = px[i].g * 255.f / 255.f, r = px[i].r * 255.f / 255.f;
        b *= p0; g *= p1; r *= p2;
        px[i] = {q8(b * 255.f) * (1.f / 255.f), q8(g * 255.f) * (1.f / 255.f), q8(r * 255.f) * (1.f / 255.f)};
    }
}

// Reinhard: tonemap_kernel<TM_REINHARD>'s pixel expression with si = so = 255; p0 = key / log-average luminance, p1 = 1 / Lwhite^2
__device__ __forceinline__ void reinhard_all(float p0, float p1, f3 *px) {
#pragma unroll
    for (int i = 0; i < 2 * PXT; ++i) {
        float b = fmaxf(px[i].b * 255.f / 255.f, 0.f), g = fmaxf(px[i].g * 255.f / 255.f, 0.f), r = fmaxf(px[i].r * 255.f / 255.f, 0.f);
        const float L = 0.114f * b + 0.587f * g + 0.299f * r;
        const float ls = p0 * L;
        const float s = ls * (1.f + ls * p1) / (1.f + ls) / fmaxf(L, 1e-6f);
        b *= s; g *= s; r *= s;
        px[i] = {q8(b * 255.f) * (1.f / 255.f), q8(g * 255.f) * (1.f / 255.f), q8(r * 255.f) * (1.f / 255.f)};
    }
}

// sum or maximum of three values over the workgroup, in a fixed order: wavefront shuffles, then one LDS step in wave order.
// Thread 0 receives the result.  Contains a barrier: every thread of the workgroup calls it
template <bool MAX>
__device__ __forceinline__ void block_reduce3(float (&v)[3], float *lds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        float s = v[i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float t = __shfl_down(s, o, 64);
            s = MAX ? fmaxf(s, t) : s + t;
        }
        if (lane == 0) lds[i * 4 + wave] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float *q = lds + i * 4;
            v[i] = MAX ? fmaxf(fmaxf(fmaxf(q[0], q[1]), q[2]), q[3]) : ((q[0] + q[1]) + q[2]) + q[3];
        }
    }
}

// KIND: RISP_DEMOSAIC_*.  px, py and every coordinate derived from them are those of the mirrored image, which is RGGB; only
// row_at / ld2 / ld4 and the store know where the samples really are.  STATS: no image is stored; the values behind the
// n_ops stages are reduced over the workgroup's tile and one row of four floats goes to partials[(n * G + tile) * 4 ..]
template <int KIND, bool WBQ, bool STATS>
__global__ __launch_bounds__(256) void serve_scene_kernel(const SceneArgs a) {
    const int H = a.H, W = a.W;
    int bxi, byi, bzi;
    xcd_tile(bxi, byi, bzi);
    const int n = bzi;
    const int px = (bxi * STX + (int)(threadIdx.x % STX)) * 4, py = (byi * STY + (int)(threadIdx.x / STX)) * 2;
    const bool live = px < W && py < H;                 // W % 4 == 0, H % 2 == 0: a patch is in or out as a whole
    if (!STATS && !live) return;                        // (the statistics launch keeps its idle threads for the workgroup reduction)
    f3 pix[2][PXT];
    if (live) {
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

        if constexpr (KIND == RISP_DEMOSAIC_NEAREST) {
            // ---- no stencil: the patch's own two quads, in the [0,1] domain
            const ushort4 r0 = ld4(row_at(py), px), r1 = ld4(row_at(py + 1), px);
            const float R0 = smp(r0.x) / div, G10 = smp(r0.y) / div, R1 = smp(r0.z) / div, G11 = smp(r0.w) / div;
            const float G20 = smp(r1.x) / div, B0 = smp(r1.y) / div, G21 = smp(r1.z) / div, B1 = smp(r1.w) / div;
            pix[0][0] = pix[0][1] = {B0, G10, R0};
            pix[0][2] = pix[0][3] = {B1, G11, R1};
            pix[1][0] = pix[1][1] = {B0, G20, R0};
            pix[1][2] = pix[1][3] = {B1, G21, R1};
        } else {
            // ---- m[r][c]: mosaic row py - 2 + r, column px - 2 + c in the 0..255 domain, reflect-101 over radius 2 (H, W >= 4:
            // one reflection reaches every tap).  The left pair at px = 0 reflects to columns 2 and 1 and the right pair at
            // px = W - 4 to W - 2 and W - 3: both lie in the thread's own centre vector (as .z, .y), so the pair load of a border
            // patch only has to stay in bounds.  Bilinear needs the inner ring alone: rows 1 .. 4
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

        // ---- stages: the tone curves and the two scene applies here, the rest in risp_ops.h.  A scene stage's block is the
        // (N,4) constants of risp_serve_scene_finish
        for (int k = 0; k < a.n_ops; ++k) {
            const int op = a.ops[k];
            const float *p = a.params[k];
            if (op == RISP_OP_TONE_CRYSIS) {               // p (N,1): lum_adapted
                tone_all<false>(0.5f / (p[n] + 0.05f), 0.f, &pix[0][0]);
            } else if (op == RISP_OP_TONE_FILMIC) {        // p (N,2): white_point, exposure_bias
                tone_all<true>(p[2 * n + 1], 1.f / hable(fmaxf(p[2 * n], 0.01f) * 11.2f), &pix[0][0]);
            } else if (op == RISP_OP_GAIN3_Q8) {
                gain_q8_all(p[4 * n], p[4 * n + 1], p[4 * n + 2], &pix[0][0]);
            } else if (op == RISP_OP_TONE_REINHARD) {
                reinhard_all(p[4 * n], p[4 * n + 1], &pix[0][0]);
            } else {
                apply_op<2 * PXT, WBQ>(op, p, n, &pix[0][0]);
            }
        }
    }

    if constexpr (STATS) {
        // ---- the thread's eight pixels in row order, then the workgroup.  A thread outside the image holds the identity: 0
        // for a sum, -inf for a maximum (behind WbQuadratic every value of an image can be negative)
        __shared__ float red[12];
        const int stat = a.stat;
        float acc[3];
        if (stat == RISP_SCENE_MAX3) {
            acc[0] = acc[1] = acc[2] = -INFINITY;
            if (live) {
#pragma unroll
                for (int i = 0; i < 2 * PXT; ++i) {
                    const f3 v = (&pix[0][0])[i];
                    acc[0] = fmaxf(acc[0], v.b); acc[1] = fmaxf(acc[1], v.g); acc[2] = fmaxf(acc[2], v.r);
                }
            }
            block_reduce3<true>(acc, red);
        } else {
            acc[0] = acc[1] = acc[2] = 0.f;
            if (live) {
#pragma unroll
                for (int i = 0; i < 2 * PXT; ++i) {
                    const f3 v = (&pix[0][0])[i];
                    if (stat == RISP_SCENE_MEAN3) {
                        acc[0] += v.b; acc[1] += v.g; acc[2] += v.r;
                    } else {                            // loglum_kernel's expression with si = 255
                        const float bb = fmaxf(v.b * 255.f, 0.f), gg = fmaxf(v.g * 255.f, 0.f), rr = fmaxf(v.r * 255.f, 0.f);
                        acc[0] += __logf((0.114f * bb + 0.587f * gg + 0.299f * rr) / 255.f + 1e-4f);
                    }
                }
            }
            block_reduce3<false>(acc, red);
        }
        if (threadIdx.x == 0) {                         // the logical tile after the remap: the order of the partials is the image's
            const size_t tile = (size_t)byi * gridDim.x + bxi;
            *reinterpret_cast<float4 *>(a.partials + ((size_t)n * gridDim.x * gridDim.y + tile) * 4) = float4{acc[0], acc[1], acc[2], 0.f};
        }
    } else {
        // ---- the result alone: 4 pixels x 3 bytes of a row are three dwords (the row offset is a multiple of 12 bytes).
        // Mirrored along x the four pixels land at W-4-px in reverse order (the bytes of a pixel keep theirs)
        const int flip = a.flip;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            unsigned b[PXT][3];
#pragma unroll
            for (int c = 0; c < PXT; ++c) {
                const f3 v = pix[p][c], m = pix[p][PXT - 1 - c];
                const bool fx = flip & 1;                   // value selects (a ?: between the two array elements selects an address)
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
    }
}

// One workgroup of one wavefront per image.  Lane l adds (or takes the maximum of) a contiguous run of the image's G partial
// rows in index order, in double precision; thread 0 then combines the 64 runs in lane order: index order throughout, and
// one rounding to float at the end (an fp32 running sum over the 5922 partials of a 3000 x 4000 frame would cost more than
// the comparison rule of the tests allows).  The constants are those of the composed route's prepare kernels.
__global__ __launch_bounds__(64) void scene_finish_kernel(int stat, const float *__restrict__ partials, const float *__restrict__ pa,
                                                          const float *__restrict__ pb, float *__restrict__ consts, int N, int G,
                                                          float inv_hw) {
    __shared__ double red[3][64];
    const int n = blockIdx.x, lane = threadIdx.x;
    const int run = (G + 63) / 64;
    const int g0 = lane * run, g1 = g0 + run < G ? g0 + run : G;
    const bool mx = stat == RISP_SCENE_MAX3;
    double acc[3];
    acc[0] = acc[1] = acc[2] = mx ? -(double)INFINITY : 0.0;
    const float4 *rows = reinterpret_cast<const float4 *>(partials) + (size_t)n * G;
    for (int g = g0; g < g1; ++g) {
        const float4 v = rows[g];
        if (mx) { acc[0] = fmax(acc[0], (double)v.x); acc[1] = fmax(acc[1], (double)v.y); acc[2] = fmax(acc[2], (double)v.z); }
        else { acc[0] += (double)v.x; acc[1] += (double)v.y; acc[2] += (double)v.z; }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) red[c][lane] = acc[c];
    __syncthreads();
    if (lane != 0) return;
    float tot[3];
    for (int c = 0; c < 3; ++c) {
        double s = red[c][0];
        for (int l = 1; l < 64; ++l) s = mx ? fmax(s, red[c][l]) : s + red[c][l];
        tot[c] = (float)s;
    }
    float p0 = 0.f, p1 = 0.f, p2 = 0.f;
    if (stat == RISP_SCENE_MEAN3) {              // gray_gains_kernel's expression (risp_reduce.hip)
        const float m0 = tot[0] * inv_hw, m1 = tot[1] * inv_hw, m2 = tot[2] * inv_hw;
        const float gray = (m0 + m1 + m2) / 3.f;
        p0 = gray / fmaxf(m0, 1e-6f);
        p1 = gray / fmaxf(m1, 1e-6f);
        p2 = gray / fmaxf(m2, 1e-6f);
        // the block RISP_OP_GAIN3 takes: (N,3), packed at the front of consts; the last N floats are written as zeros
        consts[n * 3] = p0; consts[n * 3 + 1] = p1; consts[n * 3 + 2] = p2; consts[3 * N + n] = 0.f;
        return;
    }
    if (stat == RISP_SCENE_MAX3) {               // tonemap_prepare_kernel's white-world branch with si = 255; pa = ratio
        float m[3], big = 0.f;
        for (int c = 0; c < 3; ++c) { m[c] = fmaxf(tot[c] * 255.f, 1e-3f); big = fmaxf(big, m[c]); }
        p0 = 1.f + pa[n] * (big / m[0] - 1.f);
        p1 = 1.f + pa[n] * (big / m[1] - 1.f);
        p2 = 1.f + pa[n] * (big / m[2] - 1.f);
    } else {                                     // ... its Reinhard branch; pa = white_point, pb = middle_grey
        const float lw = fmaxf(pa[n], 0.01f) * 10.f;
        p0 = fmaxf(pb[n], 0.01f) / __expf(tot[0] * inv_hw);
        p1 = 1.f / (lw * lw);
    }
    *reinterpret_cast<float4 *>(consts + (size_t)n * 4) = float4{p0, p1, p2, 0.f};
}

template <int KIND, bool STATS>
void launch_kind(bool wbq, dim3 grid, hipStream_t s, const SceneArgs &a) {
    if (wbq) hipLaunchKernelGGL((serve_scene_kernel<KIND, true, STATS>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((serve_scene_kernel<KIND, false, STATS>), grid, dim3(256), 0, s, a);
}

template <bool STATS>
void launch(int demosaic, bool wbq, dim3 grid, hipStream_t s, const SceneArgs &a) {
    if (demosaic == RISP_DEMOSAIC_LAPLACIAN) launch_kind<RISP_DEMOSAIC_LAPLACIAN, STATS>(wbq, grid, s, a);
    else if (demosaic == RISP_DEMOSAIC_BILINEAR) launch_kind<RISP_DEMOSAIC_BILINEAR, STATS>(wbq, grid, s, a);
    else launch_kind<RISP_DEMOSAIC_NEAREST, STATS>(wbq, grid, s, a);
}

dim3 scene_grid(int N, int H, int W) { return dim3((W / 4 + STX - 1) / STX, (H / 2 + STY - 1) / STY, N); }

// the rules both pixel launches share; fills a (but for out / partials / stat / reverse)
int scene_args(const char *name, const uint16_t *raw, float divisor, int demosaic, int n_ops, const int *ops, const float *const *params,
               int N, int H, int W, int black_level, int cfa, SceneArgs &a, bool &wbq) {
    RISP_CHECK_ARG(raw, "%s: null argument (raw)", name);
    RISP_CHECK_ARG(divisor > 0.f, "%s: divisor %g", name, (double)divisor);
    RISP_CHECK_ARG(demosaic >= RISP_DEMOSAIC_NEAREST && demosaic <= RISP_DEMOSAIC_LAPLACIAN,
                   "%s: demosaic %d (RISP_DEMOSAIC_NEAREST 0, BILINEAR 1, LAPLACIAN 2)", name, demosaic);
    RISP_CHECK_ARG(cfa >= 0 && cfa <= 3, "%s: cfa %d (RISP_CFA_RGGB 0, GRBG 1, GBRG 2, BGGR 3)", name, cfa);
    RISP_CHECK_ARG(black_level >= 0 && black_level <= 65535, "%s: black_level %d outside 0 .. 65535", name, black_level);
    RISP_CHECK_ARG(n_ops >= 0 && n_ops <= RISP_MAX_CHAIN && (n_ops == 0 || (ops && params)), "%s: bad op list (n_ops %d)", name, n_ops);
    RISP_CHECK_ARG(N >= 1 && N <= 65535 && H >= 4 && H % 2 == 0 && W >= 4 && W % 4 == 0,
                   "%s: bad shape N=%d H=%d W=%d (H even and >= 4, W a multiple of 4)", name, N, H, W);
    RISP_CHECK_ARG(reinterpret_cast<uintptr_t>(raw) % 8 == 0, "%s: raw must be 8-byte aligned", name);
    a.raw = raw;
    a.out = nullptr;
    a.partials = nullptr;
    a.divisor = divisor;
    a.n_ops = n_ops;
    a.N = N;
    a.H = H;
    a.W = W;
    a.reverse = 0;
    a.black = black_level;
    a.flip = cfa;
    a.stat = 0;
    wbq = false;
    for (int k = 0; k < RISP_MAX_CHAIN; ++k) {
        a.ops[k] = RISP_OP_SKIP;
        a.params[k] = nullptr;
    }
    for (int k = 0; k < n_ops; ++k) {
        const bool scene = ops[k] == RISP_OP_GAIN3_Q8 || ops[k] == RISP_OP_TONE_REINHARD;
        RISP_CHECK_ARG(ops[k] == RISP_OP_SKIP || (ops[k] >= RISP_OP_WB_MANUAL && ops[k] <= RISP_OP_TONE_FILMIC) || scene,
                       "%s: op %d not allowed", name, ops[k]);
        RISP_CHECK_ARG(!scene || params[k], "%s: stage %d (op %d) needs the constants of risp_serve_scene_finish", name, k, ops[k]);
        RISP_CHECK_ARG(!scene || reinterpret_cast<uintptr_t>(params[k]) % 16 == 0, "%s: the constants of stage %d must be 16-byte aligned",
                       name, k);
        RISP_CHECK_ARG(ops[k] == RISP_OP_SKIP || params[k], "%s: stage %d has no parameter block", name, k);
        a.ops[k] = ops[k];
        a.params[k] = ops[k] == RISP_OP_SKIP ? nullptr : params[k];
        wbq |= ops[k] == RISP_OP_WB_QUADRATIC;
    }
    return 0;
}

bool stat_ok(int stat) { return stat == RISP_SCENE_MEAN3 || stat == RISP_SCENE_MAX3 || stat == RISP_SCENE_LOGLUM; }

}  // namespace

extern "C" int risp_serve_scene_groups(int H, int W) {
    if (H < 4 || H % 2 || W < 4 || W % 4) return 0;
    const dim3 g = scene_grid(1, H, W);
    return (int)(g.x * g.y);
}

extern "C" int risp_serve_scene_stats(const uint16_t *raw, float divisor, int demosaic, int n_ops, const int *ops,
                                      const float *const *params, int stat, float *partials, int N, int H, int W, int black_level,
                                      int cfa, void *stream) {
    const char *name = "risp_serve_scene_stats";
    SceneArgs a;
    bool wbq;
    if (int e = scene_args(name, raw, divisor, demosaic, n_ops, ops, params, N, H, W, black_level, cfa, a, wbq)) return e;
    RISP_CHECK_ARG(stat_ok(stat), "%s: stat %d (RISP_SCENE_MEAN3 0, MAX3 1, LOGLUM 2)", name, stat);
    RISP_CHECK_ARG(partials, "%s: null argument (partials)", name);
    RISP_CHECK_ARG(reinterpret_cast<uintptr_t>(partials) % 16 == 0, "%s: partials must be 16-byte aligned", name);
    a.partials = partials;
    a.stat = stat;
    launch<true>(demosaic, wbq, scene_grid(N, H, W), (hipStream_t)stream, a);
    RISP_LAUNCH_CHECK("risp_serve_scene_stats");
    return 0;
}

extern "C" int risp_serve_scene_finish(int stat, const float *partials, const float *a, const float *b, float *consts, int N, int G,
                                       int HW, void *stream) {
    const char *name = "risp_serve_scene_finish";
    RISP_CHECK_ARG(stat_ok(stat), "%s: stat %d (RISP_SCENE_MEAN3 0, MAX3 1, LOGLUM 2)", name, stat);
    RISP_CHECK_ARG(partials && consts, "%s: null argument", name);
    RISP_CHECK_ARG(N >= 1 && N <= 65535 && G >= 1 && HW >= 1, "%s: bad shape N=%d G=%d HW=%d", name, N, G, HW);
    RISP_CHECK_ARG(stat == RISP_SCENE_MEAN3 || a, "%s: stat %d needs the parameter a", name, stat);
    RISP_CHECK_ARG(stat != RISP_SCENE_LOGLUM || b, "%s: stat %d needs the parameter b", name, stat);
    RISP_CHECK_ARG(reinterpret_cast<uintptr_t>(partials) % 16 == 0 && reinterpret_cast<uintptr_t>(consts) % 16 == 0,
                   "%s: partials and consts must be 16-byte aligned", name);
    hipLaunchKernelGGL(scene_finish_kernel, dim3(N), dim3(64), 0, (hipStream_t)stream, stat, partials, a, b, consts, N, G,
                       1.0f / (float)HW);
    RISP_LAUNCH_CHECK("risp_serve_scene_finish");
    return 0;
}

extern "C" int risp_serve_scene_u8(const uint16_t *raw, float divisor, int demosaic, int n_ops, const int *ops,
                                   const float *const *params, uint8_t *out, int reverse_channels, int N, int H, int W, int black_level,
                                   int cfa, void *stream) {
    const char *name = "risp_serve_scene_u8";
    SceneArgs a;
    bool wbq;
    if (int e = scene_args(name, raw, divisor, demosaic, n_ops, ops, params, N, H, W, black_level, cfa, a, wbq)) return e;
    RISP_CHECK_ARG(out, "%s: null argument (out)", name);
    RISP_CHECK_ARG(reinterpret_cast<uintptr_t>(out) % 4 == 0, "%s: out must be 4-byte aligned", name);
    a.out = out;
    a.reverse = reverse_channels ? 1 : 0;
    launch<false>(demosaic, wbq, scene_grid(N, H, W), (hipStream_t)stream, a);
    RISP_LAUNCH_CHECK("risp_serve_scene_u8");
    return 0;
}
