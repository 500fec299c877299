// Serving path for pipelines with a scene-adaptive stage: gray-world, white-world, Reinhard.  Each needs one whole-image
// quantity first - three sums, three maxima, one sum of logarithms - and every value that feeds it is a pure function of a
// 6 x 8 mosaic neighbourhood.  So the 2-byte mosaic is read twice instead of fp32 planes being written once:
//
//     risp_serve_scene_stats    the pixel pipeline of risp_serve_classical_u8 up to the scene stage, reduced per workgroup
//     risp_serve_scene_finish   the partials of an image, added in double precision, become its per-image constants
//     risp_serve_scene_u8       risp_serve_classical_u8 with two more stages that take those constants
//
// The patch - loads, demosaic, stages, store - is risp_serve_patch.h's; this file owns the two scene applies, the reduction and
// the finish kernel.  One kernel template serves both the statistics and the serving launch; STATS is a compile-time switch.
// With -ffp-contract=off a pixel's value in front of the scene stage has the bits of the composed route, so a maximum - which
// has no order - gives the composed route's constants and bytes; a sum taken in another order gives constants that differ in
// their last bits.
#include <math.h>

#include "risp_serve_patch.h"

namespace {

using namespace risp_patch;

struct SceneArgs : PatchArgs {
    uint8_t *out;               // (N,H,W,3); the serving launch
    float *partials;            // (N,G,4); the statistics launch
    int reverse;                // store R, G, B instead of B, G, R
    int stat;                   // RISP_SCENE_*
};

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

// KIND: RISP_DEMOSAIC_*.  STATS: no image is stored; the values behind the n_ops stages are reduced over the workgroup's tile and
// one row of four floats goes to partials[(n * G + tile) * 4 ..]
template <int KIND, bool WBQ, bool STATS>
__global__ __launch_bounds__(256) void serve_scene_kernel(const SceneArgs a) {
    const int H = a.H, W = a.W;
    int bxi, byi, bzi;
    xcd_tile(bxi, byi, bzi);
    const int n = bzi;
    const int px = (bxi * STX + (int)(threadIdx.x % STX)) * 4, py = (byi * STY + (int)(threadIdx.x / STX)) * 2;
    const bool live = px < W && py < H;                 // W % 4 == 0, H % 2 == 0: a patch is in or out as a whole
    if (!STATS && !live) return;                        // (the statistics launch keeps its idle threads for the workgroup reduction)
    f3 pix[2][PXT];                                     // (the patch is copied into the kernel's own array: risp_serve_patch.h)
    if (live) {
        const Mosaic mo(a, n);
        Patch d;
        if constexpr (KIND == RISP_DEMOSAIC_NEAREST) d = mo.nearest(px, py);
        else {
            // Mosaic::window's fill, kept here: through the shared function the four stencil serving instantiations take one VGPR
            // more than they had (64 / 63 against 63 / 62; profiles/serve_patch_resources.txt)
            constexpr bool LAP = KIND == RISP_DEMOSAIC_LAPLACIAN;
            constexpr int R0 = LAP ? 0 : 1, R1 = LAP ? 6 : 5;
            const bool left = px > 0, right = px + 4 < W;
            const int xl = left ? px - 2 : 0, xr = right ? px + 4 : px;
            float m[6][8];
#pragma unroll
            for (int r = R0; r < R1; ++r) {
                int y = py - 2 + r;
                y = y < 0 ? -y : (y >= H ? 2 * H - 2 - y : y);
                const uint16_t *row = mo.row_at(y);
                const ushort2 l = mo.ld2(row, xl), e = mo.ld2(row, xr);
                const ushort4 c = mo.ld4(row, px);
                const unsigned short s[8] = {left ? l.x : c.z, left ? l.y : c.y, c.x, c.y, c.z, c.w, right ? e.x : c.z, right ? e.y : c.y};
#pragma unroll
                for (int k = 0; k < 8; ++k) m[r][k] = (mo.smp(s[k]) / mo.div) * 255.f;
            }
            d = demosaic_sites<LAP>(m);
        }
#pragma unroll
        for (int i = 0; i < 2 * PXT; ++i) (&pix[0][0])[i] = (&d.p[0][0])[i];
        // ---- stages: the two scene applies here, the rest in risp_serve_patch.h.  A scene stage's block is the (N,4) constants
        // of risp_serve_scene_finish
        for (int k = 0; k < a.n_ops; ++k) {
            const int op = a.ops[k];
            const float *p = a.params[k];
            if (op == RISP_OP_GAIN3_Q8) gain_q8_all<2 * PXT>(p + 4 * n, &pix[0][0]);
            else if (op == RISP_OP_TONE_REINHARD) reinhard_all(p[4 * n], p[4 * n + 1], &pix[0][0]);
            else stage<2 * PXT, WBQ>(op, p, n, &pix[0][0]);
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
#pragma unroll
        for (int p = 0; p < 2; ++p) store_bgr4(a.out, n, H, W, py + p, px, a.flip, a.reverse, pix[p]);
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

template <bool STATS>
void launch(int demosaic, bool wbq, dim3 grid, hipStream_t s, const SceneArgs &a) {
    with_form(demosaic, wbq, [&](auto kind_c, auto wbq_c) {
        hipLaunchKernelGGL((serve_scene_kernel<decltype(kind_c)::value, decltype(wbq_c)::value, STATS>), grid, dim3(256), 0, s, a);
    });
}

bool stat_ok(int stat) { return stat == RISP_SCENE_MEAN3 || stat == RISP_SCENE_MAX3 || stat == RISP_SCENE_LOGLUM; }

// the rules both pixel launches share; fills a (but for out / partials / stat / reverse)
int scene_args(const char *name, const uint16_t *raw, float divisor, int demosaic, int n_ops, const int *ops, const float *const *params,
               int N, int H, int W, int black_level, int cfa, SceneArgs &a, bool &wbq) {
    ArgRules r;
    r.out_here = false;
    r.gain_q8 = r.reinhard = true;
    a.out = nullptr;
    a.partials = nullptr;
    a.reverse = 0;
    a.stat = 0;
    return serve_args(name, r, a, wbq, raw, nullptr, divisor, demosaic, n_ops, ops, params, 0, nullptr, nullptr, N, H, W, black_level, cfa);
}

}  // namespace

extern "C" int risp_serve_scene_groups(int H, int W) {
    if (H < 4 || H % 2 || W < 4 || W % 4) return 0;
    const dim3 g = patch_grid(1, H, W);
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
    launch<true>(demosaic, wbq, patch_grid(N, H, W), (hipStream_t)stream, a);
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
    launch<false>(demosaic, wbq, patch_grid(N, H, W), (hipStream_t)stream, a);
    RISP_LAUNCH_CHECK("risp_serve_scene_u8");
    return 0;
}
