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
//            serve_classical_kernel evaluates a patch (risp_serve_patch.h) - written to LDS in the 0..255 domain (the median
//            stages the 8-bit codes).  Patches outside the image are skipped; after a barrier the ring positions outside the image copy the pixel at the
//            reflect-101 IMAGE coordinate from LDS (H >= 4, W >= 4 and a ring of 2: one reflection, and its source lies in the
//            same tile's image).
//   phase 2  after the barrier a thread denoises its own 2 x 4 patch row by row with the expression sequence of
//            bilateral4_kernel<1> / median3x4_kernel / fastnlm4_kernel<true>'s fast branch (risp_origin.hip), emits
//            q8(v) * (1 / 255) and runs the Q stages in registers.  The serving launch stores 12 bytes per row as serve_kernel
//            does.  The statistics launch stores no image: the thread's eight pixels are accumulated in row order, then
//            block_reduce3 (wavefront shuffles, one LDS step in wave order, no atomics) and one row of four floats per workgroup.  A thread of a ragged tile that owns no pixel holds 0 for a sum and -inf for a maximum.
//
// The patch, the stage loop with white-world's apply and the reduction are risp_serve_patch.h's; the tile phases around the
// denoiser are a second copy of serve_denoise_kernel's (risp_serve_denoise.hip).  One kernel template serves both launches;
// STATS is a compile-time switch.  With -ffp-contract=off a pixel's value has the bits of the composed route, so a
// maximum - which has no order - gives the composed route's constants and bytes; a sum taken in this order gives constants
// that differ in their last bits, and given the constants the bytes are the composed route's.  Black level and Bayer phase as
// in risp_serve_u8_cfa: the phase is a mirror of addresses; coordinates, reflection, parity and the tile grid live in the
// mirrored (RGGB) image.
#include <math.h>

#include "risp_serve_patch.h"

namespace {

using namespace risp_patch;

struct DenoiseSceneArgs : PatchArgs {
    uint8_t *out;               // (N,H,W,3); the serving launch
    float *partials;            // (N,G,4); the statistics launch
    int reverse;                // store R, G, B instead of B, G, R
    int stat;                   // RISP_SCENE_MEAN3 | RISP_SCENE_MAX3; the statistics launch
    const float *da, *db;       // bilateral: sigma_color, sigma_space (N); non-local means: decay (N), -
};

constexpr int RING_Y = 2, RING_X = 4;                  // LDS rows above / columns left of the tile (whole patches)
constexpr int LW = TILE_W + 2 * RING_X, LH = TILE_H + 2 * RING_Y, LPLANE = LW * LH;   // 72 x 36 per plane
constexpr int PCOLS = LW / PXT, PROWS = LH / 2;        // 18 x 18 patches
constexpr int REACH = 2;                               // ring positions a denoiser may read (non-local means: 1 + 1)
// KIND: RISP_DEMOSAIC_*, DEN: RISP_DENOISE_*.  Every coordinate is one of the mirrored image, which is RGGB.  STATS: no image is
// stored; the values behind the last stage are reduced over the workgroup's tile and one row of four floats goes to
// partials[(n * G + tile) * 4 ..].  A scene stage's block is the (N,4) constants of risp_serve_scene_finish
template <int KIND, int DEN, bool WBQ, bool STATS>
__global__ __launch_bounds__(256) void serve_denoise_scene_kernel(const DenoiseSceneArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[3 * LPLANE];
    const int H = a.H, W = a.W;
    int bxi, byi, bzi;
    xcd_tile(bxi, byi, bzi);
    const int n = bzi, x0 = bxi * TILE_W, y0 = byi * TILE_H;
    const int flip = a.flip;
    const Mosaic mo(a, n);

    // ---- phase 1: demosaic and the stages in front of the denoiser for every patch of the LDS image that lies in the image
#pragma unroll 1
    for (int t = threadIdx.x; t < PROWS * PCOLS; t += 256) {
        const int pr = t / PCOLS, pc = t - pr * PCOLS;
        const int px = x0 - RING_X + pc * PXT, py = y0 - RING_Y + pr * 2;
        if (px < 0 || px >= W || py < 0 || py >= H) continue;      // W % 4 == 0, H % 2 == 0: a patch is in or out as a whole
        const Patch d = mo.patch<KIND>(px, py);
        f3 pix[2][PXT];                                            // (the patch is copied into the kernel's own array: risp_serve_patch.h)
#pragma unroll
        for (int i = 0; i < 2 * PXT; ++i) (&pix[0][0])[i] = (&d.p[0][0])[i];
        run_stages<2 * PXT, WBQ, true>(a, 0, a.n_pre, n, &pix[0][0]);
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

        run_stages<PXT, WBQ, true>(a, a.n_pre, a.n_ops, n, o);

        if constexpr (STATS) {
            // the row's four pixels in order: with the loop over p the thread's eight pixels in row order
#pragma unroll
            for (int i = 0; i < PXT; ++i) {
                if (smax) { acc[0] = fmaxf(acc[0], o[i].b); acc[1] = fmaxf(acc[1], o[i].g); acc[2] = fmaxf(acc[2], o[i].r); }
                else { acc[0] += o[i].b; acc[1] += o[i].g; acc[2] += o[i].r; }
            }
            continue;
        }
        store_bgr4(a.out, n, H, W, py + p, px, flip, a.reverse, o);
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

// the rules both launches share; fills a (but for out / partials / stat / reverse)
int denoise_scene_args(const char *name, const uint16_t *raw, float divisor, int demosaic, int n_pre, const int *pre_ops,
                       const float *const *pre_params, int denoise, int window, int search, const float *den_a, const float *den_b,
                       int n_post, const int *post_ops, const float *const *post_params, int N, int H, int W, int black_level, int cfa,
                       DenoiseSceneArgs &a, bool &wbq) {
    if (int e = denoiser_args(name, denoise, window, search, den_a, den_b)) return e;
    ArgRules r;
    r.out_here = false;
    r.split = true;
    r.gain_q8 = true;
    a.out = nullptr;
    a.partials = nullptr;
    a.reverse = 0;
    a.stat = 0;
    a.da = den_a;
    a.db = den_b;
    return serve_args(name, r, a, wbq, raw, nullptr, divisor, demosaic, n_pre, pre_ops, pre_params, n_post, post_ops, post_params, N, H, W,
                      black_level, cfa);
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
    launch<true>(demosaic, denoise, wbq, patch_grid(N, H, W), (hipStream_t)stream, a);
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
    launch<false>(demosaic, denoise, wbq, patch_grid(N, H, W), (hipStream_t)stream, a);
    RISP_LAUNCH_CHECK("risp_serve_denoise_scene_u8");
    return 0;
}
