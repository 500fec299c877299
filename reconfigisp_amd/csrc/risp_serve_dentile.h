// The tile routes behind risp_serve_u8 - a stencil between two stage lists - stated once: what risp_serve_denoise.hip,
// risp_serve_denoise_scene.hip and risp_serve_median.hip share on top of risp_serve_patch.h.
//
// A workgroup owns a 64 x 32 pixel tile and works in two phases around one LDS image of the tile and a ring of whole 2 x 4 patches:
//
//   phase 1  front_patches: the patches that cover the LDS image - demosaic and the front stages exactly as
//            serve_classical_kernel evaluates a patch (risp_serve_patch.h: the same loads, reflection inside the mosaic,
//            per-site expressions, 8-bit rounding, tone curves) - handed to the route's store (fp32 planes here, packed codes in
//            risp_serve_median.hip).  Patches outside the image are skipped; after a barrier the ring positions outside the
//            image that a stencil can reach (border_tile) copy the pixel at the reflect-101 IMAGE coordinate
//            (reflect101) from LDS: one reflection, and its source lies in the same tile's image - the full pipeline at that
//            coordinate, which is what the composed route's stage_tile4 reads from the fp32 planes.
//   phase 2  after the barrier a thread takes its own 2 x 4 patch row by row through the stencil, runs the stages behind it in
//            registers and stores 12 bytes per row as serve_kernel does.
//
// serve_denoise_kernel is the ONE kernel behind risp_serve_denoise_u8 (<.., false, false>), risp_serve_denoise_scene_u8
// (<.., true, false>) and risp_serve_denoise_stats (<.., true, true>): the LDS image is 36 x 72 pixels (a ring of 2 rows / 4 columns,
// three fp32 planes, 31104 bytes; 324 patches on 256 threads: the ring is 27 % more phase-1 work) in the 0..255 domain (value
// x 255: the denoisers' in_scale; the median stages the 8-bit codes, as stage_tile4<true> does), and the stencil is one of
// bilateral_row / median3_row / fastnlm_row - the expression sequences of bilateral4_kernel<1> / median3x4_kernel /
// fastnlm4_kernel<true>'s fast branch (risp_origin.hip), each emitting q8(v) * (1 / 255).  With -ffp-contract=off the bytes are the
// composed route's; that depends on the sequences as they stand: association, builtins and the order of taps.  The statistics
// form stores no image: the thread's eight pixels are accumulated in row order, then block_reduce3 and one row of four floats
// per workgroup; a thread of a ragged tile that owns no pixel holds 0 for a sum and -inf for a maximum.
#pragma once
#include <math.h>

#include "risp_serve_patch.h"

namespace risp_patch {

// ---- what the tile routes share
// reflect-101 over one reflection
__device__ __forceinline__ int reflect101(int v, int n) { return v < 0 ? -v : (v >= n ? 2 * n - 2 - v : v); }

// whether the tile at (x0, y0) has ring positions outside the image within `reach`: a workgroup-uniform condition
__device__ __forceinline__ bool border_tile(int x0, int y0, int H, int W, int reach) {
    return y0 == 0 || x0 == 0 || y0 + TILE_H + reach > H || x0 + TILE_W + reach > W;
}

// phase 1: demosaic and the stages in front of the stencil for every patch of the LDS image (PROWS x PCOLS patches, RING_Y rows
// above and RING_X columns left of the tile at (x0, y0)) that lies in the image; store(pr, pc, pix) takes a finished patch
template <int KIND, bool WBQ, bool GAIN, int RING_X, int RING_Y, int PCOLS, int PROWS, class Store>
__device__ __forceinline__ void front_patches(const PatchArgs &a, const Mosaic &mo, int n, int x0, int y0, Store store) {
#pragma unroll 1
    for (int t = threadIdx.x; t < PROWS * PCOLS; t += 256) {
        const int pr = t / PCOLS, pc = t - pr * PCOLS;
        const int px = x0 - RING_X + pc * PXT, py = y0 - RING_Y + pr * 2;
        if (px < 0 || px >= a.W || py < 0 || py >= a.H) continue;  // W % 4 == 0, H % 2 == 0: a patch is in or out as a whole
        const Patch d = mo.patch<KIND>(px, py);
        f3 pix[2][PXT];                                            // (the patch is copied into the walk's own array: risp_serve_patch.h)
#pragma unroll
        for (int i = 0; i < 2 * PXT; ++i) (&pix[0][0])[i] = (&d.p[0][0])[i];
        run_stages<2 * PXT, WBQ, GAIN>(a, 0, a.n_pre, n, &pix[0][0]);
        store(pr, pc, pix);
    }
}

// ---- the 3 x 3 / block 3 search 3 denoisers
struct DenoiseTileArgs : PatchArgs {
    uint8_t *out;               // (N,H,W,3); the serving launches
    float *partials;            // (N,G,4); the statistics launch
    int reverse;                // store R, G, B instead of B, G, R
    int stat;                   // RISP_SCENE_MEAN3 | RISP_SCENE_MAX3; the statistics launch
    const float *da, *db;       // bilateral: sigma_color, sigma_space (N); non-local means: decay (N), -
};

constexpr int RING_Y = 2, RING_X = 4;                  // LDS rows above / columns left of the tile (whole patches)
constexpr int LW = TILE_W + 2 * RING_X, LH = TILE_H + 2 * RING_Y, LPLANE = LW * LH;   // 72 x 36 per plane
constexpr int PCOLS = LW / PXT, PROWS = LH / 2;        // 18 x 18 patches
constexpr int REACH = 2;                               // ring positions a denoiser may read (non-local means: 1 + 1)

// A denoiser takes a row of the LDS image to four pixels.  own: the first of the four in plane 0 (16-byte aligned)
// bilateral4_kernel<1>, every image at radius 1
__device__ __forceinline__ void bilateral_row(const float *own, float sig_c, float sig_s, f3 (&o)[PXT]) {
    const float inv255 = 1.f / 255.f;
    const float ks = -1.f / (2.f * sig_s * sig_s), kc = -1.f / (2.f * sig_c * sig_c);
    const float ks2 = ks * 1.4426950408889634f, kc2 = kc * 1.4426950408889634f;
#pragma unroll
    for (int i = 0; i < PXT; ++i) {
        const float *ctr = own + i;
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
}

// median3x4_kernel: the six window columns sorted once, a pixel's median from three of them
__device__ __forceinline__ void median3_row(const float *own, f3 (&o)[PXT]) {
    const float inv255 = 1.f / 255.f;
    float res[3][PXT];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float *top = own + c * LPLANE - LW - 1;              // the row above, image columns px-1 .. px+4
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
}

// fastnlm4_kernel<true>, block 3 and search 3.  v[row][col][ch]: image rows y-2 .. y+2, columns px-2 .. px+5
__device__ __forceinline__ void fastnlm_row(const float *own, float dec, f3 (&o)[PXT]) {
    const float inv255 = 1.f / 255.f;
    const float scale = -1.f / (3.f * (float)(3 * 3) * dec * dec);
    float v[5][8][3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int rr = 0; rr < 5; ++rr) {
            const float *row = own + c * LPLANE + (rr - 2) * LW;
            const float2 l2 = *reinterpret_cast<const float2 *>(row - 2), e2 = *reinterpret_cast<const float2 *>(row + 4);
            const float4 d = *reinterpret_cast<const float4 *>(row);
            v[rr][0][c] = l2.x; v[rr][1][c] = l2.y; v[rr][2][c] = d.x; v[rr][3][c] = d.y;
            v[rr][4][c] = d.z; v[rr][5][c] = d.w; v[rr][6][c] = e2.x; v[rr][7][c] = e2.y;
        }
    float nb[4] = {0.f, 0.f, 0.f, 0.f}, ng[4] = {0.f, 0.f, 0.f, 0.f}, nr[4] = {0.f, 0.f, 0.f, 0.f}, den[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int sy = -1; sy <= 1; ++sy)
#pragma unroll
        for (int sx = -1; sx <= 1; ++sx) {
            float e[3][6];                         // q = (y + qy, px + qx), qy = -1..1, qx = -1..4
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

// KIND: RISP_DEMOSAIC_*, DEN: RISP_DENOISE_*.  Every coordinate is one of the mirrored image, which is RGGB.  GAIN:
// RISP_OP_GAIN3_Q8 is served among the stages; a scene stage's block is the (N,4) constants of risp_serve_scene_finish.  STATS: no
// image is stored; the values behind the last stage are reduced over the workgroup's tile and one row of four floats goes to
// partials[(n * G + tile) * 4 ..]
template <int KIND, int DEN, bool WBQ, bool GAIN, bool STATS>
__global__ __launch_bounds__(256) void serve_denoise_kernel(const DenoiseTileArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[3 * LPLANE];
    const int H = a.H, W = a.W;
    int bxi, byi, bzi;
    xcd_tile(bxi, byi, bzi);
    const int n = bzi, x0 = bxi * TILE_W, y0 = byi * TILE_H;
    const int flip = a.flip;
    const Mosaic mo(a, n);

    // ---- phase 1, stored in the denoisers' domain: value x in_scale (255); the median works on the 8-bit codes
    front_patches<KIND, WBQ, GAIN, RING_X, RING_Y, PCOLS, PROWS>(a, mo, n, x0, y0, [&](int pr, int pc, const f3 (&pix)[2][PXT]) {
        auto conv = [&](float v) { v *= 255.f; return DEN == RISP_DENOISE_MEDIAN ? q8(v) : v; };
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            float *dst = lds + (pr * 2 + p) * LW + pc * PXT;
            *reinterpret_cast<float4 *>(dst) = make_float4(conv(pix[p][0].b), conv(pix[p][1].b), conv(pix[p][2].b), conv(pix[p][3].b));
            *reinterpret_cast<float4 *>(dst + LPLANE) = make_float4(conv(pix[p][0].g), conv(pix[p][1].g), conv(pix[p][2].g), conv(pix[p][3].g));
            *reinterpret_cast<float4 *>(dst + 2 * LPLANE) = make_float4(conv(pix[p][0].r), conv(pix[p][1].r), conv(pix[p][2].r), conv(pix[p][3].r));
        }
    });
    __syncthreads();

    // ---- ring positions outside the image: the pixel at the reflect-101 image coordinate (H >= 4, W >= 4 and a ring of 2: one
    // reflection, and its source lies in the same tile's image).  Only tiles on the image border have any (the barrier inside
    // is reached by all or by none)
    if (border_tile(x0, y0, H, W, REACH)) {
        for (int idx = threadIdx.x; idx < LPLANE; idx += 256) {
            const int r = idx / LW, c = idx - r * LW;
            const int gy = y0 - RING_Y + r, gx = x0 - RING_X + c;
            if (gy < -REACH || gy >= H + REACH || gx < -REACH || gx >= W + REACH) continue;
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) continue;
            const int src = (reflect101(gy, H) - y0 + RING_Y) * LW + reflect101(gx, W) - x0 + RING_X;
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
        const float *own = lds + (ly + p + RING_Y) * LW + lx + RING_X;
        if constexpr (DEN == RISP_DENOISE_BILATERAL) bilateral_row(own, a.da[n], a.db[n], o);
        else if constexpr (DEN == RISP_DENOISE_MEDIAN) median3_row(own, o);
        else fastnlm_row(own, a.da[n], o);

        run_stages<PXT, WBQ, GAIN>(a, a.n_pre, a.n_ops, n, o);

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

// ---- host side
// calls f(std::integral_constant<int, DEN>) for the denoiser (as denoiser_args passed it)
template <class F>
inline void with_denoiser(int denoise, F &&f) {
    if (denoise == RISP_DENOISE_BILATERAL) f(std::integral_constant<int, RISP_DENOISE_BILATERAL>{});
    else if (denoise == RISP_DENOISE_MEDIAN) f(std::integral_constant<int, RISP_DENOISE_MEDIAN>{});
    else f(std::integral_constant<int, RISP_DENOISE_FASTNLM>{});
}

// the launch of serve_denoise_kernel<.., GAIN, STATS> every entry point ends in
template <bool GAIN, bool STATS>
inline void launch_denoise(int demosaic, int denoise, bool wbq, hipStream_t s, const DenoiseTileArgs &a) {
    with_form(demosaic, wbq, [&](auto kind_c, auto wbq_c) {
        with_denoiser(denoise, [&](auto den_c) {
            hipLaunchKernelGGL((serve_denoise_kernel<decltype(kind_c)::value, decltype(den_c)::value, decltype(wbq_c)::value, GAIN, STATS>),
                               patch_grid(a.N, a.H, a.W), dim3(256), 0, s, a);
        });
    });
}

}  // namespace risp_patch
