// Serving path for the classical pipelines: a 16-bit Bayer frame in, a packed 8-bit image out, ONE launch.
//
//     max(sample - black, 0) / divisor -> nearest | bilinear | Malvar-He-Cutler demosaic -> stages -> clip(v * 255) truncated
//
// where a stage is an element-wise operator of risp_ops.h or one of the two tone curves that need no whole-image quantity
// (Crysis, Filmic).  risp_serve_u8 takes the nearest demosaic only; every other classical pipeline went through
// risp_raw_crop[_cfa] -> risp_origin_demosaic -> a chain launch per element-wise run -> two launches per tone curve ->
// risp_quantise_u8[_flip], every stage output in fp32 planes.  Each of these operators is a pure function of a 5 x 5 mosaic
// neighbourhood, or of one pixel and per-image scalars, so they join a launch shaped like serve_kernel (risp_serve.hip): a
// thread owns a 2 x 4 pixel patch and loads the mosaic rows py-2 .. py+3, columns px-2 .. px+5 itself - no LDS, no barrier.
//
// The arithmetic is that of the composed route restated in the same order.  The routes that serve more than this one (a scene
// stage, a conditional head, a denoiser) evaluate the same patch, so the helpers, the two demosaics, the stage loop, the store
// and the host rules live in risp_serve_patch.h; this file owns its loads (below), the NV12 epilogue and its four entry points.
// With -ffp-contract=off the bytes are the composed route's (tests/test_gpu_serve_classical.py, torch.equal).  Black level and Bayer phase as in
// risp_serve_u8_cfa: the phase is a mirror of addresses, coordinates, reflection and parity live in the mirrored (RGGB) image.
//
// MIPI-packed RAW10 / RAW12 in (risp_serve_classical_packed): a template parameter PACK = 0 / 10 / 12 replaces row_at / ld2 / ld4
// by the loads of risp_rawpack.h, as in serve_kernel; the PACK = 0 instantiations do not see it.
//
// Lens-shading correction in (risp_serve_classical_shaded): a template parameter SHADE replaces smp alone - the float that enters
// smp(s) / div is the shaded sample of risp_shade.h - on uint16 frames (PACK == 0).  The map belongs to the sensor, the kernel
// works in mirrored coordinates: a row's eight columns px-2 .. px+5 are the eight sensor columns b .. b+7 (b = px - 2, or
// W - 6 - px read backwards), b = 2 mod 4, so they fall into the aligned groups [b, b+1], [b+2, b+5], [b+6, b+7], each inside one
// cell.  Per row and group the two planes of the node columns beside it are interpolated down the cell (a group in the cell of
// the one before it reuses them: at cell >= 8 two of three do), then each sample interpolates across.  A reflected sample
// carries the gain of the place it was read from.  The existing instantiations do not see the parameter.
#include "risp_nv12.h"
#include "risp_rawpack.h"
#include "risp_serve_patch.h"
#include "risp_shade.h"

namespace {

using namespace risp_patch;

struct ClassicalArgs : PatchArgs {
    uint8_t *out;               // (N,H,W,3)
    int reverse;                // store R, G, B instead of B, G, R
};

// risp_serve_classical_nv12: the same block first, then the matrix by value (`reverse` is not read)
struct ClassicalNv12Args : ClassicalArgs {
    risp_nv12::Coef yuv;
};
// risp_serve_classical_packed: that block (`raw` holds the byte pointer; BGR out reads `reverse`, NV12 out `yuv`), then the pitch
struct ClassicalPackedArgs : ClassicalNv12Args {
    int stride;                 // bytes from a packed row to the next
};
// risp_serve_classical_shaded: the NV12 block (BGR out reads `reverse`, NV12 out `yuv`), then the map
struct ClassicalShadedArgs : ClassicalNv12Args {
    const uint16_t *gains;      // (GH,GW,4) Q12
    int cell_log2, GW;
};
template <bool NV12, int PACK = 0, bool SHADE = false> struct classical_args { using type = ClassicalPackedArgs; };
template <> struct classical_args<false, 0, false> { using type = ClassicalArgs; };
template <> struct classical_args<true, 0, false> { using type = ClassicalNv12Args; };
template <bool NV12> struct classical_args<NV12, 0, true> { using type = ClassicalShadedArgs; };

// KIND: RISP_DEMOSAIC_*.  px, py and every coordinate derived from them are those of the mirrored image, which is RGGB; only
// row_at / ld2 / ld4 and the store know where the samples really are.  The loads and the window fill are this kernel's own, not
// risp_patch::Mosaic's: PACK replaces the three loads and SHADE gives every sample a gain, which the uint16 loader knows nothing
// of.  NV12: the store epilogue alone differs - the patch's eight codes leave as two Y dwords and one UV dword of a (3H/2, W)
// image (risp_nv12.h)
template <int KIND, bool WBQ, bool NV12 = false, int PACK = 0, bool SHADE = false>
__global__ __launch_bounds__(256) void serve_classical_kernel(const typename classical_args<NV12, PACK, SHADE>::type a) {
    static_assert(!SHADE || PACK == 0, "the fused shading load reads uint16 frames");
    const int H = a.H, W = a.W;
    int bxi, byi, bzi;
    xcd_tile(bxi, byi, bzi);
    const int n = bzi;
    const int px = (bxi * STX + (int)(threadIdx.x % STX)) * 4, py = (byi * STY + (int)(threadIdx.x / STX)) * 2;
    if (px >= W || py >= H) return;                     // W % 4 == 0, H % 2 == 0: a patch is in or out as a whole
    const uint16_t *bay = a.raw + (size_t)n * H * W;
    const float div = a.divisor;
    const int black = a.black, flip = a.flip;
    f3 pix[2][PXT];
    auto row_at = [&](int y) {
        if constexpr (PACK != 0)
            return reinterpret_cast<const uint8_t *>(a.raw) + ((size_t)n * H + (flip & 2 ? H - 1 - y : y)) * a.stride;
        else return bay + (size_t)(flip & 2 ? H - 1 - y : y) * W;
    };
    auto ld2 = [&](auto *row, int x) {                  // samples x, x + 1 of the mirrored row (x even)
        const bool fx = flip & 1;
        ushort2 v;
        if constexpr (PACK != 0) v = risp_rawpack::ld2<PACK>(row, fx ? W - 2 - x : x);
        else v = *reinterpret_cast<const ushort2 *>(row + (fx ? W - 2 - x : x));
        return fx ? ushort2{v.y, v.x} : v;
    };
    auto ld4 = [&](auto *row, int x) {                  // x .. x + 3 (x % 4 == 0)
        const bool fx = flip & 1;
        ushort4 v;
        if constexpr (PACK != 0) v = risp_rawpack::ld4<PACK>(row, fx ? W - 4 - x : x);
        else v = *reinterpret_cast<const ushort4 *>(row + (fx ? W - 4 - x : x));
        return fx ? ushort4{v.w, v.z, v.y, v.x} : v;
    };
    // g: the sample's Q12 gain (SHADE only)
    auto smp = [&](unsigned short s, [[maybe_unused]] unsigned g) {
        if constexpr (SHADE) return (float)risp_shade::shade(s, (unsigned)black, g);
        else return (float)((int)s > black ? (int)s - black : 0);
    };
    // SHADE: g[t] = the gain at mirrored row y (already reflected into the image), mirrored column px - 2 + t.  The centre four
    // always; the pairs left / right of them only with `lo` / `hi` (false at a border patch, and for the nearest demosaic, which
    // has no stencil): no node is read for a column outside the image, and such a g[t] is not used
    [[maybe_unused]] auto row_gains = [&](int y, bool lo, bool hi, unsigned *g) {
        if constexpr (SHADE) {
            const int k = a.cell_log2;
            const bool fx = flip & 1;
            const risp_shade::MapRow map(a.gains, a.GW, k, flip & 2 ? H - 1 - y : y);
            const int b = fx ? W - 6 - px : px - 2;     // sensor column of gs[0]
            const bool va = fx ? hi : lo, vc = fx ? lo : hi;
            unsigned gs[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // in sensor order
            const int jb = (b + 2) >> k;
            const uint2 nl = map.node(jb), nr = map.node(jb + 1);
            const risp_shade::Cell cb{nl, nr};
            const unsigned fb = risp_shade::cell_fx(b + 2, k);
            gs[2] = cb.gain<0>(fb, k), gs[3] = cb.gain<1>(fb + 1, k), gs[4] = cb.gain<0>(fb + 2, k), gs[5] = cb.gain<1>(fb + 3, k);
            if constexpr (KIND != RISP_DEMOSAIC_NEAREST) {
                if (va) {
                    const int ja = b >> k;
                    risp_shade::Cell ca = cb;
                    if (ja != jb) ca = risp_shade::Cell{map.node(ja), nl};       // the cell before: ja + 1 == jb
                    const unsigned fa = risp_shade::cell_fx(b, k);
                    gs[0] = ca.gain<0>(fa, k), gs[1] = ca.gain<1>(fa + 1, k);
                }
                if (vc) {
                    const int jc = (b + 6) >> k;
                    risp_shade::Cell cc = cb;
                    if (jc != jb) cc = risp_shade::Cell{nr, map.node(jc + 1)};   // the cell behind: jc == jb + 1
                    const unsigned fc = risp_shade::cell_fx(b + 6, k);
                    gs[6] = cc.gain<0>(fc, k), gs[7] = cc.gain<1>(fc + 1, k);
                }
            }
#pragma unroll
            for (int t = 0; t < 8; ++t) g[t] = fx ? gs[7 - t] : gs[t];
        }
    };

    if constexpr (KIND == RISP_DEMOSAIC_NEAREST) {
        const ushort4 r0 = ld4(row_at(py), px), r1 = ld4(row_at(py + 1), px);
        [[maybe_unused]] unsigned g0[8] = {}, g1[8] = {};                   // columns px .. px + 3 are [2] .. [5]
        row_gains(py, false, false, g0);
        row_gains(py + 1, false, false, g1);
        const Patch d = nearest_patch({smp(r0.x, g0[2]) / div, smp(r0.y, g0[3]) / div, smp(r0.z, g0[4]) / div, smp(r0.w, g0[5]) / div},
                                      {smp(r1.x, g1[2]) / div, smp(r1.y, g1[3]) / div, smp(r1.z, g1[4]) / div, smp(r1.w, g1[5]) / div});
#pragma unroll
        for (int i = 0; i < 2 * PXT; ++i) (&pix[0][0])[i] = (&d.p[0][0])[i];
    } else {
        // ---- m: risp_patch::Window's, filled as Mosaic::window fills it
        constexpr bool LAP = KIND == RISP_DEMOSAIC_LAPLACIAN;
        constexpr int R0 = LAP ? 0 : 1, R1 = LAP ? 6 : 5;
        const bool left = px > 0, right = px + 4 < W;
        const int xl = left ? px - 2 : 0, xr = right ? px + 4 : px;
        float m[6][8];
#pragma unroll
        for (int r = R0; r < R1; ++r) {
            int y = py - 2 + r;
            y = y < 0 ? -y : (y >= H ? 2 * H - 2 - y : y);
            const auto *row = row_at(y);
            const ushort2 l = ld2(row, xl), e = ld2(row, xr);
            const ushort4 c = ld4(row, px);
            const unsigned short s[8] = {left ? l.x : c.z, left ? l.y : c.y, c.x, c.y, c.z, c.w, right ? e.x : c.z, right ? e.y : c.y};
            [[maybe_unused]] unsigned gm[8] = {}, g[8] = {};
            if constexpr (SHADE) {
                row_gains(y, left, right, gm);
                const unsigned gr[8] = {left ? gm[0] : gm[4], left ? gm[1] : gm[3], gm[2], gm[3], gm[4], gm[5], right ? gm[6] : gm[4],
                                        right ? gm[7] : gm[3]};
#pragma unroll
                for (int k = 0; k < 8; ++k) g[k] = gr[k];
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) m[r][k] = (smp(s[k], g[k]) / div) * 255.f; // risp_raw_crop_cfa's expression, x 255 on load
        }
        const Patch d = demosaic_sites<LAP>(m);
#pragma unroll
        for (int i = 0; i < 2 * PXT; ++i) (&pix[0][0])[i] = (&d.p[0][0])[i];
    }

    run_stages<2 * PXT, WBQ>(a, 0, a.n_ops, n, &pix[0][0]);

    if constexpr (NV12) {
        // ---- the codes the BGR store would write, as 4:2:0: three dwords instead of six
        unsigned cr[2][PXT], cg[2][PXT], cb[2][PXT];
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int c = 0; c < PXT; ++c) cb[p][c] = u8(pix[p][c].b), cg[p][c] = u8(pix[p][c].g), cr[p][c] = u8(pix[p][c].r);
        risp_nv12::nv12_store_patch(a.out + (size_t)n * (H + H / 2) * W, a.yuv, cr, cg, cb, H, W, py, px, flip);
        return;
    }
#pragma unroll
    for (int p = 0; p < 2; ++p) store_bgr4(a.out, n, H, W, py + p, px, flip, a.reverse, pix[p]);
}

// the rules the entry points share; `raw_align` 1: packed bytes
int classical_args_fill(const char *name, ClassicalArgs &a, bool &wbq, const void *raw, float divisor, int demosaic, int n_ops, const int *ops,
                   const float *const *params, uint8_t *out, int reverse_channels, int N, int H, int W, int black_level, int cfa,
                   int raw_align = 8) {
    ArgRules r;
    r.raw_align = raw_align;
    if (int e = serve_args(name, r, a, wbq, raw, out, divisor, demosaic, n_ops, ops, params, 0, nullptr, nullptr, N, H, W, black_level, cfa))
        return e;
    a.out = out;
    a.reverse = reverse_channels ? 1 : 0;
    return 0;
}

template <bool NV12, int PACK = 0, bool SHADE = false, class Args>
void launch_classical(int demosaic, bool wbq, hipStream_t s, const Args &a) {
    with_form(demosaic, wbq, [&](auto kind_c, auto wbq_c) {
        hipLaunchKernelGGL((serve_classical_kernel<decltype(kind_c)::value, decltype(wbq_c)::value, NV12, PACK, SHADE>),
                           patch_grid(a.N, a.H, a.W), dim3(256), 0, s, a);
    });
}

}  // namespace

extern "C" int risp_serve_classical_u8(const uint16_t *raw, float divisor, int demosaic, int n_ops, const int *ops,
                                       const float *const *params, uint8_t *out, int reverse_channels, int N, int H, int W,
                                       int black_level, int cfa, void *stream) {
    ClassicalArgs a;
    bool wbq = false;
    if (int err = classical_args_fill("risp_serve_classical_u8", a, wbq, raw, divisor, demosaic, n_ops, ops, params, out,
                                      reverse_channels, N, H, W, black_level, cfa))
        return err;
    launch_classical<false>(demosaic, wbq, (hipStream_t)stream, a);
    RISP_LAUNCH_CHECK("risp_serve_classical_u8");
    return 0;
}

extern "C" int risp_serve_classical_nv12(const uint16_t *raw, float divisor, int demosaic, int n_ops, const int *ops,
                                         const float *const *params, uint8_t *out, const int32_t coef[12], int N, int H, int W,
                                         int black_level, int cfa, void *stream) {
    ClassicalNv12Args a;
    bool wbq = false;
    if (int err = classical_args_fill("risp_serve_classical_nv12", a, wbq, raw, divisor, demosaic, n_ops, ops, params, out, 0, N, H,
                                      W, black_level, cfa))
        return err;
    if (int err = risp_nv12::nv12_check("risp_serve_classical_nv12", coef, a.yuv)) return err;
    launch_classical<true>(demosaic, wbq, (hipStream_t)stream, a);
    RISP_LAUNCH_CHECK("risp_serve_classical_nv12");
    return 0;
}

extern "C" int risp_serve_classical_packed(const uint8_t *raw, int bits, int stride, float divisor, int demosaic, int n_ops,
                                           const int *ops, const float *const *params, uint8_t *out, int reverse_channels,
                                           const int32_t *coef, int N, int H, int W, int black_level, int cfa, void *stream) {
    const char *name = "risp_serve_classical_packed";
    ClassicalPackedArgs a;
    bool wbq = false;
    if (int err = classical_args_fill(name, a, wbq, raw, divisor, demosaic, n_ops, ops, params, out,
                                      coef ? 0 : reverse_channels, N, H, W, black_level, cfa, 1))
        return err;
    if (int err = risp_rawpack::rawpack_check(name, bits, W, stride)) return err;
    for (int i = 0; i < 12; ++i) a.yuv.k[i] = 0;
    if (coef)
        if (int err = risp_nv12::nv12_check(name, coef, a.yuv)) return err;
    a.stride = stride;
    hipStream_t s = (hipStream_t)stream;
    if (bits == 10) {
        if (coef) launch_classical<true, 10>(demosaic, wbq, s, a);
        else launch_classical<false, 10>(demosaic, wbq, s, a);
    } else {
        if (coef) launch_classical<true, 12>(demosaic, wbq, s, a);
        else launch_classical<false, 12>(demosaic, wbq, s, a);
    }
    RISP_LAUNCH_CHECK(name);
    return 0;
}

extern "C" int risp_serve_classical_shaded(const uint16_t *raw, float divisor, int demosaic, int n_ops, const int *ops,
                                           const float *const *params, uint8_t *out, int reverse_channels, const int32_t *coef,
                                           const uint16_t *gains, int cell_log2, int GH, int GW, int N, int H, int W,
                                           int black_level, int cfa, void *stream) {
    const char *name = "risp_serve_classical_shaded";
    ClassicalShadedArgs a;
    bool wbq = false;
    if (int err = classical_args_fill(name, a, wbq, raw, divisor, demosaic, n_ops, ops, params, out, coef ? 0 : reverse_channels, N, H,
                                      W, black_level, cfa))
        return err;
    if (int err = risp_shade::shade_check(name, gains, cell_log2, GH, GW, black_level, H, W)) return err;
    for (int i = 0; i < 12; ++i) a.yuv.k[i] = 0;
    if (coef)
        if (int err = risp_nv12::nv12_check(name, coef, a.yuv)) return err;
    a.gains = gains;
    a.cell_log2 = cell_log2;
    a.GW = GW;
    hipStream_t s = (hipStream_t)stream;
    if (coef) launch_classical<true, 0, true>(demosaic, wbq, s, a);
    else launch_classical<false, 0, true>(demosaic, wbq, s, a);
    RISP_LAUNCH_CHECK(name);
    return 0;
}
