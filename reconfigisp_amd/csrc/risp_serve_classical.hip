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
// The arithmetic is that of the composed route restated in the same order (its device code lives in anonymous namespaces and
// stays as measured): origin_demosaic_kernel's per-site expressions and 8-bit rounding, tonemap_prepare_kernel's constants and
// tonemap_kernel's pixel expression with both scales 255 (risp_origin.hip), apply_op for the rest.  With -ffp-contract=off the
// bytes are the composed route's (tests/test_gpu_serve_classical.py, torch.equal).  Black level and Bayer phase as in
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
#include "risp_common.h"
#include "risp_nv12.h"
#include "risp_ops.h"
#include "risp_rawpack.h"
#include "risp_shade.h"

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

struct ClassicalArgs {
    const uint16_t *raw;        // (N,H,W) mosaic of the sensor
    uint8_t *out;               // (N,H,W,3)
    float divisor;
    int n_ops, N, H, W;
    int reverse;                // store R, G, B instead of B, G, R
    int black;                  // subtracted from every sample in integers, clamped at 0
    int flip;                   // RISP_CFA_*: bit 0 mirrors x, bit 1 mirrors y
    int ops[RISP_MAX_CHAIN];
    const float *params[RISP_MAX_CHAIN];
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

// KIND: RISP_DEMOSAIC_*.  px, py and every coordinate derived from them are those of the mirrored image, which is RGGB; only
// row_at / ld2 / ld4 and the store know where the samples really are.  NV12: the store epilogue alone differs - the patch's
// eight codes leave as two Y dwords and one UV dword of a (3H/2, W) image (risp_nv12.h)
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
        // ---- no stencil: the patch's own two quads, in the [0,1] domain (serve_kernel's branch)
        const ushort4 r0 = ld4(row_at(py), px), r1 = ld4(row_at(py + 1), px);
        [[maybe_unused]] unsigned g0[8] = {}, g1[8] = {};                   // columns px .. px + 3 are [2] .. [5]
        row_gains(py, false, false, g0);
        row_gains(py + 1, false, false, g1);
        const float R0 = smp(r0.x, g0[2]) / div, G10 = smp(r0.y, g0[3]) / div, R1 = smp(r0.z, g0[4]) / div, G11 = smp(r0.w, g0[5]) / div;
        const float G20 = smp(r1.x, g1[2]) / div, B0 = smp(r1.y, g1[3]) / div, G21 = smp(r1.z, g1[4]) / div, B1 = smp(r1.w, g1[5]) / div;
        pix[0][0] = pix[0][1] = {B0, G10, R0};
        pix[0][2] = pix[0][3] = {B1, G11, R1};
        pix[1][0] = pix[1][1] = {B0, G20, R0};
        pix[1][2] = pix[1][3] = {B1, G21, R1};
    } else {
        // ---- m[r][c]: mosaic row py - 2 + r, column px - 2 + c in the 0..255 domain, reflect-101 over radius 2 (H, W >= 4: one
        // reflection reaches every tap).  Row -2 / -1 reflect to 2 / 1, row H / H + 1 to H - 2 / H - 3.  The left pair at
        // px = 0 reflects to columns 2 and 1 and the right pair at px = W - 4 to W - 2 and W - 3: both lie in the thread's own
        // centre vector (as .z, .y), so the pair load of a border patch only has to stay in bounds.  Bilinear needs the inner
        // ring alone: rows 1 .. 4
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

    // ---- stages: the two tone curves here (their per-image constants are cheap enough to form in every thread), the rest in
    // risp_ops.h
    for (int k = 0; k < a.n_ops; ++k) {
        const int op = a.ops[k];
        const float *p = a.params[k];
        if (op == RISP_OP_TONE_CRYSIS) {               // p (N,1): lum_adapted
            tone_all<false>(0.5f / (p[n] + 0.05f), 0.f, &pix[0][0]);
        } else if (op == RISP_OP_TONE_FILMIC) {        // p (N,2): white_point, exposure_bias
            tone_all<true>(p[2 * n + 1], 1.f / hable(fmaxf(p[2 * n], 0.01f) * 11.2f), &pix[0][0]);
        } else {
            apply_op<2 * PXT, WBQ>(op, p, n, &pix[0][0]);
        }
    }

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

    // ---- the result alone: 4 pixels x 3 bytes of a row are three dwords (the row offset is a multiple of 12 bytes).  Mirrored
    // along x the four pixels land at W-4-px in reverse order (the bytes of a pixel keep theirs)
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

template <int KIND, bool NV12, int PACK, bool SHADE, class Args>
void launch_kind(bool wbq, dim3 grid, hipStream_t s, const Args &a) {
    if (wbq) hipLaunchKernelGGL((serve_classical_kernel<KIND, true, NV12, PACK, SHADE>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((serve_classical_kernel<KIND, false, NV12, PACK, SHADE>), grid, dim3(256), 0, s, a);
}

// the rules both entry points share (include/risp.h), and the argument block; `name` is the entry point's, for the message
int classical_args_fill(const char *name, ClassicalArgs &a, bool &wbq, const uint16_t *raw, float divisor, int demosaic, int n_ops,
                        const int *ops, const float *const *params, uint8_t *out, int reverse_channels, int N, int H, int W,
                        int black_level, int cfa, int raw_align = 8) {
    RISP_CHECK_ARG(raw && out, "%s: null argument", name);
    RISP_CHECK_ARG(divisor > 0.f, "%s: divisor %g", name, (double)divisor);
    RISP_CHECK_ARG(demosaic >= RISP_DEMOSAIC_NEAREST && demosaic <= RISP_DEMOSAIC_LAPLACIAN,
                   "%s: demosaic %d (RISP_DEMOSAIC_NEAREST 0, BILINEAR 1, LAPLACIAN 2)", name, demosaic);
    RISP_CHECK_ARG(cfa >= 0 && cfa <= 3, "%s: cfa %d (RISP_CFA_RGGB 0, GRBG 1, GBRG 2, BGGR 3)", name, cfa);
    RISP_CHECK_ARG(black_level >= 0 && black_level <= 65535, "%s: black_level %d outside 0 .. 65535", name, black_level);
    RISP_CHECK_ARG(n_ops >= 0 && n_ops <= RISP_MAX_CHAIN && (n_ops == 0 || (ops && params)), "%s: bad op list", name);
    RISP_CHECK_ARG(N >= 1 && N <= 65535 && H >= 4 && H % 2 == 0 && W >= 4 && W % 4 == 0,
                   "%s: bad shape N=%d H=%d W=%d (H even and >= 4, W a multiple of 4)", name, N, H, W);
    RISP_CHECK_ARG(reinterpret_cast<uintptr_t>(raw) % raw_align == 0 && reinterpret_cast<uintptr_t>(out) % 4 == 0,
                   "%s: raw must be %d-byte and out 4-byte aligned", name, raw_align);
    a.raw = raw;
    a.out = out;
    a.divisor = divisor;
    a.n_ops = n_ops;
    a.N = N;
    a.H = H;
    a.W = W;
    a.reverse = reverse_channels ? 1 : 0;
    a.black = black_level;
    a.flip = cfa;
    wbq = false;
    for (int k = 0; k < RISP_MAX_CHAIN; ++k) {
        a.ops[k] = RISP_OP_SKIP;
        a.params[k] = nullptr;
    }
    for (int k = 0; k < n_ops; ++k) {
        RISP_CHECK_ARG(ops[k] == RISP_OP_SKIP || (ops[k] >= RISP_OP_WB_MANUAL && ops[k] <= RISP_OP_TONE_FILMIC), "%s: op %d not allowed",
                       name, ops[k]);
        RISP_CHECK_ARG(ops[k] == RISP_OP_SKIP || params[k], "%s: stage %d has no parameter block", name, k);
        a.ops[k] = ops[k];
        a.params[k] = ops[k] == RISP_OP_SKIP ? nullptr : params[k];
        wbq |= ops[k] == RISP_OP_WB_QUADRATIC;
    }
    return 0;
}

template <bool NV12, int PACK = 0, bool SHADE = false, class Args>
void launch_classical(int demosaic, bool wbq, hipStream_t s, const Args &a) {
    const dim3 grid((a.W / 4 + STX - 1) / STX, (a.H / 2 + STY - 1) / STY, a.N);
    if (demosaic == RISP_DEMOSAIC_LAPLACIAN) launch_kind<RISP_DEMOSAIC_LAPLACIAN, NV12, PACK, SHADE>(wbq, grid, s, a);
    else if (demosaic == RISP_DEMOSAIC_BILINEAR) launch_kind<RISP_DEMOSAIC_BILINEAR, NV12, PACK, SHADE>(wbq, grid, s, a);
    else launch_kind<RISP_DEMOSAIC_NEAREST, NV12, PACK, SHADE>(wbq, grid, s, a);
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
    if (int err = classical_args_fill(name, a, wbq, reinterpret_cast<const uint16_t *>(raw), divisor, demosaic, n_ops, ops, params, out,
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
