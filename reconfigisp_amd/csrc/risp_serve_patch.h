// What the serving routes behind risp_serve_u8 share (risp_serve_classical / _scene / _cond / _denoise / _median /
// _denoise_scene.hip): a thread evaluates a 2 x 4 pixel patch of the mirrored (RGGB) image from the 16-bit mosaic -
//
//     max(sample - black, 0) / divisor -> nearest | bilinear | Malvar-He-Cutler demosaic -> stages -> clip(v * 255) truncated
//
// - and every route does so with the same loads, the same expressions in the same order and the same store.  The arithmetic is
// that of the composed route restated (its device code lives in anonymous namespaces of risp_origin.hip): origin_demosaic_kernel's
// per-site expressions and 8-bit rounding, tonemap_prepare_kernel's constants and tonemap_kernel's pixel expression with both
// scales 255, apply_op (risp_ops.h) for the rest.  With -ffp-contract=off the bytes are the composed route's.
//
// The form is part of the result: these kernels sit at 59 .. 64 VGPRs, the edge of 8 waves per SIMD, and a helper that writes the
// patch through a reference to the caller's array costs half the occupancy (99 .. 104 VGPRs; profiles/serve_patch_resources.txt,
// DESIGN 4.6).  So a helper here RETURNS its patch or window by value.
//
// Host side: the argument block every route's block starts with, the rules of include/risp.h every entry point repeats, the
// launch grid and the dispatch over demosaic kind x WbQuadratic (with_form).  The tile routes' walk and the 3 x 3 denoisers' kernel
// are risp_serve_dentile.h's.
#pragma once
#include <type_traits>

#include "risp_common.h"
#include "risp_ops.h"

namespace risp_patch {

using risp_ops::apply_op;

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

// what every route's argument block starts with (serve_args fills it)
struct PatchArgs {
    const uint16_t *raw;        // (N,H,W) mosaic of the sensor
    float divisor;
    int n_pre, n_ops, N, H, W;  // stages 0 .. n_pre - 1 run in front of a route's stencil, n_pre .. n_ops - 1 behind it (no stencil: n_pre = 0)
    int black;                  // subtracted from every sample in integers, clamped at 0
    int flip;                   // RISP_CFA_*: bit 0 mirrors x, bit 1 mirrors y
    int ops[RISP_MAX_CHAIN];
    const float *params[RISP_MAX_CHAIN];
};

struct Patch {                  // rows py, py + 1; columns px .. px + 3
    f3 p[2][PXT];
};
struct Window {                 // m[r][c]: mosaic row py - 2 + r, column px - 2 + c in the 0..255 domain
    float m[6][8];
};

// ---- stages
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

// one stage on NPX pixels in registers: the two tone curves that need no whole-image quantity here (their per-image constants are
// cheap enough to form in every thread), the rest in risp_ops.h
template <int NPX, bool WBQ>
__device__ __forceinline__ void stage(int op, const float *p, int n, f3 *px) {
    if (op == RISP_OP_TONE_CRYSIS) {                   // p (N,1): lum_adapted
        tone_all<false, NPX>(0.5f / (p[n] + 0.05f), 0.f, px);
    } else if (op == RISP_OP_TONE_FILMIC) {            // p (N,2): white_point, exposure_bias
        tone_all<true, NPX>(p[2 * n + 1], 1.f / hable(fmaxf(p[2 * n], 0.01f) * 11.2f), px);
    } else {
        apply_op<NPX, WBQ>(op, p, n, px);
    }
}

// white-world apply: tonemap_kernel<TM_GAIN>'s pixel expression with si = so = 255; p: the image's row of the (N,4) constants of
// risp_serve_scene_finish.  Only the scene routes accept the op
template <int NPX>
__device__ __forceinline__ void gain_q8_all(const float *p, f3 *px) {
    const float p0 = p[0], p1 = p[1], p2 = p[2];
#pragma unroll
    for (int i = 0; i < NPX; ++i) {
        float b = px[i].b * 255.f / 255.f, g = px[i].g * 255.f / 255.f, r = px[i].r * 255.f / 255.f;
        b *= p0; g *= p1; r *= p2;
        px[i] = {q8(b * 255.f) * (1.f / 255.f), q8(g * 255.f) * (1.f / 255.f), q8(r * 255.f) * (1.f / 255.f)};
    }
}

// stages k0 .. k1 - 1.  GAIN: RISP_OP_GAIN3_Q8 is among them
template <int NPX, bool WBQ, bool GAIN = false>
__device__ __forceinline__ void run_stages(const PatchArgs &a, int k0, int k1, int n, f3 *px) {
    for (int k = k0; k < k1; ++k) {
        const int op = a.ops[k];
        const float *p = a.params[k];
        if (GAIN && op == RISP_OP_GAIN3_Q8) gain_q8_all<NPX>(p + 4 * n, px);
        else stage<NPX, WBQ>(op, p, n, px);
    }
}

// ---- demosaics
// nearest: no stencil, the patch's own two quads (rows py and py + 1 of columns px .. px + 3) in the [0,1] domain
__device__ __forceinline__ Patch nearest_patch(const float (&t)[4], const float (&b)[4]) {
    const float R0 = t[0], G10 = t[1], R1 = t[2], G11 = t[3], G20 = b[0], B0 = b[1], G21 = b[2], B1 = b[3];
    Patch o;
    o.p[0][0] = o.p[0][1] = {B0, G10, R0};
    o.p[0][2] = o.p[0][3] = {B1, G11, R1};
    o.p[1][0] = o.p[1][1] = {B0, G20, R0};
    o.p[1][2] = o.p[1][3] = {B1, G21, R1};
    return o;
}

// bilinear (rows 1 .. 4 of m alone) | Malvar-He-Cutler
template <bool LAP>
__device__ __forceinline__ Patch demosaic_sites(const float (&m)[6][8]) {
    Patch o;
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
            o.p[p][i] = {q8(B_) * inv255, q8(G_) * inv255, q8(R_) * inv255};
        }
    return o;
}

// ---- the loads of a uint16 frame.  px, py and every coordinate derived from them are those of the mirrored image, which is RGGB;
// only row_at / ld2 / ld4 (and the store) know where the samples really are.  Black level and Bayer phase as in risp_serve_u8_cfa
struct Mosaic {
    const uint16_t *bay;        // image n
    int H, W, black, flip;
    float div;
    __device__ __forceinline__ Mosaic(const PatchArgs &a, int n)
        : bay(a.raw + (size_t)n * a.H * a.W), H(a.H), W(a.W), black(a.black), flip(a.flip), div(a.divisor) {}
    __device__ __forceinline__ const uint16_t *row_at(int y) const { return bay + (size_t)(flip & 2 ? H - 1 - y : y) * W; }
    __device__ __forceinline__ ushort2 ld2(const uint16_t *row, int x) const {      // samples x, x + 1 of the mirrored row (x even)
        const bool fx = flip & 1;
        const ushort2 v = *reinterpret_cast<const ushort2 *>(row + (fx ? W - 2 - x : x));
        return fx ? ushort2{v.y, v.x} : v;
    }
    __device__ __forceinline__ ushort4 ld4(const uint16_t *row, int x) const {      // x .. x + 3 (x % 4 == 0)
        const bool fx = flip & 1;
        const ushort4 v = *reinterpret_cast<const ushort4 *>(row + (fx ? W - 4 - x : x));
        return fx ? ushort4{v.w, v.z, v.y, v.x} : v;
    }
    __device__ __forceinline__ float smp(unsigned short s) const { return (float)((int)s > black ? (int)s - black : 0); }

    __device__ __forceinline__ Patch nearest(int px, int py) const {
        const ushort4 r0 = ld4(row_at(py), px), r1 = ld4(row_at(py + 1), px);
        return nearest_patch({smp(r0.x) / div, smp(r0.y) / div, smp(r0.z) / div, smp(r0.w) / div},
                             {smp(r1.x) / div, smp(r1.y) / div, smp(r1.z) / div, smp(r1.w) / div});
    }
    // reflect-101 over radius 2 (H, W >= 4: one reflection reaches every tap).  Row -2 / -1 reflect to 2 / 1, row H / H + 1 to
    // H - 2 / H - 3.  The left pair at px = 0 reflects to columns 2 and 1 and the right pair at px = W - 4 to W - 2 and W - 3: both
    // lie in the thread's own centre vector (as .z, .y), so the pair load of a border patch only has to stay in bounds.  Bilinear
    // needs the inner ring alone: rows 1 .. 4
    template <bool LAP>
    __device__ __forceinline__ Window window(int px, int py) const {
        constexpr int R0 = LAP ? 0 : 1, R1 = LAP ? 6 : 5;
        const bool left = px > 0, right = px + 4 < W;
        const int xl = left ? px - 2 : 0, xr = right ? px + 4 : px;
        Window w;
#pragma unroll
        for (int r = R0; r < R1; ++r) {
            int y = py - 2 + r;
            y = y < 0 ? -y : (y >= H ? 2 * H - 2 - y : y);
            const uint16_t *row = row_at(y);
            const ushort2 l = ld2(row, xl), e = ld2(row, xr);
            const ushort4 c = ld4(row, px);
            const unsigned short s[8] = {left ? l.x : c.z, left ? l.y : c.y, c.x, c.y, c.z, c.w, right ? e.x : c.z, right ? e.y : c.y};
#pragma unroll
            for (int k = 0; k < 8; ++k) w.m[r][k] = (smp(s[k]) / div) * 255.f;     // risp_raw_crop_cfa's expression, x 255 on load
        }
        return w;
    }
    // KIND: RISP_DEMOSAIC_*
    template <int KIND>
    __device__ __forceinline__ Patch patch(int px, int py) const {
        if constexpr (KIND == RISP_DEMOSAIC_NEAREST) return nearest(px, py);
        else {
            constexpr bool LAP = KIND == RISP_DEMOSAIC_LAPLACIAN;
            const Window w = window<LAP>(px, py);
            return demosaic_sites<LAP>(w.m);
        }
    }
};

// ---- the result alone: 4 pixels x 3 bytes of image row y are three dwords (the row offset is a multiple of 12 bytes).  Mirrored
// along x the four pixels land at W-4-px in reverse order (the bytes of a pixel keep theirs)
__device__ __forceinline__ void store_bgr4(uint8_t *out, int n, int H, int W, int y, int px, int flip, int reverse, const f3 (&o)[PXT]) {
    unsigned b[PXT][3];
#pragma unroll
    for (int c = 0; c < PXT; ++c) {
        const f3 v = o[c], m = o[PXT - 1 - c];
        const bool fx = flip & 1;                       // value selects (a ?: between the two array elements selects an address)
        const unsigned vb = u8(fx ? m.b : v.b), vg = u8(fx ? m.g : v.g), vr = u8(fx ? m.r : v.r);
        b[c][0] = reverse ? vr : vb;
        b[c][1] = vg;
        b[c][2] = reverse ? vb : vr;
    }
    unsigned *dst = reinterpret_cast<unsigned *>(out + (((size_t)n * H + (flip & 2 ? H - 1 - y : y)) * W + (flip & 1 ? W - 4 - px : px)) * 3);
    dst[0] = b[0][0] | b[0][1] << 8 | b[0][2] << 16 | b[1][0] << 24;
    dst[1] = b[1][1] | b[1][2] << 8 | b[2][0] << 16 | b[2][1] << 24;
    dst[2] = b[2][2] | b[3][0] << 8 | b[3][1] << 16 | b[3][2] << 24;
}

// ---- sum or maximum of three values over the workgroup, in a fixed order: wavefront shuffles, then one LDS step in wave order
// (lds: 12 floats).  Thread 0 receives the result.  Contains a barrier: every thread of the workgroup calls it
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

// ---- host side
// the patch grid (W / 4, H / 2) in workgroups of STX x STY threads; the tile routes' grid of 64 x 32 pixel tiles is the same
inline dim3 patch_grid(int N, int H, int W) { return dim3((W / 4 + STX - 1) / STX, (H / 2 + STY - 1) / STY, N); }

// calls f(std::integral_constant<int, KIND>, std::bool_constant<WBQ>) for the form a launch takes (demosaic as serve_args passed it)
template <class F>
inline void with_form(int demosaic, bool wbq, F &&f) {
    auto kind = [&](auto kind_c) {
        if (wbq) f(kind_c, std::true_type{});
        else f(kind_c, std::false_type{});
    };
    if (demosaic == RISP_DEMOSAIC_LAPLACIAN) kind(std::integral_constant<int, RISP_DEMOSAIC_LAPLACIAN>{});
    else if (demosaic == RISP_DEMOSAIC_BILINEAR) kind(std::integral_constant<int, RISP_DEMOSAIC_BILINEAR>{});
    else kind(std::integral_constant<int, RISP_DEMOSAIC_NEAREST>{});
}

// what differs between the entry points' rules
struct ArgRules {
    bool out_here = true;       // `out` is checked here, beside raw (one message for both); else the entry point checks its destination
    bool split = false;         // two op lists, around a stencil
    bool gain_q8 = false;       // RISP_OP_GAIN3_Q8 is served: its block is the 16-byte aligned constants of risp_serve_scene_finish
    bool reinhard = false;      // ... and RISP_OP_TONE_REINHARD (only where gain_q8 is)
    int raw_align = 8;
    const char *shape_note = "H even and >= 4, W a multiple of 4";
};

// The rules the entry points share (include/risp.h), and the block; `name` is the entry point's, for the message.  A route
// with one list passes it as the front one.  wbq: a stage is WbQuadratic
inline int serve_args(const char *name, const ArgRules &r, PatchArgs &a, bool &wbq, const void *raw, const void *out, float divisor,
                      int demosaic, int n_pre, const int *pre_ops, const float *const *pre_params, int n_post, const int *post_ops,
                      const float *const *post_params, int N, int H, int W, int black_level, int cfa) {
    if (r.out_here) RISP_CHECK_ARG(raw && out, "%s: null argument", name);
    else RISP_CHECK_ARG(raw, "%s: null argument (raw)", name);
    RISP_CHECK_ARG(divisor > 0.f, "%s: divisor %g", name, (double)divisor);
    RISP_CHECK_ARG(demosaic >= RISP_DEMOSAIC_NEAREST && demosaic <= RISP_DEMOSAIC_LAPLACIAN,
                   "%s: demosaic %d (RISP_DEMOSAIC_NEAREST 0, BILINEAR 1, LAPLACIAN 2)", name, demosaic);
    RISP_CHECK_ARG(cfa >= 0 && cfa <= 3, "%s: cfa %d (RISP_CFA_RGGB 0, GRBG 1, GBRG 2, BGGR 3)", name, cfa);
    RISP_CHECK_ARG(black_level >= 0 && black_level <= 65535, "%s: black_level %d outside 0 .. 65535", name, black_level);
    if (r.split) {
        RISP_CHECK_ARG(n_pre >= 0 && n_post >= 0 && n_pre <= RISP_MAX_CHAIN && n_post <= RISP_MAX_CHAIN && n_pre + n_post <= RISP_MAX_CHAIN,
                       "%s: bad op list: %d + %d stages (at most %d in all)", name, n_pre, n_post, RISP_MAX_CHAIN);
        RISP_CHECK_ARG((n_pre == 0 || (pre_ops && pre_params)) && (n_post == 0 || (post_ops && post_params)), "%s: bad op list: null",
                       name);
    } else {
        const bool ok = n_pre >= 0 && n_pre <= RISP_MAX_CHAIN && (n_pre == 0 || (pre_ops && pre_params));
        if (r.out_here) RISP_CHECK_ARG(ok, "%s: bad op list", name);
        else RISP_CHECK_ARG(ok, "%s: bad op list (n_ops %d)", name, n_pre);
    }
    RISP_CHECK_ARG(N >= 1 && N <= 65535 && H >= 4 && H % 2 == 0 && W >= 4 && W % 4 == 0, "%s: bad shape N=%d H=%d W=%d (%s)", name, N,
                   H, W, r.shape_note);
    if (r.out_here)
        RISP_CHECK_ARG(reinterpret_cast<uintptr_t>(raw) % r.raw_align == 0 && reinterpret_cast<uintptr_t>(out) % 4 == 0,
                       "%s: raw must be %d-byte and out 4-byte aligned", name, r.raw_align);
    else RISP_CHECK_ARG(reinterpret_cast<uintptr_t>(raw) % r.raw_align == 0, "%s: raw must be %d-byte aligned", name, r.raw_align);
    a.raw = static_cast<const uint16_t *>(raw);
    a.divisor = divisor;
    a.n_pre = r.split ? n_pre : 0;
    a.n_ops = n_pre + n_post;
    a.N = N;
    a.H = H;
    a.W = W;
    a.black = black_level;
    a.flip = cfa;
    wbq = false;
    for (int k = 0; k < RISP_MAX_CHAIN; ++k) {
        a.ops[k] = RISP_OP_SKIP;
        a.params[k] = nullptr;
    }
    for (int k = 0; k < n_pre + n_post; ++k) {
        const int op = k < n_pre ? pre_ops[k] : post_ops[k - n_pre];
        const float *p = k < n_pre ? pre_params[k] : post_params[k - n_pre];
        const bool scene = (r.gain_q8 && op == RISP_OP_GAIN3_Q8) || (r.reinhard && op == RISP_OP_TONE_REINHARD);
        if (r.gain_q8 && !r.reinhard)
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

// the rules of the routes that hold a 3 x 3 / block 3 search 3 denoiser
inline int denoiser_args(const char *name, int denoise, int window, int search, const float *den_a, const float *den_b) {
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
    return 0;
}

}  // namespace risp_patch
