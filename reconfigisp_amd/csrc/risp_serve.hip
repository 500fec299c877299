// Serving path (inference): a 16-bit RGGB frame in, a packed 8-bit image out.
//
//     uint16 sample / divisor -> nearest demosaic -> [bilateral, 3 x 3] -> element-wise chain -> clip(v * 255) truncated
//
// in ONE launch that stores the result alone: 2 bytes read and 3 written per pixel, where the route through the fp32 kernels
// (risp_raw_crop, risp_bilateral_chain_fwd with every stage output, a conversion pass) moves about 85.  risp_serve_u8 has the
// shape of bilateral_chain_quad_kernel (risp_fused.hip): a thread owns a 2 x 4 pixel patch and loads the ring of mosaic quads
// around it itself - no LDS, no barrier.  The per-pixel expressions are that kernel's, restated in the same order (its device
// code lives in an anonymous namespace and stays as measured), and the element-wise stages are risp_ops.h's: with
// -ffp-contract=off the bytes are those of the fp32 route followed by tensor2bgr (tests/test_gpu_serve.py holds them to it).
//
// risp_quantise_u8 is the conversion alone, for pipelines that do not fit the one launch: planar fp32 (N,C,H,W) to packed
// (N,H,W,C) bytes, the arithmetic of utils/util.py tensor2bgr (risp_reduce.hip to_u8 scores the same bytes).
//
// The other Bayer phases and a sensor black level (risp_serve_u8_cfa, risp_quantise_u8_flip).  A GRBG / GBRG / BGGR mosaic with
// even H and W is an RGGB mosaic mirrored along x / y / both, so the phase is a mirror of ADDRESSES and nothing else: a thread's
// patch coordinates live in the mirrored (RGGB) image, a load reads W-1-x / H-1-y and reverses its samples in registers, the ring's
// clamping happens in mirrored coordinates, and the result is stored at the un-mirrored place.  The arithmetic between load and
// store is the RGGB kernel's, so the bytes are those of flip -> risp_serve_u8 -> flip (tests/test_gpu_serve_cfa.py, torch.equal).
// The black level is subtracted in integers, clamped at 0, before the conversion to float.  Both are a further template parameter:
// the instantiations risp_serve_u8 launches do not see them.
//
// MIPI-packed RAW10 / RAW12 in (risp_serve_packed): a third template parameter, PACK = 0 / 10 / 12, which replaces row_at / ld2 /
// ld4 - the three places that know where samples are - by the loads of risp_rawpack.h.  A thread's four centre pixels are one
// 5-byte group or two 3-byte groups, the pairs at xl / xr half a group or one group, and mirrored along x the group at W-4-x is
// read and reversed.  Everything behind the sample is the CFA form's; the PACK = 0 instantiations do not see the parameter.
#include "risp_common.h"
#include "risp_nv12.h"
#include "risp_ops.h"
#include "risp_rawpack.h"

namespace {

using namespace risp_ops;

// clip(v * 255, 0, 255).astype(uint8): the product in fp32, the conversion truncates
__device__ __forceinline__ unsigned u8(float v) {
    float t = v * 255.f;
    t = t < 0.f ? 0.f : (t > 255.f ? 255.f : t);
    return (unsigned)(int)t;
}

// ---------------------------------------------------------------- planar fp32 -> packed bytes
// four pixels of one image per thread: 16-byte plane loads, C dwords stored
template <int C>
__global__ __launch_bounds__(256) void quantise_vec_kernel(const float *__restrict__ x, uint8_t *__restrict__ out, size_t nvec,
                                                           int hw4, int reverse) {
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < nvec; t += (size_t)gridDim.x * blockDim.x) {
        const size_t n = t / hw4, i = t - n * hw4;
        const float4 *src = reinterpret_cast<const float4 *>(x) + n * C * hw4 + i;
        unsigned *dst = reinterpret_cast<unsigned *>(out) + t * C;
        if (C == 1) {
            const float4 v = *src;
            *dst = u8(v.x) | u8(v.y) << 8 | u8(v.z) << 16 | u8(v.w) << 24;
        } else {
            const float4 c0 = src[reverse ? 2 * (size_t)hw4 : 0], c1 = src[hw4], c2 = src[reverse ? 0 : 2 * (size_t)hw4];
            dst[0] = u8(c0.x) | u8(c1.x) << 8 | u8(c2.x) << 16 | u8(c0.y) << 24;
            dst[1] = u8(c1.y) | u8(c2.y) << 8 | u8(c0.z) << 16 | u8(c1.z) << 24;
            dst[2] = u8(c2.z) | u8(c0.w) << 8 | u8(c1.w) << 16 | u8(c2.w) << 24;
        }
    }
}

// any size and any alignment: one output byte per thread
__global__ __launch_bounds__(256) void quantise_any_kernel(const float *__restrict__ x, uint8_t *__restrict__ out, size_t total,
                                                           int C, size_t hw, int reverse) {
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const size_t pixel = t / C, n = pixel / hw, i = pixel - n * hw;
        const int c = (int)(t - pixel * C);
        out[t] = (uint8_t)u8(x[(n * C + (reverse ? C - 1 - c : c)) * hw + i]);
    }
}

// mirrored forms: output pixel (y, x) takes input (fy ? H-1-y : y, fx ? W-1-x : x).  W % 4 == 0 here, so that a vector is four
// pixels of one row: the mirrored vector starts at W-4-x and is reversed in registers
template <int C>
__global__ __launch_bounds__(256) void quantise_flip_vec_kernel(const float *__restrict__ x, uint8_t *__restrict__ out, size_t nvec,
                                                                int H, int w4, int reverse, int fx, int fy) {
    const size_t hw4 = (size_t)H * w4;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < nvec; t += (size_t)gridDim.x * blockDim.x) {
        const size_t n = t / hw4, i = t - n * hw4;
        const int y = (int)(i / w4), xv = (int)(i - (size_t)y * w4);
        const float4 *src = reinterpret_cast<const float4 *>(x) + n * C * hw4 + (size_t)(fy ? H - 1 - y : y) * w4 + (fx ? w4 - 1 - xv : xv);
        unsigned *dst = reinterpret_cast<unsigned *>(out) + t * C;
        auto ld = [&](size_t plane) {
            const float4 v = src[plane * hw4];
            return fx ? make_float4(v.w, v.z, v.y, v.x) : v;
        };
        if (C == 1) {
            const float4 v = ld(0);
            *dst = u8(v.x) | u8(v.y) << 8 | u8(v.z) << 16 | u8(v.w) << 24;
        } else {
            const float4 c0 = ld(reverse ? 2 : 0), c1 = ld(1), c2 = ld(reverse ? 0 : 2);
            dst[0] = u8(c0.x) | u8(c1.x) << 8 | u8(c2.x) << 16 | u8(c0.y) << 24;
            dst[1] = u8(c1.y) | u8(c2.y) << 8 | u8(c0.z) << 16 | u8(c1.z) << 24;
            dst[2] = u8(c2.z) | u8(c0.w) << 8 | u8(c1.w) << 16 | u8(c2.w) << 24;
        }
    }
}

__global__ __launch_bounds__(256) void quantise_flip_any_kernel(const float *__restrict__ x, uint8_t *__restrict__ out, size_t total,
                                                                int C, int H, int W, int reverse, int fx, int fy) {
    const size_t hw = (size_t)H * W;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const size_t pixel = t / C, n = pixel / hw, i = pixel - n * hw;
        const int c = (int)(t - pixel * C), y = (int)(i / W), xx = (int)(i - (size_t)y * W);
        out[t] = (uint8_t)u8(x[(n * C + (reverse ? C - 1 - c : c)) * hw + (size_t)(fy ? H - 1 - y : y) * W + (fx ? W - 1 - xx : xx)]);
    }
}

// ---------------------------------------------------------------- the one launch
struct ServeArgs {
    const uint16_t *raw;        // (N,H,W) RGGB
    uint8_t *out;               // (N,H,W,3)
    const int *win;             // (N) window per image (bilateral only)
    const float *sig_c, *sig_s; // (N)
    float divisor;
    int n_ops, N, H, W;
    int full_window;            // max_window == 3: images whose window reaches 3 take the nine taps
    int reverse;                // store R, G, B instead of B, G, R
    int ops[RISP_MAX_CHAIN];
    const float *params[RISP_MAX_CHAIN];
};

// risp_serve_u8_cfa: the same block first (the kernel arguments of the RGGB instantiations keep their layout), then the two more
struct ServeCfaArgs : ServeArgs {
    int black;                  // subtracted from every sample in integers, clamped at 0
    int flip;                   // RISP_CFA_*: bit 0 mirrors x, bit 1 mirrors y
};
// risp_serve_nv12: the block of risp_serve_u8_cfa, then the matrix by value (`reverse` is not read)
struct ServeNv12Args : ServeCfaArgs {
    risp_nv12::Coef yuv;
};
template <bool CFA, bool NV12 = false> struct serve_args { using type = ServeArgs; };
template <> struct serve_args<true, false> { using type = ServeCfaArgs; };
template <bool CFA> struct serve_args<CFA, true> { using type = ServeNv12Args; };
// risp_serve_packed: the block of risp_serve_nv12 (`raw` holds the byte pointer; BGR out reads `reverse`, NV12 out `yuv`), then
// the row pitch
struct ServePackedArgs : ServeNv12Args {
    int stride;                 // bytes from a packed row to the next
};
template <bool CFA, bool NV12, int PACK> struct serve_args_of { using type = typename serve_args<CFA, NV12>::type; };
template <bool NV12> struct serve_args_of<true, NV12, 10> { using type = ServePackedArgs; };
template <bool NV12> struct serve_args_of<true, NV12, 12> { using type = ServePackedArgs; };

__device__ __forceinline__ float q8f(float v) {
    return floorf(__builtin_amdgcn_fmed3f(v, 0.f, 255.f) + 0.5f);   // clamp in one instruction (v is never NaN here)
}

// XCD-aware tile order, as in risp_fused.hip: XCD k works through the k-th contiguous eighth of the tile list, so the ring a
// tile shares with its neighbours is read through one L2
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

// CFA: black level and mirror (wave-uniform at run time).  px, py and every coordinate derived from them are those of the mirrored
// image, which is RGGB; only ld2 / ld4 / smp and the store know where the samples really are.  NV12: the store epilogue alone
// differs - the patch's eight codes leave as two Y dwords and one UV dword of a (3H/2, W) image (risp_nv12.h)
// PACK (with CFA): the mosaic is MIPI-packed RAW10 / RAW12 and row_at / ld2 / ld4 alone differ (risp_rawpack.h)
template <bool BIL, bool WBQ, bool CFA = false, bool NV12 = false, int PACK = 0>
__global__ __launch_bounds__(256) void serve_kernel(const typename serve_args_of<CFA, NV12, PACK>::type a) {
    static_assert(PACK == 0 || CFA, "the packed instantiations use the CFA form");
    const int H = a.H, W = a.W;
    int bxi, byi, bzi;
    xcd_tile(bxi, byi, bzi);
    const int n = bzi;
    const int px = (bxi * STX + (int)(threadIdx.x % STX)) * 4, py = (byi * STY + (int)(threadIdx.x / STX)) * 2;
    if (px >= W || py >= H) return;                     // W % 4 == 0, H % 2 == 0: a patch is in or out as a whole
    const uint16_t *bay = a.raw + (size_t)n * H * W;
    const float div = a.divisor;
    f3 pix[2][PXT];
    int black = 0, flip = 0;
    if constexpr (CFA) black = a.black, flip = a.flip;
    // row y of the mirrored image; its samples x, x + 1 (x even) and x .. x + 3 (x % 4 == 0); (float)max(s - black, 0)
    auto row_at = [&](int y) {
        if constexpr (PACK != 0)
            return reinterpret_cast<const uint8_t *>(a.raw) + ((size_t)n * H + (flip & 2 ? H - 1 - y : y)) * a.stride;
        else if constexpr (CFA) return bay + (size_t)(flip & 2 ? H - 1 - y : y) * W;
        else return bay + (size_t)y * W;
    };
    auto ld2 = [&](auto *row, int x) {
        if constexpr (PACK != 0) {
            const bool fx = flip & 1;
            const ushort2 v = risp_rawpack::ld2<PACK>(row, fx ? W - 2 - x : x);
            return fx ? ushort2{v.y, v.x} : v;
        } else if constexpr (CFA) {
            const bool fx = flip & 1;
            const ushort2 v = *reinterpret_cast<const ushort2 *>(row + (fx ? W - 2 - x : x));
            return fx ? ushort2{v.y, v.x} : v;
        } else {
            return *reinterpret_cast<const ushort2 *>(row + x);
        }
    };
    auto ld4 = [&](auto *row, int x) {
        if constexpr (PACK != 0) {
            const bool fx = flip & 1;
            const ushort4 v = risp_rawpack::ld4<PACK>(row, fx ? W - 4 - x : x);
            return fx ? ushort4{v.w, v.z, v.y, v.x} : v;
        } else if constexpr (CFA) {
            const bool fx = flip & 1;
            const ushort4 v = *reinterpret_cast<const ushort4 *>(row + (fx ? W - 4 - x : x));
            return fx ? ushort4{v.w, v.z, v.y, v.x} : v;
        } else {
            return *reinterpret_cast<const ushort4 *>(row + x);
        }
    };
    auto smp = [&](unsigned short s) {
        if constexpr (CFA) return (float)((int)s > black ? (int)s - black : 0);
        else return (float)s;
    };

    if constexpr (BIL) {
        // ---- the 3 x 4 quads around the patch: quad rows j-1, j, j+1 and quad columns i-1 .. i+2, clamped to the image
        // (reflect-101 of the pixel one step outside the image is the same row parity of the border quad)
        const int j = py >> 1, i = px >> 1, qh = H >> 1, qw = W >> 1;
        const int jr[3] = {j > 0 ? j - 1 : 0, j, j + 1 < qh ? j + 1 : qh - 1};
        const int xl = 2 * (i > 0 ? i - 1 : 0), xr = 2 * (i + 2 < qw ? i + 2 : qw - 1);
        ushort2 ml[6], mr[6];
        ushort4 mc[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            // (the RGGB instantiations keep their own statements, here and at the store: their instruction stream stays the one
            // profiles/serve_u8.txt timed)
            if constexpr (CFA) {
                const auto *row = row_at(2 * jr[k >> 1] + (k & 1));
                ml[k] = ld2(row, xl);
                mc[k] = ld4(row, px);
                mr[k] = ld2(row, xr);
            } else {
                const uint16_t *row = bay + (size_t)(2 * jr[k >> 1] + (k & 1)) * W;
                ml[k] = *reinterpret_cast<const ushort2 *>(row + xl);
                mc[k] = *reinterpret_cast<const ushort4 *>(row + px);
                mr[k] = *reinterpret_cast<const ushort2 *>(row + xr);
            }
        }
        // RGGB: R (even row, even column), G1 (even, odd), G2 (odd, even), B (odd, odd); qg[..][p] is the green of row parity p.
        // sample / divisor is risp_raw_crop's expression; x 255 is the bilateral's domain
        float qb[3][4], qg[3][4][2], qr[3][4];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const unsigned short e[4][2] = {{ml[2 * k].x, ml[2 * k].y}, {mc[2 * k].x, mc[2 * k].y}, {mc[2 * k].z, mc[2 * k].w},
                                            {mr[2 * k].x, mr[2 * k].y}};
            const unsigned short o[4][2] = {{ml[2 * k + 1].x, ml[2 * k + 1].y}, {mc[2 * k + 1].x, mc[2 * k + 1].y},
                                            {mc[2 * k + 1].z, mc[2 * k + 1].w}, {mr[2 * k + 1].x, mr[2 * k + 1].y}};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                qr[k][c] = (smp(e[c][0]) / div) * 255.f;
                qg[k][c][0] = (smp(e[c][1]) / div) * 255.f;
                qg[k][c][1] = (smp(o[c][0]) / div) * 255.f;
                qb[k][c] = (smp(o[c][1]) / div) * 255.f;
            }
        }
        const bool full = a.full_window && a.win[n] / 2 >= 1;      // wave-uniform; the radius is clamped to [0, 1]
        const float ks = -1.f / (2.f * a.sig_s[n] * a.sig_s[n]), kc = -1.f / (2.f * a.sig_c[n] * a.sig_c[n]);
        const float ks2 = ks * 1.4426950408889634f, kc2 = kc * 1.4426950408889634f;     // base-2 exponent coefficients
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int c = 0; c < PXT; ++c) {
                // pixel (p, c) of the patch sits at row 2 + p, column 2 + c of the 6 x 8 pixels the 3 x 4 quads cover
                const float cb = qb[1][1 + c / 2], cg = qg[1][1 + c / 2][p], cr = qr[1][1 + c / 2];
                float nb = 0.f, ng = 0.f, nr = 0.f, den = 0.f;
                auto tap = [&](int dy, int dx) {       // bilateral_chain_quad_kernel's tap()
                    if (dy == 0 && dx == 0) {
                        nb += cb; ng += cg; nr += cr; den += 1.f;
                        return;
                    }
                    const int ty = 2 + p + dy, tx = 2 + c + dx;
                    const float tb = qb[ty / 2][tx / 2], tg = qg[ty / 2][tx / 2][ty & 1], tr = qr[ty / 2][tx / 2];
                    const float dist = fabsf(tb - cb) + fabsf(tg - cg) + fabsf(tr - cr);
                    const float wgt = __builtin_amdgcn_exp2f(__builtin_fmaf(dist * dist, kc2, (float)(dy * dy + dx * dx) * ks2));
                    nb = __builtin_fmaf(wgt, tb, nb); ng = __builtin_fmaf(wgt, tg, ng); nr = __builtin_fmaf(wgt, tr, nr); den += wgt;
                };
                if (full) {
#pragma unroll
                    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                        for (int dx = -1; dx <= 1; ++dx) tap(dy, dx);
                } else {
                    tap(0, 0);                          // window 1: the weighted mean of one tap, then the 8-bit rounding
                }
                const float inv255 = 1.f / 255.f, rden = 1.f / den;
                pix[p][c] = {q8f(nb * rden) * inv255, q8f(ng * rden) * inv255, q8f(nr * rden) * inv255};
            }
    } else {
        // ---- no stencil: the patch's own two quads
        const ushort4 r0 = ld4(row_at(py), px), r1 = ld4(row_at(py + 1), px);
        const float R0 = smp(r0.x) / div, G10 = smp(r0.y) / div, R1 = smp(r0.z) / div, G11 = smp(r0.w) / div;
        const float G20 = smp(r1.x) / div, B0 = smp(r1.y) / div, G21 = smp(r1.z) / div, B1 = smp(r1.w) / div;
        pix[0][0] = pix[0][1] = {B0, G10, R0};
        pix[0][2] = pix[0][3] = {B1, G11, R1};
        pix[1][0] = pix[1][1] = {B0, G20, R0};
        pix[1][2] = pix[1][3] = {B1, G21, R1};
    }

    // ---- element-wise stages
    for (int k = 0; k < a.n_ops; ++k) apply_op<2 * PXT, WBQ>(a.ops[k], a.params[k], n, &pix[0][0]);

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
            f3 v = pix[p][c];
            if constexpr (CFA) {                        // value selects (a ?: between the two array elements selects an address)
                const f3 m = pix[p][PXT - 1 - c];
                const bool fx = flip & 1;
                v = {fx ? m.b : v.b, fx ? m.g : v.g, fx ? m.r : v.r};
            }
            const unsigned vb = u8(v.b), vg = u8(v.g), vr = u8(v.r);
            b[c][0] = a.reverse ? vr : vb;
            b[c][1] = vg;
            b[c][2] = a.reverse ? vb : vr;
        }
        unsigned *dst;
        if constexpr (CFA)
            dst = reinterpret_cast<unsigned *>(
                a.out + (((size_t)n * H + (flip & 2 ? H - 1 - py - p : py + p)) * W + (flip & 1 ? W - 4 - px : px)) * 3);
        else dst = reinterpret_cast<unsigned *>(a.out + (((size_t)n * H + py + p) * W + px) * 3);
        dst[0] = b[0][0] | b[0][1] << 8 | b[0][2] << 16 | b[1][0] << 24;
        dst[1] = b[1][1] | b[1][2] << 8 | b[2][0] << 16 | b[2][1] << 24;
        dst[2] = b[2][2] | b[3][0] << 8 | b[3][1] << 16 | b[3][2] << 24;
    }
}

// the rules both serving entry points share (include/risp.h), and the argument block; `name` is the entry point's, for the message
int serve_args_fill(const char *name, ServeArgs &a, bool &wbq, const uint16_t *raw, float divisor, const int32_t *window,
                    const float *sigma_color, const float *sigma_space, int max_window, int n_ops, const int *ops,
                    const float *const *params, uint8_t *out, int reverse_channels, int N, int H, int W, int raw_align = 8) {
    RISP_CHECK_ARG(raw && out, "%s: null argument", name);
    RISP_CHECK_ARG(divisor > 0.f, "%s: divisor %g", name, (double)divisor);
    RISP_CHECK_ARG(max_window == 0 || max_window == 1 || max_window == 3, "%s: window %d (0 = no bilateral, 1 or 3)", name, max_window);
    RISP_CHECK_ARG(max_window == 0 || (window && sigma_color && sigma_space), "%s: bilateral argument missing", name);
    RISP_CHECK_ARG(n_ops >= 0 && n_ops <= RISP_MAX_CHAIN && (n_ops == 0 || (ops && params)), "%s: bad op list", name);
    RISP_CHECK_ARG(N >= 1 && N <= 65535 && H >= 2 && H % 2 == 0 && W >= 4 && W % 4 == 0,
                   "%s: bad shape N=%d H=%d W=%d (H even, W a multiple of 4)", name, N, H, W);
    RISP_CHECK_ARG(reinterpret_cast<uintptr_t>(raw) % raw_align == 0 && reinterpret_cast<uintptr_t>(out) % 4 == 0,
                   "%s: raw must be %d-byte and out 4-byte aligned", name, raw_align);
    a.raw = raw;
    a.out = out;
    a.win = window;
    a.sig_c = sigma_color;
    a.sig_s = sigma_space;
    a.divisor = divisor;
    a.n_ops = n_ops;
    a.N = N;
    a.H = H;
    a.W = W;
    a.full_window = max_window == 3;
    a.reverse = reverse_channels ? 1 : 0;
    wbq = false;
    for (int k = 0; k < RISP_MAX_CHAIN; ++k) {
        a.ops[k] = RISP_OP_SKIP;
        a.params[k] = nullptr;
    }
    for (int k = 0; k < n_ops; ++k) {
        RISP_CHECK_ARG(ops[k] == RISP_OP_SKIP || (ops[k] >= RISP_OP_WB_MANUAL && ops[k] <= RISP_OP_GAIN3), "%s: op %d not allowed",
                       name, ops[k]);
        RISP_CHECK_ARG(ops[k] == RISP_OP_SKIP || params[k], "%s: stage %d has no parameter block", name, k);
        a.ops[k] = ops[k];
        a.params[k] = ops[k] == RISP_OP_SKIP ? nullptr : params[k];
        wbq |= ops[k] == RISP_OP_WB_QUADRATIC;
    }
    return 0;
}

dim3 serve_grid(int N, int H, int W) { return dim3((W / 4 + STX - 1) / STX, (H / 2 + STY - 1) / STY, N); }

template <int PACK, bool NV12>
void launch_packed(bool bil, bool wbq, dim3 grid, hipStream_t s, const ServePackedArgs &a) {
    if (bil) {
        if (wbq) hipLaunchKernelGGL((serve_kernel<true, true, true, NV12, PACK>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((serve_kernel<true, false, true, NV12, PACK>), grid, dim3(256), 0, s, a);
    } else {
        if (wbq) hipLaunchKernelGGL((serve_kernel<false, true, true, NV12, PACK>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((serve_kernel<false, false, true, NV12, PACK>), grid, dim3(256), 0, s, a);
    }
}

}  // namespace

extern "C" {

int risp_quantise_u8(const float *x, uint8_t *out, int N, int C, int H, int W, int reverse_channels, void *stream) {
    RISP_CHECK_ARG(x && out, "risp_quantise_u8: null argument");
    RISP_CHECK_ARG(N >= 1 && (C == 1 || C == 3) && H >= 1 && W >= 1, "risp_quantise_u8: bad shape N=%d C=%d H=%d W=%d (C is 1 or 3)", N,
                   C, H, W);
    const size_t hw = (size_t)H * W, total = (size_t)N * C * hw;
    hipStream_t s = (hipStream_t)stream;
    const int rev = reverse_channels ? 1 : 0;
    if (hw % 4 == 0 && hw / 4 <= 0x7fffffff && reinterpret_cast<uintptr_t>(x) % 16 == 0 && reinterpret_cast<uintptr_t>(out) % 4 == 0) {
        const size_t nvec = (size_t)N * (hw / 4), blocks = (nvec + 255) / 256;
        const dim3 grid((unsigned)(blocks > 65536 ? 65536 : blocks));
        if (C == 1) hipLaunchKernelGGL(quantise_vec_kernel<1>, grid, dim3(256), 0, s, x, out, nvec, (int)(hw / 4), rev);
        else hipLaunchKernelGGL(quantise_vec_kernel<3>, grid, dim3(256), 0, s, x, out, nvec, (int)(hw / 4), rev);
    } else {
        const size_t blocks = (total + 255) / 256;
        hipLaunchKernelGGL(quantise_any_kernel, dim3((unsigned)(blocks > 65536 ? 65536 : blocks)), dim3(256), 0, s, x, out, total, C,
                           hw, rev);
    }
    RISP_LAUNCH_CHECK("risp_quantise_u8");
    return 0;
}

int risp_quantise_u8_flip(const float *x, uint8_t *out, int N, int C, int H, int W, int reverse_channels, int flip, void *stream) {
    RISP_CHECK_ARG(x && out, "risp_quantise_u8_flip: null argument");
    RISP_CHECK_ARG(N >= 1 && (C == 1 || C == 3) && H >= 1 && W >= 1, "risp_quantise_u8_flip: bad shape N=%d C=%d H=%d W=%d (C is 1 or 3)",
                   N, C, H, W);
    RISP_CHECK_ARG(flip >= 0 && flip <= 3, "risp_quantise_u8_flip: flip %d (bit 0 mirrors x, bit 1 mirrors y)", flip);
    if (flip == 0) return risp_quantise_u8(x, out, N, C, H, W, reverse_channels, stream);
    const size_t hw = (size_t)H * W, total = (size_t)N * C * hw;
    hipStream_t s = (hipStream_t)stream;
    const int rev = reverse_channels ? 1 : 0, fx = flip & 1, fy = flip >> 1;
    if (W % 4 == 0 && reinterpret_cast<uintptr_t>(x) % 16 == 0 && reinterpret_cast<uintptr_t>(out) % 4 == 0) {
        const size_t nvec = (size_t)N * (hw / 4), blocks = (nvec + 255) / 256;
        const dim3 grid((unsigned)(blocks > 65536 ? 65536 : blocks));
        if (C == 1) hipLaunchKernelGGL(quantise_flip_vec_kernel<1>, grid, dim3(256), 0, s, x, out, nvec, H, W / 4, rev, fx, fy);
        else hipLaunchKernelGGL(quantise_flip_vec_kernel<3>, grid, dim3(256), 0, s, x, out, nvec, H, W / 4, rev, fx, fy);
    } else {
        const size_t blocks = (total + 255) / 256;
        hipLaunchKernelGGL(quantise_flip_any_kernel, dim3((unsigned)(blocks > 65536 ? 65536 : blocks)), dim3(256), 0, s, x, out,
                           total, C, H, W, rev, fx, fy);
    }
    RISP_LAUNCH_CHECK("risp_quantise_u8_flip");
    return 0;
}

int risp_serve_u8(const uint16_t *raw, float divisor, const int32_t *window, const float *sigma_color, const float *sigma_space,
                  int max_window, int n_ops, const int *ops, const float *const *params, uint8_t *out, int reverse_channels, int N,
                  int H, int W, void *stream) {
    ServeArgs a;
    bool wbq = false;
    if (int err = serve_args_fill("risp_serve_u8", a, wbq, raw, divisor, window, sigma_color, sigma_space, max_window, n_ops, ops,
                                  params, out, reverse_channels, N, H, W))
        return err;
    const dim3 grid = serve_grid(N, H, W);
    hipStream_t s = (hipStream_t)stream;
    if (max_window) {
        if (wbq) hipLaunchKernelGGL((serve_kernel<true, true>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((serve_kernel<true, false>), grid, dim3(256), 0, s, a);
    } else {
        if (wbq) hipLaunchKernelGGL((serve_kernel<false, true>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((serve_kernel<false, false>), grid, dim3(256), 0, s, a);
    }
    RISP_LAUNCH_CHECK("risp_serve_u8");
    return 0;
}

int risp_serve_u8_cfa(const uint16_t *raw, float divisor, const int32_t *window, const float *sigma_color,
                      const float *sigma_space, int max_window, int n_ops, const int *ops, const float *const *params, uint8_t *out,
                      int reverse_channels, int N, int H, int W, int black_level, int cfa, void *stream) {
    RISP_CHECK_ARG(cfa >= 0 && cfa <= 3, "risp_serve_u8_cfa: cfa %d (RISP_CFA_RGGB 0, GRBG 1, GBRG 2, BGGR 3)", cfa);
    RISP_CHECK_ARG(black_level >= 0 && black_level <= 65535, "risp_serve_u8_cfa: black_level %d outside 0 .. 65535", black_level);
    ServeCfaArgs a;
    bool wbq = false;
    if (int err = serve_args_fill("risp_serve_u8_cfa", a, wbq, raw, divisor, window, sigma_color, sigma_space, max_window, n_ops,
                                  ops, params, out, reverse_channels, N, H, W))
        return err;
    a.black = black_level;
    a.flip = cfa;
    const dim3 grid = serve_grid(N, H, W);
    hipStream_t s = (hipStream_t)stream;
    if (max_window) {
        if (wbq) hipLaunchKernelGGL((serve_kernel<true, true, true>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((serve_kernel<true, false, true>), grid, dim3(256), 0, s, a);
    } else {
        if (wbq) hipLaunchKernelGGL((serve_kernel<false, true, true>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((serve_kernel<false, false, true>), grid, dim3(256), 0, s, a);
    }
    RISP_LAUNCH_CHECK("risp_serve_u8_cfa");
    return 0;
}

int risp_serve_nv12(const uint16_t *raw, float divisor, const int32_t *window, const float *sigma_color, const float *sigma_space,
                    int max_window, int n_ops, const int *ops, const float *const *params, uint8_t *out, const int32_t coef[12], int N,
                    int H, int W, int black_level, int cfa, void *stream) {
    RISP_CHECK_ARG(cfa >= 0 && cfa <= 3, "risp_serve_nv12: cfa %d (RISP_CFA_RGGB 0, GRBG 1, GBRG 2, BGGR 3)", cfa);
    RISP_CHECK_ARG(black_level >= 0 && black_level <= 65535, "risp_serve_nv12: black_level %d outside 0 .. 65535", black_level);
    ServeNv12Args a;
    bool wbq = false;
    if (int err = serve_args_fill("risp_serve_nv12", a, wbq, raw, divisor, window, sigma_color, sigma_space, max_window, n_ops, ops,
                                  params, out, 0, N, H, W))
        return err;
    if (int err = risp_nv12::nv12_check("risp_serve_nv12", coef, a.yuv)) return err;
    a.black = black_level;
    a.flip = cfa;
    const dim3 grid = serve_grid(N, H, W);
    hipStream_t s = (hipStream_t)stream;
    // an RGGB sensor without a black level takes the instantiations without the mirror, as risp_serve_u8 is to risp_serve_u8_cfa
    // (max(s - 0, 0) == s and no address is mirrored: the same bytes, profiles/serve_cfa.txt has what the mirror costs)
    if (black_level == 0 && cfa == 0) {
        if (max_window) {
            if (wbq) hipLaunchKernelGGL((serve_kernel<true, true, false, true>), grid, dim3(256), 0, s, a);
            else hipLaunchKernelGGL((serve_kernel<true, false, false, true>), grid, dim3(256), 0, s, a);
        } else {
            if (wbq) hipLaunchKernelGGL((serve_kernel<false, true, false, true>), grid, dim3(256), 0, s, a);
            else hipLaunchKernelGGL((serve_kernel<false, false, false, true>), grid, dim3(256), 0, s, a);
        }
    } else if (max_window) {
        if (wbq) hipLaunchKernelGGL((serve_kernel<true, true, true, true>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((serve_kernel<true, false, true, true>), grid, dim3(256), 0, s, a);
    } else {
        if (wbq) hipLaunchKernelGGL((serve_kernel<false, true, true, true>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((serve_kernel<false, false, true, true>), grid, dim3(256), 0, s, a);
    }
    RISP_LAUNCH_CHECK("risp_serve_nv12");
    return 0;
}

int risp_serve_packed(const uint8_t *raw, int bits, int stride, float divisor, const int32_t *window, const float *sigma_color,
                      const float *sigma_space, int max_window, int n_ops, const int *ops, const float *const *params, uint8_t *out,
                      int reverse_channels, const int32_t *coef, int N, int H, int W, int black_level, int cfa, void *stream) {
    const char *name = "risp_serve_packed";
    RISP_CHECK_ARG(cfa >= 0 && cfa <= 3, "%s: cfa %d (RISP_CFA_RGGB 0, GRBG 1, GBRG 2, BGGR 3)", name, cfa);
    RISP_CHECK_ARG(black_level >= 0 && black_level <= 65535, "%s: black_level %d outside 0 .. 65535", name, black_level);
    ServePackedArgs a;
    bool wbq = false;
    if (int err = serve_args_fill(name, a, wbq, reinterpret_cast<const uint16_t *>(raw), divisor, window, sigma_color, sigma_space,
                                  max_window, n_ops, ops, params, out, coef ? 0 : reverse_channels, N, H, W, 1))
        return err;
    if (int err = risp_rawpack::rawpack_check(name, bits, W, stride)) return err;
    for (int i = 0; i < 12; ++i) a.yuv.k[i] = 0;
    if (coef)
        if (int err = risp_nv12::nv12_check(name, coef, a.yuv)) return err;
    a.black = black_level;
    a.flip = cfa;
    a.stride = stride;
    const dim3 grid = serve_grid(N, H, W);
    hipStream_t s = (hipStream_t)stream;
    if (bits == 10) {
        if (coef) launch_packed<10, true>(max_window != 0, wbq, grid, s, a);
        else launch_packed<10, false>(max_window != 0, wbq, grid, s, a);
    } else {
        if (coef) launch_packed<12, true>(max_window != 0, wbq, grid, s, a);
        else launch_packed<12, false>(max_window != 0, wbq, grid, s, a);
    }
    RISP_LAUNCH_CHECK(name);
    return 0;
}

}  // extern "C"
