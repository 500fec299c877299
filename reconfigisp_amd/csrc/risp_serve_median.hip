// Serving path for the classical pipelines that hold ONE median of a learned size above 3: a 16-bit Bayer frame in, a packed
// 8-bit image out, ONE launch.
//
//     max(sample - black, 0) / divisor -> nearest | bilinear | Malvar-He-Cutler demosaic -> P stages
//         -> K x K median of the 8-bit codes (K = 5, 7, 9, 11, 13, 15) -> Q stages -> clip(v * 255) truncated
//
// risp_serve_denoise_u8 serves the median at 3 x 3, the size OriginNoiseMedian's rule gives below p = 1/7; this is the same
// route for 2 * int(p * 7) + 3 at every other unsaturated p.  A workgroup owns a 64 x 32 pixel tile, as there, and works in
// two phases around one LDS image of 8-bit CODES packed four to a dword (a patch row is one dword per channel):
//
//     K          5      7      9      11     13     15
//     ring rows  2      4      4      6      6      8       the radius rounded up to even: whole 2 x 4 patches
//     ring cols  4      4      4      8      8      8
//     image      36x72  40x72  40x72  44x80  44x80  48x80   bytes per channel; 7776 .. 11520 bytes of LDS in all
//     patches    324    360    360    440    440    480     against the 256 inside the tile
//
//   phase 1  the patches of 2 x 4 pixels that cover the LDS image - demosaic and the P stages as every route evaluates a patch
//            (risp_serve_dentile.h's front_patches, the walk the 3 x 3 denoisers' kernel takes) - stored as the codes
//            q8(value x 255), the median's input (stage_tile4<true> / median4_kernel's staging form them from the fp32 planes
//            of the composed route).
//            Patches outside the image are skipped; after a barrier the ring positions outside the image that a window can
//            reach copy the code at the reflect-101 IMAGE coordinate from LDS.  H > K/2 and W > K/2 make that a single
//            reflection, and its source lies in the same workgroup's LDS image: above the image the source row -y <= K/2 lies
//            in the tile at y0 = 0, which holds rows up to 31 + ring >= K/2; below it the source 2H-2-y >= H-1-K/2, and a tile
//            that holds row y >= H starts at y0 <= H-2, so its first LDS row y0 - ring <= H-2-ring < H-1-K/2 - also for a last
//            tile of 2 rows, thinner than the ring.  Columns alike with x0 <= W-4 and ring + 3 >= K/2.
//   phase 2  after the barrier a thread takes its own 2 x 4 patch pixel by pixel and channel by channel: the K window rows
//            are 3 or 5 dwords each, v_alignbyte cuts the pixel's K codes out, the window stays in registers (K*K/4 dwords)
//            through a bisection on the code whose rank counts come from v_sad_u8 - median4_kernel's method
//            (risp_origin.hip), restated: the smallest code whose rank reaches K*K/2 + 1, which is what median_kernel computes
//            too.  The code x (1 / 255) enters the Q stages in registers and 12 bytes per row are stored as serve_kernel does.
//
// With -ffp-contract=off the bytes are the composed route's (tests/test_gpu_serve_median.py, torch.equal).  Black level and
// Bayer phase as in risp_serve_u8_cfa: the phase is a mirror of addresses; coordinates, reflection, parity and the tile grid
// live in the mirrored (RGGB) image.
#include "risp_serve_dentile.h"

namespace {

using namespace risp_patch;

struct MedianArgs : PatchArgs {
    uint8_t *out;               // (N,H,W,3)
    int reverse;                // store R, G, B instead of B, G, R
};

// KIND: RISP_DEMOSAIC_*, K: the median's size.  Every coordinate is one of the mirrored image, which is RGGB
template <int KIND, int K, bool WBQ>
__global__ __launch_bounds__(256) void serve_median_kernel(const MedianArgs a) {
    constexpr int R = K / 2;
    // the LDS image of this K (the names hide risp_serve_dentile.h's, which are the 3 x 3 denoisers' image)
    constexpr int RING_Y = (R + 1) & ~1, RING_X = R <= 4 ? 4 : 8;          // LDS rows above / columns left of the tile (whole patches)
    constexpr int LWD = (TILE_W + 2 * RING_X) / 4, LH = TILE_H + 2 * RING_Y, LPLANE = LH * LWD;   // dwords per row, rows, dwords per channel
    constexpr int PCOLS = LWD, PROWS = LH / 2;
    static_assert(R <= RING_X && R <= RING_Y && K >= 5 && K <= 15 && (K & 1), "the ring must hold the window");
    __shared__ unsigned tile[3 * LPLANE];              // [3][LH][LWD] packed codes: byte k of a dword is column 4 * dword + k
    const int H = a.H, W = a.W;
    int bxi, byi, bzi;
    xcd_tile(bxi, byi, bzi);
    const int n = bzi, x0 = bxi * TILE_W, y0 = byi * TILE_H;
    const int flip = a.flip;
    const Mosaic mo(a, n);

    // ---- phase 1, stored in the median's domain: the 8-bit code of value x in_scale (255), four of a row to a dword
    front_patches<KIND, WBQ, false, RING_X, RING_Y, PCOLS, PROWS>(a, mo, n, x0, y0, [&](int pr, int pc, const f3 (&pix)[2][PXT]) {
        auto code = [&](float v) { return (unsigned)q8(v * 255.f); };
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            unsigned *dst = tile + (pr * 2 + p) * LWD + pc;
            dst[0] = code(pix[p][0].b) | code(pix[p][1].b) << 8 | code(pix[p][2].b) << 16 | code(pix[p][3].b) << 24;
            dst[LPLANE] = code(pix[p][0].g) | code(pix[p][1].g) << 8 | code(pix[p][2].g) << 16 | code(pix[p][3].g) << 24;
            dst[2 * LPLANE] = code(pix[p][0].r) | code(pix[p][1].r) << 8 | code(pix[p][2].r) << 16 | code(pix[p][3].r) << 24;
        }
    });
    __syncthreads();

    // ---- ring positions outside the image within a window's reach: the code at the reflect-101 image coordinate.  A dword
    // lies inside the image or outside it as a whole (its first column is a multiple of 4, and so is W); the dwords written
    // here lie outside, the bytes read inside.  Only tiles on the image border have any (a workgroup-uniform condition: the
    // barrier inside is reached by all or by none)
    if (border_tile(x0, y0, H, W, R)) {
        const unsigned char *codes = reinterpret_cast<const unsigned char *>(tile);
        // the columns of the image this LDS image holds: a byte beyond the reach is read by no window, its source only has to exist
        const int cx0 = x0 - RING_X > 0 ? x0 - RING_X : 0, cx1 = (x0 + TILE_W + RING_X < W ? x0 + TILE_W + RING_X : W) - 1;
        for (int idx = threadIdx.x; idx < LPLANE; idx += 256) {
            const int r = idx / LWD, dj = idx - r * LWD;
            const int gy = y0 - RING_Y + r, gx = x0 - RING_X + 4 * dj;
            if (gy < -R || gy >= H + R || gx + 3 < -R || gx >= W + R) continue;
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) continue;
            const int sy = reflect101(gy, H);
            const int srow = (sy - y0 + RING_Y) * LWD * 4 - x0 + RING_X;
            unsigned v[3] = {0u, 0u, 0u};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                int sx = reflect101(gx + k, W);
                sx = sx < cx0 ? cx0 : (sx > cx1 ? cx1 : sx);
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c] |= (unsigned)codes[c * LPLANE * 4 + srow + sx] << (8 * k);
            }
            tile[idx] = v[0];
            tile[idx + LPLANE] = v[1];
            tile[idx + 2 * LPLANE] = v[2];
        }
        __syncthreads();
    }

    // ---- phase 2: the thread's own patch, a row of 4 pixels at a time
    const int lxd = (int)(threadIdx.x % STX), ly = (int)(threadIdx.x / STX) * 2;
    const int px = x0 + lxd * PXT, py = y0 + ly;
    if (px >= W || py >= H) return;
    constexpr int NDW = (2 * RING_X + 4) / 4;          // dwords of an LDS row that cover the thread's four windows
    constexpr int ND = K / 4, NE = K % 4;              // full dwords and leftover codes per window row
    constexpr int NL = K * NE, NLD = NL / 4, NLS = NL % 4;   // the leftovers of all rows, packed four to a dword again
    constexpr int NW = K * ND + NLD;
    constexpr int OFF = RING_X - R;                    // first byte of pixel 0's window row among the bytes loaded
#pragma unroll 1
    for (int p = 0; p < 2; ++p) {
        unsigned cb = 0, cg = 0, cr = 0;               // the four medians of a channel, packed as the codes are
#pragma unroll 1
        for (int c = 0; c < 3; ++c) {
            unsigned acc = 0;
#pragma unroll 1
            for (int i = 0; i < PXT; ++i) {
                unsigned wd[NW];                                   // the window as packed dwords: row pieces, then leftovers
                int ws[NLS > 0 ? NLS : 1], left[NL];               // codes that fill no dword
#pragma unroll
                for (int r = 0; r < K; ++r) {
                    const unsigned *row = tile + c * LPLANE + (ly + p + RING_Y - R + r) * LWD + lxd;   // image columns px-RING_X .. px+RING_X+3
                    unsigned d[NDW];
#pragma unroll
                    for (int j = 0; j < NDW; ++j) d[j] = row[j];
                    // pixel i's bytes start i further on: shift the row once, then every offset is known at compile time
#pragma unroll
                    for (int j = 0; j + 1 < NDW; ++j) d[j] = __builtin_amdgcn_alignbyte(d[j + 1], d[j], (unsigned)i);
                    d[NDW - 1] = __builtin_amdgcn_alignbyte(0u, d[NDW - 1], (unsigned)i);
#pragma unroll
                    for (int j = 0; j < ND; ++j) {
                        const int b = OFF + 4 * j;
                        wd[r * ND + j] = (b & 3) ? __builtin_amdgcn_alignbyte(d[(b >> 2) + 1 < NDW ? (b >> 2) + 1 : NDW - 1], d[b >> 2], (unsigned)(b & 3))
                                                 : d[b >> 2];
                    }
#pragma unroll
                    for (int e = 0; e < NE; ++e) {
                        const int b = OFF + 4 * ND + e;
                        left[r * NE + e] = (int)((d[b >> 2] >> (8 * (b & 3))) & 0xffu);
                    }
                }
#pragma unroll
                for (int g = 0; g < NLD; ++g)
                    wd[K * ND + g] = (unsigned)left[4 * g] | ((unsigned)left[4 * g + 1] << 8) | ((unsigned)left[4 * g + 2] << 16) |
                                     ((unsigned)left[4 * g + 3] << 24);
#pragma unroll
                for (int e = 0; e < NLS; ++e) ws[e] = left[4 * NLD + e];
                int lo = 0, hi = 255;                  // smallest code v with #(x <= v) >= need
                constexpr int need = (K * K) / 2 + 1, n8 = 4 * NW;
#pragma unroll 1
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;    // <= 254
                    const unsigned m4 = (unsigned)mid * 0x01010101u, m4p = m4 + 0x01010101u;
                    unsigned sm = 0, sp = 0;
                    int cnt = 0;
#pragma unroll
                    for (int j = 0; j < NW; ++j) {
                        sm = __builtin_amdgcn_sad_u8(wd[j], m4, sm);
                        sp = __builtin_amdgcn_sad_u8(wd[j], m4p, sp);
                    }
#pragma unroll
                    for (int e = 0; e < NLS; ++e) cnt += ws[e] <= mid ? 1 : 0;
                    cnt += ((int)sp - (int)sm + n8) >> 1;
                    if (cnt >= need) hi = mid; else lo = mid + 1;
                }
                acc |= (unsigned)lo << (8 * i);
            }
            if (c == 0) cb = acc;
            else if (c == 1) cg = acc;
            else cr = acc;
        }
        f3 o[PXT];
        const float inv255 = 1.f / 255.f;
#pragma unroll
        for (int i = 0; i < PXT; ++i)
            o[i] = {(float)((cb >> (8 * i)) & 0xffu) * inv255, (float)((cg >> (8 * i)) & 0xffu) * inv255,
                    (float)((cr >> (8 * i)) & 0xffu) * inv255};

        run_stages<PXT, WBQ>(a, a.n_pre, a.n_ops, n, o);
        store_bgr4(a.out, n, H, W, py + p, px, flip, a.reverse, o);
    }
}

// calls f(std::integral_constant<int, K>) for the median's size (as the entry point passed it)
template <class F>
void with_size(int size, F &&f) {
    if (size == 5) f(std::integral_constant<int, 5>{});
    else if (size == 7) f(std::integral_constant<int, 7>{});
    else if (size == 9) f(std::integral_constant<int, 9>{});
    else if (size == 11) f(std::integral_constant<int, 11>{});
    else if (size == 13) f(std::integral_constant<int, 13>{});
    else f(std::integral_constant<int, 15>{});
}

}  // namespace

extern "C" int risp_serve_median_u8(const uint16_t *raw, float divisor, int demosaic, int n_pre, const int *pre_ops,
                                    const float *const *pre_params, int size, int n_post, const int *post_ops,
                                    const float *const *post_params, uint8_t *out, int reverse_channels, int N, int H, int W,
                                    int black_level, int cfa, void *stream) {
    const char *name = "risp_serve_median_u8";
    RISP_CHECK_ARG(size >= 5 && size <= 15 && (size & 1),
                   "%s: median size %d (5, 7, .. 15 are served here; 3 is risp_serve_denoise_u8's, 17 composes)", name, size);
    RISP_CHECK_ARG(N >= 1 && N <= 65535 && H >= 4 && H % 2 == 0 && H > size / 2 && W >= 4 && W % 4 == 0 && W > size / 2,
                   "%s: bad shape N=%d H=%d W=%d for size %d (H even, >= 4 and > size / 2, W a multiple of 4 and > size / 2)", name,
                   N, H, W, size);
    ArgRules r;
    r.split = true;
    MedianArgs a;
    bool wbq;
    if (int e = serve_args(name, r, a, wbq, raw, out, divisor, demosaic, n_pre, pre_ops, pre_params, n_post, post_ops, post_params, N, H, W,
                           black_level, cfa))
        return e;
    a.out = out;
    a.reverse = reverse_channels ? 1 : 0;
    with_form(demosaic, wbq, [&](auto kind_c, auto wbq_c) {
        with_size(size, [&](auto size_c) {
            hipLaunchKernelGGL((serve_median_kernel<decltype(kind_c)::value, decltype(size_c)::value, decltype(wbq_c)::value>),
                               patch_grid(N, H, W), dim3(256), 0, (hipStream_t)stream, a);
        });
    });
    RISP_LAUNCH_CHECK("risp_serve_median_u8");
    return 0;
}
