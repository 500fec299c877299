// Serving path for pipelines with conditional heads (ConditionalGamma / ConditionalWbManual / ConditionalWbQuadratic): an MLP on
// the per-channel histogram of the head's input predicts the head's parameters per image.  A histogram is a whole-image
// quantity, and every value that feeds it is a pure function of a 6 x 8 mosaic neighbourhood, so - as on the scene route - the
// 2-byte mosaic is read once more per head instead of fp32 planes being written and read:
//
//     risp_serve_cond_hist     the pixel pipeline of risp_serve_classical_u8 up to the head, binned: integer counts
//     risp_serve_cond_finish   the counts of an image, summed in integers, through the head's MLP: the head's (N,k) block
//
// and risp_serve_classical_u8 serves with the head as its element-wise op.  The patch loader, the two demosaics and the stage
// loop restate serve_scene_kernel<KIND, WBQ, true> (risp_serve_scene.hip), the bin rule restates histc_kernel
// (risp_reduce.hip) and the MLP restates cond_fc_fwd_kernel (risp_condfc.hip): those files stay as measured.  With
// -ffp-contract=off a pixel's value in front of the head has the bits of the composed route; counts are integers, which have no
// summation order; so the block - and every byte served with it - is the composed route's.
#include <math.h>

#include "risp_common.h"
#include "risp_ops.h"

namespace {

using namespace risp_ops;

// the 8-bit code of a value in the 0..255 domain (risp_origin.hip q8; v is never NaN here)
__device__ __forceinline__ float q8(float v) { return floorf(__builtin_amdgcn_fmed3f(v, 0.f, 255.f) + 0.5f); }

__device__ __forceinline__ float hable(float t) {
    const float A = 0.15f, B = 0.50f, C = 0.10f, D = 0.20f, E = 0.02f, F = 0.30f;
    return (t * (A * t + C * B) + D * E) / (t * (A * t + B) + D * F) - E / F;
}

// (ablation builds of tools/ab_serve_cond.py set these two; the library is built with the header's shard count and 64 copies)
#ifndef RISP_COND_AB_SHARDS
#define RISP_COND_AB_SHARDS RISP_COND_SHARDS
#endif
#ifndef RISP_COND_AB_COPIES
#define RISP_COND_AB_COPIES 64
#endif
constexpr int SHARDS = RISP_COND_AB_SHARDS;
constexpr int LDS_WORDS = 4096;                          // 16 KB of private histograms per workgroup at the most

struct CondArgs {
    const uint16_t *raw;        // (N,H,W) mosaic of the sensor
    unsigned int *counts;       // (N,SHARDS,3*bins), zeroed by the entry point
    float divisor;
    int n_ops, N, H, W;
    int black;                  // subtracted from every sample in integers, clamped at 0
    int flip;                   // RISP_CFA_*: bit 0 mirrors x, bit 1 mirrors y
    int bins, copies;           // copies: private histograms per workgroup, a power of two
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

// KIND: RISP_DEMOSAIC_*.  px, py and every coordinate derived from them are those of the mirrored image, which is RGGB; only
// row_at / ld2 / ld4 know where the samples really are (a histogram does not).  Nothing is stored but counts: the values behind
// the n_ops stages are binned into private LDS histograms, and the workgroup adds its totals to shard (tile % SHARDS) of its image
template <int KIND, bool WBQ>
__global__ __launch_bounds__(256) void serve_cond_hist_kernel(const CondArgs a) {
    extern __shared__ unsigned int sh[];                // [3 * bins][copies]: bin-major, lane l counts into copy l % copies
    const int H = a.H, W = a.W;
    const int bins = a.bins, copies = a.copies, words = 3 * bins;
    for (int b = threadIdx.x; b < words * copies; b += 256) sh[b] = 0u;
    int bxi, byi, bzi;
    xcd_tile(bxi, byi, bzi);
    const int n = bzi;
    const int px = (bxi * STX + (int)(threadIdx.x % STX)) * 4, py = (byi * STY + (int)(threadIdx.x / STX)) * 2;
    const bool live = px < W && py < H;                 // W % 4 == 0, H % 2 == 0: a patch is in or out as a whole
    f3 pix[2][PXT];                                     // (a thread outside the image counts nothing and stays for the barriers)
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

        // ---- the prefix stages: the tone curves here, the rest in risp_ops.h.  An earlier head is its element-wise op with
        // the block of its own risp_serve_cond_finish
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
    }

    // ---- histc_kernel's rule on the thread's 8 pixels x 3 channels (B, G, R as histc01 sees the planes): NaN and values
    // outside [0,1] count nowhere, 1 lands in the last bin
    __syncthreads();                                    // the zeros above
    if (live) {
        const int cp = threadIdx.x & (copies - 1);
        const float fb = (float)bins;
        auto count = [&](float v, int c) {
            if (v >= 0.f && v <= 1.f) {
                int pos = (int)(v * fb);
                if (pos >= bins) pos = bins - 1;
                atomicAdd(&sh[(c * bins + pos) * copies + cp], 1u);
            }
        };
#pragma unroll
        for (int i = 0; i < 2 * PXT; ++i) {
            const f3 v = (&pix[0][0])[i];
            count(v.b, 0);
            count(v.g, 1);
            count(v.r, 2);
        }
    }
    __syncthreads();
    // ---- the workgroup's totals: thread b adds the copies of word b (starting at copy b, so that neighbouring threads read
    // different banks) and adds a total that is not zero to its shard.  Integers: no order enters the result
    const unsigned tile = (unsigned)byi * gridDim.x + (unsigned)bxi;
    unsigned int *dst = a.counts + ((size_t)n * SHARDS + tile % SHARDS) * words;
    for (int b = threadIdx.x; b < words; b += 256) {
        unsigned int t = 0u;
        for (int k = 0; k < copies; ++k) t += sh[b * copies + ((k + b) & (copies - 1))];
        if (t) atomicAdd(&dst[b], t);
    }
}

// ---- the head's MLP: FcShape, make_shape and the expression sequence of cond_fc_fwd_kernel (risp_condfc.hip)
constexpr int FC_MAXL = 8;          // layers
constexpr int FC_MAXW = 1024;       // widest layer

struct FcShape {
    int n_layers;                   // number of weight matrices
    int w[FC_MAXL + 1];             // widths w[0] .. w[n_layers]
    int wofs[FC_MAXL], bofs[FC_MAXL];   // offsets of W_l, b_l in flat
    int gofs;                       // offset of the global scalar
};

// One workgroup per image.  Word i of the image's SHARDS rows, added in integers and converted once (exact up to 2^24, the
// entry point's H * W rule), is what risp_histc gives the composed route; then its layers, + global, sigmoid, and * scale as one
// fp32 multiply (the * 5 of ConditionalWbManual).  No activation row: serving has no backward
__global__ __launch_bounds__(256) void serve_cond_finish_kernel(const unsigned int *__restrict__ counts, int shards,
                                                                const float *__restrict__ flat, float *__restrict__ block, float scale,
                                                                FcShape s) {
    __shared__ float a[2][FC_MAXW];
    const int n = blockIdx.x, t = threadIdx.x;
    const unsigned int *rows = counts + (size_t)n * shards * s.w[0];
    for (int i = t; i < s.w[0]; i += 256) {
        unsigned int c = 0u;
        for (int k = 0; k < shards; ++k) c += rows[(size_t)k * s.w[0] + i];
        a[0][i] = (float)c;
    }
    __syncthreads();
    for (int l = 0; l < s.n_layers; ++l) {
        const int fi = s.w[l], fo = s.w[l + 1];
        const float *W = flat + s.wofs[l], *b = flat + s.bofs[l];
        const float *src = a[l & 1];
        float *dst = a[(l + 1) & 1];
        const bool last = l == s.n_layers - 1;
        for (int j = t; j < fo; j += 256) {
            float z = 0.f;
            for (int i = 0; i < fi; ++i) z += src[i] * W[(size_t)i * fo + j];     // feat @ weight: k-ordered like the reference
            z += b[j];
            if (last) {
                z += flat[s.gofs];
                const float o = 1.f / (1.f + __expf(-z));
                block[(size_t)n * fo + j] = scale == 1.f ? o : o * scale;
            } else {
                z = z > 0.f ? z : 0.f;
            }
            dst[j] = z;
        }
        __syncthreads();
    }
}

int make_shape(const int *widths, int n_layers, FcShape &s, const char *who) {
    RISP_CHECK_ARG(widths && n_layers >= 1 && n_layers <= FC_MAXL, "%s: 1..%d layers (n_layers %d)", who, FC_MAXL, n_layers);
    s.n_layers = n_layers;
    for (int l = 0; l <= n_layers; ++l) {
        RISP_CHECK_ARG(widths[l] >= 1 && widths[l] <= FC_MAXW, "%s: layer width %d (1..%d)", who, widths[l], FC_MAXW);
        s.w[l] = widths[l];
    }
    int at = 0;
    for (int l = 0; l < n_layers; ++l) {
        s.wofs[l] = at;
        at += widths[l] * widths[l + 1];
        s.bofs[l] = at;
        at += widths[l + 1];
    }
    s.gofs = at;
    return 0;
}

template <int KIND>
void launch_kind(bool wbq, dim3 grid, size_t lds, hipStream_t s, const CondArgs &a) {
    if (wbq) hipLaunchKernelGGL((serve_cond_hist_kernel<KIND, true>), grid, dim3(256), lds, s, a);
    else hipLaunchKernelGGL((serve_cond_hist_kernel<KIND, false>), grid, dim3(256), lds, s, a);
}

}  // namespace

extern "C" int risp_serve_cond_hist(const uint16_t *raw, float divisor, int demosaic, int n_ops, const int *ops,
                                    const float *const *params, int bins, unsigned int *counts, int N, int H, int W, int black_level,
                                    int cfa, void *stream) {
    const char *name = "risp_serve_cond_hist";
    RISP_CHECK_ARG(raw && counts, "%s: null argument (%s)", name, raw ? "counts" : "raw");
    RISP_CHECK_ARG(divisor > 0.f, "%s: divisor %g", name, (double)divisor);
    RISP_CHECK_ARG(demosaic >= RISP_DEMOSAIC_NEAREST && demosaic <= RISP_DEMOSAIC_LAPLACIAN,
                   "%s: demosaic %d (RISP_DEMOSAIC_NEAREST 0, BILINEAR 1, LAPLACIAN 2)", name, demosaic);
    RISP_CHECK_ARG(cfa >= 0 && cfa <= 3, "%s: cfa %d (RISP_CFA_RGGB 0, GRBG 1, GBRG 2, BGGR 3)", name, cfa);
    RISP_CHECK_ARG(black_level >= 0 && black_level <= 65535, "%s: black_level %d outside 0 .. 65535", name, black_level);
    RISP_CHECK_ARG(bins >= 1 && 3 * (long long)bins <= FC_MAXW, "%s: bins %d (1 <= bins, 3 * bins <= %d)", name, bins, FC_MAXW);
    RISP_CHECK_ARG(!((cfa & 1) && W % 2) && !((cfa & 2) && H % 2), "%s: cfa %d mirrors an odd axis (H=%d W=%d)", name, cfa, H, W);
    RISP_CHECK_ARG(N >= 1 && N <= 65535 && H >= 4 && H % 2 == 0 && W >= 4 && W % 4 == 0,
                   "%s: bad shape N=%d H=%d W=%d (1 <= N <= 65535, H even and >= 4, W a multiple of 4)", name, N, H, W);
    RISP_CHECK_ARG((long long)H * W <= (1ll << 24), "%s: H * W = %lld above 2^24 (float counts stop being exact)", name, (long long)H * W);
    RISP_CHECK_ARG(n_ops >= 0 && n_ops <= RISP_MAX_CHAIN && (n_ops == 0 || (ops && params)), "%s: bad op list (n_ops %d)", name, n_ops);
    RISP_CHECK_ARG(reinterpret_cast<uintptr_t>(raw) % 8 == 0, "%s: raw must be 8-byte aligned", name);
    RISP_CHECK_ARG(reinterpret_cast<uintptr_t>(counts) % 4 == 0, "%s: counts must be 4-byte aligned", name);
    CondArgs a;
    a.raw = raw;
    a.counts = counts;
    a.divisor = divisor;
    a.n_ops = n_ops;
    a.N = N;
    a.H = H;
    a.W = W;
    a.black = black_level;
    a.flip = cfa;
    a.bins = bins;
    bool wbq = false;
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
    // private histograms per workgroup: as many as a wavefront has lanes while they fit 16 KB (no two lanes of a wavefront
    // then share a word, and copy c lies on bank c), halved until they do.  (profiles/serve_cond_ab.txt: 16 copies measured
    // about 10 % faster for this launch alone - fewer words to zero and add up; not adopted before the whole suite ran with it)
    int copies = RISP_COND_AB_COPIES;
    while (copies > 1 && 3 * bins * copies > LDS_WORDS) copies >>= 1;
    a.copies = copies;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(counts, 0, sizeof(unsigned int) * (size_t)N * SHARDS * 3 * bins, s) != hipSuccess) {
        risp_set_error("%s: memset failed", name);
        return 2;
    }
    const dim3 grid((W / 4 + STX - 1) / STX, (H / 2 + STY - 1) / STY, N);
    const size_t lds = sizeof(unsigned int) * 3 * bins * copies;
    if (demosaic == RISP_DEMOSAIC_LAPLACIAN) launch_kind<RISP_DEMOSAIC_LAPLACIAN>(wbq, grid, lds, s, a);
    else if (demosaic == RISP_DEMOSAIC_BILINEAR) launch_kind<RISP_DEMOSAIC_BILINEAR>(wbq, grid, lds, s, a);
    else launch_kind<RISP_DEMOSAIC_NEAREST>(wbq, grid, lds, s, a);
    RISP_LAUNCH_CHECK("risp_serve_cond_hist");
    return 0;
}

extern "C" int risp_serve_cond_finish(const unsigned int *counts, int shards, const float *flat, const int *widths, int n_layers,
                                      float scale, float *block, int N, void *stream) {
    const char *name = "risp_serve_cond_finish";
    RISP_CHECK_ARG(counts && flat && block, "%s: null argument", name);
    RISP_CHECK_ARG(shards >= 1 && shards <= 65535, "%s: shards %d (1 .. 65535; risp_serve_cond_hist writes RISP_COND_SHARDS)", name, shards);
    RISP_CHECK_ARG(N >= 1 && N <= 65535, "%s: N=%d outside 1 .. 65535", name, N);
    RISP_CHECK_ARG(scale > 0.f && scale <= 3.4e38f, "%s: scale %g", name, (double)scale);
    FcShape s;
    if (int e = make_shape(widths, n_layers, s, name)) return e;
    hipLaunchKernelGGL(serve_cond_finish_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, counts, shards, flat, block, scale, s);
    RISP_LAUNCH_CHECK("risp_serve_cond_finish");
    return 0;
}
