// Serving path for pipelines with conditional heads (ConditionalGamma / ConditionalWbManual / ConditionalWbQuadratic): an MLP on
// the per-channel histogram of the head's input predicts the head's parameters per image.  A histogram is a whole-image
// quantity, and every value that feeds it is a pure function of a 6 x 8 mosaic neighbourhood, so - as on the scene route - the
// 2-byte mosaic is read once more per head instead of fp32 planes being written and read:
//
//     risp_serve_cond_hist     the pixel pipeline of risp_serve_classical_u8 up to the head, binned: integer counts
//     risp_serve_cond_finish   the counts of an image, summed in integers, through the head's MLP: the head's (N,k) block
//
// and risp_serve_classical_u8 serves with the head as its element-wise op.  The patch - loads, demosaic, stages - is
// risp_serve_patch.h's; this file owns the histogram and the MLP.  The bin rule restates histc_kernel (risp_reduce.hip) and the
// MLP restates cond_fc_fwd_kernel (risp_condfc.hip): those files stay as measured.  With -ffp-contract=off a pixel's value in
// front of the head has the bits of the composed route; counts are integers, which have no summation order; so the block - and
// every byte served with it - is the composed route's.
#include <math.h>

#include "risp_serve_patch.h"

namespace {

using namespace risp_patch;

// (ablation builds of tools/ab_serve_cond.py set these two; the library is built with the header's shard count and 64 copies)
#ifndef RISP_COND_AB_SHARDS
#define RISP_COND_AB_SHARDS RISP_COND_SHARDS
#endif
#ifndef RISP_COND_AB_COPIES
#define RISP_COND_AB_COPIES 64
#endif
constexpr int SHARDS = RISP_COND_AB_SHARDS;
constexpr int LDS_WORDS = 4096;                          // 16 KB of private histograms per workgroup at the most

struct CondArgs : PatchArgs {
    unsigned int *counts;       // (N,SHARDS,3*bins), zeroed by the entry point
    int bins, copies;           // copies: private histograms per workgroup, a power of two
};

// KIND: RISP_DEMOSAIC_*.  Nothing is stored but counts: the values behind the n_ops stages are binned into private LDS histograms,
// and the workgroup adds its totals to shard (tile % SHARDS) of its image (a histogram does not know the Bayer phase)
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
        const Patch d = Mosaic(a, n).patch<KIND>(px, py);
#pragma unroll
        for (int i = 0; i < 2 * PXT; ++i) (&pix[0][0])[i] = (&d.p[0][0])[i];
        // ---- the prefix stages.  An earlier head is its element-wise op with the block of its own risp_serve_cond_finish
        run_stages<2 * PXT, WBQ>(a, 0, a.n_ops, n, &pix[0][0]);
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

}  // namespace

extern "C" int risp_serve_cond_hist(const uint16_t *raw, float divisor, int demosaic, int n_ops, const int *ops,
                                    const float *const *params, int bins, unsigned int *counts, int N, int H, int W, int black_level,
                                    int cfa, void *stream) {
    const char *name = "risp_serve_cond_hist";
    RISP_CHECK_ARG(bins >= 1 && 3 * (long long)bins <= FC_MAXW, "%s: bins %d (1 <= bins, 3 * bins <= %d)", name, bins, FC_MAXW);
    RISP_CHECK_ARG(!((cfa & 1) && W % 2) && !((cfa & 2) && H % 2), "%s: cfa %d mirrors an odd axis (H=%d W=%d)", name, cfa, H, W);
    ArgRules r;
    r.out_here = false;
    r.shape_note = "1 <= N <= 65535, H even and >= 4, W a multiple of 4";
    CondArgs a;
    bool wbq;
    if (int e = serve_args(name, r, a, wbq, raw, nullptr, divisor, demosaic, n_ops, ops, params, 0, nullptr, nullptr, N, H, W, black_level, cfa))
        return e;
    RISP_CHECK_ARG(counts, "%s: null argument (counts)", name);
    RISP_CHECK_ARG((long long)H * W <= (1ll << 24), "%s: H * W = %lld above 2^24 (float counts stop being exact)", name, (long long)H * W);
    RISP_CHECK_ARG(reinterpret_cast<uintptr_t>(counts) % 4 == 0, "%s: counts must be 4-byte aligned", name);
    a.counts = counts;
    a.bins = bins;
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
    const size_t lds = sizeof(unsigned int) * 3 * bins * copies;
    with_form(demosaic, wbq, [&](auto kind_c, auto wbq_c) {
        hipLaunchKernelGGL((serve_cond_hist_kernel<decltype(kind_c)::value, decltype(wbq_c)::value>), patch_grid(N, H, W), dim3(256), lds, s, a);
    });
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
