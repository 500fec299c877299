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
// stencil needs finished neighbours, so the statistic takes the tile form: serve_denoise_kernel of risp_serve_dentile.h, the ONE
// kernel template behind all three denoise entry points - <.., GAIN = true, STATS = false> for the serving launch (the stage loop
// with white-world's apply), <.., true, true> for the statistics launch (no image; the reduction per workgroup).  This file is the
// two entry points and their rules.
//
// With -ffp-contract=off a pixel's value has the bits of the composed route, so a maximum - which has no order - gives the
// composed route's constants and bytes; a sum taken in this order gives constants that differ in their last bits, and given
// the constants the bytes are the composed route's.  Black level and Bayer phase as in risp_serve_u8_cfa: the phase is a mirror
// of addresses; coordinates, reflection, parity and the tile grid live in the mirrored (RGGB) image.
#include "risp_serve_dentile.h"

namespace {

using namespace risp_patch;

// the rules both launches share; fills a (but for out / partials / stat / reverse)
int denoise_scene_args(const char *name, const uint16_t *raw, float divisor, int demosaic, int n_pre, const int *pre_ops,
                       const float *const *pre_params, int denoise, int window, int search, const float *den_a, const float *den_b,
                       int n_post, const int *post_ops, const float *const *post_params, int N, int H, int W, int black_level, int cfa,
                       DenoiseTileArgs &a, bool &wbq) {
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
    DenoiseTileArgs a;
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
    launch_denoise<true, true>(demosaic, denoise, wbq, (hipStream_t)stream, a);
    RISP_LAUNCH_CHECK("risp_serve_denoise_stats");
    return 0;
}

extern "C" int risp_serve_denoise_scene_u8(const uint16_t *raw, float divisor, int demosaic, int n_pre, const int *pre_ops,
                                           const float *const *pre_params, int denoise, int window, int search, const float *den_a,
                                           const float *den_b, int n_post, const int *post_ops, const float *const *post_params,
                                           uint8_t *out, int reverse_channels, int N, int H, int W, int black_level, int cfa,
                                           void *stream) {
    const char *name = "risp_serve_denoise_scene_u8";
    DenoiseTileArgs a;
    bool wbq;
    if (int e = denoise_scene_args(name, raw, divisor, demosaic, n_pre, pre_ops, pre_params, denoise, window, search, den_a, den_b, n_post,
                                   post_ops, post_params, N, H, W, black_level, cfa, a, wbq))
        return e;
    RISP_CHECK_ARG(out, "%s: null argument (out)", name);
    RISP_CHECK_ARG(reinterpret_cast<uintptr_t>(out) % 4 == 0, "%s: out must be 4-byte aligned", name);
    a.out = out;
    a.reverse = reverse_channels ? 1 : 0;
    launch_denoise<true, false>(demosaic, denoise, wbq, (hipStream_t)stream, a);
    RISP_LAUNCH_CHECK("risp_serve_denoise_scene_u8");
    return 0;
}
