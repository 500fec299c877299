// Serving path for the classical pipelines that hold ONE classical denoiser: a 16-bit Bayer frame in, a packed 8-bit image
// out, ONE launch.
//
//     max(sample - black, 0) / divisor -> nearest | bilinear | Malvar-He-Cutler demosaic -> P stages
//         -> bilateral (window 3) | median (3 x 3) | non-local means (block 3, search 3) -> Q stages -> clip(v * 255) truncated
//
// risp_serve_classical_u8 stops at a denoiser: a 3 x 3 (bilateral, median) or 5 x 5 (non-local means) stencil needs finished
// pixels on a ring around its own.  Here a workgroup owns a 64 x 32 pixel tile and works in two phases around one LDS image of
// 36 x 72 pixels: serve_denoise_kernel<.., GAIN = false, STATS = false> of risp_serve_dentile.h, which has the phases, the
// denoisers and the launch.  This file is the entry point and its rules.
//
// With -ffp-contract=off the bytes are the composed route's (tests/test_gpu_serve_denoise.py, torch.equal).  Black level and
// Bayer phase as in risp_serve_u8_cfa: the phase is a mirror of addresses; coordinates, reflection, parity and the tile grid
// live in the mirrored (RGGB) image.
#include "risp_serve_dentile.h"

using namespace risp_patch;

extern "C" int risp_serve_denoise_u8(const uint16_t *raw, float divisor, int demosaic, int n_pre, const int *pre_ops,
                                     const float *const *pre_params, int denoise, int window, int search, const float *den_a,
                                     const float *den_b, int n_post, const int *post_ops, const float *const *post_params,
                                     uint8_t *out, int reverse_channels, int N, int H, int W, int black_level, int cfa,
                                     void *stream) {
    const char *name = "risp_serve_denoise_u8";
    if (int e = denoiser_args(name, denoise, window, search, den_a, den_b)) return e;
    ArgRules r;
    r.split = true;
    DenoiseTileArgs a;
    bool wbq;
    if (int e = serve_args(name, r, a, wbq, raw, out, divisor, demosaic, n_pre, pre_ops, pre_params, n_post, post_ops, post_params, N, H, W,
                           black_level, cfa))
        return e;
    a.out = out;
    a.partials = nullptr;
    a.reverse = reverse_channels ? 1 : 0;
    a.stat = 0;
    a.da = den_a;
    a.db = den_b;
    launch_denoise<false, false>(demosaic, denoise, wbq, (hipStream_t)stream, a);
    RISP_LAUNCH_CHECK("risp_serve_denoise_u8");
    return 0;
}
