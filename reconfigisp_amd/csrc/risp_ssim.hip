// SSIM (gfx950): the structural-similarity index the reference's get_ssim selects in scikit-image
// (utils/util_path_restore.py:27-44) - uniform 7 x 7 window, K1 = 0.01, K2 = 0.03, sample covariance, mean over the
// windows that lie wholly inside the image and over the channels - and its gradient with respect to the first image.
//
// Forward: a workgroup owns 64 window columns x 4 R window rows of one plane.  Both planes' pixels (a 6-pixel halo to the
// right and below) go to LDS once, MINUS a per-workgroup pivot (the tile's first pixel): variances and the covariance are
// shift-invariant, and sums of (x - pivot) do not carry the image's brightness into the cancellation of E[xx] - E[x]^2
// (a flat bright image, 0.9 +- 1e-3: the plain fp32 restatement is 3.6e-6 off, these sums 2e-8).  A thread then walks one window column downwards: per pixel row the five
// 7-tap horizontal sums (x, y, xx, yy, xy; neighbouring lanes read neighbouring words: no bank conflicts at any pitch),
// the last seven rows of them in registers, one window per step.  Per-workgroup partial sums go to caller scratch; a
// finishing launch adds them in index order in fp64.  No atomics: the same bits on every run.
//
// Backward: dS/dx(p) of a window containing p is (1/49) [a + b y(p) - c x(p)] with three per-window values, so the
// gradient is a transposed 7 x 7 box over three window maps that are zero outside the valid range.  One launch recomputes
// the maps on a tile with a 12-pixel halo (LDS), then the same column walk sums them: 12 bytes per pixel and channel
// (read x, y, write gx) against 24 + 12 in the forward had the maps been stored.
#include "risp_common.h"

namespace {

constexpr int kWin = 7;
constexpr int kFwdCols = 64;                 // window columns per forward workgroup: one per lane
constexpr int kFwdPitch = kFwdCols + 8;      // 70 pixel columns used
constexpr int kBwdCols = 56;                 // output pixel columns per backward workgroup (a multiple of 4: vector stores)
constexpr int kBwdWinCols = kBwdCols + 6;    // 62 window columns ...
constexpr int kBwdPixCols = kBwdCols + 12;   // ... over 68 pixel columns
constexpr int kBwdPixPitch = kBwdPixCols;
constexpr int kBwdWinPitch = 64;
constexpr int kBwdR = 8;                     // window rows per wave in the backward launch: 26 output rows per workgroup

// tensor2bgr's arithmetic (utils/util.py:130-131): clip(v * 255, 0, 255), truncated - the code as a float
__device__ __forceinline__ float ssim_code(float v) {
    float t = v * 255.f;
    t = t < 0.f ? 0.f : (t > 255.f ? 255.f : t);
    return floorf(t);
}

struct Moments {
    float x, y, xx, yy, xy;
};

// the five 7-tap sums of one pixel row at window column j (px / py: the row's first word in LDS)
__device__ __forceinline__ Moments row_moments(const float *px, const float *py, int j) {
    float a[kWin], b[kWin];
#pragma unroll
    for (int t = 0; t < kWin; ++t) { a[t] = px[j + t]; b[t] = py[j + t]; }
    Moments m = {a[0], b[0], a[0] * a[0], b[0] * b[0], a[0] * b[0]};
#pragma unroll
    for (int t = 1; t < kWin; ++t) {
        m.x += a[t];
        m.y += b[t];
        m.xx = __builtin_fmaf(a[t], a[t], m.xx);
        m.yy = __builtin_fmaf(b[t], b[t], m.yy);
        m.xy = __builtin_fmaf(a[t], b[t], m.xy);
    }
    return m;
}

// the seven rows of a window, oldest first (ring[(k + 1) % 7] .. ring[k % 7]; k is a compile-time constant at every use)
template <int K>
__device__ __forceinline__ Moments window_moments(const Moments (&ring)[kWin]) {
    Moments s = ring[(K + 1) % kWin];
#pragma unroll
    for (int t = 2; t <= kWin; ++t) {
        const Moments &r = ring[(K + t) % kWin];
        s.x += r.x; s.y += r.y; s.xx += r.xx; s.yy += r.yy; s.xy += r.xy;
    }
    return s;
}

struct WindowTerms {
    float ux, uy, mx, my, A1, A2, B1, B2, S;
};

// sums about the pivots (px, py) -> the window's SSIM.  Identical planes give A1 == B1 and A2 == B2 bit for bit: S == 1.
// (That rests on -ffp-contract=off in the Makefile: contracted, ux * ux + uy * uy would round differently from 2 ux uy.)
__device__ __forceinline__ WindowTerms window_ssim(const Moments &s, float px, float py, float c1, float c2) {
    WindowTerms w;
    w.mx = s.x * (1.f / 49.f);
    w.my = s.y * (1.f / 49.f);
    const float vx = (s.xx - s.x * w.mx) * (1.f / 48.f);
    const float vy = (s.yy - s.y * w.my) * (1.f / 48.f);
    const float vxy = (s.xy - s.x * w.my) * (1.f / 48.f);
    w.ux = px + w.mx;
    w.uy = py + w.my;
    w.A1 = 2.f * w.ux * w.uy + c1;
    w.A2 = 2.f * vxy + c2;
    w.B1 = (w.ux * w.ux + w.uy * w.uy) + c1;
    w.B2 = (vx + vy) + c2;
    w.S = (w.A1 * w.A2) / (w.B1 * w.B2);
    return w;
}

template <bool Q>
__device__ __forceinline__ float ssim_value(float v) { return Q ? ssim_code(v) : v; }

// rows x cols pixels from (r0, c0) of a plane into LDS minus the pivot; 0 outside the plane (only windows that are not
// counted reach those)
template <bool Q>
__device__ __forceinline__ void load_tile(const float *__restrict__ plane, float *lds, int rows, int cols, int pitch, int r0,
                                          int c0, int H, int W, float pivot) {
    for (int i = threadIdx.x; i < rows * cols; i += 256) {
        const int r = i / cols, c = i - r * cols, gr = r0 + r, gc = c0 + c;
        float v = 0.f;
        if (gr >= 0 && gr < H && gc >= 0 && gc < W) v = ssim_value<Q>(plane[(size_t)gr * W + gc]) - pivot;
        lds[r * pitch + c] = v;
    }
}

// one window column downwards: R + 6 pixel rows of LDS (row pitch PITCH) from row0, a window per step after the first six
template <int R, int PITCH, int K = 0>
struct ColumnWalk {
    template <class F>
    static __device__ __forceinline__ void run(Moments (&ring)[kWin], const float *xs, const float *ys, int row0, int j, F &&emit) {
        if constexpr (K < R + 6) {
            ring[K % kWin] = row_moments(xs + (row0 + K) * PITCH, ys + (row0 + K) * PITCH, j);
            if constexpr (K >= 6) emit(window_moments<K>(ring), row0 + K - 6);
            ColumnWalk<R, PITCH, K + 1>::run(ring, xs, ys, row0, j, emit);
        }
    }
};

template <int R, bool Q>
__global__ __launch_bounds__(256) void ssim_fwd_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                       const float *__restrict__ dr, float dr_scalar,
                                                       float *__restrict__ part, int H, int W, int C, int tiles_x) {
    constexpr int TH = 4 * R, PH = TH + 6, PW = kFwdCols + 6;
    __shared__ float xs[PH * kFwdPitch], ys[PH * kFwdPitch];
    __shared__ float red[4];
    const int plane = blockIdx.y, ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int r0 = ty * TH, c0 = tx * kFwdCols;                  // first window = first pixel of the tile: inside the plane
    const float *xp = x + (size_t)plane * H * W, *yp = y + (size_t)plane * H * W;
    const float px = ssim_value<Q>(xp[(size_t)r0 * W + c0]), py = ssim_value<Q>(yp[(size_t)r0 * W + c0]);
    load_tile<Q>(xp, xs, PH, PW, kFwdPitch, r0, c0, H, W, px);
    load_tile<Q>(yp, ys, PH, PW, kFwdPitch, r0, c0, H, W, py);
    const float L = dr ? dr[plane / C] : dr_scalar;
    const float c1 = (0.01f * L) * (0.01f * L), c2 = (0.03f * L) * (0.03f * L);
    __syncthreads();
    const int j = threadIdx.x & 63, strip = threadIdx.x >> 6;
    const bool col_ok = c0 + j < W - 6;
    float acc[1] = {0.f};
    Moments ring[kWin];
    ColumnWalk<R, kFwdPitch>::run(ring, xs, ys, strip * R, j, [&](const Moments &s, int wi) {
        const WindowTerms w = window_ssim(s, px, py, c1, c2);
        if (col_ok && r0 + wi < H - 6) acc[0] += w.S;
    });
    block_sum<1>(acc, red);
    if (threadIdx.x == 0) part[(size_t)plane * gridDim.x + blockIdx.x] = acc[0];
}

// ssim[n] = the partial sums of image n in index order (lane l: l, l + 64, ...; a fixed tree over the lanes), in fp64, over the
// number of windows and channels
__global__ __launch_bounds__(64) void ssim_finish_kernel(const float *__restrict__ part, float *__restrict__ ssim, int per_image,
                                                         double inv_count) {
    const float *p = part + (size_t)blockIdx.x * per_image;
    double acc = 0.0;
    for (int i = threadIdx.x; i < per_image; i += 64) acc += (double)p[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if (threadIdx.x == 0) ssim[blockIdx.x] = (float)(acc * inv_count);
}

// ---- backward
struct Abc {
    float a, b, c;
};

template <int K>
__device__ __forceinline__ Abc window_abc(const Abc (&ring)[kWin]) {
    Abc s = ring[(K + 1) % kWin];
#pragma unroll
    for (int t = 2; t <= kWin; ++t) {
        const Abc &r = ring[(K + t) % kWin];
        s.a += r.a; s.b += r.b; s.c += r.c;
    }
    return s;
}

template <int RS, int K>
struct BwdSumWalk {
    template <class F>
    static __device__ __forceinline__ void run(Abc (&ring)[kWin], const float *as, const float *bs, const float *cs, int row0,
                                               int rows, int j, F &&emit) {
        if constexpr (K < RS + 6) {
            Abc h = {0.f, 0.f, 0.f};
            if (row0 + K < rows) {
                const int at = (row0 + K) * kBwdWinPitch + j;
#pragma unroll
                for (int t = 0; t < kWin; ++t) { h.a += as[at + t]; h.b += bs[at + t]; h.c += cs[at + t]; }
            }
            ring[K % kWin] = h;
            if constexpr (K >= 6) emit(window_abc<K>(ring), row0 + K - 6);
            BwdSumWalk<RS, K + 1>::run(ring, as, bs, cs, row0, rows, j, emit);
        }
    }
};

// gx = scale[n] * sum over the windows that contain the pixel of [a + b (y - py) - c (x - px)], the maps formed about the
// same pivots as the pixels
template <int R>
__global__ __launch_bounds__(256) void ssim_bwd_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                       const float *__restrict__ dr, float dr_scalar,
                                                       const float *__restrict__ gs, float *__restrict__ gx, int H, int W, int C,
                                                       int tiles_x, float inv, int vec) {
    constexpr int WR = 4 * R, TPH = WR - 6, PR = WR + 6, RS = (TPH + 3) / 4;
    __shared__ float xs[PR * kBwdPixPitch], ys[PR * kBwdPixPitch];
    __shared__ float as[WR * kBwdWinPitch], bs[WR * kBwdWinPitch], cs[WR * kBwdWinPitch];
    const int plane = blockIdx.y, ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int r0 = ty * TPH, c0 = tx * kBwdCols;                 // first output pixel; windows and pixels start 6 up and left
    const float *xp = x + (size_t)plane * H * W, *yp = y + (size_t)plane * H * W;
    const float px = xp[(size_t)r0 * W + c0], py = yp[(size_t)r0 * W + c0];
    load_tile<false>(xp, xs, PR, kBwdPixCols, kBwdPixPitch, r0 - 6, c0 - 6, H, W, px);
    load_tile<false>(yp, ys, PR, kBwdPixCols, kBwdPixPitch, r0 - 6, c0 - 6, H, W, py);
    const float L = dr ? dr[plane / C] : dr_scalar;
    const float c1 = (0.01f * L) * (0.01f * L), c2 = (0.03f * L) * (0.03f * L);
    const float scale = gs[plane / C] * inv;
    __syncthreads();
    const int j = threadIdx.x & 63, strip = threadIdx.x >> 6;
    if (j < kBwdWinCols) {
        const int gj = c0 - 6 + j;
        const bool col_ok = gj >= 0 && gj < W - 6;
        Moments ring[kWin];
        ColumnWalk<R, kBwdPixPitch>::run(ring, xs, ys, strip * R, j, [&](const Moments &s, int wi) {
            const int gi = r0 - 6 + wi;
            Abc m = {0.f, 0.f, 0.f};
            if (col_ok && gi >= 0 && gi < H - 6) {
                const WindowTerms w = window_ssim(s, px, py, c1, c2);
                const float cn2 = 2.f * (49.f / 48.f);
                m.b = cn2 * w.S / w.A2;
                m.c = cn2 * w.S / w.B2;
                // a + b y - c x with x, y about the pivots: the means inside a's covariance terms are the pivoted ones
                m.a = w.S * (2.f * w.uy / w.A1 - 2.f * w.ux / w.B1) - m.b * w.my + m.c * w.mx;
            }
            as[wi * kBwdWinPitch + j] = m.a;
            bs[wi * kBwdWinPitch + j] = m.b;
            cs[wi * kBwdWinPitch + j] = m.c;
        });
    }
    __syncthreads();
    float *gp = gx + (size_t)plane * H * W;
    if (j < kBwdCols) {
        Abc ring[kWin];
        BwdSumWalk<RS, 0>::run(ring, as, bs, cs, strip * RS, WR, j, [&](const Abc &s, int pr) {
            const int gr = r0 + pr, gc = c0 + j;
            if (pr < TPH && gr < H && gc < W) {
                const int at = (pr + 6) * kBwdPixPitch + j + 6;
                const float g = scale * ((s.a + s.b * ys[at]) - s.c * xs[at]);
                if (vec) xs[at] = g;                             // this thread alone reads the word: staged for the vector stores
                else gp[(size_t)gr * W + gc] = g;
            }
        });
    }
    if (vec) {                                                   // W % 4 == 0, 16-byte aligned gx
        __syncthreads();
        for (int i = threadIdx.x; i < TPH * (kBwdCols / 4); i += 256) {
            const int pr = i / (kBwdCols / 4), q = i - pr * (kBwdCols / 4), gr = r0 + pr, gc = c0 + 4 * q;
            if (gr < H && gc < W) {
                const float *s = xs + (pr + 6) * kBwdPixPitch + 6 + 4 * q;
                *reinterpret_cast<float4 *>(gp + (size_t)gr * W + gc) = make_float4(s[0], s[1], s[2], s[3]);
            }
        }
    }
}

struct SsimGrid {
    int rows, tiles_x, tiles;       // forward: window rows per workgroup
};

// 64 window rows per workgroup (6 halo rows on 64: 1.09 x the loads) unless that leaves most of the chip idle (patches)
SsimGrid ssim_fwd_grid(int NC, int H, int W) {
    SsimGrid g;
    g.tiles_x = (W - 6 + kFwdCols - 1) / kFwdCols;
    const long long big = (long long)((H - 6 + 63) / 64) * g.tiles_x * NC;
    g.rows = big >= 512 ? 64 : 16;
    g.tiles = ((H - 6 + g.rows - 1) / g.rows) * g.tiles_x;
    return g;
}

int ssim_check(const char *name, const void *x, const void *y, int N, int C, int H, int W) {
    RISP_CHECK_ARG(x && y, "%s: null image", name);
    RISP_CHECK_ARG(N > 0 && C > 0 && H >= kWin && W >= kWin, "%s: needs N, C > 0 and H, W >= 7 (N=%d C=%d H=%d W=%d)", name, N, C,
                   H, W);
    RISP_CHECK_ARG((long long)N * C * H * W < (1ll << 31), "%s: N C H W must be below 2^31 (N=%d C=%d H=%d W=%d)", name, N, C, H, W);
    RISP_CHECK_ARG((long long)N * C <= 65535, "%s: at most 65535 planes (N=%d C=%d H=%d W=%d)", name, N, C, H, W);
    return 0;
}

}  // namespace

extern "C" {

size_t risp_ssim_scratch_floats(int N, int C, int H, int W) {
    if (N <= 0 || C <= 0 || H < kWin || W < kWin || (long long)N * C > 65535) return 0;
    return (size_t)N * C * ssim_fwd_grid(N * C, H, W).tiles;
}

int risp_ssim_fwd(const float *x, const float *y, const float *data_range, float data_range_scalar, int quantise, float *ssim,
                  float *scratch, size_t scratch_floats, int N, int C, int H, int W, void *stream) {
    if (int e = ssim_check("risp_ssim_fwd", x, y, N, C, H, W)) return e;
    RISP_CHECK_ARG(ssim && scratch, "risp_ssim_fwd: null output or scratch");
    RISP_CHECK_ARG(scratch_floats >= risp_ssim_scratch_floats(N, C, H, W),
                   "risp_ssim_fwd: scratch holds %zu floats, needs risp_ssim_scratch_floats() = %zu", scratch_floats,
                   risp_ssim_scratch_floats(N, C, H, W));
    const SsimGrid g = ssim_fwd_grid(N * C, H, W);
    const dim3 grid(g.tiles, N * C);
#define RISP_SSIM_FWD(R, Q)                                                                                              \
    hipLaunchKernelGGL((ssim_fwd_kernel<R, Q>), grid, dim3(256), 0, (hipStream_t)stream, x, y, data_range, data_range_scalar, \
                       scratch, H, W, C, g.tiles_x)
    if (g.rows == 64) {
        if (quantise) RISP_SSIM_FWD(16, true);
        else RISP_SSIM_FWD(16, false);
    } else {
        if (quantise) RISP_SSIM_FWD(4, true);
        else RISP_SSIM_FWD(4, false);
    }
#undef RISP_SSIM_FWD
    hipLaunchKernelGGL(ssim_finish_kernel, dim3(N), dim3(64), 0, (hipStream_t)stream, scratch, ssim, C * g.tiles,
                       1.0 / ((double)C * (H - 6) * (W - 6)));
    RISP_LAUNCH_CHECK("risp_ssim_fwd");
    return 0;
}

int risp_ssim_bwd(const float *x, const float *y, const float *data_range, float data_range_scalar, const float *gs, float *gx,
                  int N, int C, int H, int W, void *stream) {
    if (int e = ssim_check("risp_ssim_bwd", x, y, N, C, H, W)) return e;
    RISP_CHECK_ARG(gs && gx, "risp_ssim_bwd: null gradient");
    constexpr int TPH = 4 * kBwdR - 6;
    const int tiles_x = (W + kBwdCols - 1) / kBwdCols, tiles = ((H + TPH - 1) / TPH) * tiles_x;
    const int vec = (W % 4 == 0 && (reinterpret_cast<uintptr_t>(gx) & 15) == 0) ? 1 : 0;
    const float inv = (float)(1.0 / (49.0 * (double)C * (H - 6) * (W - 6)));
    hipLaunchKernelGGL((ssim_bwd_kernel<kBwdR>), dim3(tiles, N * C), dim3(256), 0, (hipStream_t)stream, x, y, data_range,
                       data_range_scalar, gs, gx, H, W, C, tiles_x, inv, vec);
    RISP_LAUNCH_CHECK("risp_ssim_bwd");
    return 0;
}

}  // extern "C"
