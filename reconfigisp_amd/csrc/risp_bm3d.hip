// Classical BM3D of the Origin set (sRGB index 15; the reference only has a proxy net for it, origin_universal.py:12).
// Build-defined OPSPEC: DESIGN.md section 2, include/risp.h "'bm3d'", restated in float64 in tests/bm3d_reference.py.
//
// Six launches per chunk of images, all of them deterministic (no atomics; every sum runs in a fixed order):
//   prep       codes q, the integer matching plane S = B+G+R and the colour-space planes Z of the noisy image
//   match      one wave per reference block: the S window with its +-R halo in LDS, lanes own candidates, int32 squared
//              distances, the group (ordered by (D, y, x), reference first) chosen by repeated wave minima of 64-bit keys
//   filter<1>  one wave per group (n1 = 8) or per four groups (n1 = 4, 16 lanes each): lane = pixel position of a block,
//              the N2 blocks of one channel in registers; 2D transform through LDS, 1D Haar along the group in registers,
//              hard threshold, inverse; K (x) block per member and the group weight into scratch slots
//   aggregate<1> a 16 x 16 output tile walks, in reference index order, the references whose members can reach it and
//              adds the members that cover each pixel: the basic estimate (colour space)
//   filter<2>, aggregate<2>  the Wiener pass on the same groups, then the inverse colour transform and the 8-bit codes
#include "risp_common.h"

namespace {

constexpr int MAXG = 16, TCOLS = 1 + MAXG, GSTEP = 3, RMAX = 9, MAXN1 = 8;
constexpr int WIN = 2 * RMAX + MAXN1;            // staged S window side (candidate corners +-R, plus a block)
constexpr float HARD = 2.7f;
constexpr float RSQRT2 = 7.071067812e-01f;

// 2D block transforms, row k = basis function k (orthonormal DCT-II; orthonormal Haar, full decomposition
// H_2m = [H_m (x) (1,1); I_m (x) (1,-1)] / sqrt(2))
__constant__ float c_dct4[16] = {5.000000000e-01f, 5.000000000e-01f, 5.000000000e-01f, 5.000000000e-01f, 6.532814824e-01f,
                                 2.705980501e-01f, -2.705980501e-01f, -6.532814824e-01f, 5.000000000e-01f, -5.000000000e-01f,
                                 -5.000000000e-01f, 5.000000000e-01f, 2.705980501e-01f, -6.532814824e-01f, 6.532814824e-01f,
                                 -2.705980501e-01f};
__constant__ float c_haar4[16] = {5.000000000e-01f, 5.000000000e-01f, 5.000000000e-01f, 5.000000000e-01f, 5.000000000e-01f,
                                  5.000000000e-01f, -5.000000000e-01f, -5.000000000e-01f, 7.071067812e-01f, -7.071067812e-01f,
                                  0.f, 0.f, 0.f, 0.f, 7.071067812e-01f, -7.071067812e-01f};
__constant__ float c_dct8[64] = {
    3.535533906e-01f, 3.535533906e-01f, 3.535533906e-01f, 3.535533906e-01f, 3.535533906e-01f, 3.535533906e-01f, 3.535533906e-01f, 3.535533906e-01f,
    4.903926402e-01f, 4.157348062e-01f, 2.777851165e-01f, 9.754516101e-02f, -9.754516101e-02f, -2.777851165e-01f, -4.157348062e-01f, -4.903926402e-01f,
    4.619397663e-01f, 1.913417162e-01f, -1.913417162e-01f, -4.619397663e-01f, -4.619397663e-01f, -1.913417162e-01f, 1.913417162e-01f, 4.619397663e-01f,
    4.157348062e-01f, -9.754516101e-02f, -4.903926402e-01f, -2.777851165e-01f, 2.777851165e-01f, 4.903926402e-01f, 9.754516101e-02f, -4.157348062e-01f,
    3.535533906e-01f, -3.535533906e-01f, -3.535533906e-01f, 3.535533906e-01f, 3.535533906e-01f, -3.535533906e-01f, -3.535533906e-01f, 3.535533906e-01f,
    2.777851165e-01f, -4.903926402e-01f, 9.754516101e-02f, 4.157348062e-01f, -4.157348062e-01f, -9.754516101e-02f, 4.903926402e-01f, -2.777851165e-01f,
    1.913417162e-01f, -4.619397663e-01f, 4.619397663e-01f, -1.913417162e-01f, -1.913417162e-01f, 4.619397663e-01f, -4.619397663e-01f, 1.913417162e-01f,
    9.754516101e-02f, -2.777851165e-01f, 4.157348062e-01f, -4.903926402e-01f, 4.903926402e-01f, -4.157348062e-01f, 2.777851165e-01f, -9.754516101e-02f};
__constant__ float c_haar8[64] = {
    3.535533906e-01f, 3.535533906e-01f, 3.535533906e-01f, 3.535533906e-01f, 3.535533906e-01f, 3.535533906e-01f, 3.535533906e-01f, 3.535533906e-01f,
    3.535533906e-01f, 3.535533906e-01f, 3.535533906e-01f, 3.535533906e-01f, -3.535533906e-01f, -3.535533906e-01f, -3.535533906e-01f, -3.535533906e-01f,
    5.000000000e-01f, 5.000000000e-01f, -5.000000000e-01f, -5.000000000e-01f, 0.f, 0.f, 0.f, 0.f,
    0.f, 0.f, 0.f, 0.f, 5.000000000e-01f, 5.000000000e-01f, -5.000000000e-01f, -5.000000000e-01f,
    7.071067812e-01f, -7.071067812e-01f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f,
    0.f, 0.f, 7.071067812e-01f, -7.071067812e-01f, 0.f, 0.f, 0.f, 0.f,
    0.f, 0.f, 0.f, 0.f, 7.071067812e-01f, -7.071067812e-01f, 0.f, 0.f,
    0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 7.071067812e-01f, -7.071067812e-01f};
// Kaiser windows, beta = 2
__constant__ float c_kaiser4[4] = {4.386762798e-01f, 9.243138756e-01f, 9.243138756e-01f, 4.386762798e-01f};
__constant__ float c_kaiser8[8] = {4.386762798e-01f, 6.813242630e-01f, 8.768399053e-01f, 9.858225062e-01f,
                                   9.858225062e-01f, 8.768399053e-01f, 6.813242630e-01f, 4.386762798e-01f};
// colour transforms, rows = channels, columns = (B, G, R); [0] orthonormal opponent, [1] BT.601 full-range YCbCr
// without offsets.  c_cinv = the float64 inverse rounded to fp32, c_cnorm = the row norms (sigma_c = sigma * norm).
__constant__ float c_cfwd[2][9] = {
    {5.773502692e-01f, 5.773502692e-01f, 5.773502692e-01f, -7.071067812e-01f, 0.f, 7.071067812e-01f, 4.082482905e-01f,
     -8.164965809e-01f, 4.082482905e-01f},
    {1.140000000e-01f, 5.870000000e-01f, 2.990000000e-01f, 5.000000000e-01f, -3.312640000e-01f, -1.687360000e-01f,
     -8.131200000e-02f, -4.186880000e-01f, 5.000000000e-01f}};
__constant__ float c_cinv[2][9] = {
    {5.773502692e-01f, -7.071067812e-01f, 4.082482905e-01f, 5.773502692e-01f, 0.f, -8.164965809e-01f, 5.773502692e-01f,
     7.071067812e-01f, 4.082482905e-01f},
    {1.000000000e+00f, 1.772000066e+00f, 4.062980629e-07f, 1.000000000e+00f, -3.441356782e-01f, -7.141361556e-01f,
     1.000000000e+00f, -1.218894189e-06f, 1.401999589e+00f}};
__constant__ float c_cnorm[2][3] = {{1.f, 1.f, 1.f}, {6.685551585e-01f, 6.230631392e-01f, 6.571995760e-01f}};

__device__ __forceinline__ float q8(float v) { return floorf(__builtin_amdgcn_fmed3f(v, 0.f, 255.f) + 0.5f); }
__device__ __forceinline__ float emit(float v, float so) { return so > 0.f ? q8(v) * (1.f / so) : v * (1.f / -so); }

// reference-block grid along one axis: min(3 i, n - n1), i < grid_n = ceil((n - n1) / 3) + 1
__host__ __device__ __forceinline__ int grid_n(int n, int n1) { return (n - n1 + GSTEP - 1) / GSTEP + 1; }
__host__ __device__ __forceinline__ int grid_at(int i, int n, int n1) { return GSTEP * i < n - n1 ? GSTEP * i : n - n1; }
__host__ __device__ __forceinline__ size_t align256(size_t b) { return (b + 255) & ~size_t(255); }
// member corners packed y << 16 | x (both < 65536): unpacked as unsigned - y >= 32768 sets the sign bit of the int
__device__ __forceinline__ int corner_y(int c) { return (int)((unsigned)c >> 16); }
__device__ __forceinline__ int corner_x(int c) { return (int)((unsigned)c & 0xffffu); }
// image sizes the kernels index with int arithmetic (3 planes of H x W) and the packed corners hold
__host__ __device__ __forceinline__ bool shape_ok(int H, int W) {
    return H >= 4 && W >= 4 && H <= 65535 && W <= 65535 && 3 * (size_t)H * W <= 0x7fffffff;
}

// per-image scratch: S (int32 HW), Z and the basic estimate (3 HW floats each), the group table (rows x 17 int32,
// corners packed y << 16 | x), the group weights (rows floats) and the member slots (16 x 3 x n1^2 floats per row)
struct Layout {
    size_t s, z, b, tab, wt, slot, total;
    int rows;
};
__host__ __device__ inline Layout layout(int H, int W) {
    Layout l;
    l.rows = grid_n(H, 4) * grid_n(W, 4);
    const size_t r8 = (H >= 8 && W >= 8) ? (size_t)grid_n(H, 8) * grid_n(W, 8) : 0;
    const size_t slot4 = (size_t)l.rows * MAXG * 3 * 16, slot8 = r8 * MAXG * 3 * 64;
    l.s = 0;
    l.z = l.s + align256(sizeof(int) * (size_t)H * W);
    l.b = l.z + align256(sizeof(float) * 3 * (size_t)H * W);
    l.tab = l.b + align256(sizeof(float) * 3 * (size_t)H * W);
    l.wt = l.tab + align256(sizeof(int) * (size_t)l.rows * TCOLS);
    l.slot = l.wt + align256(sizeof(float) * (size_t)l.rows);
    l.total = l.slot + align256(sizeof(float) * (slot4 > slot8 ? slot4 : slot8));
    return l;
}

struct Args {
    const float *x;                     // chunk's first image
    float *y;
    const float *sigma;
    const int *n1, *cspace, *wtransform, *radius;
    int *groups;                        // nullable, chunk's first image
    char *scratch;
    size_t per;                         // scratch bytes per image
    int H, W, rows;
    float si, so;
};

// per-image values as the kernels use them: out-of-contract values never reach memory outside the image or the
// scratch (the callers validate; see risp.h)
struct Img {
    int n1, R, cs, wt;
    float sigma;
};
__device__ __forceinline__ Img image(const Args &a, int n) {
    Img m;
    m.n1 = (a.n1[n] == 4 || a.H < 8 || a.W < 8) ? 4 : 8;
    const int r = a.radius[n];
    m.R = r < 0 ? 0 : (r > RMAX ? RMAX : r);
    m.cs = a.cspace[n] != 0;
    m.wt = a.wtransform[n] != 0;
    m.sigma = a.sigma[n];
    return m;
}

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---------------------------------------------------------------- prep
__global__ __launch_bounds__(256) void bm3d_prep_kernel(Args a) {
    const int n = blockIdx.y, hw = a.H * a.W;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= hw) return;
    const float *x = a.x + (size_t)n * 3 * hw;
    char *base = a.scratch + (size_t)n * a.per;
    const Layout l = layout(a.H, a.W);
    const float qb = q8(x[p] * a.si), qg = q8(x[hw + p] * a.si), qr = q8(x[2 * hw + p] * a.si);
    reinterpret_cast<int *>(base + l.s)[p] = (int)qb + (int)qg + (int)qr;
    const int cs = a.cspace[n] != 0;
    float *z = reinterpret_cast<float *>(base + l.z);
#pragma unroll
    for (int c = 0; c < 3; ++c)
        z[c * hw + p] = c_cfwd[cs][3 * c] * qb + c_cfwd[cs][3 * c + 1] * qg + c_cfwd[cs][3 * c + 2] * qr;
}

// ---------------------------------------------------------------- match
template <int N1>
__device__ __forceinline__ int block_distance(const int *win, int cy, int cx, int ry, int rx) {
    int d = 0;
#pragma unroll
    for (int u = 0; u < N1; ++u)
#pragma unroll
        for (int v = 0; v < N1; ++v) {
            const int e = win[(cy + u) * WIN + cx + v] - win[(ry + u) * WIN + rx + v];
            d += e * e;
        }
    return d;
}

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long k) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)k, off), hi = __shfl_xor((unsigned)(k >> 32), off);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        k = o < k ? o : k;
    }
    return k;
}

constexpr int MATCH_PER_LANE = ((2 * RMAX + 1) * (2 * RMAX + 1) + 63) / 64;   // 361 candidates: 6 per lane

__global__ __launch_bounds__(256) void bm3d_match_kernel(Args a) {
    __shared__ int lds[4][WIN * WIN];
    const int n = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + wave;
    if (row >= a.rows) return;
    const Img m = image(a, n);
    const int H = a.H, W = a.W, nx = grid_n(W, m.n1), nref = grid_n(H, m.n1) * nx;
    int *ug = a.groups ? a.groups + ((size_t)n * a.rows + row) * TCOLS : nullptr;
    if (row >= nref) {                                    // beyond this image's grid: an empty row of the caller's table
        if (ug && lane < TCOLS) ug[lane] = lane == 0 ? 0 : -1;
        return;
    }
    const Layout l = layout(H, W);
    char *base = a.scratch + (size_t)n * a.per;
    const int *S = reinterpret_cast<const int *>(base + l.s);
    const int ry = grid_at(row / nx, H, m.n1), rx = grid_at(row % nx, W, m.n1);
    const int y0 = max(0, ry - m.R), y1 = min(H - m.n1, ry + m.R), x0 = max(0, rx - m.R), x1 = min(W - m.n1, rx + m.R);
    const int th = y1 - y0 + m.n1, tw = x1 - x0 + m.n1;   // <= WIN each
    int *win = lds[wave];
    for (int idx = lane; idx < th * tw; idx += 64) {
        const int r = idx / tw, c = idx - r * tw;
        win[r * WIN + c] = S[(y0 + r) * W + x0 + c];
    }
    wave_sync();
    const int ncx = x1 - x0 + 1, nc = (y1 - y0 + 1) * ncx;
    const int thr = 22500 * m.n1 * m.n1;
    unsigned long long key[MATCH_PER_LANE];
    int kept = 0;
#pragma unroll
    for (int j = 0; j < MATCH_PER_LANE; ++j) {
        const int t = lane + 64 * j;
        key[j] = ~0ull;
        if (t < nc) {
            const int cy = t / ncx, cx = t - cy * ncx;
            const int d = m.n1 == 4 ? block_distance<4>(win, cy, cx, ry - y0, rx - x0)
                                    : block_distance<8>(win, cy, cx, ry - y0, rx - x0);
            const int gy = y0 + cy, gx = x0 + cx;
            if (d <= thr && !(gy == ry && gx == rx)) {
                key[j] = ((unsigned long long)d << 32) | ((unsigned)gy << 16) | (unsigned)gx;
                ++kept;
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) kept += __shfl_xor(kept, o);
    ++kept;                            // + the reference block itself
    const int g = kept < MAXG ? kept : MAXG;
    const int n2 = 1 << (31 - __builtin_clz(g));          // largest power of two <= min(kept, 16)
    unsigned mine = ((unsigned)ry << 16) | (unsigned)rx;  // lane r + 1 keeps the member of rank r (lane 1: rank 0)
    unsigned long long lo = 0;
    for (int r = 1; r < n2; ++r) {                        // the next smallest key, ties impossible (keys hold y, x)
        unsigned long long best = ~0ull;
#pragma unroll
        for (int j = 0; j < MATCH_PER_LANE; ++j) best = (key[j] >= lo && key[j] < best) ? key[j] : best;
        best = wave_min_u64(best);
        if (lane == r + 1) mine = (unsigned)best;
        lo = best + 1;
    }
    int *tab = reinterpret_cast<int *>(base + l.tab) + (size_t)row * TCOLS;
    if (lane < TCOLS) {
        const bool member = lane >= 1 && lane <= n2;
        tab[lane] = lane == 0 ? n2 : (member ? (int)mine : -1);
        if (ug) ug[lane] = lane == 0 ? n2 : (member ? (int)(mine >> 16) * W + (int)(mine & 0xffffu) : -1);
    }
}

// ---------------------------------------------------------------- filter
template <int L>
__device__ __forceinline__ void haar_fwd(float (&v)[MAXG]) {
#pragma unroll
    for (int len = L; len > 1; len >>= 1) {
        float t[MAXG];
#pragma unroll
        for (int i = 0; i < len / 2; ++i) {
            t[i] = (v[2 * i] + v[2 * i + 1]) * RSQRT2;
            t[len / 2 + i] = (v[2 * i] - v[2 * i + 1]) * RSQRT2;
        }
#pragma unroll
        for (int i = 0; i < len; ++i) v[i] = t[i];
    }
}
template <int L>
__device__ __forceinline__ void haar_inv(float (&v)[MAXG]) {
#pragma unroll
    for (int len = 2; len <= L; len <<= 1) {
        float t[MAXG];
#pragma unroll
        for (int i = 0; i < len / 2; ++i) {
            t[2 * i] = (v[i] + v[len / 2 + i]) * RSQRT2;
            t[2 * i + 1] = (v[i] - v[len / 2 + i]) * RSQRT2;
        }
#pragma unroll
        for (int i = 0; i < len; ++i) v[i] = t[i];
    }
}
__device__ __forceinline__ void haar_group(float (&v)[MAXG], int n2, bool inverse) {
    switch (n2) {
    case 2: inverse ? haar_inv<2>(v) : haar_fwd<2>(v); break;
    case 4: inverse ? haar_inv<4>(v) : haar_fwd<4>(v); break;
    case 8: inverse ? haar_inv<8>(v) : haar_fwd<8>(v); break;
    case 16: inverse ? haar_inv<16>(v) : haar_fwd<16>(v); break;
    default: break;                                       // N2 = 1: identity
    }
}

// one separable pass over the wave's blocks through LDS (buf: [16][64], lane = block position):
// ROWS: v[i][j] <- sum_b v[i][b] t[b];  COLS: v[i][j] <- sum_a v[a][j] t[a]
template <int N1, bool ROWS>
__device__ __forceinline__ void pass(float (&v)[MAXG], float *buf, int lane, int i, int j, const float (&t)[N1], int kmax) {
    const int sub = lane & ~(N1 * N1 - 1);
#pragma unroll
    for (int k = 0; k < MAXG; ++k)
        if (k < kmax) buf[k * 64 + lane] = v[k];
    wave_sync();
#pragma unroll
    for (int k = 0; k < MAXG; ++k)
        if (k < kmax) {
            float acc = 0.f;
#pragma unroll
            for (int b = 0; b < N1; ++b) acc += buf[k * 64 + sub + (ROWS ? i * N1 + b : b * N1 + j)] * t[b];
            v[k] = acc;
        }
    wave_sync();
}

__device__ __forceinline__ float sub_sum(float v, int width) {
    for (int off = 1; off < width; off <<= 1) v += __shfl_xor(v, off);
    return v;
}

template <int N1, int WT, int STEP>
__device__ void filter_groups(const Args &a, const Img &m, int n, float *buf) {
    constexpr int NP = N1 * N1, G = 64 / NP, ITER = 4 / G;
    const int H = a.H, W = a.W, hw = H * W, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int pos = lane & (NP - 1), i = pos / N1, j = pos % N1;
    const int nref = grid_n(H, N1) * grid_n(W, N1);
    const Layout l = layout(H, W);
    char *base = a.scratch + (size_t)n * a.per;
    const int *tab = reinterpret_cast<const int *>(base + l.tab);
    const float *Z = reinterpret_cast<const float *>(base + l.z);
    float *B = reinterpret_cast<float *>(base + l.b);
    float *wt = reinterpret_cast<float *>(base + l.wt);
    float *slot = reinterpret_cast<float *>(base + l.slot);
    const float *T = N1 == 4 ? (WT ? c_haar4 : c_dct4) : (WT ? c_haar8 : c_dct8);
    const float *K = N1 == 4 ? c_kaiser4 : c_kaiser8;
    float trj[N1], tri[N1], tcj[N1], tci[N1];
#pragma unroll
    for (int b = 0; b < N1; ++b) {
        trj[b] = T[j * N1 + b]; tri[b] = T[i * N1 + b]; tcj[b] = T[b * N1 + j]; tci[b] = T[b * N1 + i];
    }
    const float kw = K[i] * K[j];
    for (int it = 0; it < ITER; ++it) {
        const int ref = blockIdx.x * 16 + wave * 4 + it * G + lane / NP;
        const bool active = ref < nref;
        const int n2 = active ? tab[(size_t)ref * TCOLS] : 0;
        int off[MAXG];                                    // pixel offset of this lane's position in member k
#pragma unroll
        for (int k = 0; k < MAXG; ++k) {
            const int c = k < n2 ? tab[(size_t)ref * TCOLS + 1 + k] : 0;
            off[k] = (corner_y(c) + i) * W + corner_x(c) + j;
        }
        int kmax = n2;
        for (int o = 32; o > 0; o >>= 1) kmax = max(kmax, __shfl_xor(kmax, o));
        float wsum = 0.f;
#pragma unroll 1
        for (int c = 0; c < 3; ++c) {
            const float sc = m.sigma * c_cnorm[m.cs][c];
            float z[MAXG], p[MAXG];
#pragma unroll
            for (int k = 0; k < MAXG; ++k) {
                z[k] = k < n2 ? Z[c * hw + off[k]] : 0.f;
                if (STEP == 2) p[k] = k < n2 ? B[c * hw + off[k]] : 0.f;
            }
            pass<N1, true>(z, buf, lane, i, j, trj, kmax);
            pass<N1, false>(z, buf, lane, i, j, tri, kmax);
            haar_group(z, n2, false);
            if (STEP == 1) {
                const float thr = HARD * sc;
                float cnt = 0.f;
#pragma unroll
                for (int k = 0; k < MAXG; ++k) {
                    if (fabsf(z[k]) > thr) cnt += 1.f;
                    else z[k] = 0.f;
                }
                cnt = sub_sum(cnt, NP);                   // exact: integer counts
                wsum += sc * sc * fmaxf(cnt, 1.f);
            } else {
                pass<N1, true>(p, buf, lane, i, j, trj, kmax);
                pass<N1, false>(p, buf, lane, i, j, tri, kmax);
                haar_group(p, n2, false);
                float w2 = 0.f;
#pragma unroll
                for (int k = 0; k < MAXG; ++k) {
                    const float pp = p[k] * p[k];
                    const float wien = pp / (pp + sc * sc);
                    z[k] *= wien;
                    w2 += wien * wien;
                }
                w2 = sub_sum(w2, NP);
                wsum += sc * sc * fmaxf(w2, 1.f);
            }
            haar_group(z, n2, true);
            pass<N1, true>(z, buf, lane, i, j, tcj, kmax);
            pass<N1, false>(z, buf, lane, i, j, tci, kmax);
            float *dst = slot + ((size_t)ref * MAXG * 3 + c) * NP + pos;
#pragma unroll
            for (int k = 0; k < MAXG; ++k)
                if (k < n2) dst[(size_t)k * 3 * NP] = kw * z[k];
        }
        if (active && pos == 0) wt[ref] = 1.f / wsum;
    }
}

template <int STEP>
__global__ __launch_bounds__(256) void bm3d_filter_kernel(Args a) {
    __shared__ float lds[4][MAXG * 64];
    const int n = blockIdx.y;
    const Img m = image(a, n);
    if (!(m.sigma >= 1e-3f)) return;                       // sigma < 1e-3: the codes are the result
    float *buf = lds[threadIdx.x >> 6];
    if (m.n1 == 4) {
        if (m.wt) filter_groups<4, 1, STEP>(a, m, n, buf);
        else filter_groups<4, 0, STEP>(a, m, n, buf);
    } else {
        if (m.wt) filter_groups<8, 1, STEP>(a, m, n, buf);
        else filter_groups<8, 0, STEP>(a, m, n, buf);
    }
}

// ---------------------------------------------------------------- aggregate
constexpr int AT = 16;                                    // output tile side
template <int STEP>
__global__ __launch_bounds__(256) void bm3d_aggregate_kernel(Args a) {
    __shared__ float kk[64];
    const int n = blockIdx.z, H = a.H, W = a.W, hw = H * W;
    const int tx0 = blockIdx.x * AT, ty0 = blockIdx.y * AT;
    const int px = tx0 + (threadIdx.x & (AT - 1)), py = ty0 + threadIdx.x / AT;
    const bool inside = px < W && py < H;
    const Img m = image(a, n);
    const size_t plane = (size_t)hw, o = (size_t)n * 3 * plane + (size_t)py * W + px;
    if (!(m.sigma >= 1e-3f)) {                             // the codes themselves, in both output forms
        if (STEP == 2 && inside)
            for (int c = 0; c < 3; ++c) a.y[o + c * plane] = q8(a.x[o + c * plane] * a.si) * (1.f / fabsf(a.so));
        return;
    }
    const int n1 = m.n1, np = n1 * n1;
    if (threadIdx.x < np) {
        const float *K = n1 == 4 ? c_kaiser4 : c_kaiser8;
        kk[threadIdx.x] = K[threadIdx.x / n1] * K[threadIdx.x % n1];
    }
    __syncthreads();
    const Layout l = layout(H, W);
    char *base = a.scratch + (size_t)n * a.per;
    const int *tab = reinterpret_cast<const int *>(base + l.tab);
    const float *wt = reinterpret_cast<const float *>(base + l.wt);
    const float *slot = reinterpret_cast<const float *>(base + l.slot);
    const int ny = grid_n(H, n1), nx = grid_n(W, n1);
    // references whose members (corners within +-R) can cover a pixel of the tile
    const int ylo = ty0 - m.R - n1 + 1, yhi = ty0 + AT - 1 + m.R, xlo = tx0 - m.R - n1 + 1, xhi = tx0 + AT - 1 + m.R;
    const int i0 = max(0, ylo / GSTEP), i1 = min(ny - 1, yhi / GSTEP + 1);
    const int j0 = max(0, xlo / GSTEP), j1 = min(nx - 1, xhi / GSTEP + 1);
    float num0 = 0.f, num1 = 0.f, num2 = 0.f, den = 0.f;
    for (int ii = i0; ii <= i1; ++ii)
        for (int jj = j0; jj <= j1; ++jj) {
            const int ref = ii * nx + jj;
            const int *row = tab + (size_t)ref * TCOLS;
            const int n2 = row[0];
            const float w = wt[ref];
            for (int k = 0; k < n2; ++k) {
                const int c = row[1 + k], my = corner_y(c), mx = corner_x(c);
                if (my > ty0 + AT - 1 || my + n1 <= ty0 || mx > tx0 + AT - 1 || mx + n1 <= tx0) continue;
                const int u = py - my, v = px - mx;
                if (!inside || u < 0 || u >= n1 || v < 0 || v >= n1) continue;
                const float *s = slot + ((size_t)ref * MAXG + k) * 3 * np + u * n1 + v;
                num0 = __builtin_fmaf(w, s[0], num0);
                num1 = __builtin_fmaf(w, s[np], num1);
                num2 = __builtin_fmaf(w, s[2 * np], num2);
                den = __builtin_fmaf(w, kk[u * n1 + v], den);
            }
        }
    if (!inside) return;
    const float e0 = num0 / den, e1 = num1 / den, e2 = num2 / den;
    if (STEP == 1) {
        float *B = reinterpret_cast<float *>(base + l.b);
        const int p = py * W + px;
        B[p] = e0; B[hw + p] = e1; B[2 * hw + p] = e2;
    } else {
        const float *mi = c_cinv[m.cs];
#pragma unroll
        for (int c = 0; c < 3; ++c) a.y[o + c * plane] = emit(mi[3 * c] * e0 + mi[3 * c + 1] * e1 + mi[3 * c + 2] * e2, a.so);
    }
}

}  // namespace

extern "C" {

size_t risp_origin_bm3d_scratch_bytes(int N, int H, int W) {
    if (N <= 0 || !shape_ok(H, W)) return 0;
    return (size_t)N * layout(H, W).total;
}

int risp_origin_bm3d(const float *x, float *y, const float *sigma, const int32_t *n1, const int32_t *cspace,
                     const int32_t *wtransform, const int32_t *radius, int N, int H, int W, float in_scale, float out_div,
                     void *scratch, size_t scratch_bytes, int32_t *groups, void *stream) {
    RISP_CHECK_ARG(x && y && sigma && n1 && cspace && wtransform && radius && scratch && N > 0 && N <= 65535 &&
                       shape_ok(H, W) && out_div != 0.f,
                   "risp_origin_bm3d: bad arguments (N=%d H=%d W=%d)", N, H, W);
    RISP_CHECK_ARG((reinterpret_cast<uintptr_t>(scratch) & 255) == 0, "risp_origin_bm3d: scratch must be 256-byte aligned");
    const size_t per = layout(H, W).total;
    RISP_CHECK_ARG(scratch_bytes >= per, "risp_origin_bm3d: scratch of %zu bytes holds no image (%zu needed per image)",
                   scratch_bytes, per);
    const int chunk = (int)((scratch_bytes / per) < (size_t)N ? scratch_bytes / per : (size_t)N);
    const int rows = layout(H, W).rows;
    hipStream_t s = (hipStream_t)stream;
    for (int n0 = 0; n0 < N; n0 += chunk) {
        const int nb = N - n0 < chunk ? N - n0 : chunk;
        Args a;
        a.x = x + (size_t)n0 * 3 * H * W;
        a.y = y + (size_t)n0 * 3 * H * W;
        a.sigma = sigma + n0; a.n1 = n1 + n0; a.cspace = cspace + n0; a.wtransform = wtransform + n0; a.radius = radius + n0;
        a.groups = groups ? groups + (size_t)n0 * rows * TCOLS : nullptr;
        a.scratch = static_cast<char *>(scratch);
        a.per = per; a.H = H; a.W = W; a.rows = rows; a.si = in_scale; a.so = out_div;
        hipLaunchKernelGGL(bm3d_prep_kernel, dim3((H * W + 255) / 256, nb), dim3(256), 0, s, a);
        hipLaunchKernelGGL(bm3d_match_kernel, dim3((rows + 3) / 4, nb), dim3(256), 0, s, a);
        hipLaunchKernelGGL(bm3d_filter_kernel<1>, dim3((rows + 15) / 16, nb), dim3(256), 0, s, a);
        hipLaunchKernelGGL(bm3d_aggregate_kernel<1>, dim3((W + AT - 1) / AT, (H + AT - 1) / AT, nb), dim3(256), 0, s, a);
        hipLaunchKernelGGL(bm3d_filter_kernel<2>, dim3((rows + 15) / 16, nb), dim3(256), 0, s, a);
        hipLaunchKernelGGL(bm3d_aggregate_kernel<2>, dim3((W + AT - 1) / AT, (H + AT - 1) / AT, nb), dim3(256), 0, s, a);
        RISP_LAUNCH_CHECK("risp_origin_bm3d");
    }
    return 0;
}

}  // extern "C"
