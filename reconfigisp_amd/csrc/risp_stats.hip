// 3A statistics of (N,H,W) sensor frames, one launch over the frame behind the zeroing: per zone and Bayer plane the sum and the
// count of the samples inside lo .. hi and the horizontal same-colour focus measure, per image and plane a histogram.  The
// definition is in include/risp.h; tests/stats_reference.py restates it in numpy int64.  Everything is a count or a sum of
// integers: there is no summation order and the result is exact.  The frames come as uint16 rows or MIPI-packed RAW10 / RAW12
// (risp_rawpack.h) and are decoded on the way: bits / 8 bytes read per pixel, nothing written but the statistics.
//
// A workgroup of four waves owns one tile of TILE_W = 256 columns x TH rows (TH 64, 32 or 16, picked by the host).  A lane owns a
// group of four columns x .. x+3 (x % 4 == 0), which lies in one zone column (zone_w % 4 == 0) and in one 5-byte or 3-byte group
// pair; a wave owns TH / 4 consecutive rows and walks them in pairs, which lie in one zone row (zone_h even, H even).  Per row
// the lane loads the group and the pairs left and right of it, columns x-2 .. x+5, with risp_rawframe.h's load_row; a pair outside
// the row is not loaded (it is 0 and unused: the form without the reflection) and its two pixels add nothing to the focus term.
//
// Accumulation.  The lane keeps [sum, count, sharp] of the four planes in twelve 32-bit registers while its zone row lasts.  At
// a zone-row change and behind its last row they go to the tile's table in LDS, twelve LDS adds into the lane's copy of the
// entry (below).  Every sample also adds 1 to the
// workgroup's private histogram in LDS.  Behind the tile one 64-bit global atomic goes out per non-zero table entry - a (zone,
// plane, quantity) the tile touched, and one 32-bit global atomic per non-empty bin.  Integer atomics only.  (A form in which a
// launch had at most 1024 workgroups, each with a run of consecutive tiles and one histogram flush per image of the run, was
// measured and lost where it differed: profiles/serve_stats_forms.txt.)
//
// 32-bit partials.  A table entry holds at most a tile's samples of one plane: 256 * 64 / 4 = 4096 samples, each at most
// 65535 in sum and 2 * 65535 = 131070 in sharp: 4096 * 131070 = 536 862 720 < 2^32 (a tile could be eight times as large).
// A histogram bin holds at most the pixels of one plane of one image, H * W / 4, which the host keeps below 2^31 (the output
// is int32).
#include "risp_common.h"
#include "risp_rawframe.h"

namespace {

using namespace risp_rawframe;

constexpr int TILE_W = 256;                 // 64 lanes x 4 columns
#ifndef RISP_STATS_MAX_TH
#define RISP_STATS_MAX_TH 64                // (make EXTRA=-DRISP_STATS_MAX_TH=32 / 16: lower tiles, profiles/serve_stats.txt)
#endif
constexpr int MAX_TH = RISP_STATS_MAX_TH;   // the largest tile height: the bound of the 32-bit partials above rests on it
static_assert(MAX_TH == 16 || MAX_TH == 32 || MAX_TH == 64, "a wave owns TH / 4 rows in pairs; the bound of the partials is stated for 64 rows");
#ifndef RISP_STATS_MIN_TILES
#define RISP_STATS_MIN_TILES 512            // a taller tile is taken only while the launch keeps this many tiles
#endif
constexpr size_t LDS_BYTES = 64 * 1024;     // what a workgroup may ask for
// Lanes that share a zone add to one LDS address, and such adds are served one after the other: with zones wider than the tile
// twelve adds of 64 lanes each.  So an entry has up to MAX_COPIES copies, lane l adds to copy l % copies, and the flush behind the
// tile adds the copies up.  The copies are halved until the table has at most COPY_ENTRIES words: small zones, which spread
// the lanes by themselves, get one.
#ifndef RISP_STATS_MAX_COPIES
#define RISP_STATS_MAX_COPIES 16            // (make EXTRA=-DRISP_STATS_MAX_COPIES=1: one entry per zone, profiles/serve_stats.txt)
#endif
constexpr int MAX_COPIES = RISP_STATS_MAX_COPIES, COPY_ENTRIES = 2048;

struct Stats {
    unsigned long long *zones;              // (N,ZH,ZW,4,3)
    unsigned *hist;                         // (N,4,bins)
    int H, W, stride;
    unsigned black, lo, hi;
    int zone_h, zone_w, ZH, ZW, bins, shift;
    int th, tiles_x, tiles_y;               // tile height, tiles per row of tiles, rows of tiles per image
    long long tiles;                        // all tiles: one workgroup each
    int table, copies;                      // entries of the zone table in LDS: 12 per zone a tile can touch and copy; copies of an entry
};

// one row of the lane's group: YP is the row's parity, acc[3 * plane + (0 sum, 1 count, 2 sharp)]
template <int YP>
__device__ __forceinline__ void add_row(const Row &r, const Stats &a, bool left, bool right, unsigned *hist, unsigned (&acc)[12]) {
    unsigned s[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) s[i] = r.v[i] > a.black ? r.v[i] - a.black : 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = 2 * YP + (i & 1);                 // the plane: 2 * (y & 1) + (x & 1), x % 4 == 0
        const unsigned v = s[i + 2];
        const bool in = v >= a.lo && v <= a.hi;
        acc[3 * c] += in ? v : 0u;
        acc[3 * c + 1] += in ? 1u : 0u;
        const int d = (int)(2u * v) - (int)s[i] - (int)s[i + 4];
        const bool edge = i < 2 ? left : right;        // x + i < 2 or x + i >= W - 2: a neighbour lies outside the frame
        acc[3 * c + 2] += edge ? 0u : (unsigned)(d < 0 ? -d : d);
        const unsigned bin = v >> a.shift;
        atomicAdd(&hist[c * a.bins + (bin < (unsigned)a.bins ? bin : (unsigned)a.bins - 1u)], 1u);
    }
}

template <int BITS, bool WIDE>
__global__ __launch_bounds__(256) void raw_stats_kernel(const uint8_t *__restrict__ raw, const Stats a) {
    extern __shared__ unsigned lds[];
    unsigned *hist = lds, *table = lds + 4 * a.bins;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int e = tid; e < 4 * a.bins + a.table; e += 256) lds[e] = 0u;
    __syncthreads();
    const int per_image = a.tiles_x * a.tiles_y, rows = a.th / 4;
    const unsigned n = blockIdx.x / (unsigned)per_image;
    const int rest = (int)(blockIdx.x - n * (unsigned)per_image);       // the workgroup's tile: image n, at (y0, x0)
    const int x0 = (rest % a.tiles_x) * TILE_W, y0 = (rest / a.tiles_x) * a.th;
    const int xe = x0 + TILE_W < a.W ? x0 + TILE_W : a.W, ye = y0 + a.th < a.H ? y0 + a.th : a.H;
    // the zones the tile touches: columns zc0 .. zc0 + ncol - 1, rows zr0 .. zr0 + nrow - 1
    const int zc0 = x0 / a.zone_w, ncol = (xe - 1) / a.zone_w - zc0 + 1;
    const int zr0 = y0 / a.zone_h, nrow = (ye - 1) / a.zone_h - zr0 + 1;
    const int x = x0 + 4 * lane;
    const bool active = x < a.W, left = x == 0, right = x + 4 >= a.W;
    const int zc = (active ? x / a.zone_w : zc0) - zc0;
    const uint8_t *img = raw + (size_t)n * (size_t)a.H * (size_t)a.stride;
    unsigned acc[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) acc[k] = 0u;

    // the lane's partials into its copy of the table entry of zone row `zr`
    auto flush = [&](int zr) {
        unsigned *dst = table + (((zr - zr0) * ncol + zc) * a.copies + (lane & (a.copies - 1))) * 12;
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            if (acc[k]) atomicAdd(dst + k, acc[k]);
            acc[k] = 0u;
        }
    };

    const int yw = y0 + wave * rows;                // even: th % 8 == 0
    int zr = yw < ye ? yw / a.zone_h : zr0;
    for (int p = 0; p < rows; p += 2) {
        const int y = yw + p;
        if (y >= ye) break;                         // (wave-uniform; H is even, so row y + 1 exists)
        const int z = y / a.zone_h;
        if (z != zr) {
            flush(zr);
            zr = z;
        }
        if (active) {
            const uint8_t *row = img + (size_t)y * (size_t)a.stride;
            const Row r0 = load_row<BITS, WIDE, false>(row, x, left, right);
            const Row r1 = load_row<BITS, WIDE, false>(row + a.stride, x, left, right);
            add_row<0>(r0, a, left, right, hist, acc);
            add_row<1>(r1, a, left, right, hist, acc);
        }
    }
    if (yw < ye) flush(zr);
    __syncthreads();
    // one 64-bit atomic per (zone, plane, quantity) the tile touched
    for (int e = tid; e < nrow * ncol * 12; e += 256) {
        const int z = e / 12, k = e - z * 12, r = z / ncol, c = z - r * ncol;
        unsigned v = 0u;
        for (int j = 0; j < a.copies; ++j) v += table[(z * a.copies + j) * 12 + k];
        if (v) atomicAdd(&a.zones[(((size_t)n * a.ZH + (zr0 + r)) * a.ZW + (zc0 + c)) * 12 + k], (unsigned long long)v);
    }
    // and one 32-bit atomic per non-empty bin of the tile's plane histograms
    for (int e = tid; e < 4 * a.bins; e += 256) {
        const unsigned v = hist[e];
        if (v) atomicAdd(&a.hist[(size_t)n * 4 * a.bins + e], v);
    }
}

// the zones a tile of `span` columns or rows can touch when its owners start every `step`: zone indices over a range of
// span - step differ by at most (span - step) / zone + 1, and there are span / step owners
inline int zones_across(int span, int step, int zone) {
    const int a = (span - step) / zone + 2, b = span / step;
    return a < b ? a : b;
}

}  // namespace

extern "C" int risp_raw_stats(const void *raw, int bits, int stride, int black_level, long long *zones, int *hist, int zone_h,
                              int zone_w, int bins, int hist_shift, int lo, int hi, int N, int H, int W, void *stream) {
    const char *name = "risp_raw_stats";
    RISP_CHECK_ARG(raw && zones && hist, "%s: null argument", name);
    RISP_CHECK_ARG(N >= 1 && H >= 2 && H % 2 == 0, "%s: bad shape N=%d H=%d (H even: a row pair lies in one zone row)", name, N, H);
    if (int err = frame_check(name, raw, bits, W, stride)) return err;
    RISP_CHECK_ARG(black_level >= 0 && black_level <= 65535, "%s: black_level %d outside 0 .. 65535", name, black_level);
    RISP_CHECK_ARG(zone_h >= 2 && zone_h % 2 == 0, "%s: zone_h %d (even, at least 2)", name, zone_h);
    RISP_CHECK_ARG(zone_w >= 4 && zone_w % 4 == 0, "%s: zone_w %d (a multiple of 4)", name, zone_w);
    const long long ZH = ((long long)H + zone_h - 1) / zone_h, ZW = ((long long)W + zone_w - 1) / zone_w;
    RISP_CHECK_ARG(ZH * ZW <= 65536, "%s: %lld x %lld zones, more than 65536", name, ZH, ZW);
    RISP_CHECK_ARG(bins >= 1 && bins <= 1024, "%s: bins %d outside 1 .. 1024", name, bins);
    RISP_CHECK_ARG(hist_shift >= 0 && hist_shift <= 16, "%s: hist_shift %d outside 0 .. 16", name, hist_shift);
    RISP_CHECK_ARG(0 <= lo && lo <= hi && hi <= 65535, "%s: lo %d, hi %d (0 <= lo <= hi <= 65535)", name, lo, hi);
    RISP_CHECK_ARG((long long)H * W / 4 <= 2147483647LL, "%s: %d x %d frames: a plane's count does not fit the int32 histogram", name, H, W);
    RISP_CHECK_ARG(reinterpret_cast<uintptr_t>(zones) % 8 == 0 && reinterpret_cast<uintptr_t>(hist) % 4 == 0,
                   "%s: zones %p must be 8-byte and hist %p 4-byte aligned", name, (void *)zones, (void *)hist);
    Stats a;
    a.zones = reinterpret_cast<unsigned long long *>(zones), a.hist = reinterpret_cast<unsigned *>(hist);
    a.H = H, a.W = W, a.stride = stride;
    a.black = (unsigned)black_level, a.lo = (unsigned)lo, a.hi = (unsigned)hi;
    a.zone_h = zone_h, a.zone_w = zone_w, a.ZH = (int)ZH, a.ZW = (int)ZW, a.bins = bins, a.shift = hist_shift;
    a.tiles_x = (W + TILE_W - 1) / TILE_W;
    // the tallest tile that leaves the launch RISP_STATS_MIN_TILES tiles and whose zone table fits half the LDS beside the
    // histogram; 16 rows otherwise (there the table has at most 64 x 8 zones, 24 KiB, beside at most 16 KiB of histogram)
    for (a.th = MAX_TH;; a.th /= 2) {
        a.tiles_y = (H + a.th - 1) / a.th;
        a.tiles = (long long)N * a.tiles_x * a.tiles_y;
        a.table = 12 * zones_across(TILE_W, 4, zone_w) * zones_across(a.th, 2, zone_h);
        for (a.copies = MAX_COPIES; a.copies > 1 && a.table * a.copies > COPY_ENTRIES; a.copies /= 2) {}
        a.table *= a.copies;
        if (a.th <= 16 || (a.tiles >= RISP_STATS_MIN_TILES && sizeof(unsigned) * (size_t)(4 * bins + a.table) <= LDS_BYTES / 2)) break;
    }
    RISP_CHECK_ARG(a.tiles <= 2147483647LL, "%s: %lld tiles of %d x %d, more than a launch has workgroups", name, a.tiles, TILE_W, a.th);
    const size_t shared = sizeof(unsigned) * (size_t)(4 * bins + a.table);
    const dim3 grid((unsigned)a.tiles);
    hipStream_t s = (hipStream_t)stream;
    // both outputs are overwritten: zeroed on the stream, so a captured call replays from zero.  One memset where the histogram
    // lies right behind the zones (functional.RawStatistics allocates them so), two otherwise
    const size_t zone_bytes = sizeof(long long) * (size_t)N * (size_t)(ZH * ZW) * 12, hist_bytes = sizeof(int) * (size_t)N * 4 * bins;
    const bool joined = reinterpret_cast<char *>(zones) + zone_bytes == reinterpret_cast<char *>(hist);
    if (hipMemsetAsync(zones, 0, joined ? zone_bytes + hist_bytes : zone_bytes, s) != hipSuccess ||
        (!joined && hipMemsetAsync(hist, 0, hist_bytes, s) != hipSuccess)) {
        risp_set_error("%s: memset failed", name);
        return 2;
    }
    const uint8_t *src = static_cast<const uint8_t *>(raw);
    dispatch(bits, raw, stride, [&](auto bits_c, auto wide_c) {
        hipLaunchKernelGGL((raw_stats_kernel<decltype(bits_c)::value, decltype(wide_c)::value>), grid, dim3(256), shared, s, src, a);
    });
    RISP_LAUNCH_CHECK(name);
    return 0;
}
