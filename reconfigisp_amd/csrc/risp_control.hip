// Auto white balance and auto exposure on the device: the controller that reads the 3A statistics of risp_stats.hip and writes the
// gains of the next frame into a lens-shading map.  The definition is in include/risp.h; tests/control_reference.py restates it in
// numpy int64.  Everything is integers: counts, sums, floor divisions and shifts, so the result is exact and has no summation
// order.
//
// risp_control_solve is ONE launch.  A workgroup of four waves takes zones and green histogram rows grid-stride:
//   zones      a thread per zone: four 64-bit divisions, the candidate test, then [AR, AG, AB, K] by wave shuffles and through LDS
//   histogram  a row is the `bins` words of one image and green plane; its words are added into the workgroup's copy of Hg in LDS
//              (64-bit LDS adds: a bin of one image is below 2^31, a workgroup may see many images)
// and then adds what is not zero to scratch = [ticket, AR, AG, AB, K, Hg[bins]] with 64-bit agent-scope atomics, one per value.
//
// The hand-off (the counter form of an in-launch reduction).  Per-XCD L2s are not coherent and a CU's L1 is never refreshed by
// another CU's stores, so the payload moves ONLY in agent-scope atomics, which are carried out at the memory side: adds on the way
// in, exchanges on the way out.  There is no plain store that another workgroup reads in the same launch.  Order on the way in:
// every wave waits for its own atomics (s_waitcnt vmcnt(0): atomics without a return count there like stores), the workgroup
// meets at a barrier, thread 0 issues an agent-scope release fence and waits again (inline asm: the compiler may drop the
// fence's own wait), and only then draws the ticket with a returning agent-scope add.  So when the ticket of workgroup w is
// visible, every add of w has been carried out.  The workgroup that draws gridDim.x - 1 has seen every other ticket drawn, hence
// every add done; its thread 0 issues an agent-scope acquire and waits, a barrier lets the other waves on, and every accumulator
// is taken with an atomic exchange against 0 - the read of the total and the zeroing for the next launch or replay in one.  No
// workgroup waits for another or polls: whoever comes last does the work, whoever does not leaves.  The ticket is reset by the
// same workgroup at the end; the caller zeroes scratch once, before the first launch.
//
// The last workgroup: Hg lies in its LDS; wave 0 sums T and the sum of Hg * v lane-strided, then walks the bins 64 at a time with a
// wave prefix sum (shuffles) and a ballot for b*; thread 0 solves - a few dozen scalar integer operations - and stores the
// sixteen state words.
//
// risp_gain_map is a streaming launch behind it: a thread per node, 8 bytes in, 8 bytes out.
#include <string.h>
#include "risp_common.h"

namespace {

typedef unsigned long long u64;

constexpr int ZONES_PER_WG = 256, MAX_WGS = 1024;       // the grid rule of include/risp.h
constexpr int SLOT_TICKET = 0, SLOT_SUMS = 1, SLOT_HG = 5;

// the nineteen integers of a control specification, in the order of include/risp.h
struct Spec {
    int fill, y_lo, y_hi, rg_lo, rg_hi, bg_lo, bg_hi, min_share, wb_dead, wb_speed, wb_min, wb_max, pct, target, ceil, ae_dead,
        ae_speed, e_min, e_max;
};
static_assert(sizeof(Spec) == sizeof(int) * RISP_CONTROL_SPEC_INTS, "Spec mirrors the specification of include/risp.h");

struct Control {
    Spec s;
    int N, ZH, ZW, H, W, zone_h, zone_w, bins, shift, cfa;
    unsigned all_zones;                                 // N * ZH * ZW <= 2^24
};

__device__ __forceinline__ void agent_add(u64 *p, u64 v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ u64 agent_take(u64 *p) {
    return __hip_atomic_exchange(p, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

__device__ __forceinline__ unsigned clampu(unsigned v, unsigned lo, unsigned hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ unsigned damp(unsigned cur, unsigned corr, int dead, int speed, int lo, int hi) {
    int d = (int)corr - 4096;
    if ((d < 0 ? -d : d) <= dead) d = 0;
    const int step = 4096 + ((d * speed) >> 8);         // an arithmetic shift: floor
    return clampu((cur * (unsigned)step + 2048u) >> 12, (unsigned)lo, (unsigned)hi);
}

__global__ __launch_bounds__(256) void control_solve_kernel(const u64 *__restrict__ zones, const unsigned *__restrict__ hist,
                                                            int *state, u64 *scratch, const Control a) {
    extern __shared__ __attribute__((aligned(16))) u64 lds[];
    u64 *part = lds, *last = lds + 16, *hg = lds + 18;          // [4 waves][AR, AG, AB, K]; "this workgroup drew the last ticket"; Hg
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k = a.cfa;
    for (int b = tid; b < a.bins; b += 256) hg[b] = 0ull;
    __syncthreads();

    // ---- the zones
    u64 acc[4] = {0ull, 0ull, 0ull, 0ull};
    const unsigned per_image = (unsigned)a.ZH * (unsigned)a.ZW;
    for (unsigned z = blockIdx.x * 256u + tid; z < a.all_zones; z += gridDim.x * 256u) {
        const unsigned rest = z % per_image, zy = rest / (unsigned)a.ZW, zx = rest - zy * (unsigned)a.ZW;
        const int rows = a.H - (int)zy * a.zone_h < a.zone_h ? a.H - (int)zy * a.zone_h : a.zone_h;
        const int cols = a.W - (int)zx * a.zone_w < a.zone_w ? a.W - (int)zx * a.zone_w : a.zone_w;
        const u64 need = (u64)a.s.fill * ((u64)(rows / 2) * (u64)(cols / 2));
        const u64 *p = zones + (size_t)z * 12;
        u64 sums[4], counts[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) sums[c] = p[3 * c], counts[c] = p[3 * c + 1];
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // the eight loads fly together (left alone, each sinks to its division)
        unsigned m[4];
        bool filled = true;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const u64 sum = sums[c], count = counts[c];
            filled = filled && count >= 1 && count * 256ull >= need;
            const u64 q = count ? (sum + (count >> 1)) / count : 0ull;
            m[c] = q > 65535ull ? 65535u : (unsigned)q;
        }
        const unsigned mr = m[0 ^ k], mg = (m[1 ^ k] + m[2 ^ k] + 1u) >> 1, mb = m[3 ^ k];
        const bool cand = filled && mg >= (unsigned)a.s.y_lo && mg <= (unsigned)a.s.y_hi &&
                          (unsigned)a.s.rg_lo * mg <= 256u * mr && 256u * mr <= (unsigned)a.s.rg_hi * mg &&
                          (unsigned)a.s.bg_lo * mg <= 256u * mb && 256u * mb <= (unsigned)a.s.bg_hi * mg;
        if (cand) {
            acc[0] += mr, acc[1] += mg, acc[2] += mb, acc[3] += 1ull;
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const u64 t = wave_sum_u64(acc[i]);
        if (lane == 0) part[4 * wave + i] = t;
    }

    // ---- the green histogram rows: row r is image r / 2, plane gr (r even) or gb (r odd)
    for (long long r = blockIdx.x; r < 2LL * a.N; r += gridDim.x) {
        const unsigned *row = hist + ((size_t)(r >> 1) * 4 + (size_t)(((r & 1) ? 2 : 1) ^ k)) * (size_t)a.bins;
        for (int b = tid; b < a.bins; b += 256) {
            const unsigned v = row[b];
            if (v) atomicAdd(&hg[b], (u64)v);
        }
    }
    __syncthreads();

    // ---- what is not zero goes to scratch, then the ticket
    if (tid < 4) {
        const u64 t = part[tid] + part[4 + tid] + part[8 + tid] + part[12 + tid];
        if (t) agent_add(scratch + SLOT_SUMS + tid, t);
    }
    for (int b = tid; b < a.bins; b += 256) {
        const u64 v = hg[b];
        if (v) agent_add(scratch + SLOT_HG + b, v);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");            // every wave: its adds have been carried out
    __syncthreads();
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const u64 ticket = __hip_atomic_fetch_add(scratch + SLOT_TICKET, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const bool mine = ticket == (u64)gridDim.x - 1ull;
        if (mine) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        *last = mine ? 1ull : 0ull;
    }
    __syncthreads();
    if (*last == 0ull) return;

    // ---- the last workgroup: take the totals, leave zeros
    for (int b = tid; b < a.bins; b += 256) hg[b] = agent_take(scratch + SLOT_HG + b);
    if (tid < 4) part[tid] = agent_take(scratch + SLOT_SUMS + tid);
    __syncthreads();
    if (wave != 0) return;

    u64 T = 0ull, S = 0ull;
    const unsigned half = (1u << a.shift) >> 1;
    for (int b = lane; b < a.bins; b += 64) {
        const unsigned c = ((unsigned)b << a.shift) + half;
        T += hg[b];
        S += hg[b] * (u64)(c > 65535u ? 65535u : c);
    }
    // (every lane needs T: down-shuffles leave the total in lane 0)
    T = __shfl(wave_sum_u64(T), 0, 64);
    S = wave_sum_u64(S);
    int bstar = a.bins - 1;
    if (T) {
        const u64 want = T * (u64)a.s.pct;
        u64 carry = 0ull;
        for (int b0 = 0; b0 < a.bins; b0 += 64) {                   // wave-uniform
            u64 c = b0 + lane < a.bins ? hg[b0 + lane] : 0ull;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const u64 up = __shfl_up(c, o, 64);
                if (lane >= o) c += up;
            }
            c += carry;
            const u64 hit = __ballot(b0 + lane < a.bins && c * 65536ull >= want);
            if (hit) {
                bstar = b0 + __ffsll((long long)hit) - 1;
                break;
            }
            carry = __shfl(c, 63, 64);
        }
    }
    if (lane != 0) return;

    const Spec &s = a.s;
    const unsigned e = (unsigned)state[0], wr = (unsigned)state[1], wb = (unsigned)state[2];
    unsigned e2 = e, wr2 = wr, wb2 = wb, M = 0u, P = 0u, flags = 0u;
    const u64 AR = part[0], AG = part[1], AB = part[2], K = part[3];
    if (K >= 1ull && K * 256ull >= (u64)s.min_share * (u64)a.all_zones && AR > 0ull && AB > 0ull) {
        const u64 qr = (AG << 12) / AR, qb = (AG << 12) / AB;
        const unsigned cr = qr < 1024ull ? 1024u : (qr > 16384ull ? 16384u : (unsigned)qr);
        const unsigned cb = qb < 1024ull ? 1024u : (qb > 16384ull ? 16384u : (unsigned)qb);
        wr2 = damp(wr, cr, s.wb_dead, s.wb_speed, s.wb_min, s.wb_max);
        wb2 = damp(wb, cb, s.wb_dead, s.wb_speed, s.wb_min, s.wb_max);
        flags |= 1u;
    }
    if (T) {
        M = (unsigned)((S + (T >> 1)) / T);
        const unsigned edge = ((unsigned)(bstar + 1) << a.shift) - 1u;
        P = edge > 65535u ? 65535u : edge;
        unsigned corr = clampu(((unsigned)s.target << 12) / (M ? M : 1u), 1024u, 16384u);
        if (P * corr > ((unsigned)s.ceil << 12)) {
            corr = clampu(((unsigned)s.ceil << 12) / (P ? P : 1u), 1024u, 16384u);
            flags |= 4u;
        }
        e2 = damp(e, corr, s.ae_dead, s.ae_speed, s.e_min, s.e_max);
        flags |= 2u;
    }
    state[0] = (int)e2, state[1] = (int)wr2, state[2] = (int)wb2;
    state[3] = (int)(((unsigned)state[3] + 1u) & 0x7fffffffu);
    state[4] = (int)M, state[5] = (int)P;
    state[6] = K > 2147483647ull ? 2147483647 : (int)K;
    state[7] = (int)flags;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int q = p ^ k;
        const unsigned g = (e2 * (q == 0 ? wr2 : (q == 3 ? wb2 : 4096u)) + 2048u) >> 12;
        state[8 + p] = (int)(g > 65535u ? 65535u : g);
    }
    state[12] = state[13] = state[14] = state[15] = 0;
    agent_take(scratch + SLOT_TICKET);
}

__global__ __launch_bounds__(256) void gain_map_kernel(const ushort4 *__restrict__ base, const int *__restrict__ state,
                                                       ushort4 *__restrict__ out, unsigned nodes) {
    const unsigned g0 = (unsigned)state[8], g1 = (unsigned)state[9], g2 = (unsigned)state[10], g3 = (unsigned)state[11];
    auto one = [](unsigned b, unsigned g) {
        const unsigned v = (b * g + 2048u) >> 12;
        return (unsigned short)(v > 65535u ? 65535u : v);
    };
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < nodes; i += gridDim.x * 256u) {
        const ushort4 b = base ? base[i] : ushort4{4096, 4096, 4096, 4096};
        out[i] = ushort4{one(b.x, g0), one(b.y, g1), one(b.z, g2), one(b.w, g3)};
    }
}

struct Range {
    const char *field;
    int lo, hi;
};
// the ranges of the specification, in its order
const Range RANGES[RISP_CONTROL_SPEC_INTS] = {
    {"fill", 0, 256},       {"y_lo", 0, 65535},    {"y_hi", 0, 65535},    {"rg_lo", 0, 4095},      {"rg_hi", 0, 4095},
    {"bg_lo", 0, 4095},     {"bg_hi", 0, 4095},    {"min_share", 0, 256}, {"wb_dead", 0, 4095},    {"wb_speed", 0, 256},
    {"wb_min", 256, 65535}, {"wb_max", 256, 65535}, {"pct", 1, 65536},    {"target", 1, 65535},    {"ceil", 1, 65535},
    {"ae_dead", 0, 4095},   {"ae_speed", 0, 256},  {"e_min", 256, 65535}, {"e_max", 256, 65535}};
// the pairs lo <= hi, as indices into the specification
const int PAIRS[5][2] = {{1, 2}, {3, 4}, {5, 6}, {10, 11}, {17, 18}};

}  // namespace

extern "C" int risp_control_solve(const long long *zones, const int *hist, int *state, unsigned long long *scratch, const int *spec,
                                  int N, int ZH, int ZW, int H, int W, int zone_h, int zone_w, int bins, int hist_shift, int cfa,
                                  void *stream) {
    const char *name = "risp_control_solve";
    RISP_CHECK_ARG(zones && hist && state && scratch && spec, "%s: null argument", name);
    for (int i = 0; i < RISP_CONTROL_SPEC_INTS; ++i)
        RISP_CHECK_ARG(spec[i] >= RANGES[i].lo && spec[i] <= RANGES[i].hi, "%s: %s %d outside %d .. %d", name, RANGES[i].field, spec[i],
                       RANGES[i].lo, RANGES[i].hi);
    for (const auto &pr : PAIRS)
        RISP_CHECK_ARG(spec[pr[0]] <= spec[pr[1]], "%s: %s %d above %s %d", name, RANGES[pr[0]].field, spec[pr[0]], RANGES[pr[1]].field,
                       spec[pr[1]]);
    RISP_CHECK_ARG(N >= 1 && H >= 2 && H % 2 == 0, "%s: bad shape N=%d H=%d (H even)", name, N, H);
    RISP_CHECK_ARG(W >= 4 && W % 4 == 0, "%s: W %d (a multiple of 4)", name, W);
    RISP_CHECK_ARG(zone_h >= 2 && zone_h % 2 == 0, "%s: zone_h %d (even, at least 2)", name, zone_h);
    RISP_CHECK_ARG(zone_w >= 4 && zone_w % 4 == 0, "%s: zone_w %d (a multiple of 4)", name, zone_w);
    const long long zh = ((long long)H + zone_h - 1) / zone_h, zw = ((long long)W + zone_w - 1) / zone_w;
    RISP_CHECK_ARG(ZH == zh && ZW == zw, "%s: ZH %d, ZW %d: a %d x %d frame has %lld x %lld zones of %d x %d", name, ZH, ZW, H, W, zh,
                   zw, zone_h, zone_w);
    RISP_CHECK_ARG(zh * zw <= (1LL << 24) && (long long)N * zh * zw <= (1LL << 24), "%s: %d x %lld x %lld zones, more than 2^24", name,
                   N, zh, zw);
    // N * (H * W / 2) < 2^40 without the product: H * W / 2 < ceil(2^40 / N)
    RISP_CHECK_ARG((long long)H * W / 2 < ((1LL << 40) + N - 1) / N, "%s: %d frames of %d x %d: N * H * W / 2 reaches 2^40", name, N, H, W);
    RISP_CHECK_ARG(bins >= 1 && bins <= 1024, "%s: bins %d outside 1 .. 1024", name, bins);
    RISP_CHECK_ARG(hist_shift >= 0 && hist_shift <= 16, "%s: hist_shift %d outside 0 .. 16", name, hist_shift);
    RISP_CHECK_ARG(cfa >= 0 && cfa <= 3, "%s: cfa %d outside 0 .. 3", name, cfa);
    RISP_CHECK_ARG(reinterpret_cast<uintptr_t>(zones) % 8 == 0 && reinterpret_cast<uintptr_t>(scratch) % 8 == 0 &&
                       reinterpret_cast<uintptr_t>(hist) % 4 == 0 && reinterpret_cast<uintptr_t>(state) % 4 == 0,
                   "%s: zones %p and scratch %p must be 8-byte, hist %p and state %p 4-byte aligned", name, (const void *)zones,
                   (void *)scratch, (const void *)hist, (void *)state);
    Control a;
    memcpy(&a.s, spec, sizeof(Spec));
    a.N = N, a.ZH = ZH, a.ZW = ZW, a.H = H, a.W = W, a.zone_h = zone_h, a.zone_w = zone_w, a.bins = bins, a.shift = hist_shift, a.cfa = cfa;
    a.all_zones = (unsigned)((long long)N * zh * zw);
    unsigned wgs = (a.all_zones + ZONES_PER_WG - 1) / ZONES_PER_WG;
    wgs = wgs < 1 ? 1 : (wgs > MAX_WGS ? MAX_WGS : wgs);
    const size_t shared = sizeof(u64) * (size_t)(18 + bins);
    hipLaunchKernelGGL(control_solve_kernel, dim3(wgs), dim3(256), shared, (hipStream_t)stream,
                       reinterpret_cast<const u64 *>(zones), reinterpret_cast<const unsigned *>(hist), state, scratch, a);
    RISP_LAUNCH_CHECK(name);
    return 0;
}

extern "C" int risp_gain_map(const uint16_t *base, const int *state, uint16_t *out, int GH, int GW, void *stream) {
    const char *name = "risp_gain_map";
    RISP_CHECK_ARG(state && out, "%s: null argument", name);
    RISP_CHECK_ARG(GH >= 2 && GW >= 2 && (long long)GH * GW <= (1LL << 30), "%s: a map of %d x %d nodes (at least 2 x 2, at most 2^30 nodes)",
                   name, GH, GW);
    RISP_CHECK_ARG(reinterpret_cast<uintptr_t>(base) % 8 == 0 && reinterpret_cast<uintptr_t>(out) % 8 == 0 &&
                       reinterpret_cast<uintptr_t>(state) % 4 == 0,
                   "%s: base %p and out %p must be 8-byte, state %p 4-byte aligned", name, (const void *)base, (void *)out,
                   (const void *)state);
    const unsigned nodes = (unsigned)GH * (unsigned)GW;
    if (base) {
        const uintptr_t b = reinterpret_cast<uintptr_t>(base), o = reinterpret_cast<uintptr_t>(out), bytes = 8 * (uintptr_t)nodes;
        RISP_CHECK_ARG(b + bytes <= o || o + bytes <= b, "%s: out %p overlaps base %p (%d x %d nodes of 8 bytes)", name, (void *)out,
                       (const void *)base, GH, GW);
    }
    const unsigned blocks = (nodes + 255u) / 256u;
    hipLaunchKernelGGL(gain_map_kernel, dim3(blocks > 4096u ? 4096u : blocks), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const ushort4 *>(base), state, reinterpret_cast<ushort4 *>(out), nodes);
    RISP_LAUNCH_CHECK(name);
    return 0;
}
