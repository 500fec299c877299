"""The device-side auto white balance / auto exposure controller restated in numpy int64 - the definition of include/risp.h,
independent of the kernels.

``solve_ref`` is one update: zones (N,ZH,ZW,4,3) int64 [sum, count, sharp], hist (N,4,bins) int32 and the sixteen state words
-> the sixteen new state words.  ``gain_map_ref`` is the map a state gives.  ``loop_ref`` chains the lens shading, the 3A
statistics and the solve over a frame sequence, as ``serve(lens_shading=ctl.shading, statistics=st); ctl.update(st)`` does.
Every value here is non-negative and below 2^63, so int64 floor division is the unsigned 64-bit division of the definition;
the places where the definition promises 32 bits are asserted.

``VARIANTS`` are plausible mistakes.  ``SOLVE_CASES`` and ``MAP_CASES`` are the inputs of tests/test_gpu_control.py;
tests/test_control_reference_cpu.py shows that they tell every variant from the definition.  ``DEFAULTS`` are the settings of
``functional.control_spec`` and of the loop test, ``scene`` is that test's frame sequence."""
import numpy as np

import lens_shading_reference as LS
import stats_reference as SR

FIELDS = ('fill', 'y_lo', 'y_hi', 'rg_lo', 'rg_hi', 'bg_lo', 'bg_hi', 'min_share', 'wb_dead', 'wb_speed', 'wb_min', 'wb_max',
          'pct', 'target', 'ceil', 'ae_dead', 'ae_speed', 'e_min', 'e_max')
RANGES = dict(fill=(0, 256), y_lo=(0, 65535), y_hi=(0, 65535), rg_lo=(0, 4095), rg_hi=(0, 4095), bg_lo=(0, 4095), bg_hi=(0, 4095),
              min_share=(0, 256), wb_dead=(0, 4095), wb_speed=(0, 256), wb_min=(256, 65535), wb_max=(256, 65535), pct=(1, 65536),
              target=(1, 65535), ceil=(1, 65535), ae_dead=(0, 4095), ae_speed=(0, 256), e_min=(256, 65535), e_max=(256, 65535))
PAIRS = (('y_lo', 'y_hi'), ('rg_lo', 'rg_hi'), ('bg_lo', 'bg_hi'), ('wb_min', 'wb_max'), ('e_min', 'e_max'))
# the settings of the loop test (the issue's prototype), which functional.control_spec takes as its defaults; the four bounds of
# the gains, which the prototype does not name, are the full range of the correction a single update may ask for, 1/4 .. 16 -
# wide enough that no bound is active in the loop
DEFAULTS = dict(fill=192, y_lo=16, y_hi=900, rg_lo=64, rg_hi=1024, bg_lo=64, bg_hi=1024, min_share=32, wb_dead=40, wb_speed=160,
                wb_min=1024, wb_max=65535, pct=64880, target=170, ceil=900, ae_dead=120, ae_speed=160, e_min=1024, e_max=65535)

VARIANTS = ('mean_floor', 'green_gr', 'cfa_ignored', 'full_area', 'pct_strict', 'lower_edge', 'shift_trunc', 'no_deadband',
            'share_per_image', 'ag_32bit', 'hist_all_planes', 'map_floor', 'map_no_clamp')
STATE_INTS = 16
U32 = (1 << 32) - 1


def spec_tuple(**fields):
    """the nineteen integers of a specification in the header's order, ``DEFAULTS`` where a field is not given"""
    assert set(fields) <= set(FIELDS), set(fields) - set(FIELDS)
    return tuple(int(dict(DEFAULTS, **fields)[f]) for f in FIELDS)


def new_state(exposure=4096, wb=(4096, 4096), cfa=0):
    """the sixteen words ``reset`` writes: the gains, no update so far, g[] of these gains"""
    s = np.zeros(STATE_INTS, dtype=np.int64)
    s[0], s[1], s[2] = exposure, wb[0], wb[1]
    s[8:12] = _plane_gains(exposure, wb[0], wb[1], cfa)
    return s.astype(np.int32)


def _plane_gains(e, wr, wb, k):
    w = [wr if (p ^ k) == 0 else wb if (p ^ k) == 3 else 4096 for p in range(4)]
    return [min((int(e) * int(x) + 2048) >> 12, 65535) for x in w]


def _damp(cur, corr, dead, speed, lo, hi, variant):
    d = corr - 4096
    if variant != 'no_deadband' and abs(d) <= dead:
        d = 0
    if variant == 'shift_trunc':
        step = 4096 + (abs(d * speed) >> 8) * (1 if d >= 0 else -1)
    else:
        step = 4096 + ((d * speed) >> 8)                # Python's >> is the arithmetic shift: floor
    assert 1024 <= step <= 16384 and cur * step < 1 << 30
    return min(max((cur * step + 2048) >> 12, lo), hi)


def _clamp(v, lo=1024, hi=16384):
    return min(max(int(v), lo), hi)


def solve_ref(zones, hist, state, spec, geometry, variant=None):
    """One update.  ``spec``: the nineteen integers (``spec_tuple``); ``geometry`` = (H, W, zone_h, zone_w, hist_shift, cfa code);
    ``state``: sixteen integers.  -> the sixteen new words as int32.  ``variant``: None, or a name of ``VARIANTS``."""
    assert variant is None or variant in VARIANTS, variant
    f = dict(zip(FIELDS, (int(v) for v in spec)))
    h, w, zone_h, zone_w, shift, cfa = (int(v) for v in geometry)
    zones, hist = np.asarray(zones).astype(np.int64), np.asarray(hist).astype(np.int64)
    n, gh, gw = zones.shape[:3]
    bins = hist.shape[2]
    assert zones.shape == (n, gh, gw, 4, 3) and hist.shape == (n, 4, bins)
    assert (gh, gw) == SR.grid(h, w, (zone_h, zone_w)) and n * gh * gw <= 1 << 24 and n * h * w // 2 < 1 << 40
    assert zones[..., :2].min() >= 0 and hist.min() >= 0
    k = 0 if variant == 'cfa_ignored' else cfa
    e, wr, wb = (int(v) for v in state[:3])

    # ---- white balance
    zy, zx = np.mgrid[0:gh, 0:gw]
    if variant == 'full_area':
        area = np.full((gh, gw), (zone_h // 2) * (zone_w // 2), dtype=np.int64)
    else:
        area = (np.minimum(zone_h, h - zy * zone_h) // 2) * (np.minimum(zone_w, w - zx * zone_w) // 2)
    total, count = zones[..., 0], zones[..., 1]                                 # (N,ZH,ZW,4)
    assert count.max(initial=0) < 1 << 54 and total.max(initial=0) < 1 << 62
    filled = ((count >= 1) & (count * 256 >= f['fill'] * area[None, :, :, None])).all(axis=-1)
    safe = np.maximum(count, 1)
    m = np.where(count >= 1, (total + (0 if variant == 'mean_floor' else safe >> 1)) // safe, 0)
    m = np.minimum(m, 65535)
    mr, mb = m[..., 0 ^ k], m[..., 3 ^ k]
    mg = m[..., 1 ^ k] if variant == 'green_gr' else (m[..., 1 ^ k] + m[..., 2 ^ k] + 1) >> 1
    cand = (filled & (mg >= f['y_lo']) & (mg <= f['y_hi']) & (f['rg_lo'] * mg <= 256 * mr) & (256 * mr <= f['rg_hi'] * mg)
            & (f['bg_lo'] * mg <= 256 * mb) & (256 * mb <= f['bg_hi'] * mg))
    ar, ag, ab, kk = int(mr[cand].sum()), int(mg[cand].sum()), int(mb[cand].sum()), int(cand.sum())
    if variant == 'share_per_image':
        enough = all(int(cand[i].sum()) * 256 >= f['min_share'] * gh * gw for i in range(n))
    else:
        enough = kk * 256 >= f['min_share'] * n * gh * gw
    flags, wr2, wb2 = 0, wr, wb
    if kk >= 1 and enough and ar > 0 and ab > 0:
        num = (ag << 12) & U32 if variant == 'ag_32bit' else ag << 12
        wr2 = _damp(wr, _clamp(num // ar), f['wb_dead'], f['wb_speed'], f['wb_min'], f['wb_max'], variant)
        wb2 = _damp(wb, _clamp(num // ab), f['wb_dead'], f['wb_speed'], f['wb_min'], f['wb_max'], variant)
        flags |= 1

    # ---- exposure
    planes = [0, 1, 2, 3] if variant == 'hist_all_planes' else [1 ^ k, 2 ^ k]
    hg = hist[:, planes, :].sum(axis=(0, 1))
    t = int(hg.sum())
    big_m = big_p = 0
    e2 = e
    if t > 0:
        flags |= 2
        v = np.minimum((np.arange(bins, dtype=np.int64) << shift) + ((1 << shift) >> 1), 65535)
        assert t < 1 << 40
        big_m = (int((hg * v).sum()) + (t >> 1)) // t
        cum = np.cumsum(hg)
        hit = cum * 65536 > t * f['pct'] if variant == 'pct_strict' else cum * 65536 >= t * f['pct']
        bstar = int(np.argmax(hit)) if hit.any() else bins - 1
        big_p = min(bstar << shift, 65535) if variant == 'lower_edge' else min(((bstar + 1) << shift) - 1, 65535)
        corr = _clamp((f['target'] << 12) // max(big_m, 1))
        if big_p * corr > f['ceil'] << 12:
            corr = _clamp((f['ceil'] << 12) // max(big_p, 1))
            flags |= 4
        e2 = _damp(e, corr, f['ae_dead'], f['ae_speed'], f['e_min'], f['e_max'], variant)
    out = np.zeros(STATE_INTS, dtype=np.int64)
    out[:8] = e2, wr2, wb2, (int(state[3]) + 1) & 0x7FFFFFFF, big_m, big_p, min(kk, (1 << 31) - 1), flags
    out[8:12] = _plane_gains(e2, wr2, wb2, k)
    return out.astype(np.int32)


def gain_map_ref(base, state, shape=None, variant=None):
    """the (GH,GW,4) uint16 map of a state: ``base`` (GH,GW,4) uint16 scaled by g[0..3], or ``shape`` = (GH, GW) without a base"""
    g = np.asarray(state)[8:12].astype(np.int64)
    b = np.full(tuple(shape) + (4,), 4096, dtype=np.int64) if base is None else np.asarray(base).astype(np.int64)
    prod = b * g[None, None, :] + (0 if variant == 'map_floor' else 2048)
    assert prod.max() <= U32
    out = prod >> 12
    return (out & 0xFFFF if variant == 'map_no_clamp' else np.minimum(out, 65535)).astype(np.uint16)


def loop_ref(frames, black_level, spec, stats, cell_log2, cfa, base=None, exposure=4096, wb=(4096, 4096)):
    """The closed loop over ``frames`` - a sequence of (N,H,W) raw frames.  ``stats`` = (zone, bins, hist_shift, lo, hi).  Frame t
    is shaded with the map of the state behind frame t-1 (the initial gains for t = 0), its statistics - black level 0 behind the
    shading - update the state.  -> a list, per frame, of (the map frame t was shaded with, the state behind it, the map
    behind it)."""
    zone, bins, shift, lo, hi = stats
    n, h, w = np.asarray(frames[0]).shape
    shape = LS.map_shape(h, w, cell_log2)
    state = new_state(exposure, wb, cfa)
    gains = gain_map_ref(base, state, shape)
    out = []
    for x in frames:
        shaded = LS.shade_ref(x, black_level, gains, cell_log2)
        zones, hist = SR.stats_ref(shaded, 0, zone, bins, shift, lo, hi)
        state = solve_ref(zones, hist, state, spec, (h, w, zone[0], zone[1], shift, cfa))
        used, gains = gains, gain_map_ref(base, state, shape)
        out.append((used, state, gains))
    return out


# ---------------------------------------------------------------- the loop test's scene
SCENE_SHAPE, SCENE_BLACK, SCENE_WHITE, SCENE_CAST, SCENE_EXPOSURE, SCENE_FRAMES = (48, 64), 64, 1023, (0.45, 1.0, 0.6), 0.22, 12
SCENE_STATS = ((8, 16), 64, 4, 8, 950)          # zones of 8 x 16, 64 bins of 16 codes, lo 8, hi 950
SCENE_CELL_LOG2 = 4


def scene(n, cfa=0, seed=0, frames=SCENE_FRAMES):
    """``frames`` raw 10-bit frames (N,48,64) uint16 of one still scene: textured grey with two saturated patches under a colour
    cast of (0.45, 1, 0.6) at 0.22 x exposure, black level 64, fresh noise of sigma 2 in every frame and image"""
    h, w = SCENE_SHAPE
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    grey = 0.36 + 0.12 * np.sin(xx / 7.0) * np.cos(yy / 5.0) + 0.15 * rng.random((h // 4, w // 4)).repeat(4, 0).repeat(4, 1)
    colour = (2 * (yy & 1) + (xx & 1)) ^ cfa                                    # 0 r, 1 gr, 2 gb, 3 b
    cast = np.array([SCENE_CAST[0], SCENE_CAST[1], SCENE_CAST[1], SCENE_CAST[2]])[colour]
    clean = SCENE_BLACK + (SCENE_WHITE - SCENE_BLACK) * SCENE_EXPOSURE * grey * cast
    clean[8:12, 20:24] = SCENE_WHITE                # 24 pixels, 0.8 %: below the 1 % the percentile leaves out
    clean[34:36, 40:44] = SCENE_WHITE
    out = []
    for _ in range(frames):
        noisy = clean[None] + rng.normal(0.0, 2.0, (n, h, w))
        noisy[:, clean == SCENE_WHITE] = SCENE_WHITE
        out.append(np.clip(np.rint(noisy), 0, SCENE_WHITE).astype(np.uint16))
    return out


# ---------------------------------------------------------------- the inputs of the GPU test
def synthetic_stats(n, h, w, zone, bins, shift, seed, cast=(0.5, 1.0, 0.7), cfa=0, empty=0.1, level=(40, 800)):
    """zones and hist as risp_raw_stats could have written them for N frames of H x W, without the frames: per zone a grey level
    and a cast with some scatter, counts between 0 and the zone's area (a share ``empty`` of the zones has a plane with count 0),
    sum <= 65535 * count; histograms of random counts.  The sharp column holds junk: the controller does not read it."""
    rng = np.random.default_rng(seed)
    gh, gw = SR.grid(h, w, zone)
    zy, zx = np.mgrid[0:gh, 0:gw]
    area = (np.minimum(zone[0], h - zy * zone[0]) // 2) * (np.minimum(zone[1], w - zx * zone[1]) // 2)
    area = np.broadcast_to(area[None, :, :, None], (n, gh, gw, 4))
    count = np.where(rng.random((n, gh, gw, 4)) < 0.85, area, rng.integers(0, area + 1))
    count = np.where(rng.random((n, gh, gw, 4)) < empty / 4, 0, count)
    grey = rng.integers(level[0], level[1] + 1, (n, gh, gw, 1)).astype(np.float64)
    gains = np.array([cast[0], cast[1], cast[1], cast[2]])[np.arange(4) ^ cfa]
    mean = np.clip(grey * gains * rng.uniform(0.8, 1.25, (n, gh, gw, 4)), 0, 65535)
    total = np.minimum(np.rint(mean * count).astype(np.int64) + rng.integers(0, 2, count.shape), 65535 * count)
    zones = np.stack([total, count, rng.integers(0, 1 << 40, count.shape)], axis=-1).astype(np.int64)
    peak = max(1, min(h * w // 4, (1 << 31) - 1) // bins)
    hist = rng.integers(0, peak + 1, (n, 4, bins)).astype(np.int32)
    hist[:, :, bins // 2:] //= 8                                               # (a falling tail: the percentile is not the last bin)
    return zones, hist


# (name, (N, H, W), zone, bins, hist_shift, cfa, the fields that differ from DEFAULTS, what synthetic_stats is told)
SOLVE_CASES = [
    ('one-zone', (1, 2, 4), (2, 4), 16, 6, 0, dict(y_hi=60000, ceil=60000, target=9000), dict(level=(400, 8000))),
    ('247-zones', (1, 38, 52), (2, 4), 1024, 0, 0, {}, {}),
    ('partial-rggb', (3, 34, 156), (6, 8), 16, 6, 0, dict(fill=230), dict(level=(40, 700))),
    ('partial-grbg', (3, 34, 156), (6, 8), 16, 6, 1, dict(fill=230), dict(level=(40, 700))),
    ('partial-gbrg', (3, 34, 156), (6, 8), 16, 6, 2, dict(fill=230), dict(level=(40, 700))),
    ('partial-bggr', (3, 34, 156), (6, 8), 16, 6, 3, dict(fill=230), dict(level=(40, 700))),
    ('327680-zones', (5, 512, 1024), (2, 4), 1, 0, 0, dict(min_share=8), {}),
    ('bins-1-shift-6', (2, 12, 24), (4, 8), 1, 6, 3, {}, {}),
    ('bins-1024-shift-6', (2, 12, 24), (4, 8), 1024, 6, 2, dict(y_hi=60000, target=20000, ceil=64000, pct=65536), dict(level=(400, 40000))),
    ('share-per-image', (2, 12, 24), (4, 8), 16, 6, 0, dict(min_share=40), dict(level=(40, 700), empty=0)),
]
# with these, (3,34,156) has 6 x 20 zones with partial last zones on both axes: 34 = 5 * 6 + 4, 156 = 19 * 8 + 4


def solve_case(index):
    """-> (zones, hist, state, spec, geometry) of SOLVE_CASES[index]"""
    name, (n, h, w), zone, bins, shift, cfa, fields, told = SOLVE_CASES[index]
    zones, hist = synthetic_stats(n, h, w, zone, bins, shift, seed=100 + index, cfa=cfa, **told)
    if name == 'one-zone':                          # the zone by hand, so that it is a candidate: odd sums over a count of 2
        zones[0, 0, 0, :, 0], zones[0, 0, 0, :, 1] = (4001, 9000, 9101, 6003), 2
    if name == 'share-per-image':                   # image 1 has no candidate at all: pooled, 3 of 18 zones are still enough
        zones[1, :, :, :, 1] = 0
    state = new_state(5000, (7000, 3000), cfa)
    state[3] = 0x7FFFFFFF                           # the counter wraps to 0
    return zones, hist, state, spec_tuple(**fields), (h, w, zone[0], zone[1], shift, cfa)


def special_case(name):
    """-> (zones, hist, state, spec, geometry) of a case built by hand: see SPECIAL_CASES"""
    n, h, w, zone, bins, shift, cfa = 2, 12, 24, (4, 8), 16, 6, 1
    fields = {}
    state = new_state(4096, (4096, 4096), cfa)
    zones, hist = synthetic_stats(n, h, w, zone, bins, shift, seed=7, cfa=cfa, level=(40, 700))
    if name == 'no-candidate':                      # every zone too dark for y_lo: white balance holds, bit 0 clear
        fields = dict(y_lo=60000, y_hi=65535)
    elif name == 'all-empty':                       # count 0 everywhere and an empty histogram: everything holds
        zones[..., :2] = 0
        hist[:] = 0
    elif name == 'hist-empty':                      # T == 0 with a white balance that solves
        hist[:] = 0
    elif name == 'green-empty':                     # T == 0 although the red and blue planes have counts
        hist[:, [1 ^ cfa, 2 ^ cfa], :] = 0
    elif name == 'ceiling':                         # a dark mean and a bright tail: highlight protection takes over
        hist[:] = 0
        hist[:, :, 0], hist[:, :, 15] = 1000, 40
        fields = dict(target=600, ceil=700, pct=64880)
    elif name == 'speeds-0':                        # both halves off: the gains move only into their bounds
        fields = dict(wb_speed=0, ae_speed=0)
        state = new_state(900, (300, 65535), cfa)
        fields.update(e_min=1000, wb_min=400, wb_max=60000)
    elif name == 'deadband':                        # corrections inside the deadbands: nothing moves
        for q, mean in enumerate((303, 300, 300, 297)):                        # cr = 4055, cb = 4137: 41 off, the deadband's edge
            zones[..., q ^ cfa, 0] = mean * zones[..., q ^ cfa, 1]
        fields = dict(wb_dead=41, ae_dead=4095)
    elif name == 'shift-down':                      # corrections below 1: the damping shift acts on negative numbers
        zones, hist = synthetic_stats(n, h, w, zone, bins, shift, seed=7, cast=(1.37, 1.0, 1.21), cfa=cfa, level=(300, 700))
        fields = dict(wb_speed=77, ae_speed=33, target=35, wb_dead=0, ae_dead=0)
    elif name == 'T-above-2^32':                    # 16 images of 32768 x 32768, one zone each: T = 2^33, sums at the bounds
        n, h, w, zone, bins, shift = 16, 32768, 32768, (32768, 32768), 16, 12
        area = (h // 2) * (w // 2)                  # 2^28 samples a plane; N * H * W / 2 = 2^33
        zones = np.zeros((n, 1, 1, 4, 3), dtype=np.int64)
        zones[..., 1] = area
        zones[..., 0] = np.array([20000, 40000, 40001, 30000])[np.arange(4) ^ cfa] * area
        zones[..., 2] = (1 << 62) + 12345
        hist = np.zeros((n, 4, bins), dtype=np.int32)
        hist[:, :, 3], hist[:, :, 9], hist[:, :, 15] = area // 2, area // 4, area // 4
        fields = dict(y_hi=65535, target=30000, ceil=65535, fill=256)
    elif name == 'sums-at-the-bounds':              # 2^24 - 1 is not reachable in a test: the largest sums one zone can hold
        n, h, w, zone, bins, shift = 1, 1 << 20, 1 << 20, (1 << 20, 1 << 20), 16, 12
        area = (h // 2) * (w // 2)                  # 2^38 samples a plane, N * H * W / 2 = 2^39 < 2^40
        zones = np.zeros((1, 1, 1, 4, 3), dtype=np.int64)
        zones[..., 1] = area
        zones[..., 0] = 65535 * area                # 2^54 - 2^38
        zones[..., 2] = -1                          # (all 64 bits set in the column nobody reads)
        hist = np.full((1, 4, bins), (1 << 31) - 1, dtype=np.int32)
        fields = dict(y_hi=65535, target=65535, ceil=65535, fill=256, rg_hi=4095, bg_hi=4095)
    else:
        raise KeyError(name)
    return zones, hist, state, spec_tuple(**fields), (h, w, zone[0], zone[1], shift, cfa)


SPECIAL_CASES = ['no-candidate', 'all-empty', 'hist-empty', 'green-empty', 'ceiling', 'speeds-0', 'deadband', 'shift-down',
                 'T-above-2^32', 'sums-at-the-bounds']

# (GH, GW, with a base map, the state words 8 .. 11)
MAP_CASES = [
    (2, 2, False, (4096, 4097, 1, 65535)),
    (2, 2, True, (4096, 9000, 2500, 4095)),
    (3, 5, True, (7436, 8827, 8827, 6580)),
    (49, 64, False, (0, 16384, 30000, 65535)),
    (49, 64, True, (65535, 40000, 4099, 12345)),        # gains that clamp at 65535
]


def map_case(index):
    """-> (base or None, state, (GH, GW)) of MAP_CASES[index]: a base of random gains over the whole uint16 range, its extremes in"""
    gh, gw, with_base, g = MAP_CASES[index]
    state = new_state()
    state = state.astype(np.int64)
    state[8:12] = g
    base = None
    if with_base:
        base = np.random.default_rng(200 + index).integers(0, 65536, (gh, gw, 4), dtype=np.uint16)
        base[0, 0], base[-1, -1] = (65535, 0, 4096, 1), (1, 65535, 4095, 4097)
    return base, state.astype(np.int32), (gh, gw)
