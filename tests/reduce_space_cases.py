"""The argument space of the per-image reduction kernels: a mirror of their host-side grid arithmetic, the table of
cases (each the smallest shape at which a named branch of a kernel is taken), the inputs and the rounding bounds.
Plain CPU code: tests/test_reduce_reference_cpu.py asserts that every case reaches the branch it names, that the
gate margins hold and that the integer inputs stay exact; tests/test_gpu_reduce_space.py launches the cases.

The bound of a rounded sum: a sum taken in a fixed order errs by at most depth x 2^-24 x sum |term| to first order,
depth the longest chain of roundings a term passes through (its own products, the per-thread trips, 6 shuffle steps,
the additions across the four waves, the finishing trips and shuffles).  The bound of a case is that expression times
MARGIN = 2 for the second-order terms.
"""
import numpy as np

import reduce_reference as R

F32, F64 = np.float32, np.float64
U, MARGIN = 2.0 ** -24, 2.0
MAX_MIX, FC_MAXW, FC_MAXL = 16, 1024, 8


def rng(*key):
    return np.random.Generator(np.random.PCG64([int(k) & 0xffffffff for k in key]))


def ceil_div(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ the grid mirror
def stat_blocks(hw):
    return min(max(hw // (4 * 256 * 8), 1), 64)


def stats_walk(hw, off):
    """risp_channel_stats: form, workgroups per plane, trips of the busiest thread, whether the 4-vector trip runs,
    rounding depth of the sum (two additions inside a vector, the trips, 6 shuffles, 3 waves, 6 shuffles of the final wave)"""
    vec = hw % 4 == 0 and off % 4 == 0
    nb, n = stat_blocks(hw), (hw // 4 if vec else hw)
    step = nb * 256
    trips = ceil_div(n, step)
    return dict(vec=vec, nb=nb, n=n, step=step, trips=trips, unrolled=vec and n > 3 * step, capped=hw // 8192 >= 64,
                depth=trips + (2 if vec else 0) + 6 + 3 + 6)


def stats_bwd_walk(hw, off):
    vec = hw % 4 == 0 and off % 4 == 0
    n = hw // 4 if vec else hw
    bx = min(ceil_div(n, 256), 64)
    return dict(vec=vec, bx=bx, trips=ceil_div(n, bx * 256))


def histc_walk(hw, bins, off):
    bx, copies = min(ceil_div(hw, 4096), 64), 16
    while copies > 1 and bins * copies > 4096:
        copies >>= 1
    vec = hw % 4 == 0 and off % 4 == 0
    return dict(bx=bx, copies=copies, vec=vec, capped=ceil_div(hw, 4096) > 64, trips=ceil_div(hw // 4 if vec else hw, bx * 256))


def mix_walk(numel, K):
    n4 = numel // 4
    fg, bg = min(ceil_div(n4, 256), 2048), min(max(ceil_div(n4, 1024), 1), 1024)
    trips, ftrips = ceil_div(n4, bg * 256), ceil_div(bg, 64)
    # gw: the product, two additions inside a vector, the trips, 6 shuffles, 4 waves, the finishing trips, 6 shuffles
    return dict(fwd_grid=fg, fwd_capped=ceil_div(n4, 256) > 2048, fwd_trips=ceil_div(n4, fg * 256), bwd_grid=bg,
                bwd_capped=ceil_div(n4, 1024) > 1024, bwd_trips=trips, finish_trips=ftrips,
                gw_depth=1 + 2 + trips + 6 + 4 + ftrips + 6, y_depth=1 + K)


def plane_walk(hw, off):
    vec = hw % 4 == 0 and off % 4 == 0
    trips = ceil_div(hw // 4 if vec else hw, 256)
    return dict(vec=vec, trips=trips, depth=(2 if vec else 0) + trips + 6 + 4)


def sse_walk(numel):
    grid = min(max(ceil_div(numel, 4096), 1), 1024)
    return dict(grid=grid, capped=ceil_div(numel, 4096) > 1024, trips=ceil_div(numel, grid * 256), finish_trips=ceil_div(grid, 64))


def loss_walk(numel):
    n4 = numel // 4
    blocks = min(ceil_div(n4, 256), 256)
    trips, ftrips = ceil_div(n4, blocks * 256), ceil_div(blocks, 64)
    # a term: the difference (twice in a square) and the product; two additions inside a vector, the trips, 6 shuffles,
    # two additions across the waves, the finishing trips, 6 shuffles, the rounded 1 / numel and the product with it
    return dict(blocks=blocks, capped=ceil_div(n4, 256) > 256, trips=trips, finish_trips=ftrips,
                depth=3 + 2 + trips + 6 + 2 + ftrips + 6 + 2)


def lg_walk(N, C, H, W):
    hw = H * W
    bx = min(max(ceil_div(hw // 4, 2048), 1), 64)
    ltrips, gtrips, ftrips = ceil_div(hw // 4, bx * 256), ceil_div(hw // 16, bx * 256), ceil_div(N * C * bx, 64)
    ps = plane_walk(hw, 0)
    return dict(bx=bx, capped=ceil_div(hw // 4, 2048) > 64, local_trips=ltrips, global_trips=gtrips, finish_trips=ftrips,
                plane_depth=ps['depth'], sum_depth=max(2 + ltrips, gtrips) + 6 + 2 + ftrips + 6 + 3)


def sum_bound(depth, mags):
    return MARGIN * depth * U * mags


# ------------------------------------------------------------------------------------------------ statistics
STATS_HW = [1, 2, 3, 4, 5, 4092, 4096, 16380, 16384, 129 * 129, 524288, 524292]
STATS_NC = [(1, 1), (2, 3), (1, 5)]
# what each size is there for (asserted against stats_walk by the CPU test): form aligned / moved by one float
STATS_BRANCH = {1: 'element form, one value', 2: 'element form', 3: 'element form (3 x 1)', 4: 'one vector', 5: 'element form past a vector',
                4092: 'unrolled trip for the first 255 threads, the single-vector loop for the last', 4096: 'unrolled trip alone',
                16380: 'one workgroup at its largest', 16384: 'two workgroups', 129 * 129: 'element form, two workgroups',
                524288: 'the cap of 64 workgroups', 524292: 'past the cap: a second trip of the capped grid'}


def stats_cases():
    return [(hw, n, c) for hw in STATS_HW for n, c in STATS_NC]


def stats_input(hw, n, c, integer):
    g = rng(11, hw, n, c, integer)
    if integer:
        return g.integers(0, 4, size=(n * c, hw)).astype(F32)            # sums below 3 x 524292 < 2^24: every partial exact
    return g.uniform(-40.0, 300.0, size=(n * c, hw)).astype(F32)


def tie_positions(hw, off):
    """pairs of positions either side of each boundary of the walk of an (hw, off) plane"""
    w = stats_walk(hw, off)
    e = 4 if w['vec'] else 1                                   # elements per load
    pairs = {'first and last element': (0, hw - 1), 'either side of a thread\'s load': (e - 1, e),
             'either side of a wave (lane 63 / 64)': (64 * e - 1, 64 * e), 'either side of a workgroup\'s walk': (256 * e - 1, 256 * e),
             'either side of a trip': (w['step'] * e - 1, w['step'] * e)}
    if w['unrolled']:
        pairs['either side of an unrolled trip'] = (4 * w['step'] * e - 1, 4 * w['step'] * e)
    return {k: v for k, v in pairs.items() if v[1] < hw}


TIE_HW = [16384, 129 * 129, 4 * 4 * 512 * 2 + 8]                # two workgroups in either form; the unrolled trip taken twice
TIE_KINDS = list(tie_positions(TIE_HW[2], 0)) + ['constant plane', 'one distinct value at the last index']


def tie_cases():
    """(HW, kind) for every boundary that a form of that size has"""
    return [(hw, k) for hw in TIE_HW for k in TIE_KINDS if any(tie_input(hw, k, off) is not None for off in (0, 1))]


def tie_input(hw, kind, off):
    """plane 0: the minimum at two places, plane 1: the maximum at two places (the other extreme single, at a third place)"""
    x = rng(12, hw).uniform(1.0, 2.0, size=(2, hw)).astype(F32)
    if kind == 'constant plane':
        x[:] = F32(0.75)
        return x, np.zeros((2, 2), np.int64)
    if kind == 'one distinct value at the last index':
        x[:] = F32(0.75)
        x[0, -1], x[1, -1] = F32(0.5), F32(3.0)
        return x, np.array([[hw - 1, 0], [0, hw - 1]])
    if kind not in tie_positions(hw, off):
        return None                                            # this form of this size has no such boundary
    p, q = tie_positions(hw, off)[kind]
    third = hw // 2 + 7
    assert third not in (p, q)
    x[0, [p, q]], x[0, third] = F32(0.25), F32(5.0)
    x[1, [p, q]], x[1, third] = F32(5.0), F32(0.25)
    return x, np.array([[p, third], [third, p]])


# statistics gradient: (HW, N, C, gstride or None for risp_stats_bwd, which of min / mean / max, branch)
STATS_BWD = [(1, 1, 1, None, 'min mean max', 'one element: argmin == argmax'), (5, 2, 3, 3, 'min mean max', 'element form'),
             (4096, 2, 3, 5, 'min mean max', 'gstride > C'), (4096, 1, 3, None, 'mean', 'mean alone, arg NULL (the gray-world backward)'),
             (129 * 129, 1, 2, 2, 'min max', 'element form, a second trip'), (64 * 256 * 4 + 4, 1, 2, 4, 'min mean max', 'more than 64 x 256 vectors: the grid-stride trip'),
             (64 * 256 + 1, 1, 1, None, 'min mean max', 'element form past 64 x 256 elements')]


def stats_bwd_input(row, constant):
    hw, n, c, gs, which, _ = row
    g = rng(13, hw, n, c)
    P, stride = n * c, (gs or 1)
    x = np.full((P, hw), F32(0.5)) if constant else g.uniform(0, 1, size=(P, hw)).astype(F32)
    ng = P if gs is None else n * stride
    grads = {k: (g.uniform(-2, 2, size=ng).astype(F32) if k in which else None) for k in ('min', 'mean', 'max')}
    return x, g.uniform(-1, 1, size=(P, hw)).astype(F32), grads


# ------------------------------------------------------------------------------------------------ gray-world
def gray_case(HW=4096):
    """sums of 8 images: ordinary, one black plane (mean exactly 0), one negative mean, all black, two ordinary, then a small positive
    mean either side of the gate (eps / 4: clamped, no gradient of its own; 4 eps: passed)"""
    s = np.array([[0.3, 0.5, 0.2], [0.0, 0.4, 0.6], [-0.1, 0.5, 0.3], [0.0, 0.0, 0.0], [0.01, 0.9, 0.02], [0.6, 0.6, 0.6],
                  [R.GRAY_EPS / 4, 0.5, 0.3], [0.4, 4 * R.GRAY_EPS, 0.2]]) * HW
    gk = rng(14).uniform(-1, 1, size=s.shape)
    return s.astype(F32), gk.astype(F32), HW


def gray_gate_margin(sums, HW):
    """distance of the float64 means from the gate m >= eps over what the fp32 mean can err by (the rounded 1 / HW and the product,
    2 u |m|, times MARGIN): above 1 the two arithmetics decide alike; infinite for a mean of exactly 0, which both hold exactly"""
    m = np.asarray(sums, F64) / HW
    with np.errstate(divide='ignore'):
        return np.abs(m - R.GRAY_EPS) / (MARGIN * 2 * U * np.abs(m))


def gray_bounds(sums, gk, HW):
    """m_c: the rounded 1 / HW and the product (2); gray: two additions and a division on top (5 of sum |m| / 3); a gain: gray's error over
    mc, the 2 of an unclamped mc and the division (3).  Backward: a term gk / mc 3, two additions, the division by 3 (6 of A = sum |gk / mc| / 3);
    own = gk gray / mc^2: gray's error, 7 roundings of its own; the difference 1."""
    m, gk = np.asarray(sums, F64) / HW, np.asarray(gk, F64)
    mc, sm = np.maximum(m, R.GRAY_EPS), np.abs(m).sum(1, keepdims=True) / 3
    gain = np.abs(R.grayworld_gains(sums, HW))
    fwd = MARGIN * U * (5 * sm / mc + 3 * gain)
    A = np.abs(gk / mc).sum(1, keepdims=True) / 3
    own = np.where(m >= R.GRAY_EPS, np.abs(gk) * np.abs(m.mean(1, keepdims=True)) / mc ** 2, 0)
    bwd = MARGIN * U * (6 * A + np.where(m >= R.GRAY_EPS, np.abs(gk) / mc ** 2 * 5 * sm, 0) + 8 * own + A)
    return fwd, bwd


# ------------------------------------------------------------------------------------------------ histogram
HIST_BINS = [1, 2, 3, 30, 256, 257, 512, 513, 1024, 4096]
HIST_HW = [1, 5, 4096, 4100, 262144 + 4]
HIST_COPIES = {1: 16, 2: 16, 3: 16, 30: 16, 256: 16, 257: 8, 512: 8, 513: 4, 1024: 4, 4096: 1}


def hist_input(bins, hw):
    """plane 0: every bin edge fp32(k / bins) with its two neighbours, the specials, then uniform values; plane 1: constant"""
    k = np.arange(bins + 1, dtype=F64)
    e = (k / bins).astype(F32)
    edges = np.stack([np.nextafter(e, F32(-1)), e, np.nextafter(e, F32(2))], 1).reshape(-1)
    special = np.array([0.0, 1.0, np.nextafter(F32(1), F32(2)), -0.0, -0.25, np.nan, np.inf, -np.inf, 0.5], F32)
    pool = np.concatenate([special, edges, rng(15, bins, hw).uniform(-0.1, 1.1, size=hw).astype(F32)])
    if hw < len(special):
        pool = np.roll(pool[: len(special)], -(bins % len(special)))
    x = np.empty((2, hw), F32)
    x[0] = np.roll(pool[:hw], 3 if hw > 4 else 0)              # the edges do not start on a vector boundary
    x[1] = F32(1.0) if bins % 2 else F32(0.3)
    return x


# ------------------------------------------------------------------------------------------------ mixture
MIX_K = [1, 2, 5, 15, 16]
MIX_NUMEL = [4, 1020, 262144, 262148]
MIX_LARGE = [2 * 1024 * 1024 + 8, 4 * 1024 * 1024 + 1040]
MIX_GO = ['all', 'none', 'alternate']


def mix_cases():
    return [(k, n) for k in MIX_K for n in MIX_NUMEL] + [(2, n) for n in MIX_LARGE]


def mix_input(K, numel, integer):
    g = rng(16, K, numel, integer)
    if integer:                                                # |partial sums| <= numel < 2^24 ... see integer_range_ok
        outs = [g.integers(-1, 2, size=numel).astype(F32) for _ in range(K)]
        return outs, g.integers(-2, 3, size=K).astype(F32), g.integers(-1, 2, size=numel).astype(F32)
    w = g.uniform(-1, 1, size=K).astype(F32)
    if K > 1:
        w[K // 2] = F32(0)                                     # a zero weight
    return [g.uniform(-1, 1, size=numel).astype(F32) for _ in range(K)], w, g.uniform(-1, 1, size=numel).astype(F32)


# ------------------------------------------------------------------------------------------------ plane sums
PLANE_HW = [1, 3, 4, 1023, 1024, 1028, 16384]
PLANE_SEL = [(0, 7), (2, 3), (6, 1)]
PLANE_N = [1, 3]
PLANE_C = 7


def plane_input(hw, n, integer):
    g = rng(17, hw, n, integer)
    if integer:
        return g.integers(0, 4, size=(n, PLANE_C, hw)).astype(F32)
    return g.uniform(-1.0, 2.0, size=(n, PLANE_C, hw)).astype(F32)


# ------------------------------------------------------------------------------------------------ squared error
SSE_NUMEL = [1, 255, 4096, 4097, 262144 + 1, 4 * 1024 * 1024 + 4099]


def sse_input(numel, integer):
    g = rng(18, numel, integer)
    if integer:                                                # codes 0 / 255: every term exactly 0 or 1
        return g.integers(0, 2, size=numel).astype(F32), g.integers(0, 2, size=numel).astype(F32)
    k = (np.arange(256, dtype=F64) / 255).astype(F32)
    near = np.stack([np.nextafter(k, F32(-1)), k, np.nextafter(k, F32(2))], 1).reshape(-1)
    pool = np.concatenate([near, np.array([-0.5, -1e-8, 1.5, 1.0 + 2.0 ** -20], F32)])
    a = np.concatenate([pool, g.uniform(-0.2, 1.2, size=numel).astype(F32)])[:numel]
    b = np.concatenate([pool[::-1], g.uniform(-0.2, 1.2, size=numel).astype(F32)])[:numel]
    return np.roll(a, numel // 3), b


def sse_bound(a, b):
    """d = fl(ca / 255) - fl(cb / 255): u (ca + cb) / 255 + u |d|; the square: twice that times |d| and its own rounding; the sum is
    taken in double"""
    ca, cb = R.u8_code(a).astype(F64), R.u8_code(b).astype(F64)
    d = np.abs(ca - cb) / 255
    return MARGIN * U * float((2 * d * ((ca + cb) / 255 + d) + d * d).sum())


# ------------------------------------------------------------------------------------------------ conditional head
FC_WIDTHS = [((3, 1), 0), ((12, 8, 1), 0), ((768, 300, 3), 0), ((96, 257, 256, 30), 0), ((30, 1024, 7), 0),
             ((6, 5, 4, 6, 3, 5, 4, 3, 2), 0), ((3, 1), 600)]                   # (widths, parameters beyond the global scalar)
FC_N = [1, 3]
FC_BRANCH = ['a single layer', 'two layers', 'a 256-bin histogram: j += 256 trips on the input and the hidden layer', 'widths either side of 256',
             'the widest layer', 'the deepest net (8 layers)', 'an unused tail longer than two workgroups']


def fc_input(widths, extra, N):
    """counts of a histogram, weights of scale 1 / (fan-in x mean count), and biases moved until every hidden pre-activation is away
    from the ReLU gate by fc_gate_margin"""
    g = rng(19, len(widths), widths[0], widths[-1], N, extra)
    hist = g.integers(0, 40, size=(N, widths[0])).astype(F32)
    offs, gofs = R.fc_layout(widths)
    flat = g.uniform(-1, 1, size=gofs + 1 + extra).astype(F32)
    a = hist.astype(F64)
    for l, (wo, bo) in enumerate(offs):
        fi, fo = widths[l], widths[l + 1]
        scale = 2.0 / (np.sqrt(fi) * max(np.abs(a).mean(), 1e-3))
        flat[wo: bo] = (flat[wo: bo].astype(F64) * scale).astype(F32)
        W = flat[wo: bo].astype(F64).reshape(fi, fo)
        z0 = a @ W
        if l < len(offs) - 1:
            need = fc_gate_bound(a, W, flat[bo: bo + fo]).max(0) * 4 + 1e-3
            for j in range(fo):                                # the smallest move of the bias that clears the gate for every image
                bias = float(flat[bo + j])
                while np.any(np.abs(z0[:, j] + F64(F32(bias))) <= need[j]):
                    bias += 2.5 * need[j]
                flat[bo + j] = F32(bias)
            a = np.maximum(z0 + flat[bo: bo + fo].astype(F64), 0)
    return hist, flat, g.uniform(-1, 1, size=(N, widths[-1])).astype(F32)


def fc_gate_bound(a, W, bias):
    """the fp32 pre-activation against float64: fi products and additions and the bias, (fi + 2) u sum |terms|, times MARGIN; twice over
    for the error the inputs bring from the layer before"""
    fi = W.shape[0]
    return 2 * MARGIN * (fi + 2) * U * (np.abs(a) @ np.abs(W) + np.abs(np.asarray(bias, F64)))


def fc_gate_margin(hist, flat, widths):
    """min over hidden units of |z| / bound: > 1 means no fp32 evaluation within the bound flips a ReLU"""
    offs, _ = R.fc_layout(widths)
    a, worst = np.asarray(hist, F64), np.inf
    for l, (wo, bo) in enumerate(offs[:-1]):
        fi, fo = widths[l], widths[l + 1]
        W, b = flat[wo: bo].astype(F64).reshape(fi, fo), flat[bo: bo + fo]
        z = a @ W + b.astype(F64)
        worst = min(worst, float((np.abs(z) / fc_gate_bound(a, W, b)).min()))
        a = np.maximum(z, 0)
    return worst


# ------------------------------------------------------------------------------------------------ pixel loss
LOSS_NUMEL = [4, 1020, 1024, 262144, 262148]


def loss_input(numel, integer):
    g = rng(20, numel, integer)
    if integer:
        gt = g.integers(0, 3, size=numel).astype(F32)
        return gt + g.integers(-1, 2, size=numel).astype(F32), gt
    y, gt = g.uniform(0, 1, size=numel).astype(F32), g.uniform(0, 1, size=numel).astype(F32)
    y[::3] = gt[::3]                                           # exact zeros of y - gt
    return y, gt


# ------------------------------------------------------------------------------------------------ local / global loss
LG_SHAPES = [(1, 1, 4, 4), (2, 3, 8, 12), (3, 2, 128, 128), (2, 3, 128, 132), (1, 3, 724, 724)]
LG_FLAGS = ['local', 'global', 'mixed', 'values']
LG_GAIN_BOUND = 16                                             # relative error of the fp32 gain in units of u, beside the plane sums' depth


LG_ROTATE = [1, 2, 0, 3, 3]                                     # where each shape starts in the list of flag values


def lg_flags(kind, N, rotate=0):
    if kind == 'local':
        return np.zeros(N, F32)
    if kind == 'global':
        return np.ones(N, F32)
    if kind == 'mixed':
        return (np.arange(N) % 2 == (0 if N > 1 else 1)).astype(F32)      # a single image: local
    return np.array([0.0, 0.5, 1.0, 2.0], F32)[(np.arange(N) + rotate) % 4]     # flag < 1 is the kernel's test: 0, 0.5 local; 1, 2 global


def lg_value_flags():
    """the 'values' flags of every shape: N consecutive values from LG_ROTATE on, so that each of 0, 0.5, 1, 2 is launched"""
    return [lg_flags('values', s[0], r) for s, r in zip(LG_SHAPES, LG_ROTATE)]


def lg_input(shape, integer=None):
    """planes by turn: gain inside the clamp (b about 1.3 a), below 0.5 (b about 0.2 a), above 2 (b about 3 a), a with a negative mean
    (the mean clamp: gain pinned at 2).  integer = 'half' (b = 0: gain pinned at 0.5, a in {0, 2}), 'two' (b = 4 a, a in {0, 1}:
    gain pinned at 2), 'centres' (integer cell centres for the global branch), 'equal' (a = b in {0, 1}: a gain of mean / (mean + 1e-6),
    just below 1 and inside the clamp, every difference a cancellation)"""
    N, C, H, W = shape
    g = rng(21, N, C, H, W)
    if integer == 'half':
        return (2 * g.integers(0, 2, size=shape)).astype(F32), np.zeros(shape, F32)
    if integer == 'equal':
        a = g.integers(0, 2, size=shape).astype(F32)
        a[..., 0, 0] = 1                                       # no black plane
        return a, a.copy()
    if integer == 'two':
        a = g.integers(0, 2, size=shape).astype(F32)
        a[..., 0, 0] = 1                                       # no black plane
        return a, 4 * a
    if integer == 'centres':
        up = lambda v: np.repeat(np.repeat(v, 4, axis=2), 4, axis=3).astype(F32)
        return up(g.integers(0, 4, size=(N, C, H // 4, W // 4))), up(g.integers(0, 2, size=(N, C, H // 4, W // 4)))
    a = g.uniform(0.1, 1.0, size=shape).astype(F32)
    ratio = np.array([1.3, 0.2, 3.0, 1.0])[np.arange(N * C) % 4].reshape(N, C, 1, 1)
    b = (a * ratio + g.uniform(-0.05, 0.05, size=shape)).astype(F32)
    neg = (np.arange(N * C) % 4 == 3).reshape(N, C)
    a[neg] = -a[neg]
    b[neg] = np.abs(b[neg]) + F32(0.1)
    return a, b


def lg_gate_margin(a, b):
    """relative distance of the unclamped float64 gain from 0.5 and 2, and of mean a from 0 (relative to mean |a|)"""
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    ma, mb = a.mean((2, 3)), b.mean((2, 3))
    raw = mb / (np.maximum(ma, 0) + 1e-6)
    return float(min(np.abs(raw / 0.5 - 1).min(), np.abs(raw / 2 - 1).min())), float((np.abs(ma) / np.abs(a).mean((2, 3))).min())


def lg_bounds(a, b, flag):
    """(loss bound, per-element gradient bound).  Local: the gain carries (2 plane_depth + LG_GAIN_BOUND) u relative (two plane sums of one
    sign each, two products with 1 / HW, the clamp to 0, the sum with 1e-6, the quotient); d = a gain - b errs by |a gain| (that + u) + u |d|.
    Global: a centre mean is three additions deep (the 0.25 is exact): dd errs by 2 u (|da| + |db|) + u |dd|.  The scale of the gradient:
    a quotient and a product, 3 u with the final product."""
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    N, C, H, W = a.shape
    w = lg_walk(N, C, H, W)
    loc = np.asarray(flag, F32) < 1
    nl, ng = int(loc.sum()), int(N - loc.sum())
    gb, lb = np.zeros_like(a), 0.0
    if nl:
        gain = R.lg_gain(a, b)[loc][:, :, None, None]
        pinned = (gain == 0.5) | (gain == 2.0)
        eg = np.where(pinned, 0.0, (2 * w['plane_depth'] + LG_GAIN_BOUND) * U)
        ag, d = np.abs(a[loc] * gain), np.abs(a[loc] * gain - b[loc])
        ed = ag * (eg + U) + U * d
        cnt = nl * C * H * W
        gs = 2 * gain / cnt
        gb[loc] = MARGIN * (gs * ed + (3 * U + eg) * gs * d)
        lb += MARGIN * ((2 * d * ed).sum() + w['sum_depth'] * U * (d * d).sum()) / cnt
    if ng:
        da, db = R.lg_centres(a[~loc]), R.lg_centres(b[~loc])
        mags = R.lg_centres(np.abs(a[~loc])) + R.lg_centres(np.abs(b[~loc]))
        d = np.abs(da - db)
        ed = 2 * U * mags + U * d
        cnt = ng * C * (H // 4) * (W // 4)
        gs = 2 * 0.25 / cnt
        v = MARGIN * (gs * ed + 3 * U * gs * d)
        gg = np.zeros((ng, C, H, W))
        for i in (1, 2):
            for j in (1, 2):
                gg[..., i::4, j::4] = v
        gb[~loc] = gg
        lb += MARGIN * ((2 * d * ed).sum() + w['sum_depth'] * U * (d * d).sum()) / cnt
    return lb, gb


# ------------------------------------------------------------------------------------------------ refusals
# (entry, the argument replaced in a valid small call, a word of the message)
REFUSED = [('channel_stats', dict(NC=65536), 'risp_channel_stats'), ('histc', dict(bins=0), 'risp_histc'), ('histc', dict(bins=4097), 'risp_histc'),
           ('histc', dict(NC=65536), 'risp_histc'), ('mix_fwd', dict(K=0), 'K=0'), ('mix_fwd', dict(K=17), 'K=17'), ('mix_fwd', dict(numel=6), 'numel=6'),
           ('mix_fwd', dict(off_o=1), '16-byte'), ('mix_fwd', dict(off_y=1), '16-byte'), ('mix_bwd', dict(K=0), 'K=0'), ('mix_bwd', dict(K=17), 'K=17'),
           ('mix_bwd', dict(numel=6), 'numel=6'), ('mix_bwd', dict(off_o=1), '16-byte'), ('mix_bwd', dict(off_gy=1), '16-byte'), ('mix_bwd', dict(off_go=1), '16-byte'),
           ('pixel_loss', dict(numel=6), 'numel'), ('pixel_loss', dict(off_y=1), '16-byte'), ('pixel_loss', dict(off_g=1), '16-byte'),
           ('local_global', dict(off_a=1), '16-byte'), ('local_global', dict(off_g=1), '16-byte'), ('local_global', dict(H=6), 'multiple of 4'),
           ('local_global', dict(W=10), 'multiple of 4'), ('local_global', dict(N=256, C=256), 'risp_local_global_l2'),
           ('cond_fc', dict(widths=(3, 0, 1)), 'layer width 0'), ('cond_fc', dict(widths=(3, 1025, 1)), 'layer width 1025'),
           ('cond_fc', dict(widths=(2,) * 10), 'layers'), ('cond_fc_bwd', dict(total=4), 'parameters'), ('sse', dict(doubles=1024), 'doubles'),
           ('plane_sums', dict(c0=2, nc=2), 'risp_plane_sums'), ('stats_bwd_rows', dict(row_stride=2), 'row_stride'),
           ('stats_bwd', dict(arg=None), 'arg indices')]


def integer_range_ok():
    """every partial sum of the integer-valued inputs is an integer of magnitude below 2^24: the largest magnitude any sum can reach"""
    worst = {'stats': 3 * max(STATS_HW), 'plane sums': 3 * max(PLANE_HW), 'mix gw': max(MIX_NUMEL + MIX_LARGE),
             'mix y': 2 * MAX_MIX, 'pixel loss': max(LOSS_NUMEL), 'sse': max(SSE_NUMEL),
             'local pinned': max(4 * n * c * h * w for n, c, h, w in LG_SHAPES), 'global centres': max(9 * n * c * (h // 4) * (w // 4) for n, c, h, w in LG_SHAPES)}
    return {k: v < 2 ** 24 for k, v in worst.items()}, worst
