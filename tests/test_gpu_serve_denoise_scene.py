"""GPU: a classical denoiser beside gray-world / white-world on the serving path - risp_serve_denoise_stats (the statistic of
an image that lies behind a denoiser), risp_serve_denoise_scene_u8 (the denoise launch with the scene constants) and
``serve(fast_denoise_scene=True)``.

Every promise of the route is checkable exactly, so nothing here has a tuned tolerance:
  * where risp_serve_denoise_u8 accepts the stages the bytes are its bytes (torch.equal);
  * a MAX3 row is the maximum of the composed route's fp32 plane over its tile (equal), a MEAN3 row lies within the any-order
    summation bound of its tile's float64 sum;
  * given the constants, the bytes are those of the composed route evaluated with the same constants (torch.equal);
  * the gray-world gains lie within a bound of ``grayworld_gains`` on the composed plane that follows from the row bound.
The composed route is built by hand from the functions it calls (test_gpu_serve_denoise._composed_fp32 and its parts): the values
it holds, bit for bit, in the RGGB orientation the kernels' tile grid lives in.

Shapes (a workgroup owns a 64 x 32 pixel tile and stages it with a ring of 2 rows / 4 columns in LDS; a thread owns a 2 x 4
patch): at 1 x 4 x 4 every tap and ring pixel reflects on both sides and 254 threads of the workgroup own no pixel;
3 x 6 x 12 has an interior patch; 3 x 34 x 68 has ragged tiles, two across and two down; 2 x 66 x 132 is a 3 x 3 tile grid
with one interior tile."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

WHITE = 1023
KINDS = ['nearest', 'bilinear', 'laplacian']
DENOISERS = ['bilateral', 'median', 'fastnlm']
SHAPES = [(1, 4, 4), (3, 6, 12), (3, 34, 68), (2, 66, 132)]
SETTINGS = [(phase, black) for black in (0, 64) for phase in ('rggb', 'grbg', 'gbrg', 'bggr')]
U = 2.0 ** -24                      # unit roundoff of float32


def _shape_id(v):
    return '%dx%dx%d' % v if isinstance(v, tuple) else None


def _blocks(n, seed):
    """parameter blocks by op code (test_gpu_serve_classical._params) and white-world's per-image ratio under 'white'"""
    import test_gpu_serve_classical as CL
    pars = CL._params(n, seed, 0)
    pars['white'] = torch.tensor([[0.3, 0.9, 0.6][i % 3] for i in range(n)]).cuda()
    return pars


def _forms():
    """stage lists around the denoiser 'D' with gray-world ('gray') and white-world ('white') stages: a scene stage in front,
    one behind, one each side (both ways round), two behind - and, across them, both instantiations (with and without
    WbQuadratic), both tone curves, and every scene stage once with an earlier scene stage in its prefix"""
    import reconfigisp_amd.functional as F
    return [[F.OP_WB_MANUAL, 'gray', 'D', F.OP_GAMMA],
            [F.OP_WB_MANUAL, F.OP_TONE_FILMIC, 'D', F.OP_GAMMA, 'white', F.OP_TONE_CRYSIS],
            ['gray', F.OP_GAMMA, 'D', F.OP_WB_QUADRATIC, 'white'],
            ['white', 'D', 'gray'],
            ['D', 'gray', F.OP_GAMMA, 'white']]


def _chain(dev, kind, order, blocks, den, black, phase, reverse=False, out=None):
    """the entry points chained by hand: per scene stage its statistic - risp_serve_scene_stats in front of the denoiser,
    risp_serve_denoise_stats behind it - and risp_serve_scene_finish, then risp_serve_denoise_scene_u8.  Returns (bytes, the
    constants of the scene stages in pipeline order)"""
    import reconfigisp_amd.functional as F
    name, args = den
    n, h, w = dev.shape
    divisor = float(WHITE - black)
    pre, post, seen, consts = ([], []), ([], []), False, []
    for item in order:
        if item == 'D':
            seen = True
            continue
        ops, params = post if seen else pre
        if item in ('gray', 'white'):
            stat = F.SCENE_MEAN3 if item == 'gray' else F.SCENE_MAX3
            if seen:
                parts = F.serve_denoise_stats(dev, divisor, kind, pre[0], pre[1], name, args, ops, params, stat, None, black, phase)
            else:
                parts = F.serve_scene_stats(dev, divisor, kind, ops, params, stat, None, black, phase)
            got = F.serve_scene_finish(stat, parts, h * w, blocks['white'] if item == 'white' else None, None, None, tag=len(consts))
            consts.append(got.clone())                     # (the cached buffer belongs to the next call with this tag)
            ops.append(F.OP_GAIN3 if item == 'gray' else F.OP_GAIN3_Q8)
            params.append(consts[-1])
        else:
            ops.append(item)
            params.append(blocks[item])
    res = F.serve_denoise_scene_u8(dev, divisor, kind, pre[0], pre[1], name, args, post[0], post[1], reverse, out, black, phase)
    return res, consts


def _composed(dev, kind, order, blocks, den, consts, black, phase, upto=None):
    """the composed route by hand in fp32 (RGGB orientation) through ``order[:upto]``: gray-world applies the GIVEN constants
    as ``chain_forward`` with OP_GAIN3 (what fused_forward does with the gains it computed), white-world is
    ``origin_whiteworld``, which forms its constants from an order-free maximum itself"""
    import reconfigisp_amd.functional as F
    import test_gpu_serve_classical as CL
    import test_gpu_serve_denoise as D
    name, args = den
    x = CL._composed_fp32(dev, kind, [], [], black, phase)
    s = 0
    for item in order[:upto]:
        if item == 'D':
            x = F.origin_denoise(x, name, D._origin_params(name, args), (255., 255.))
        elif item == 'gray':
            x = F.chain_forward(x, [F.OP_GAIN3], [consts[s]])[-1]
            s += 1
        elif item == 'white':
            x = F.origin_whiteworld(x, blocks['white'], (255., 255.))
            s += 1
        else:
            x = D._stages(x, [item], [blocks[item]])
    return x


# ---------------------------------------------------------------- 1. the bytes of risp_serve_denoise_u8 where both accept the stages
def test_same_bytes_as_serve_denoise_u8_over_its_sweep_rows():
    """every row of tests/serve_denoise_cases.CASES - shape, depth, phase, demosaic, denoiser, stages, channel order - with the
    row's parameter blocks and its first input draw (the float64 reference, which alone makes a row's build slow and may ask
    for another draw, has no part in a comparison of two launches)"""
    import reconfigisp_amd.functional as F
    import serve_denoise_cases as DC
    assert len(DC.CASES) >= 100
    for index, row in enumerate(DC.CASES):
        shape, depth, phase, kind, name, pre, post, reverse = row
        n, h, w = DC.B._shape(shape)
        white, black = (int(v) for v in depth.split('/'))
        pre, post = list(DC.PRE[pre]), list(DC.POST[post])
        seed = 17000 + 13 * index
        params = [None if p is None else torch.from_numpy(p).cuda() for p in DC.make_params(pre + post, n, np.random.default_rng(seed + 1))]
        dev = torch.from_numpy(DC.make_input(n, h, w, white, black, seed).astype(np.uint16)).cuda()
        den = [torch.from_numpy(a).cuda() for a in DC.denoise_args(name, n)]
        args = {'bilateral': lambda: (3, den[0], den[1]), 'median': lambda: (3,), 'fastnlm': lambda: (3, 3, den[0])}[name]()
        call = (dev, float(white - black), kind, pre, params[:len(pre)], name, args, post, params[len(pre):], bool(reverse))
        kw = dict(black_level=black, cfa=phase)
        assert torch.equal(F.serve_denoise_scene_u8(*call, **kw), F.serve_denoise_u8(*call, **kw)), 'row %d: %s' % (index, row)


# ---------------------------------------------------------------- 2. partial rows against the composed plane
def _rows(dev, kind, pre, pre_p, den, post, post_p, stat, black, phase, fill):
    """risp_serve_denoise_stats through the wrapper into guard-banded partials"""
    import reconfigisp_amd.functional as F
    import test_gpu_serve_scene as GS
    n, h, w = dev.shape
    g = F.serve_scene_groups(h, w)
    big, part = GS._guarded(n * g * 4, torch.float32, fill)
    got = F.serve_denoise_stats(dev, float(WHITE - black), kind, pre, pre_p, den[0], den[1], post, post_p, stat, part.view(n, g, 4),
                                black, phase)
    torch.cuda.synchronize()
    assert GS._intact(big, n * g * 4, fill), 'risp_serve_denoise_stats wrote outside its partials'
    return got.cpu().numpy()


def _check_rows(got, plane, stat, what):
    """``got`` (N,G,4) against the composed route's fp32 plane (RGGB orientation: the kernels' tile grid).  Maxima EQUAL - they
    catch a wrong pixel, ring or reflection; the sums share that value path, so their bound only has to hold the reduction: a
    sum of at most 2048 float32 values in any order is within (count - 1) x 2^-24 x sum|x| of the exact sum (Higham,
    Accuracy and Stability of Numerical Algorithms, eq. 4.4)"""
    import serve_scene_reference as SC
    val = plane.cpu().numpy()
    assert val.dtype == np.float32
    assert (got[:, :, 3] == 0).all(), '%s: the last float of a row is not 0' % what
    if stat == 1:
        want = SC.tile_partials(val, 1, np.float32)
        assert np.array_equal(got, want), '%s: maxima differ in %d rows' % (what, (got != want).any(axis=2).sum())
    else:
        want = SC.tile_partials(val, 0, np.float64)
        mass = SC.tile_partials(np.abs(val), 0, np.float64)
        bound = (SC.TILE_H * SC.TILE_W - 1) * U * mass
        assert (np.abs(got - want) <= bound).all(), '%s: sums: worst %.3e of the bound' % (
            what, (np.abs(got - want) / np.maximum(bound, 1e-300)).max())


@pytest.mark.parametrize('n,h,w', SHAPES, ids=_shape_id)
def test_partial_rows_against_the_composed_plane(n, h, w):
    """each denoiser behind each demosaic with stages in front of and behind the denoiser, MAX3 and MEAN3, the four phases and
    both black levels in turn; the post stages alternate between the two instantiations (with / without WbQuadratic)"""
    import reconfigisp_amd.functional as F
    import test_gpu_serve_denoise as D
    dev = D._frames(n, h, w, seed=11 * h + n)
    blocks = _blocks(n, 17 * n + h)
    turn = 0
    for name in DENOISERS:
        den = (name, D._denoise_args(name, n))
        for kind in KINDS:
            phase, black = SETTINGS[turn % len(SETTINGS)]
            pre = [F.OP_WB_MANUAL, F.OP_TONE_FILMIC] if turn % 2 else [F.OP_WB_MANUAL]
            post = [F.OP_GAMMA, F.OP_WB_QUADRATIC] if turn % 3 else [F.OP_GAMMA]
            turn += 1
            order = pre + ['D'] + post
            plane = _composed(dev, kind, order, blocks, den, [], black, phase)
            pre_p, post_p = [blocks[op] for op in pre], [blocks[op] for op in post]
            for stat, fill in ((F.SCENE_MAX3, 123.0), (F.SCENE_MEAN3, -7.0)):
                got = _rows(dev, kind, pre, pre_p, den, post, post_p, stat, black, phase, fill)
                _check_rows(got, plane, stat, '%dx%dx%d %s %s %s black %d stat %d' % (n, h, w, kind, name, phase, black, stat))


@pytest.mark.parametrize('n,h,w', [(1, 4, 4), (3, 34, 68)], ids=_shape_id)
@pytest.mark.parametrize('name', DENOISERS)
def test_an_idle_thread_holds_minus_infinity_for_a_maximum(n, h, w, name):
    """the last post stage is WbManual with negative gains through the C ABI (the operator does not clamp) and no sample of the
    frame is small, so every value behind the denoiser is positive and every value the statistic sees negative: an idle thread
    of these ragged tiles that held 0 instead of -inf would turn its row's maximum into 0"""
    import reconfigisp_amd.functional as F
    import test_gpu_serve_denoise as D
    import test_gpu_serve_scene as GS
    from reconfigisp_amd import lib as L
    g = torch.Generator().manual_seed(5 + h)
    dev = torch.randint(300, WHITE, (n, h, w), generator=g, dtype=torch.int32).to(torch.uint16).cuda()
    gain = -(0.3 + 1.4 * torch.rand(n, 3, generator=g)).cuda()
    gam = torch.full((n, 1), 0.7).cuda()
    den = (name, D._denoise_args(name, n))
    vecs = [v for v in den[1] if torch.is_tensor(v)]
    blocks = {F.OP_GAMMA: gam, F.OP_WB_MANUAL: gain}
    rows = F.serve_scene_groups(h, w)
    for kind, phase in (('bilinear', 'grbg'), ('nearest', 'rggb')):
        plane = _composed(dev, kind, [F.OP_GAMMA, 'D', F.OP_WB_MANUAL], blocks, den, [], 0, phase)
        assert (plane < 0).all().item()
        big, part = GS._guarded(n * rows * 4, torch.float32, 123.0)
        L.call('risp_serve_denoise_stats', C.c_void_p(dev.data_ptr()), float(WHITE), F.DEMOSAIC[kind], 1, (C.c_int * 1)(F.OP_GAMMA),
               L.ptr_array([gam.data_ptr()]), F.DENOISE[name], 3, 3, C.c_void_p(vecs[0].data_ptr()) if vecs else None,
               C.c_void_p(vecs[1].data_ptr()) if len(vecs) > 1 else None, 1, (C.c_int * 1)(F.OP_WB_MANUAL), L.ptr_array([gain.data_ptr()]),
               F.SCENE_MAX3, C.c_void_p(part.data_ptr()), n, h, w, 0, F.CFA[phase], F._stream())
        torch.cuda.synchronize()
        assert GS._intact(big, n * rows * 4, 123.0)
        got = part.view(n, rows, 4).cpu().numpy()
        assert (got[:, :, :3] < 0).all(), 'a row maximum of %g: an idle thread held 0' % got[:, :, :3].max()
        _check_rows(got, plane, 1, '%s %s' % (kind, name))


# ---------------------------------------------------------------- 3. given the constants, the composed route's bytes
@pytest.mark.parametrize('name', DENOISERS)
@pytest.mark.parametrize('n,h,w', SHAPES, ids=_shape_id)
def test_given_the_constants_the_bytes_are_the_composed_routes(n, h, w, name):
    """statistic -> serve_scene_finish -> serve_denoise_scene_u8 by hand against the hand-composed route that applies the SAME
    constants, every form of _forms() behind every demosaic, the eight (phase, black level) settings in turn, both channel
    orders.  A white-world stage of the composed route forms its own constants: equal bytes say they are the chain's"""
    import reconfigisp_amd.functional as F
    import test_gpu_serve_denoise as D
    dev = D._frames(n, h, w, seed=3 * h + n)
    blocks = _blocks(n, 19 * n + h)
    den = (name, D._denoise_args(name, n))
    turn = 0
    for kind in KINDS:
        for order in _forms():
            phase, black = SETTINGS[turn % len(SETTINGS)]
            turn += 1
            got, consts = _chain(dev, kind, order, blocks, den, black, phase)
            last = _composed(dev, kind, order, blocks, den, consts, black, phase)
            what = '%dx%dx%d %s %s %s black %d %s' % (n, h, w, kind, name, phase, black, order)
            assert got.dtype == torch.uint8 and tuple(got.shape) == (n, h, w, 3)
            want = F.quantise_u8(last, False, None, F.CFA[phase])
            assert torch.equal(got, want), '%s: %d bytes differ' % (what, (got != want).sum().item())
            got_rgb, again = _chain(dev, kind, order, blocks, den, black, phase, reverse=True)
            assert all(torch.equal(a, b) for a, b in zip(consts, again)), '%s: the constants of two calls differ' % what
            assert torch.equal(got_rgb, F.quantise_u8(last, True, None, F.CFA[phase])), '%s reversed' % what


# ---------------------------------------------------------------- 4. the constants
@pytest.mark.parametrize('name', DENOISERS)
@pytest.mark.parametrize('n,h,w', SHAPES, ids=_shape_id)
def test_grayworld_gains_are_within_the_summation_bound(n, h, w, name):
    """The gray-world gains of the chain against ``grayworld_gains`` on the composed plane, in front of and behind the denoiser.

    Both form g_c = gray / max(m_c, 1e-6), gray = (m_0 + m_1 + m_2) / 3, m_c = t_c * (1 / HW) in fp32 from a total t_c of the
    same HW non-negative float32 values x (the stage's input lies in [0,1] here), taken in different orders.  With
    u = 2^-24, T = 64 * 32 and S_c the exact sum (= sum|x|):
      * chain: a row is within (T - 1) u of its tile's exact sum relative to the tile's mass (the bound test 2 holds the rows
        to), the rows are added in double precision (at most G rounding errors of 2^-53 each, below u / 2 in all) and rounded
        to float once: |t_c - S_c| <= ((T - 1) u + 2 u) S_c <= (T + 1) u S_c;
      * composed: any order of float32 additions of HW values is within (HW - 1) u S_c (Higham eq. 4.4), wider accumulators
        only lower it.
    So the two totals differ by at most d = (T + HW) u relative to S_c.  The multiplication by 1 / HW is the same operation on
    both sides (one rounding each: + 2 u), the three-term sum and the division by 3 of positive terms keep a relative
    perturbation and add 3 roundings each side (+ 6 u), the quotient gray / m_c adds the perturbations of numerator and
    denominator and one rounding each side (+ 2 u): |g - g'| <= (2 (d + 2 u) + 8 u) (1 + d) g' <= 2 (T + HW + 8) u g' to first
    order; the test allows 2 (T + HW + 16) u, the slack covering the second-order terms (d < 2^-10).  Where a mean is below
    the floor 1e-6 the denominator is the constant on both sides and the bound holds a fortiori.  Nothing here is taken from
    a run."""
    import reconfigisp_amd.functional as F
    import test_gpu_serve_denoise as D
    dev = D._frames(n, h, w, seed=5 * h + n)
    blocks = _blocks(n, 23 * n + h)
    den = (name, D._denoise_args(name, n))
    rel = 2.0 * (64 * 32 + h * w + 16) * U
    for turn, (kind, order) in enumerate([('bilinear', [F.OP_GAMMA, 'D', F.OP_GTM_MANUAL, 'gray']), ('nearest', ['D', 'gray']),
                                          ('laplacian', [F.OP_GAMMA, 'gray', 'D']), ('nearest', [F.OP_TONE_CRYSIS, 'D', 'white', 'gray'])]):
        phase, black = SETTINGS[(turn * 3 + h) % len(SETTINGS)]
        _, consts = _chain(dev, kind, order, blocks, den, black, phase)
        plane = _composed(dev, kind, order, blocks, den, consts, black, phase, upto=order.index('gray'))
        assert (plane >= 0).all().item()
        want = F.grayworld_gains(plane).double().cpu()
        got = consts[-1].double().cpu()
        assert tuple(got.shape) == (n, 3)
        err = (got - want).abs()
        print('DENOISE_SCENE gains %dx%dx%d %s %s %s: worst %.3e of the bound' % (n, h, w, kind, name, order,
                                                                                  (err / (rel * want.abs()).clamp_min(1e-300)).max().item()))
        assert (err <= rel * want.abs()).all(), (kind, order, got, want)


# ---------------------------------------------------------------- 5. serve() end to end
PIPELINES = [('Demosaic_02_sRGB_05_07_01', None),           # bilinear, gray-world, bilateral, Gamma
             ('Demosaic_03_sRGB_01_08_06_13', 'median'),    # Malvar-He-Cutler, Gamma, median, white-world, WbQuadratic
             ('Demosaic_01_sRGB_06_09_05_04', None),        # nearest, white-world, non-local means, gray-world, Filmic
             ('Demosaic_01_sRGB_05_06_09_04', None)]        # nearest, gray-world, white-world, non-local means, Filmic
# the third has a scene stage behind non-local means, which the measurement took out of the plan (profiles/serve_denoise_scene.txt,
# pipeline_fusion._DENOISE_SCENE_SLOWER): through serve() it must run as without the keyword; with the verdict lifted it is
# served like the others, which keeps serve()'s handling of a statistic behind that denoiser under test
DROPPED = {'Demosaic_01_sRGB_06_09_05_04'}


def _hand(net, dev, black, phase, reverse=False):
    """the pipeline's module list as the chain of test 3: (order, blocks, denoiser, demosaic kind)"""
    import reconfigisp_amd.functional as F
    from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF
    from reconfigisp_amd.codes.models.modules import tools_origin as T
    n = dev.shape[0]
    kind, order, blocks, den = None, [], {}, None
    with torch.no_grad():
        pars = net._stage_params(n)
    for mod, par in zip(net.all_modules, pars):
        t = type(mod)
        if t is T.Skip:
            continue
        if t in PF._CLASSICAL_DEMOSAIC:
            kind = PF._CLASSICAL_DEMOSAIC[t]
        elif t in PF._DENOISER:
            den = PF._denoise_args(mod, par)
            order.append('D')
        elif t is T.Grayworld:
            order.append('gray')
        elif t is T.OriginWbWhiteworld:
            order.append('white')
            blocks['white'] = par.detach()[:, 0].float().contiguous()
        else:
            (op,), (block,) = PF._stage_lists([mod], [par], [0])
            assert op not in blocks
            order.append(op)
            blocks[op] = block
    return order, blocks, den, kind


@pytest.mark.parametrize('arch,small', PIPELINES, ids=lambda v: v if isinstance(v, str) and '_' in v else None)
def test_pipeline_serve_denoise_scene(arch, small, monkeypatch):
    import reconfigisp_amd.functional as F
    import test_gpu_serve_denoise as D
    import test_gpu_serve_scene as GS
    from reconfigisp_amd import lib as L
    from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF
    net = D._net(arch, small)
    n, h, w = 3, 34, 68
    dev = D._frames(n, h, w, seed=90)
    if arch in DROPPED:
        # as shipped: exactly the default call
        plain = net.serve(dev, 1023.0).clone()
        assert net.last_serve_route == 'composed'
        assert torch.equal(net.serve(dev, 1023.0, fast_denoise_scene=True), plain) and net.last_serve_route == 'composed'
        monkeypatch.setattr(PF, '_DENOISE_SCENE_SLOWER', frozenset())
    order, blocks, den, kind = _hand(net, dev, 0, 'rggb')
    assert den is not None and 'D' in order
    scenes = [item for item in order if item in ('gray', 'white')]
    behind = sum(1 for i, item in enumerate(order) if item in ('gray', 'white') and i > order.index('D'))
    # the default call is today's
    want = net.serve(dev, 1023.0).clone()
    assert net.last_serve_route == 'composed'
    want_rgb = net.serve(dev, 1023.0, reverse_channels=True).clone()
    want_bggr = net.serve(dev, 1023.0, black_level=64, cfa='bggr').clone()
    kept = net.intermediate_results
    L.CALLS = {}
    try:
        got = net.serve(dev, 1023.0, fast_denoise_scene=True)
        calls = dict(L.CALLS)
    finally:
        L.CALLS = None
    assert net.last_serve_route == 'denoise_scene'
    expected = {'risp_serve_scene_finish': len(scenes), 'risp_serve_denoise_scene_u8': 1}
    if behind:
        expected['risp_serve_denoise_stats'] = behind
    if len(scenes) - behind:
        expected['risp_serve_scene_stats'] = len(scenes) - behind
    assert calls == expected and sum(calls.values()) == 2 * len(scenes) + 1, calls
    assert not set(calls) & set(GS.COMPOSED_CALLS)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (n, h, w, 3)
    got = got.clone()
    got_rgb = net.serve(dev, 1023.0, reverse_channels=True, fast_denoise_scene=True).clone()
    got_bggr = net.serve(dev, 1023.0, black_level=64, cfa='bggr', fast_denoise_scene=True).clone()
    assert net.last_serve_route == 'denoise_scene'
    if 'gray' not in scenes:
        # a maximum has no order: the default call's bytes
        assert torch.equal(got, want) and torch.equal(got_rgb, want_rgb) and torch.equal(got_bggr, want_bggr)
    else:
        # the hand chain of test 3, and with its constants the composed route's bytes
        for res, black, phase, reverse, base in ((got, 0, 'rggb', False, want), (got_rgb, 0, 'rggb', True, want_rgb),
                                                 (got_bggr, 64, 'bggr', False, want_bggr)):
            hand, consts = _chain(dev, kind, order, blocks, den, black, phase, reverse)
            assert torch.equal(res, hand), '%s black %d %s reverse %s: serve() is not the hand chain' % (arch, black, phase, reverse)
            last = _composed(dev, kind, order, blocks, den, consts, black, phase)
            assert torch.equal(res, F.quantise_u8(last, reverse, None, F.CFA[phase]))
            print('DENOISE_SCENE %s black %d %s reverse %d: %.3e of the bytes differ from the default call (worst %d)' % (
                arch, black, phase, reverse, (res != base).float().mean().item(), (res.int() - base.int()).abs().max().item()))
        assert torch.equal(got_rgb, got.flip(-1))
    # with out= a warm call allocates nothing and leaves intermediate_results alone
    buf = torch.empty_like(got)
    net.serve(dev, 1023.0, out=buf, black_level=64, cfa='bggr', fast_denoise_scene=True)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    assert net.serve(dev, 1023.0, out=buf, black_level=64, cfa='bggr', fast_denoise_scene=True) is buf
    assert torch.cuda.memory_allocated() == before
    assert torch.equal(buf, got_bggr)
    assert net.intermediate_results is kept, 'serve() touched intermediate_results'
    # the default call has not moved
    assert torch.equal(net.serve(dev, 1023.0), want) and net.last_serve_route == 'composed'
    # a parameter changed in place reaches the next call
    live = [p for p in net.all_params if p.numel()]        # (the last stage with a parameter is element-wise in all three)
    with torch.no_grad():
        live[-1].add_(1.5)
    changed = net.serve(dev, 1023.0, fast_denoise_scene=True).clone()
    assert net.last_serve_route == 'denoise_scene' and not torch.equal(changed, got), 'a changed parameter did not reach serve()'
    order, blocks, den, kind = _hand(net, dev, 0, 'rggb')
    assert torch.equal(changed, _chain(dev, kind, order, blocks, den, 0, 'rggb')[0])


def test_pipeline_serve_denoise_scene_is_capturable():
    """one capture and one replay on another frame: 2 S + 1 launches on one stream, a linear graph"""
    import test_gpu_serve_denoise as D
    net = D._net(*PIPELINES[3])
    a, b = D._frames(3, 34, 68, seed=1), D._frames(3, 34, 68, seed=2)
    eager_b = net.serve(b, 1023.0, fast_denoise_scene=True).clone()
    assert net.last_serve_route == 'denoise_scene'
    slot, buf = a.clone(), torch.zeros((3, 34, 68, 3), device='cuda', dtype=torch.uint8)
    net.serve(slot, 1023.0, out=buf, fast_denoise_scene=True)            # fills the caches
    assert not torch.equal(buf, eager_b)
    buf.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        net.serve(slot, 1023.0, out=buf, fast_denoise_scene=True)
    assert net.last_serve_route == 'denoise_scene'
    slot.copy_(b)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(buf, eager_b)


def test_isp_model_serve_takes_the_keyword():
    from collections import OrderedDict
    from reconfigisp_amd.codes.models import create_model
    import test_gpu_serve_denoise as D
    opt = OrderedDict(model='isp', gpu_ids=[0], dist=False, is_train=False,
                      network_G=dict(which_model_G='OriginUniversal', architecture='Demosaic_02_sRGB_07_06_01', module_path=None),
                      path=dict(pretrain_model_G=None, strict_load=True))
    model = create_model(opt)                              # bilinear, bilateral, white-world, Gamma: the default call's bytes
    dev = D._frames(1, 34, 68, seed=4)
    want = model.serve(dev, 1023.0, reverse_channels=True).clone()
    assert model.netG.last_serve_route == 'composed'
    assert torch.equal(model.serve(dev, 1023.0, reverse_channels=True, fast_denoise_scene=True), want)
    assert model.netG.last_serve_route == 'denoise_scene'


# ---------------------------------------------------------------- 6. fallbacks: the call runs as without the keyword
@pytest.mark.parametrize('case', ['Reinhard in the list', 'two denoisers', 'median size 5', 'bilateral window 17 in one image', 'odd H',
                                  'W % 4 = 2', 'no scene stage', 'no denoiser', 'a scene stage behind non-local means'])
def test_fallbacks_run_as_without_the_keyword(case):
    import test_gpu_serve_denoise as D
    n = 2
    u = lambda *s: torch.rand(*s, generator=torch.Generator().manual_seed(len(case))).cuda()
    gam, med3, ratio = 0.2 + 0.6 * u(n, 1), torch.tensor([[0.1], [0.1]]).cuda(), 0.9 * u(n, 1)
    shape, route, good = (n, 34, 68), 'composed', None
    if case.startswith('Reinhard'):
        names, pars = ('bilinear', 'grayworld', 'median', 'reinhard'), [None, None, med3, 0.2 + 0.6 * u(n, 2)]
    elif case == 'two denoisers':
        names, pars = ('bilinear', 'grayworld', 'median', 'median'), [None, None, med3, med3]
    elif case.startswith('median'):
        names, pars = ('laplacian', 'grayworld', 'median'), [None, None, torch.tensor([[0.2], [0.2]]).cuda()]
        good = [None, None, med3]
    elif case.startswith('bilateral'):
        names, pars = ('bilinear', 'bilateral', 'whiteworld'), [None, torch.tensor([[0.5, 0.3, 0.7], [1.0, 0.3, 0.7]]).cuda(), ratio]
        good = [None, torch.tensor([[0.5, 0.3, 0.7], [0.9, 0.3, 0.7]]).cuda(), ratio]
    elif case == 'odd H':
        names, pars, shape, route = ('bilinear', 'grayworld', 'fastnlm'), [None, None, 0.9 * u(n, 3)], (n, 7, 12), None
        good = pars
    elif case == 'W % 4 = 2':
        names, pars, shape = ('nearest', 'grayworld', 'fastnlm'), [None, None, 0.9 * u(n, 3)], (n, 12, 10)
        good = pars
    elif case == 'no scene stage':
        names, pars = ('bilinear', 'gamma', 'median'), [None, gam, med3]
    elif case.startswith('a scene stage behind'):          # measured slower than the default call: not in the plan
        names, pars = ('bilinear', 'fastnlm', 'grayworld'), [None, 0.9 * u(n, 3), None]
    else:
        names, pars, route = ('bilinear', 'grayworld', 'gamma'), [None, None, gam], 'composed'
    dev = D._frames(*shape, seed=31)
    plain = D._serve_lists(names, pars, dev)
    fast = D._serve_lists(names, pars, dev, fast_denoise_scene=True)
    assert D._same(plain, fast), (plain, fast)
    if route is None:                                      # a stencil demosaic takes no mosaic of odd height: the same refusal either way
        assert plain[0] == 'raises' or plain[2] == 'composed'
    else:
        assert plain[0] == 'bytes' and plain[2] == route
    # but for the one thing named the list is the route's: without it the keyword does take it
    if good is not None:
        ok = D._serve_lists(names, good, D._frames(n, 34, 68, seed=31), fast_denoise_scene=True)
        assert ok[0] == 'bytes' and ok[2] == 'denoise_scene', ok


# ---------------------------------------------------------------- 7. refusals through the C ABI
def test_refusals_leave_output_and_partials_alone():
    import reconfigisp_amd.functional as F
    import test_gpu_serve_denoise as D
    from reconfigisp_amd import lib as L
    lib = L.load()
    n, h, w = 2, 4, 8
    raw = D._frames(n, h, w, seed=5)
    groups = F.serve_scene_groups(h, w)
    out = torch.full((n * h * w * 3 + 16,), 0x5A, device='cuda', dtype=torch.uint8)
    part = torch.full((n * groups * 4 + 8,), 123.0, device='cuda')
    gam = torch.full((n, 1), 0.5).cuda()
    cst = torch.full((n * 4 + 4,), 1.0, device='cuda')
    sig = torch.tensor([10.0, 20.0]).cuda()
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    Q8, REINHARD = F.OP_GAIN3_Q8, F.OP_TONE_REINHARD

    def call(entry='u8', raw_p=p(raw), divisor=1023.0, demosaic=2, pre=(F.OP_GAMMA,), pre_params=(gam.data_ptr(),), denoise=0, window=3,
             search=3, a=sig, b=sig, post=(Q8,), post_params=(cst.data_ptr(),), out_p=p(out), part_p=p(part), stat=F.SCENE_MAX3, N=n, H=h,
             W=w, black=0, cfa=0):
        head = (raw_p, divisor, demosaic, len(pre), (C.c_int * max(1, len(pre)))(*pre), L.ptr_array(list(pre_params) or [None]), denoise,
                window, search, p(a), p(b), len(post), (C.c_int * max(1, len(post)))(*post), L.ptr_array(list(post_params) or [None]))
        if entry == 'u8':
            return lib.risp_serve_denoise_scene_u8(*head, out_p, 0, N, H, W, black, cfa, F._stream())
        return lib.risp_serve_denoise_stats(*head, stat, part_p, N, H, W, black, cfa, F._stream())

    g = gam.data_ptr()
    both = {
        'bilateral window 5': (dict(window=5), b'window 5'), 'median size 5': (dict(denoise=1, window=5), b'size 5'),
        'nlm block 5': (dict(denoise=2, window=5), b'block 5'), 'nlm search 5': (dict(denoise=2, search=5), b'search 5'),
        'bilateral without sigma_space': (dict(b=None), b'sigma'), 'nlm without decay': (dict(denoise=2, a=None), b'decay'),
        'H odd': (dict(H=5), b'H=5'), 'H 2': (dict(H=2), b'H=2'), 'W % 4': (dict(W=6), b'W=6'), 'W 2': (dict(W=2), b'W=2'),
        'N 65536': (dict(N=65536), b'N=65536'),
        'nine stages': (dict(pre=(F.OP_GAMMA,) * 5, pre_params=(g,) * 5, post=(F.OP_GAMMA,) * 4, post_params=(g,) * 4), b'5 + 4'),
        'Reinhard in front': (dict(pre=(REINHARD,), pre_params=(cst.data_ptr(),)), b'op 10'),
        'Reinhard behind': (dict(post=(REINHARD,)), b'op 10'),
        'op 11': (dict(post=(11,)), b'op 11'), 'demosaic in ops': (dict(pre=(F.OP_DEMOSAIC_NEAREST,)), b'op 1 '),
        'missing parameter block': (dict(pre_params=(None,)), b'stage 0 has no parameter block'),
        'missing constants': (dict(post_params=(None,)), b'stage 1 (op 9) needs the constants'),
        'misaligned constants behind': (dict(post_params=(cst.data_ptr() + 4,)), b'stage 1 must be 16-byte aligned'),
        'misaligned constants in front': (dict(pre=(Q8,), pre_params=(cst.data_ptr() + 8,)), b'stage 0 must be 16-byte aligned'),
        'demosaic 3': (dict(demosaic=3), b'demosaic 3'), 'denoiser 3': (dict(denoise=3), b'denoiser 3'), 'cfa 4': (dict(cfa=4), b'cfa 4'),
        'black 65536': (dict(black=65536), b'65536'), 'divisor 0': (dict(divisor=0.0), b'divisor'), 'null raw': (dict(raw_p=None), b'null'),
        'raw at 4 bytes': (dict(raw_p=C.c_void_p(raw.data_ptr() + 4)), b'8-byte'),
    }
    only = {
        'u8': {'null out': (dict(out_p=None), b'null'), 'out at 1 byte': (dict(out_p=C.c_void_p(out.data_ptr() + 1)), b'4-byte')},
        'stats': {'LOGLUM': (dict(stat=F.SCENE_LOGLUM), b'stat 2'), 'stat 3': (dict(stat=3), b'stat 3'), 'stat -1': (dict(stat=-1), b'stat -1'),
                  'null partials': (dict(part_p=None), b'null'),
                  'partials at 4 bytes': (dict(part_p=C.c_void_p(part.data_ptr() + 4)), b'16-byte')},
    }
    for entry, symbol in (('u8', b'risp_serve_denoise_scene_u8'), ('stats', b'risp_serve_denoise_stats')):
        for what, (kw, named) in {**both, **only[entry]}.items():
            assert call(entry, **kw) != 0, '%s: %s was accepted' % (entry, what)
            msg = lib.risp_last_error()
            assert symbol in msg and named in msg, (entry, what, msg)
    torch.cuda.synchronize()
    assert (out == 0x5A).all().item(), 'a refused call wrote to its output'
    assert (part == 123.0).all().item(), 'a refused call wrote to its partials'
    # the wrappers refuse what they can see
    with pytest.raises(ValueError, match='SCENE_MEAN3 or SCENE_MAX3'):
        F.serve_denoise_stats(raw, 1023.0, 'bilinear', [], [], 'median', (3,), [], [], F.SCENE_LOGLUM)
    with pytest.raises(ValueError, match='bilateral, median, fastnlm'):
        F.serve_denoise_scene_u8(raw, 1023.0, 'bilinear', [], [], 'bm3d', (3,), [], [])
    with pytest.raises(ValueError, match='partials must be'):
        F.serve_denoise_stats(raw, 1023.0, 'bilinear', [], [], 'median', (3,), [], [], F.SCENE_MAX3, partials=part[:4].view(1, 1, 4))
    with pytest.raises(ValueError):
        F.serve_denoise_scene_u8(raw, 1023.0, 'bilinear', [], [], 'median', (3,), [], [], out=out[1:1 + n * h * w * 3].view(n, h, w, 3))
    with pytest.raises(RuntimeError, match='op 10'):       # ... and hand the library's message on otherwise
        F.serve_denoise_scene_u8(raw, 1023.0, 'bilinear', [REINHARD], [cst[:n * 4].view(n, 4)], 'median', (3,), [], [])
    # the same arguments without the fault are accepted, by every denoiser
    for entry in ('u8', 'stats'):
        assert call(entry) == 0 and call(entry, denoise=1, search=0, a=None, b=None) == 0
        assert call(entry, denoise=2, b=None, demosaic=0, black=65535, cfa=3, stat=F.SCENE_MEAN3) == 0
    torch.cuda.synchronize()
    size, rows = n * h * w * 3, n * groups * 4
    assert not (out[:size] == 0x5A).all().item() and (out[size:] == 0x5A).all().item()
    assert not (part[:rows] == 123.0).any().item() and (part[rows:] == 123.0).all().item()
