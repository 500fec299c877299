"""Without a GPU: the restatement of tests/wgrad_reference.py agrees with float64 autograd, taps that never land inside the image are exact
zeros, the case table reaches every template instance of risp_conv2d_wgrad on both sides of every form boundary, ``accepts`` refuses
the layers and sizes the entry point refuses, and the bar of tests/test_gpu_wgrad_space.py is meaningful for the table's inputs: a float32 restatement of every
table case stays within a quarter of it."""
import pytest
import torch
import torch.nn.functional as TF

import wgrad_reference as R
from wgrad_reference import CONSTCH, PLAIN


def autograd64(case):
    x, gy, cv = R.inputs(case)
    n, h, w = case['n'], case['h'], case['w']
    full = x if cv is None else torch.cat([x, cv[:, :, None, None].expand(-1, -1, h, w)], dim=1)
    wd = torch.zeros(case['cout'], case['cin'], case['k'], case['k'], dtype=torch.float64, requires_grad=True)
    bd = torch.zeros(case['cout'], dtype=torch.float64, requires_grad=True)
    return torch.autograd.grad(TF.conv2d(full.double(), wd, bd, padding=case['k'] // 2), (wd, bd), gy.double())


SECOND_OPINION = ['1x1_33to1 k1 3x7x15', '3x3_33to40 plain 1x9x17', '3x3_10to33 thin_in 2x3x4', '3x3_64to3 thin_out 1x8x16', '5x5_7to7 plain 3x7x15', '9x9_17to64 plain 2x20x36',
                  '5x5_6to6 thin_in 1x33x30', '5x5_40to6 thin_out 3x7x15', '9x9_31to64 plain 2x3x4', '9x9_3to64 thin_in 1x1x4', '9x9_4to1 thin_out 1x9x17',
                  '9x9_17to64 thin_in 3x20x36 constch 3', '9x9_12to64 plain 2x3x9 constch 3', '5x5_40to6 thin_out 2x9x17 constch 11',
                  '9x9_3to64 thin_in 2x3x9 constch 2']


@pytest.mark.parametrize('name', SECOND_OPINION)
def test_restatement_agrees_with_float64_autograd(name):
    case = R.CASES[name]
    (dw, db), (aw, ab) = R.ref64(case), autograd64(case)
    assert dw.dtype == torch.float64 and tuple(dw.shape) == (case['cout'], case['cin'], case['k'], case['k']) and tuple(db.shape) == (case['cout'],)
    assert (dw - aw).abs().max().item() <= 1e-12 * aw.abs().max().item(), name
    assert (db - ab).abs().max().item() <= 1e-12 * ab.abs().max().item(), name


def test_taps_that_never_land_inside_the_image_are_exact_zeros():
    """k = 9 on a 3 x 4 plane: rows |ky - 4| >= 3 and columns |kx - 4| >= 4 multiply padding alone"""
    case = R.CASES['9x9_17to64 plain 2x3x4']
    dw, _ = R.ref64(case)
    out = R.never_lands(9, 3, 4)
    assert out.sum().item() == 81 - 5 * 7 and out[0, 4] and out[4, 0] and out[1, 1] and not out[2, 1] and not out[6, 7]
    assert (dw[:, :, out] == 0).all() and (dw[:, :, ~out] != 0).all()
    one = R.never_lands(9, 1, 1)
    assert one.sum().item() == 80 and not one[4, 4]
    for c in R.CASES.values():                                      # in float32 too: what the GPU test holds the kernel to
        if c['n'] * c['h'] * c['w'] <= 64:
            z = R.never_lands(c['k'], c['h'], c['w'])
            assert (R.ref64(c)[0][:, :, z] == 0).all() and (R.ref32(c)[0][:, :, z] == 0).all(), c['name']


def test_table_reaches_every_instance_boundary_and_edge():
    cases = list(R.CASES.values())
    assert len(R.ALL) < 260 and len(R.WALK) == 6 * R.SEEDS
    # the ten instantiations, each at the four common shapes at least, under the PLAIN load
    inst = {(c['k'], c['form']) for c in cases}
    assert inst == {(1, 'k1')} | {(k, f) for k in (3, 5, 9) for f in ('plain', 'thin_in', 'thin_out')}
    for k, f in inst:
        shapes = {(c['n'], c['h'], c['w']) for c in cases if (c['k'], c['form'], c['load']) == (k, f, PLAIN)}
        assert shapes >= set(R.COMMON), (k, f)
    assert {(c['n'], c['h'], c['w']) for c in cases} >= set(R.ROTATING)
    # every literal: the form of the launch the case makes; the shortcut where conv_wgrad's rule says so
    for c in cases:
        assert c['form'] == R.form(*R.launched(c)), c['name']
        assert c['shortcut'] == R.shortcut(c) and R.accepts(c), c['name']
        assert R.lds_floats(R.launched(c)[0], c['k']) * 4 <= 65536
    # both sides of each form boundary: cin * k (and cout * k) = 30 against 33 at k = 3, 30 / 35 at k = 5, 27 / 36 at k = 9
    layers = {(c['k'], c['cin'], c['cout']): c['form'] for c in cases if c['load'] == PLAIN}
    for k, below, above in ((3, 10, 11), (5, 6, 7), (9, 3, 4)):
        assert below * k <= 32 < above * k
        assert layers[(k, below, below)] == 'thin_in' and layers[(k, above, above)] == 'plain'          # both thin: thin-in wins
        assert any(f == 'thin_out' and ci == above and co * k <= 32 for (kk, ci, co), f in layers.items() if kk == k), k
        assert any(f == 'thin_in' and ci == below and co * k > 32 for (kk, ci, co), f in layers.items() if kk == k), k
        assert any(f == 'thin_out' and ci * k > 32 and co == below for (kk, ci, co), f in layers.items() if kk == k), k
    assert layers[(3, 64, 3)] == 'thin_out' and layers[(9, 31, 64)] == 'plain' and layers[(9, 31, 3)] == 'thin_out'
    assert {(c['cin'], c['cout']) for c in cases if c['k'] == 1} >= {(64, 32), (5, 5), (33, 1), (1, 64)}
    # more tiles than any slice count, for one layer of each kind; two channel blocks on either side
    many = {(c['cin'], c['cout'], c['k']) for c in cases if (c['n'], c['h'], c['w']) == R.MANY}
    assert many == set(R.MANY_LAYERS) and R.MANY[0] > R.WG_TOTAL and len(many) == 5
    assert {R.form(*m) for m in many} == set(R.FORMS)
    # CONSTCH: the shortcut and the kernel's own branch, constants across the 32-channel block in the thin-out form, the thin-in form
    const = [c for c in cases if c['load'] == CONSTCH]
    assert {c['cin'] - 12 for c in const if c['shortcut'] and c['k'] == 9} == {0, 1, 5}
    assert any(c['shortcut'] and (c['n'], c['h'], c['w']) == (2, 4, 4) for c in const)
    kern = [c for c in const if not c['shortcut']]
    assert {c['form'] for c in kern} == {'plain', 'thin_in', 'thin_out'}
    assert any(c['cin_img'] * c['k'] > 32 for c in kern) and any(c['h'] < c['k'] // 2 and c['cin_img'] * c['k'] <= 32 for c in kern)
    assert any(c['form'] == 'thin_out' and c['cin_img'] < 32 < c['cin'] for c in kern)
    assert any((c['k'], c['cin'], c['cout'], c['cin_img']) == (5, 40, 6, 3) for c in kern)
    assert {(4, 17, 9), (12, 20, 3)} <= {(c['cin_img'], c['cin'], c['k']) for c in kern}
    # the walk stays inside what the entry accepts and reaches both load modes and several forms
    walk = list(R.WALK.values())
    assert all(R.accepts(c) and c['n'] <= 4 and c['h'] <= 40 and c['w'] <= 70 for c in walk)
    if len(walk) >= 48:
        assert {c['load'] for c in walk} == {PLAIN, CONSTCH} and len({R.form(*R.launched(c)) for c in walk}) >= 3
        assert {R.shortcut(c) for c in walk if c['load'] == CONSTCH} == {False, True}


def test_refused_layers_and_limits():
    base = dict(n=2, h=9, w=17, load=PLAIN, cin_img=0)
    for cin, cout, k in R.REFUSED_LAYERS:
        assert not R.accepts(dict(base, cin=cin, cout=cout, k=k)), (cin, cout, k)
    assert {k for _, _, k in R.REFUSED_LAYERS} >= {7, 9} and any(ci == 65 for ci, _, _ in R.REFUSED_LAYERS)
    assert R.accepts(dict(base, cin=31, cout=64, k=9)) and R.accepts(dict(base, cin=64, cout=64, k=5))
    assert R.lds_floats(32, 9) * 4 == 65792 and R.lds_floats(31, 9) * 4 <= 65536           # 32 * 129 + 32 * 385 floats
    assert not R.accepts(dict(base, cin=0, cout=4, k=3)) and not R.accepts(dict(base, cin=4, cout=65, k=3))
    assert R.accepts(dict(base, cin=1, cout=64, k=1, n=1023)) and not R.accepts(dict(base, cin=1, cout=64, k=1, n=1024))
    assert not R.accepts(dict(base, cin=4, cout=4, k=3, load=R.UNSHUFFLE))
    assert not R.accepts(dict(base, cin=12, cout=4, k=3, load=CONSTCH, cin_img=3, cvals=False))
    assert not R.accepts(dict(base, cin=12, cout=4, k=3, load=CONSTCH, cin_img=0))
    assert R.accepts(dict(base, cin=12, cout=4, k=3, load=CONSTCH, cin_img=3))


def test_scratch_and_form_restate_the_header():
    assert R.scratch_floats(64, 64, 3) == 768 * 9 * 1024 and R.scratch_floats(3, 64, 9) == 768 * 9 * 1024
    assert R.scratch_floats(17, 64, 9) == 768 * 81 * 1024 and R.scratch_floats(64, 3, 3) == 768 * 3 * 1024
    assert R.scratch_floats(5, 5, 1) == 768 * 1024 and R.scratch_floats(32, 3, 5) == 768 * 5 * 1024
    assert R.form(32, 32, 1) == 'k1' and R.form(6, 6, 5) == 'thin_in' and R.form(7, 6, 5) == 'thin_out' and R.form(7, 7, 5) == 'plain'


def test_the_bar_is_meaningful_for_these_inputs():
    """float32 inputs and float32 accumulation of the restatement itself: at most a quarter of the GPU bar on every table case"""
    worst = (0.0, None)
    for c in R.CASES.values():
        e = R.errors(R.ref32(c)[0], R.ref64(c)[0])[1]
        worst = max(worst, (e, c['name']))
        assert e <= R.BAR / 4, (c['name'], e)
        assert torch.isfinite(R.ref64(c)[0]).all() and R.ref64(c)[0].abs().max().item() > 0
    print('largest float32 restatement error %.3e of max|ref| (%s), bar / 4 = %.2e' % (worst + (R.BAR / 4,)))
