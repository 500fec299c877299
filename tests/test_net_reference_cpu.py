"""The referee of tests/test_gpu_net_space.py checked on its own (tests/net_reference.py): the restatements ARE the oracle's
networks, the hooks are live, the table's declared forms agree with the dispatch predicates, and the inputs tie where they say."""
import pytest
import torch

import isp_oracle as O
import net_reference as R

ORACLE = {'srcnn_res': lambda x, pv, w: O.srcnn_res(x, pv if pv is not None else x.new_zeros((x.shape[0], 0)), w),
          'srcnn_demosaic': lambda x, pv, w: O.srcnn_demosaic(x, w),
          'path14l_bayer': lambda x, pv, w: O.path14l_bayer(x, w), 'path14l_bgr': lambda x, pv, w: O.path14l_bgr(x, w)}
SMALL = [('srcnn_res', 3, (2, 3, 12, 20)), ('srcnn_res', 0, (2, 3, 9, 17)), ('srcnn_demosaic', 0, (2, 1, 18, 26)),
         ('path14l_bayer', 0, (2, 1, 12, 20)), ('path14l_bgr', 0, (2, 3, 5, 7))]


def _setup(kind, P, shape, which='smooth', dtype=torch.float64):
    x = R.make_input(which, *shape, seed=7).to(dtype)
    pv = R.make_pv(shape[0], P, 8)
    pv = pv.to(dtype) if pv is not None else None
    w = {k: v.to(dtype) for k, v in O.make_weights(kind, 9, P).items()}
    y_shape = (shape[0], 1 if kind == 'path14l_bayer' else 3, shape[2], shape[3])
    return x, pv, w, R.make_gy(y_shape, 10).to(dtype)


@pytest.mark.parametrize('kind,P,shape', SMALL)
def test_restatements_are_the_oracle(kind, P, shape):
    """float64, no overrides: the same ``y`` bit for bit, the same autograd ``gx`` (and ``gpv``) within 1e-12"""
    x, pv, w, gy = _setup(kind, P, shape)
    xo = x.clone().requires_grad_(True)
    po = pv.clone().requires_grad_(True) if P else None
    yo = ORACLE[kind](xo, po, w)
    go = torch.autograd.grad(yo, [xo] + ([po] if P else []), gy)
    ev = R.evaluate(kind, x, pv, w, gy)
    assert torch.equal(ev['y'], yo.detach())
    assert len(ev['pre']) == R.RELUS[kind]
    assert R.rel_err(ev['gx'], go[0]) <= 1e-12
    if P:
        assert R.rel_err(ev['gpv'], go[1]) <= 1e-12
    else:
        assert ev['gpv'] is None
    # fp32 too: the yardstick of the budget report is the same code
    x32, pv32, w32, _ = _setup(kind, P, shape, dtype=torch.float32)
    assert torch.equal(R.evaluate(kind, x32, pv32, w32, dtype=torch.float32)['y'], ORACLE[kind](x32, pv32, w32))


@pytest.mark.parametrize('kind,P,shape', SMALL)
def test_own_masks_reproduce_autograd_and_the_hooks_are_live(kind, P, shape):
    x, pv, w, gy = _setup(kind, P, shape, 'quantised')
    plain = R.evaluate(kind, x, pv, w, gy, weight_grads=True)
    masks = [p > 0 for p in plain['pre']]
    arg = R.first_arg(x) if kind == 'srcnn_res' else None
    assert not R.check_arg(x, arg) if arg is not None else True
    over = R.evaluate(kind, x, pv, w, gy, masks=masks, arg=arg, weight_grads=True)
    assert R.flips(masks, plain['pre']) == 0
    assert R.rel_err(over['y'], plain['y']) <= 1e-12
    assert R.rel_err(over['gx'], plain['gx']) <= 1e-12
    for k in plain['gw']:
        assert R.rel_err(over['gw'][k], plain['gw'][k]) <= 1e-12, k
    if P:
        assert R.rel_err(over['gpv'], plain['gpv']) <= 1e-12
    # one decision flipped, in every layer in turn: gx moves
    for k in range(len(masks)):
        flipped = [m.clone() for m in masks]
        live = (plain['pre'][k] > 0).nonzero()
        at = tuple(live[len(live) // 2].tolist())
        flipped[k][at] = False
        assert R.flips(flipped, plain['pre']) == 1
        assert R.rel_err(R.evaluate(kind, x, pv, w, gy, masks=flipped, arg=arg)['gx'], plain['gx']) > 1e-9, 'mask %d is dead' % k
    # masks of another layer's shape, too few, too many: refused
    with pytest.raises(ValueError):
        R.evaluate(kind, x, pv, w, gy, masks=masks[:-1], arg=arg)
    with pytest.raises(ValueError):
        R.evaluate(kind, x, pv, w, gy, masks=masks + masks[-1:], arg=arg)
    if arg is not None:                                 # the statistics' gradient lands where ``arg`` says
        moved = arg.clone()
        moved[0, 1, 0] += 1                             # (inside the saturated patch: the same value, another pixel)
        assert x.flatten(2)[0, 1, moved[0, 1, 0]] == x.flatten(2)[0, 1, arg[0, 1, 0]]
        ev = R.evaluate(kind, x, pv, w, gy, masks=masks, arg=moved)
        assert R.rel_err(ev['y'], plain['y']) <= 1e-12 and R.rel_err(ev['gx'], plain['gx']) > 1e-9
        assert R.check_arg(x, moved)
        with pytest.raises(ValueError):
            R.evaluate('srcnn_demosaic', x[:, :1], None, w, arg=arg)


def test_check_arg_holds_the_contract():
    x = R.make_input('quantised', 2, 3, 9, 17, seed=3)
    arg = R.first_arg(x)
    assert R.check_arg(x, arg) == []
    later = arg.clone()
    later[1, 2, 1] += 1                                 # still the max, not the first
    assert any('first' in s for s in R.check_arg(x, later)) and not any('not the plane' in s for s in R.check_arg(x, later))
    wrong = arg.clone()
    wrong[0, 0, 0] = 0                                  # pixel 0 is not in the zero patch
    assert any('not the plane' in s for s in R.check_arg(x, wrong))
    assert R.check_arg(x, arg.new_full(arg.shape, 9 * 17))
    c = R.make_input('constant', 2, 3, 8, 12, seed=4)
    ac = R.first_arg(c)
    assert int(ac[0].abs().max()) == 0 and R.check_arg(c, ac) == []
    ac[0, 1, 1] = 5                                     # same value everywhere: only the index rule catches it
    assert R.check_arg(c, ac)


def test_rel_err():
    a = torch.tensor([1.0, -4.0])
    assert R.rel_err(a, a) == 0.0 and R.rel_err(a + torch.tensor([0.0, 0.5]), a) == 0.125
    assert R.rel_err(torch.zeros(3), torch.zeros(3)) == 0.0 and R.rel_err(torch.tensor([0.0, 1e-30, 0.0]), torch.zeros(3)) == float('inf')
    assert R.rel_err(torch.tensor([float('nan'), 0.0]), a) == float('inf')
    with pytest.raises(AssertionError):
        R.rel_err(torch.zeros(2), torch.zeros(3))


def test_table_forms_agree_with_the_predicates():
    from reconfigisp_amd import convnets as CN
    ids = [R.case_id(c) for c in R.CASES]
    assert len(set(ids)) == len(ids), 'two rows are one case'
    for h in range(1, 20):
        for w in (1, 7, 8, 9, 8192, 8193):
            assert R.srcnn_fold_ok(h, w) == CN._srcnn_fold_ok(h, w)
    for kind in ('srcnn_res', 'srcnn_demosaic'):
        for P in ((0, 1, 2, 3, 5) if kind == 'srcnn_res' else (0,)):
            # build_srcnn_packs: fold for a residual net with cout <= 4, the direct-kernel ends of the demosaic net
            spec = O.conv_shapes(kind, P)
            residual = kind == 'srcnn_res'
            want = {'fold': residual and spec[2][1] <= 4, 'small_bwd': (not residual) and spec[0][2] == 4,
                    'small': (not residual) and spec[2][1] <= 12 and spec[2][3] in (3, 5)}
            assert R.pack_conditions(kind, P) == want
    assert R.pack_conditions('srcnn_res', 3) == {'fold': True, 'small_bwd': False, 'small': False}
    assert R.pack_conditions('srcnn_demosaic') == {'fold': False, 'small_bwd': True, 'small': True}    # what SrcnnDemosaicGroup needs
    for c in R.CASES:
        cid = R.case_id(c)
        assert R.expected_form(c) == c['form'], '%s: the dispatch takes %r' % (cid, R.expected_form(c))
        assert c['n'] <= 4 and max(c['hw']) <= (128 if c['kind'] in ('srcnn_demosaic', 'path14l_bayer') else 96), cid
        assert c['input'] in R.INPUTS and c['arith'] in ('f16x2', 'f32') and c['kind'] in R.KINDS, cid
        assert c['arith'] == 'f16x2' or c['kind'].startswith('path14l'), cid
        if c['kind'] == 'srcnn_res':
            assert len(c['P']) == c['members'] and (c['members'] == 1) == (c['form'] != 'group'), cid
        else:
            assert c['members'] == (2 if c['form'].startswith('group') else 1), cid
    # a row that says "group" where no group may form is a table error
    bad = dict(R.CASES[0], kind='srcnn_demosaic', form='group-grad', hw=(36, 20), members=2, P=(0, 0))
    assert R.expected_form(bad) is None
    assert R.expected_form(dict(bad, kind='srcnn_res', form='group', hw=(7, 12))) is None
    assert R.expected_form(dict(bad, kind='srcnn_res', form='folded', hw=(7, 12), members=1, P=(1,))) is None


def test_every_wiring_branch_is_reached():
    for name, pred in R.BRANCHES.items():
        assert any(pred(c) for c in R.CASES), 'no row reaches: ' + name
    sizes = lambda kind: {c['hw'] for c in R.CASES if c['kind'] == kind}
    assert sizes('srcnn_res') >= {(7, 12), (8, 8), (8, 12), (20, 36), (34, 30), (40, 72), (64, 96), (9, 17), (24, 32)}
    assert {c['P'][0] for c in R.CASES if c['kind'] == 'srcnn_res' and c['members'] == 1} == {0, 1, 3, 5}
    assert sizes('srcnn_demosaic') == {(8, 8), (16, 24), (36, 20), (18, 26), (80, 72), (128, 64)}
    assert sizes('path14l_bgr') == {(5, 7), (16, 16), (33, 30), (48, 80), (64, 96)}
    assert sizes('path14l_bayer') == {(8, 8), (18, 26), (40, 72), (96, 64)}
    for kind in ('path14l_bgr', 'path14l_bayer'):       # every size differentiates under both arithmetics
        for hw in sizes(kind):
            assert {c['arith'] for c in R.CASES if c['kind'] == kind and c['hw'] == hw and c['form'] == 'grad'} == {'f16x2', 'f32'}
    groups = {(c['n'], c['hw'], len(c['P'])) for c in R.CASES if c['form'] == 'group'}
    assert {g[0] for g in groups} == {2, 4} and {g[1] for g in groups} == {(8, 12), (24, 32), (40, 72)} and {g[2] for g in groups} == {2, 8}


def test_inputs_tie_where_they_say():
    for c in R.CASES:
        x, pvs, wts, gys = R.case_inputs(c)
        assert x.dtype == torch.float32 and 0.0 <= float(x.min()) and float(x.max()) <= 1.0
        assert len(pvs) == len(wts) == len(gys) == c['members']
        flat = x.flatten(2)
        n_min = (flat == flat.min(dim=2)[0][..., None]).sum(dim=2)
        n_max = (flat == flat.max(dim=2)[0][..., None]).sum(dim=2)
        if c['input'] == 'quantised':
            assert int(n_min.min()) >= 2 and int(n_max.min()) >= 2, R.case_id(c)
            assert float(flat.min()) == 0.0 and float(flat.max()) == 1.0 and torch.equal(x, torch.round(x * 255) / 255)
            assert int(R.first_arg(x).min()) > 0                    # neither patch starts at pixel 0
        elif c['input'] == 'constant':
            assert int(n_min[0].min()) == flat.shape[2] and int(n_max[1:].max()) < flat.shape[2], R.case_id(c)
        if len(gys) > 1:
            assert not torch.equal(gys[0], gys[1])
    a, b = R.case_inputs(R.CASES[3]), R.case_inputs(R.CASES[3])
    assert torch.equal(a[0], b[0]) and torch.equal(a[3][0], b[3][0])
