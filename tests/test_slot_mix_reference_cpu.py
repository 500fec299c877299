"""CPU: the case table, the builders and the walk of tests/test_gpu_slot_mix_space.py, and its float64 restatement
(tests/slot_mix_reference.py) - what the GPU test relies on, checked without a GPU.

  coverage      every geometry class the kernels have is in the table, computed from fwd_geometry / bwd_geometry (and the mix
                kernels' own), both sides of every loop bound; every kind alone, first and last; every block frozen; both
                backward instantiations
  conditioning  on every case and walk draw the restatement's fp32 result is within COND = 2e-5 of its float64 result on every
                judged tensor (a case that misses gets another seed, never a wider bound)
  liveness      every requested gradient has a non-zero entry, every clamp has pixels on both sides
  restatement   fp32 = the oracle composition of test_gpu_slot_mix.py; wrong variants (an operand's input gradient dropped, a
                parameter-gradient block shifted by one operand, weights permuted) are >= 100 x the ErrorBudget bound away
"""
import functools

import pytest
import torch

import isp_oracle as O
from conftest import assert_close
import slot_mix_reference as R
from slot_mix_reference import T


@functools.lru_cache(maxsize=None)
def survey(name):
    """small facts about one table case (the tensors themselves are dropped)"""
    case = R.table_case(name)
    pair = R.reference_pair(case)
    r64 = pair[1]
    rel = lambda a, b: ((a.double() - b.double()).abs().max() / (b.abs().max() or 1.0)).item()
    wrong = {}
    k_of = {o: k for k, o in enumerate(case['order']) if o != T}
    for kind, k in k_of.items():                     # the input gradient with this operand's term dropped
        rest = [e for i, e in enumerate(case['entries']) if i != k]
        if any(e[0] == 'op' for e in rest):
            less = R.reference(torch.float64, case['x'], rest, torch.cat([case['w'][:k], case['w'][k + 1:]]), case['gy'])
            wrong['gx without ' + kind] = rel(less['gx'], r64['gx'])
        else:
            wrong['gx without ' + kind] = 1.0        # the only element-wise operand: nothing is left
    gps = sorted(r64['gp'].items())
    for i in range(1, len(gps)):                     # the finish kernel's element index not moved past a block: operand k's rows
        (k0, a), (k1, b) = gps[i - 1], gps[i]        # read from the operand before
        flat = torch.cat([a.flatten(), b.flatten()])
        wrong['gp of %s shifted' % case['order'][k1]] = rel(flat[:b.numel()].view_as(b), b)
        wrong['gp of %s shifted' % case['order'][k0]] = rel(flat[-a.numel():].view_as(a), a)
    if len(case['order']) > 1:
        rolled = R.reference(torch.float64, case['x'], case['entries'], case['w'].roll(1), case['gy'])
        wrong['weights permuted'] = max(rel(rolled['y'], r64['y']), rel(rolled['gx'], r64['gx']) if r64['gx'] is not None else 0.0)
    return dict(order=case['order'], n=case['n'], hw=case['hw'], needs=case['needs'], cond=R.conditioning(pair),
                live=R.liveness(case, r64), wrong=wrong, gp_rows_zero=all((r64['gp'][k][1:] == 0).all().item() for k in r64['row0'] if k in r64['gp']))


NAMES = list(R.CASES)


def test_geometry_classes_are_in_the_table():
    fwd = {nm: R.fwd_geometry(R.CASES[nm]['shape'][0], R.CASES[nm]['shape'][1] * R.CASES[nm]['shape'][2]) for nm in NAMES}
    bwd = {nm: R.bwd_geometry(R.CASES[nm]['shape'][0], R.CASES[nm]['shape'][1] * R.CASES[nm]['shape'][2]) for nm in NAMES}
    shape = {nm: R.CASES[nm]['shape'] for nm in NAMES}
    hw4 = {nm: shape[nm][1] * shape[nm][2] // 4 for nm in NAMES}
    for q in (0, 1):                                 # every class in both instantiations
        mine = [nm for nm in NAMES if R.CASES[nm]['order'] != 'shipped' and R.instantiation(R.CASES[nm]['order']) == q]
        has = lambda pred: any(pred(nm) for nm in mine)
        assert has(lambda nm: hw4[nm] == 1) and has(lambda nm: hw4[nm] == 16), 'threads without a vector'
        assert has(lambda nm: hw4[nm] == 256 and shape[nm][0] == 1), 'one full workgroup'
        assert has(lambda nm: fwd[nm][0] == 9 and bwd[nm][2] == 9 and hw4[nm] % 256), 'ragged: bx 3 both ways, 9 rows'
        assert has(lambda nm: fwd[nm][1] == 1 and hw4[nm] <= 64 * 256) and has(lambda nm: fwd[nm][1] == 2 and fwd[nm][0] == 64), \
            'both sides of the forward loop bound (64 * 256 vectors)'
        assert has(lambda nm: fwd[nm][1] == 2 and bwd[nm] == (64, 2, 64)), 'the backward second trip at bx 64'
        assert has(lambda nm: fwd[nm][1] == 5 and hw4[nm] % (64 * 256)), 'five trips, ragged last'
        assert has(lambda nm: bwd[nm] == (600, 2, 600) and hw4[nm] % 256), 'bx 1, two ragged trips, 600 rows'
        assert has(lambda nm: bwd[nm] == (512, 4, 512)), 'four trips'
        for rows in (63, 64, 65, 70):
            assert has(lambda nm: bwd[nm][2] == rows), 'the finish kernel\'s row loop at %d rows' % rows
        assert has(lambda nm: 'gtm_manual' in R.CASES[nm]['order'] and shape[nm][0] > 1 and bwd[nm][2] > shape[nm][0] and bwd[nm][1] == 1)
        assert has(lambda nm: 'gtm_manual' in R.CASES[nm]['order'] and shape[nm][0] == 40 and bwd[nm][2] == 40 * 13 and bwd[nm][1] == 2)
    assert any(R.CASES[nm]['order'][0] == 'wb_quadratic' and R.CASES[nm]['shape'] == (600, 32, 36) for nm in NAMES)   # 18000 gp elements
    assert all(R.CASES[nm]['order'].count(T) <= 2 for nm in NAMES if R.CASES[nm]['shape'] == (512, 64, 64))
    for nm in NAMES:                                 # the scratch the test allocates is what the library asks for: checked on the GPU
        assert bwd[nm][2] * 56 == R.scratch_floats(shape[nm][0], shape[nm][1] * shape[nm][2])


def test_mix_geometry_classes_are_in_the_table():
    geo = {nm: (R.mix_fwd_geometry(v[0]), R.mix_bwd_geometry(v[0]), v[1]) for nm, v in R.MIX_CASES.items()}
    assert {g[2] for g in geo.values()} == {1, 2, 5, 15, 16}
    assert any(v[0] == 4 for v in R.MIX_CASES.values())
    assert {63, 64, 65} <= {g[1][2] for g in geo.values()}                                     # partial rows around the row loop's 64
    assert any(g[0][0] == 2048 and g[0][1] == 2 and g[2] <= 3 for g in geo.values()) and any(g[0][1] == 1 for g in geo.values())
    assert any(g[1][0] == 1024 and g[1][1] > 4 and g[2] == 2 for g in geo.values()) and any(g[1][1] <= 4 for g in geo.values())
    assert any(v[2] for v in R.MIX_CASES.values()) and any(not v[2] for v in R.MIX_CASES.values())


def test_operand_axis_is_in_the_table():
    orders = {nm: (R.shipped_order() if R.CASES[nm]['order'] == 'shipped' else R.CASES[nm]['order']) for nm in NAMES}
    for kind in R.KINDS + (T,):
        assert [kind] in orders.values(), '%s alone' % kind
        assert any(o[0] == kind and len(o) > 1 for o in orders.values()), '%s first' % kind
        assert any(o[-1] == kind and len(o) > 1 for o in orders.values()), '%s last' % kind
    full = {tuple(o for o in order if o != T) for order in orders.values() if set(R.KINDS) <= set(order)}
    assert tuple(R.KINDS) in full and tuple(R.KINDS[::-1]) in full and len({tuple(o) for o in orders.values() if set(R.KINDS) <= set(o)}) >= 5
    assert any(len(o) == 16 and o.count(T) == 10 for o in orders.values())
    ship = orders['shipped']
    assert len(ship) == 15 and ship.count(T) == 9 and set(ship) - {T} == set(R.KINDS)
    frozen = [set(R.CASES[nm]['needs'].get('frozen', ())) for nm in NAMES]
    for kind in R.WIDTH:
        assert {kind} in frozen, 'only %s frozen' % kind
    assert set(R.WIDTH) in frozen
    assert {R.CASES[nm]['needs'].get('no_go') for nm in NAMES} >= {(0,), (1,), (2,)}
    no_gx = [nm for nm in NAMES if R.CASES[nm]['needs'].get('x') is False]
    assert {('grayworld' in orders[nm]) for nm in no_gx} == {True, False}
    assert any(orders[nm].count('grayworld') == 1 and len(set(orders[nm])) == 2 for nm in NAMES), 'gray world the only consumer of x'
    assert any(R.CASES[nm]['stacks'] for nm in NAMES) and any(not R.CASES[nm]['w_host'] for nm in NAMES)
    assert {R.CASES[nm]['weights'] for nm in NAMES} == {'softmax', 'zero', 'negative', 'unnormalised'}
    assert {R.instantiation(o) for o in orders.values()} == {0, 1}
    assert R.WALK_SEEDS >= 24


@pytest.mark.parametrize('name', NAMES)
def test_conditioning_rule_and_liveness(name):
    s = survey(name)
    assert s['cond'][0] <= R.COND, '%s: fp32 restatement %.2e from float64 on %s: draw another seed' % (name, *s['cond'])
    assert not s['live'], '%s: %s' % (name, '; '.join(s['live']))
    assert s['gp_rows_zero'], 'the tone curve\'s block gradient below row 0'


def test_weights_of_the_table():
    for name in ('w-zero', 'w-negative', 'w-unnormalised'):
        w = R.table_case(name)['w']
        assert {'w-zero': (w == 0).any(), 'w-negative': (w < 0).any(), 'w-unnormalised': abs(w.sum() - 1) > 0.1}[name]


@pytest.mark.parametrize('seed', range(R.WALK_SEEDS))
def test_walk_draws_are_conditioned_and_alive(seed):
    case = R.walk_case(seed)                         # raises when no draw of the seed qualifies
    assert case['missed_cond'] <= 2, '%s: %d draws outside COND' % (case['what'], case['missed_cond'])
    assert len(case['order']) >= 1 and len(set(o for o in case['order'] if o != T)) == len([o for o in case['order'] if o != T])


def test_walk_varies_every_axis():
    cases = [R.walk_case(seed) for seed in range(R.WALK_SEEDS)]
    assert len({tuple(c['order']) for c in cases}) >= 20 and len({(c['n'], c['hw']) for c in cases}) >= 5
    assert any(c['needs']['frozen'] for c in cases) and any(c['needs']['no_go'] for c in cases) and any(not c['needs']['x'] for c in cases)
    assert {R.instantiation(c['order']) for c in cases} == {0, 1} and any(c['stacks'] for c in cases)


def test_fp32_restatement_is_the_oracle_composition():
    """the composition of test_fused_slot_mixture_without_tensor_operands_and_against_oracle, on its case's order"""
    row = R._case((2, 24, 32), [o for o in R.ORDERS['interleaved'] if o != T], 9)
    case = R.build('oracle', row)
    got = R.reference(torch.float32, case['x'], case['entries'], case['w'], case['gy'])
    xc = case['x'].clone().requires_grad_(True)
    bc = {k: v.clone().requires_grad_(True) for k, v in case['blocks'].items()}
    wc = case['w'].clone().requires_grad_(True)
    ops = {'skip': lambda: xc, 'gamma': lambda: O.gamma_manual(xc, bc['gamma']), 'wb_manual': lambda: O.wb_manual(xc, bc['wb_manual']),
           'gtm_manual': lambda: O.gtm_manual(xc, bc['gtm_manual']), 'wb_quadratic': lambda: O.wb_quadratic(xc, bc['wb_quadratic']),
           'grayworld': lambda: O.grayworld(xc)}
    ref = sum(ops[o]() * wc[i] for i, o in enumerate(case['order']))
    live = [k for k in ('gamma', 'wb_manual', 'gtm_manual', 'wb_quadratic')]
    rg = torch.autograd.grad(ref, [wc, xc] + [bc[k] for k in live], case['gy'])
    assert torch.equal(got['y'], ref.detach()) and torch.equal(got['gw'], rg[0])
    assert_close(got['gx'], rg[1], rtol=1e-6, floor=1.0, what='gx')        # autograd adds the operands' terms in another order
    for name, g in zip(live, rg[2:]):
        assert_close(got['gp'][case['order'].index(name)], g, rtol=1e-6, floor=1.0, what=name)
    assert (rg[2 + live.index('gtm_manual')][1:] == 0).all()


def test_table_tells_wrong_variants_apart():
    worst = {}
    for name in NAMES:
        if R.CASES[name]['shape'][0] * R.CASES[name]['shape'][1] * R.CASES[name]['shape'][2] > 40000:
            continue                                 # the small cases are enough (and the large ones take seconds each)
        for what, dist in survey(name)['wrong'].items():
            worst[what] = max(worst.get(what, 0.0), dist)
    wanted = ['gx without ' + k for k in R.KINDS] + ['gp of %s shifted' % k for k in R.WIDTH] + ['weights permuted']
    for what in wanted:
        assert worst.get(what, 0.0) >= 100 * R.BUDGET_CAP, '%s: at most %.2e from the reference on any case' % (what, worst.get(what, 0.0))
