"""CPU: the restatement of the fused training step (tests/train_step_reference.py) against the imported reference's float64
and float32 goldens and against torch.optim.Adam, the coverage of the case table of tests/test_gpu_train_step_space.py, and
the conditioning rule that table has to meet - measured here on the restatement alone, not on the kernel."""
import os

import numpy as np
import pytest
import torch

import isp_oracle as O
import test_gpu_train_step_space as T
import train_step_reference as R
from conftest import assert_close, load_golden
from train_step_reference import OP_WB_MANUAL as WB, OP_GAMMA as GA, OP_GTM_MANUAL as GT, OP_WB_QUADRATIC as WQ

_FUZZ = int(os.environ.get('RISP_TEST_SEEDS', '8'))


# ---------------------------------------------------------------------------------------------------- the reference goldens
def _golden_run(dtype):
    """case a of tests/golden/isp_model*.npz (Bayer_02_Demosaic_01_sRGB_11_01_13, MSE, Adam as test_host_logic.isp_opt
    sets it) through reference_step, the state carried in ``dtype`` -> [(step outputs)] of both steps"""
    g = load_golden('isp_model')
    assert str(g['a_arch']) == 'Bayer_02_Demosaic_01_sRGB_11_01_13' and str(g['a_criterion']) == 'l2'
    assert O.parse_architecture(str(g['a_arch'])) == ['skip', 'nearest', 'wbmanual', 'gamma', 'wbquadratic']
    ops = [WB, GA, WQ]
    raw = [torch.tensor(O.PARAM_INIT[R.OP_NAMES[op]], dtype=torch.float32).to(dtype) for op in ops]
    m, v = [torch.zeros_like(r) for r in raw], [torch.zeros_like(r) for r in raw]
    img, gt = torch.from_numpy(g['a_img']), torch.from_numpy(g['a_gt'])
    steps = []
    for it in range(2):
        out = R.reference_step(ops, True, R.LOSS_MSE, img, gt, raw, m, v, it + 1, 1e-2, (0.9, 0.99), 1e-8, dtype)
        raw, m, v = out[3], out[4], out[5]
        steps.append(out)
    return steps


_KEYS = ['param_step3_wbmanual', 'param_step4_gamma', 'param_step5_wbquadratic']


def test_restatement_reproduces_the_reference_float64_golden():
    f = load_golden('isp_model_f64')
    for it, (y, loss, grads, raw, _, _, _) in enumerate(_golden_run(torch.float64)):
        rows = [('output', y, f['a_it%d_output' % it]), ('loss', loss.reshape(1), f['a_it%d_loss' % it].reshape(1))]
        rows += [('grad ' + k, grads[j], f['a_it%d_grad_%s' % (it, k)]) for j, k in enumerate(_KEYS)]
        rows += [('state ' + k, raw[j], f['a_it%d_%s' % (it, k)]) for j, k in enumerate(_KEYS)]
        for what, a, b in rows:
            assert b.dtype == np.float64
            err = np.abs(a.numpy() - b).max() / np.abs(b).max()
            assert err <= 1e-9, 'it%d %s: %.3e of the tensor\'s magnitude' % (it, what, err)


def test_restatement_in_float32_reproduces_the_reference_golden():
    g = load_golden('isp_model')
    for it, (y, loss, grads, raw, _, _, _) in enumerate(_golden_run(torch.float32)):
        assert y.dtype == torch.float32 and raw[0].dtype == torch.float32
        assert_close(y, g['a_it%d_output' % it], what='it%d output' % it)
        assert_close(loss.reshape(1), g['a_it%d_loss' % it].reshape(1), what='it%d loss' % it)
        for j, k in enumerate(_KEYS):
            assert_close(grads[j], g['a_it%d_grad_%s' % (it, k)], what='it%d grad %s' % (it, k))
            assert_close(raw[j], g['a_it%d_%s' % (it, k)], what='it%d %s' % (it, k))


@pytest.mark.parametrize('loss_kind', [R.LOSS_MSE, R.LOSS_L1])
def test_adam_against_torch_optim_adam_in_double(loss_kind):
    """10 steps with a MultiStepLR milestone inside, moments and parameters at every step"""
    ops, n = [WB, GA, GT, WQ], 2
    rng = np.random.Generator(np.random.PCG64(11))
    img, gt = O.synthetic_raw(n, 16, 16, seed=3)
    pars = [torch.nn.Parameter(torch.from_numpy(np.asarray(O.PARAM_INIT[R.OP_NAMES[op]]) + 0.2 * rng.standard_normal(R.PARAM_WIDTH[op])))
            for op in ops]
    assert pars[0].dtype == torch.float64
    opt = torch.optim.Adam(pars, 2e-2, (0.9, 0.99))
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, [4], gamma=0.5)
    crit = torch.nn.MSELoss() if loss_kind == R.LOSS_MSE else torch.nn.L1Loss()
    raw = [p.detach().clone() for p in pars]
    m, v = [torch.zeros_like(r) for r in raw], [torch.zeros_like(r) for r in raw]
    lrs = []
    for step in range(1, 11):
        lr = opt.param_groups[0]['lr']
        lrs.append(lr)
        x = O.demosaic_nearest(img.double())
        for op, p in zip(ops, pars):
            x = O.apply_op(R.OP_NAMES[op], x, torch.sigmoid(p).repeat(n, 1))
        loss = crit(x, gt.double())
        opt.zero_grad()
        loss.backward()
        opt.step()
        sched.step()
        y, l, grads, raw, m, v, blocks = R.reference_step(ops, True, loss_kind, img, gt, raw, m, v, step, lr, (0.9, 0.99), 1e-8,
                                                          torch.float64)
        close = lambda a, b, what: (a - b).abs().max().item() <= 1e-12 * max(b.abs().max().item(), 1e-30) or \
            pytest.fail('step %d %s: %.3e' % (step, what, (a - b).abs().max().item() / b.abs().max().item()))
        close(y, x.detach(), 'output'), close(l, loss.detach(), 'loss')
        for k, p in enumerate(pars):
            st = opt.state[p]
            assert int(st['step']) == step
            close(grads[k], p.grad, 'grad %d' % k), close(raw[k], p.detach(), 'param %d' % k)
            close(m[k], st['exp_avg'], 'exp_avg %d' % k), close(v[k], st['exp_avg_sq'], 'exp_avg_sq %d' % k)
            want = torch.sigmoid(p.detach()).repeat(n, 1) * (5 if ops[k] == WB else 1)
            assert blocks[k].shape == (n, R.PARAM_WIDTH[ops[k]])
            close(blocks[k], want, 'blocks %d' % k)
    assert lrs[0] == 2e-2 and lrs[-1] == 1e-2 and lrs[3] != lrs[4]


def test_zero_grad_at_removes_exactly_the_masked_positions():
    case = T.tie_case('tie-gamma')
    st = case['state']
    args = (case['ops'], case['from_bayer'], R.LOSS_L1, case['img'], case['gt'], st['raw'], st['exp_avg'], st['exp_avg_sq'], 1, 1e-2,
            T.BETAS, T.EPS, torch.float64)
    plain = R.reference_step(*args)
    everywhere = R.reference_step(*args, zero_grad_at=torch.ones_like(case['gt'], dtype=torch.bool))
    assert torch.equal(plain[0], everywhere[0]) and torch.equal(plain[1], everywhere[1])
    assert all(not g.any() for g in everywhere[2]) and all(torch.equal(a, b) for a, b in zip(everywhere[3], st['raw']))
    nowhere = R.reference_step(*args, zero_grad_at=torch.zeros_like(case['gt'], dtype=torch.bool))
    assert all(torch.equal(a, b) for a, b in zip(nowhere[2], plain[2]))
    # one half of the positions: what is left is the gradient of the other half's loss
    mask = torch.zeros_like(case['gt'], dtype=torch.bool)
    mask[:, :, :, : case['w'] // 2] = True
    left, right = R.reference_step(*args, zero_grad_at=mask), R.reference_step(*args, zero_grad_at=~mask)
    for a, b, c in zip(left[2], right[2], plain[2]):
        assert (a + b - c).abs().max().item() <= 1e-15


# ---------------------------------------------------------------------------------------------------- the table
def test_launch_geometry_of_the_named_classes():
    geo = lambda name: T.launch_geometry(*T.CASES[name][0][1:])
    assert geo('idle-a') == (1, 1) and geo('full-a') == (1, 8)
    assert geo('ragged-a') == (2, 9) and geo('ragged-b') == (3, 12)       # 4160 and 8514 pairs: ragged last workgroups
    assert geo('bx8-a') == (8, 16) and geo('bx32-a') == (32, 16) and geo('headline-a') == (8, 16)
    assert geo('stride2-a') == (32, 32) and geo('stride8-a') == (32, 128)
    assert all(T.CASES[n][0][2] % 4 for n in ('ragged-a', 'ragged-b', 'ragged-c', 'ragged-d'))       # W % 4 != 0


def test_table_covers_every_class_with_both_instantiations():
    seen, ns, lengths = {}, set(), set()
    for name, ((n, h, w), pipe, kind, loss, samples, state, lr, seed) in T.CASES.items():
        ops = T.PIPES[pipe]
        assert h % 2 == 0 and w % 2 == 0 and 1 <= len(ops) <= 6 and ops.count(WQ) <= 1
        f = seen.setdefault(WQ in ops, dict(geometry=set(), input=set(), loss=set(), samples=set(), state=set(), pipes=set()))
        f['geometry'].add(T.geometry_class(n, h, w)), f['input'].add(kind), f['loss'].add(loss), f['samples'].add(samples)
        f['state'].add(state), f['pipes'].add(pipe)
        ns.add(n), lengths.add(len(ops))
    classes = {'bx1-idle', 'bx1-full', 'ragged', 'bx8', 'bx32', 'stride2', 'stride8', 'batch', 'headline'}
    for wbq, f in seen.items():
        assert f['geometry'] == classes, (wbq, classes ^ f['geometry'])
        assert f['input'] == {'mosaic', 'bgr'} and f['loss'] == {'mse', 'l1'} and f['state'] == {'fresh', 'resumed'}, wbq
    assert seen[True]['samples'] | seen[False]['samples'] == set(T.SAMPLES)
    assert {'synthetic', 'uniform'} <= seen[True]['samples'] & seen[False]['samples']
    assert ns >= {1, 3, 64, 65, 70, 200} and lengths == {1, 2, 3, 4, 5, 6}
    assert {T.CASES[n][0] for n in T.CASES} >= {(1, 2, 2), (2, 8, 8), (64, 256, 256)}
    assert sum(1 for c in T.CASES.values() if c[0] == (64, 256, 256)) == 2
    assert any(c[0][1] * c[0][2] >= 1024 * 2048 for c in T.CASES.values())
    used = [T.PIPES[p] for p in seen[True]['pipes'] | seen[False]['pipes'] | {c[1] for c in T.TIES.values()}]
    assert len(used) == len(T.PIPES)                                     # no pipeline of the axis left out
    for op in (WB, GA, GT):                                              # every op repeated except WbQuadratic
        assert any(p.count(op) >= 2 for p in used), R.OP_NAMES[op]
    where = {('alone' if len(p) == 1 else 'first' if p[0] == WQ else 'last' if p[-1] == WQ else 'middle') for p in used if WQ in p}
    assert where == {'alone', 'first', 'middle', 'last'}
    assert any(len(p) == 6 and WQ in p for p in used) and any(len(p) == 6 and WQ not in p for p in used)
    # multi-step and tie runs: one of each instantiation; the ties behind a last stage that does not clamp there
    assert sorted(WQ in T.PIPES[T.CASES[n][1]] for n in T.MULTI) == [False, True]
    assert sorted(WQ in T.PIPES[c[1]] for c in T.TIES.values()) == [False, True]
    assert {T.PIPES[c[1]][-1] for c in T.TIES.values()} == {GA, GT} and all(c[3] == 'l1' for c in T.TIES.values())
    assert T.MULTI_STEPS == 12 and T.HALVE_AT == 6 and T.BETAS == (0.9, 0.99)
    # the saturated case: |raw| = 12 on the stage it names
    (name, (k, vals)), = T.SATURATED.items()
    case = T.table_case(name)
    assert case['state']['raw'][k].tolist() == vals and max(vals) == 12 and min(vals) == -12


def test_samples_reach_the_gates_they_are_meant_for():
    img, _ = T.make_samples('uniform', False, 2, 8, 8, seed=1)
    assert img.min() < 0 and img.max() > 1 and img.min() >= -0.1 and img.max() <= 1.2
    for fb in (True, False):
        img, gt = T.make_samples('constant', fb, 3, 4, 6, seed=2)
        bgr = O.demosaic_nearest(img) if fb else img
        assert (bgr == bgr[:, :, :1, :1]).all() and gt.shape == (3, 3, 4, 6)
    st = T.make_state([WB, WQ], 'resumed', np.random.Generator(np.random.PCG64(1)))
    assert st['step'] >= 2 and all((v > 0).all() for v in st['exp_avg_sq']) and all(m.abs().min() > 0 for m in st['exp_avg'])
    assert abs(st['raw'][0].mean().item() + 1.38) < 0.6


# ---------------------------------------------------------------------------------------------------- the conditioning rule
def _assert_conditioned(case, state, lr, what, zero_grad_at=None, pair=None):
    pair = pair or T.reference_pair(case, state, lr, zero_grad_at)
    err, label = T.conditioning(case, state, lr, zero_grad_at, pair)
    assert T.alive(pair[1]), '%s: %.2f of the outputs on a clamp, largest gradient per stage %s - draw another seed' % (
        what, T.clamped_share(pair[1]), ['%.1e' % g.abs().max().item() for g in pair[1][2]])
    print('%s: fp32 restatement within %.2e of float64 (worst: %s)' % (what, err, label))
    assert err <= T.COND, '%s: the restatement\'s own fp32 result is %.2e from float64 on %s (rule: %.0e) - draw another seed' % (
        what, err, label, T.COND)


@pytest.mark.parametrize('name', list(T.CASES))
def test_conditioning_rule_table(name):
    case = T.table_case(name)
    _assert_conditioned(case, case['state'], case['lr'], case['what'])


@pytest.mark.parametrize('name', T.MULTI)
def test_conditioning_rule_twelve_steps(name):
    """every step of the multi-step runs, along the restatement's own fp32 trajectory (the GPU test starts each step from
    the kernel's state, which is that trajectory up to the error under test)"""
    case = T.table_case(name)
    state = case['state']
    for i in range(T.MULTI_STEPS):
        lr = T.lr_at(case, i)
        pair = T.reference_pair(case, state, lr)
        _assert_conditioned(case, state, lr, '%s step %d' % (case['what'], i + 1), pair=pair)
        state = T.next_state(state, pair[0])
    assert state['step'] == case['state']['step'] + T.MULTI_STEPS


@pytest.mark.parametrize('name', list(T.TIES))
def test_conditioning_rule_ties(name):
    case = T.tie_case(name)
    st, mask = case['state'], T.tie_mask(T.tie_case(name))
    assert 0.28 < mask.float().mean().item() < 0.32
    y = T.reference_pair(case, st, case['lr'])[0][0]
    case['gt'] = torch.where(mask, y, case['gt'])
    _assert_conditioned(case, st, case['lr'], case['what'], zero_grad_at=mask)
    # the statement is worth something: without the ties' zero the gradient moves by far more than any bound
    with_zero, without = T.reference_pair(case, st, case['lr'], zero_grad_at=mask)[1], T.reference_pair(case, st, case['lr'])[1]
    moved = max(((a - b).abs().max() / b.abs().max()).item() for a, b in zip(without[2], with_zero[2]))
    assert moved > 1e-2, moved


def test_conditioning_rule_walk():
    """every seed the walk may draw ends within the rule (and alive) in WALK_DRAWS draws, and at most 1 seed in 8 has a
    draw that misses the rule"""
    missed, draws, classes = [], [], set()
    for seed in range(_FUZZ):
        case = T.walk_case(seed)                                  # raises when a seed runs out of draws
        _assert_conditioned(case, case['state'], case['lr'], case['what'], pair=case['pair'])
        classes.add((case['geometry'], case['wbq']))
        draws.append(case['draws'])
        if case['missed_cond']:
            missed.append(seed)
    print('walk: draws per seed %s, seeds with a draw outside the rule %s; classes %s' % (draws, missed, sorted(classes)))
    assert len(missed) <= -(-_FUZZ // 8), 'seeds %s of %d have a draw that misses the conditioning rule' % (missed, _FUZZ)
