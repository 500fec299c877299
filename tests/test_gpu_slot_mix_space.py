"""GPU: the slot mixture kernels (risp_slot_mix_fwd / _bwd, risp_slot.hip) and the plain mixture (risp_mix_fwd / _bwd,
risp_reduce.hip) through the C ABI over their argument space, against float64.

The table, the builders, the seeded walk and the float64 restatement are tests/slot_mix_reference.py (plain CPU code, checked
by tests/test_slot_mix_reference_cpu.py).  Every case builds the descriptor itself over buffers pre-filled with NaN between
guard bands and is held to

  1. float64: y, gw, gx, every go and every gp row against the restatement, by conftest.ErrorBudget with its defaults as
     test_gpu_error_budget.py uses it (ref32 = the restatement in float32).  Gray world is the C ABI's operand RISP_OP_GAIN3
     here (the gains are the GPU's own, a leaf of the restatement); the route through functional.slot_mix under autograd,
     with the gradient through the channel means, is judged the same way for the cases marked ``autograd``;
  2. fused = unfused: functional.slot_mix against the operators run one by one plus functional.mix, with the same needs;
  3. full writes: no requested output holds NaN, the tone curve's rows >= 1 are exactly 0, buffers whose pointer was NULL and
     all guard bands (64 floats on both sides of every output and of the scratch) are untouched;
  4. determinism: a second call gives the same bits; dropping one go[k] / gp[k] changes no other output's bits;
  5. refusals: every refused argument returns non-zero, names the cause and writes nothing (host-side checks only).
"""
import ctypes as C

import pytest
import torch

import slot_mix_reference as R
from conftest import ErrorBudget, assert_close
from slot_mix_reference import T

pytestmark = pytest.mark.gpu

NAN, GUARD, BAND = float('nan'), 12345.0, 64
KIND_CODE = {'skip': 0, 'wb_manual': 2, 'gamma': 3, 'gtm_manual': 4, 'wb_quadratic': 5, 'grayworld': 6}     # include/risp.h


class Guarded:
    """a device buffer between two bands of BAND sentinel floats, NaN inside"""

    def __init__(self, *shape):
        numel = 1
        for s in shape:
            numel *= s
        self.raw = torch.full((numel + 2 * BAND,), GUARD, device='cuda')
        self.t = self.raw[BAND: BAND + numel].view(*shape)
        self.t.fill_(NAN)

    def bands_intact(self):
        return (self.raw[:BAND] == GUARD).all().item() and (self.raw[-BAND:] == GUARD).all().item()

    def untouched(self):
        return self.bands_intact() and torch.isnan(self.t).all().item()


def _budget(what, got, r32, r64):
    budget = ErrorBudget()
    for (family, label, a), (_, _, b), (_, _, c) in zip(R.judged(got), R.judged(r32), R.judged(r64)):
        assert torch.isfinite(a).all().item(), '%s: %s holds NaN / inf (elements left unwritten)' % (what, label)
        budget(a, b, c, '%s %s' % (what, label), family)
    budget.finish()


class Runner:
    """Device buffers of one case and the descriptor over them, every field under the test's control."""

    def __init__(self, case):
        from reconfigisp_amd import functional as F, lib as L
        self.F, self.L, self.case = F, L, case
        self.x, self.gy = case['x'].cuda(), case['gy'].cuda()
        self.blocks = {k: v.cuda() for k, v in case['blocks'].items()}
        self.tensors = [t.cuda() for t in case['tensors']]
        self.pointwise = any(o != T for o in case['order'])
        if 'grayworld' in case['order']:
            self.blocks['grayworld'] = F.grayworld_gains(self.x)
        self.gains = self.blocks['grayworld'].cpu() if 'grayworld' in case['order'] else None
        self.want = [R.requested(case['needs'], case['entries'], k) for k in range(len(case['order']))]
        assert L.load().risp_slot_mix_scratch_floats(case['n'], case['hw']) == R.scratch_floats(case['n'], case['hw'])

    def alloc(self):
        c = self.case
        shape = (c['n'], 3, c['h'], c['w_'])
        self.y, self.gx, self.gw = Guarded(*shape), Guarded(*shape), Guarded(len(c['order']))
        self.scratch = Guarded(R.scratch_floats(c['n'], c['hw']))
        self.go, self.gp, self.stacked = {}, {}, []
        for members in (c['stacks'] or ()):          # rows of one stacked tensor
            buf = Guarded(len(members), *shape)
            self.stacked.append(buf)
            for j, k in enumerate(members):
                self.go[k] = (buf, buf.t[j])
        for k, o in enumerate(c['order']):
            if o == T and k not in self.go:
                g = Guarded(*shape)
                self.go[k] = (g, g.t)
            elif o not in (T, 'skip'):
                g = Guarded(c['n'], 3 if o == 'grayworld' else R.WIDTH[o])
                self.gp[k] = (g, g.t)

    def desc(self, drop=None):
        c, d = self.case, self.L.SlotMixDesc()
        d.K, d.N, d.HW = len(c['order']), c['n'], c['hw']
        it = iter(self.tensors)
        for k, o in enumerate(c['order']):
            d.w[k], d.pmul[k] = float(c['w'][k]), 5.0 if o == 'wb_manual' else 1.0
            d.kind[k] = self.L.SLOT_TENSOR if o == T else KIND_CODE[o]
            d.ptr[k] = next(it).data_ptr() if o == T else (None if o == 'skip' else self.blocks[o].data_ptr())
            if self.want[k] and k != drop:
                if o == T:
                    d.go[k] = self.go[k][1].data_ptr()
                else:
                    d.gp[k] = self.gp[k][1].data_ptr()
        d.x, d.y = self.x.data_ptr(), self.y.t.data_ptr()
        return d

    def run(self, drop=None):
        """forward and backward into fresh buffers -> the result as R.reference returns it (CPU tensors)"""
        F = self.F
        self.alloc()
        d = self.desc(drop)
        self.L.call('risp_slot_mix_fwd', C.byref(d), F._stream())
        self.L.call('risp_slot_mix_bwd', C.byref(d), F._p(self.gy), F._p(self.gx.t) if self.pointwise else None, F._p(self.gw.t),
                    F._p(self.scratch.t), F._stream())
        torch.cuda.synchronize()
        what = self.case['what']
        written = lambda k: self.want[k] and k != drop
        for name, g in [('y', self.y), ('gx', self.gx), ('gw', self.gw), ('scratch', self.scratch)] + [('stack', s) for s in self.stacked]:
            assert g.bands_intact(), '%s: the guard bands of %s were written' % (what, name)
        if not self.pointwise:
            assert self.gx.untouched(), '%s: gx == NULL was written' % what
        for k, (g, t) in list(self.go.items()) + list(self.gp.items()):
            assert g.bands_intact(), '%s: the guard bands of operand %d\'s gradient were written' % (what, k)
            if not written(k):
                assert torch.isnan(t).all().item(), '%s: operand %d\'s gradient buffer was not passed, and was written' % (what, k)
        res = dict(y=self.y.t.cpu(), gw=self.gw.t.cpu(), gx=self.gx.t.cpu() if self.pointwise else None,
                   go={k: t.cpu() for k, (_, t) in self.go.items() if written(k)}, gp={k: t.cpu() for k, (_, t) in self.gp.items() if written(k)},
                   row0={k for k, o in enumerate(self.case['order']) if o == 'gtm_manual'})
        for k in res['row0'] & set(res['gp']):
            assert (res['gp'][k][1:] == 0).all().item(), '%s: the tone curve\'s block gradient below row 0 is not exactly 0' % what
        return res


def same_bits(a, b, what, but=None):
    for key in ('y', 'gw', 'gx'):
        if a[key] is not None:
            assert torch.equal(a[key].view(torch.int32), b[key].view(torch.int32)), '%s: %s differs in bits' % (what, key)
    for key in ('go', 'gp'):
        for k, t in a[key].items():
            if k != but:
                assert torch.equal(t.view(torch.int32), b[key][k].view(torch.int32)), '%s: %s %d differs in bits' % (what, key, k)


def autograd_route(case, fused):
    """functional.slot_mix (fused) or the operators one by one plus functional.mix, with the gradients the needs ask for"""
    import reconfigisp_amd.functional as F
    needs, order = case['needs'], case['order']
    x = case['x'].cuda().requires_grad_(needs['x'])
    blocks = {k: v.cuda().requires_grad_(k not in needs['frozen']) for k, v in case['blocks'].items()}
    tensors = [t.cuda().requires_grad_(i not in needs['no_go']) for i, t in enumerate(case['tensors'])]
    w = case['w'].cuda().requires_grad_(True)
    w_host = case['w'].tolist() if case['w_host'] else None
    it = iter(tensors)
    if fused:
        y = F.slot_mix(w, x, [('tensor', next(it)) if o == T else ('op', o, blocks.get(o)) for o in order], w_host=w_host, stacks=case['stacks'])
    else:
        ops = {'skip': lambda: x, 'gamma': lambda: F.gamma(x, blocks['gamma']), 'wb_manual': lambda: F.wb_manual(x, blocks['wb_manual'] * 5),
               'gtm_manual': lambda: F.gtm_manual(x, blocks['gtm_manual']), 'wb_quadratic': lambda: F.wb_quadratic(x, blocks['wb_quadratic']),
               'grayworld': lambda: F.grayworld(x)}
        y = F.mix(w, [next(it) if o == T else ops[o]() for o in order], w_host=w_host, stacks=case['stacks'])
    pointwise = any(o != T for o in order)
    res = dict(y=y.detach().cpu(), go={}, gp={}, gx=None, row0={k for k, o in enumerate(order) if o == 'gtm_manual'})
    wanted, where = [w], [('gw', None)]
    if pointwise and needs['x']:
        wanted.append(x), where.append(('gx', None))
    it = iter(tensors)
    for k, o in enumerate(order):
        leaf = next(it) if o == T else blocks.get(o)
        if leaf is not None and leaf.requires_grad:
            wanted.append(leaf), where.append(('go' if o == T else 'gp', k))
    for (key, k), g in zip(where, torch.autograd.grad(y, wanted, case['gy'].cuda())):
        if k is None:
            res[key] = g.cpu()
        else:
            res[key][k] = g.cpu()
    return res


def run_case(case):
    what = case['what']
    run = Runner(case)
    first = run.run()
    # --- 1: float64 (the gains of gray world are the GPU's own: a leaf)
    r32, r64 = case.get('pair') if run.gains is None and case.get('pair') else R.reference_pair(case, gains=run.gains)
    _budget(what.split(' ')[0], first, r32, r64)
    # --- 4: determinism, and an output less
    same_bits(first, run.run(), what + ': second call')
    dropped = [k for k in range(len(case['order'])) if run.want[k] and case['order'][k] != 'skip']
    if dropped:
        same_bits(run.run(drop=dropped[0]), first, what + ': without operand %d\'s gradient' % dropped[0])
    # --- 2: fused = unfused, under autograd with the case's needs
    fused, unfused = autograd_route(case, True), autograd_route(case, False)
    assert torch.equal(fused['y'], unfused['y']) and torch.equal(fused['y'], first['y']), what + ': y'
    assert fused['go'].keys() == unfused['go'].keys() and fused['gp'].keys() == unfused['gp'].keys()
    for k in fused['go']:
        assert torch.equal(fused['go'][k], unfused['go'][k]) and torch.equal(fused['go'][k], first['go'][k]), '%s: go %d' % (what, k)
    for k in fused['gp']:
        if case['order'][k] == 'wb_quadratic':
            assert_close(fused['gp'][k], unfused['gp'][k], rtol=1e-6, floor=1.0, what='%s: gp of wb_quadratic' % what)
        else:
            assert torch.equal(fused['gp'][k], unfused['gp'][k]), '%s: gp %d (%s)' % (what, k, case['order'][k])
        assert torch.equal(fused['gp'][k], first['gp'][k]), '%s: gp %d through autograd and through the C ABI' % (what, k)
    assert_close(fused['gw'], unfused['gw'], rtol=1e-5, floor=1.0, what=what + ': architecture terms')
    assert (fused['gx'] is None) == (unfused['gx'] is None)
    if fused['gx'] is not None:
        assert_close(fused['gx'], unfused['gx'], rtol=1e-5, floor=1.0, what=what + ': input gradient')
    if case['autograd']:                             # 1 again, through autograd: gray world with the gradient through its means
        p32, p64 = case.get('pair') or R.reference_pair(case)
        if not case['needs']['x']:
            p32, p64 = dict(p32, gx=None), dict(p64, gx=None)
        _budget(what.split(' ')[0] + ' autograd', fused, p32, p64)


@pytest.mark.parametrize('name', list(R.CASES))
def test_table(name):
    run_case(R.table_case(name))


@pytest.mark.parametrize('seed', range(R.WALK_SEEDS))
def test_random_walk(seed):
    run_case(R.walk_case(seed))


# ---------------------------------------------------------------------------------------------------- risp_mix_fwd / _bwd
class MixRunner:
    def __init__(self, case):
        from reconfigisp_amd import functional as F, lib as L
        self.F, self.L, self.case = F, L, case
        self.outs, self.gy = [o.cuda() for o in case['outs']], case['gy'].cuda()

    def run(self, drop=None, edit=None):
        F, L, c = self.F, self.L, self.case
        k, numel = c['k'], c['numel']
        self.y, self.gw, self.scratch = Guarded(numel), Guarded(k), Guarded(L.load().risp_mix_scratch_floats())
        self.go = {i: Guarded(numel) for i in range(k)}
        want = [i not in c['no_go'] and i != drop for i in range(k)]
        args = dict(outs=L.ptr_array([o.data_ptr() for o in self.outs]), w=(C.c_float * k)(*c['w'].tolist()), k=k, y=F._p(self.y.t), numel=numel,
                    gy=F._p(self.gy), go=L.ptr_array([self.go[i].t.data_ptr() if want[i] else None for i in range(k)]), gw=F._p(self.gw.t),
                    scratch=F._p(self.scratch.t))
        if edit:
            edit(args)
        lib = L.load()
        status = (lib.risp_mix_fwd(args['outs'], args['w'], args['k'], args['y'], args['numel'], F._stream()),
                  lib.risp_mix_bwd(args['outs'], args['w'], args['k'], args['gy'], args['go'], args['gw'], args['scratch'], args['numel'], F._stream()))
        message = lib.risp_last_error().decode()
        torch.cuda.synchronize()
        for name, g in [('y', self.y), ('gw', self.gw), ('scratch', self.scratch)] + [('go %d' % i, g) for i, g in self.go.items()]:
            assert g.bands_intact(), '%s: the guard bands of %s were written' % (c['name'], name)
        for i in range(k):
            assert want[i] or self.go[i].untouched(), '%s: go %d was not passed, and was written' % (c['name'], i)
        return status, message, dict(y=self.y.t.cpu(), gw=self.gw.t.cpu(), gx=None, go={i: self.go[i].t.cpu() for i in range(k) if want[i]}, gp={})


@pytest.mark.parametrize('name', list(R.MIX_CASES))
def test_mix_directly(name):
    case = R.mix_case(name)
    run = MixRunner(case)
    status, _, first = run.run()
    assert status == (0, 0)
    drop = lambda r: dict(r, go={i: t for i, t in r['go'].items() if i not in case['no_go']})
    r32, r64 = (drop(R.mix_reference(dt, case['outs'], case['w'], case['gy'])) for dt in (torch.float32, torch.float64))
    _budget('mix ' + name, first, r32, r64)
    same_bits(first, run.run()[2], name + ': second call')
    kept = sorted(first['go'])
    if kept:
        same_bits(run.run(drop=kept[0])[2], first, name + ': without go %d' % kept[0])


def _arg(key, value):
    return lambda a: a.__setitem__(key, value)


def _null_operand(a):
    a['outs'][1] = None


MIX_REFUSED = {'K = 0': (_arg('k', 0), 'K=0', 3), 'K = 17': (_arg('k', 17), 'K=17', 3), 'numel = 0': (_arg('numel', 0), 'numel=0', 3),
               'numel % 4': (_arg('numel', 6), 'numel=6', 3), 'null operand list': (_arg('outs', None), 'bad arguments', 3),
               'null weights': (_arg('w', None), 'bad arguments', 3), 'null operand': (_null_operand, 'null operand 1', 3),
               'null y': (_arg('y', None), 'null output', 1), 'null gy': (_arg('gy', None), 'null argument', 2),
               'null gw': (_arg('gw', None), 'null argument', 2), 'null scratch': (_arg('scratch', None), 'null argument', 2)}


@pytest.mark.parametrize('name', list(MIX_REFUSED))
def test_mix_refused_arguments_return_before_any_launch(name):
    edit, needle, which = MIX_REFUSED[name]          # which: 1 = the forward refuses, 2 = the backward, 3 = both
    run = MixRunner(dict(R.mix_case('n4-k16'), numel=8, outs=[torch.rand(8) for _ in range(16)], gy=torch.rand(8), no_go=()))
    status, message, _ = run.run(edit=edit)
    assert [bool(s) for s in status] == [bool(which & 1), bool(which & 2)], '%s: status %s' % (name, status)
    assert 'risp_mix_' in message and needle in message, '%s: "%s" does not name the cause' % (name, message)
    if which & 1:
        assert run.y.untouched(), '%s: y was written' % name
    if which & 2:
        assert run.gw.untouched() and run.scratch.untouched() and all(g.untouched() for g in run.go.values()), '%s: an output was written' % name


# ---------------------------------------------------------------------------------------------------- refusals of the slot
def _set(field, value):
    return lambda d, run: setattr(d, field, value)


def _at(field, k, value):
    return lambda d, run: getattr(d, field).__setitem__(k, value)


def _offset_tensor(d, run):
    d.ptr[1] = run.tensors[0].data_ptr() + 4


def _second_gamma(d, run):                           # the skip becomes a second gamma, block and all
    d.kind[3], d.ptr[3] = KIND_CODE['gamma'], d.ptr[0]


# the valid call: 2 x 4 x 4, [gamma, T, wb_quadratic, skip].  name: (edit, what risp_last_error() must name, 3 = both entry points)
SLOT_REFUSED = {
    'K = 0': (_set('K', 0), 'K=0', 3), 'K = 17': (_set('K', 17), 'K=17', 3), 'HW % 4': (_set('HW', 6), 'HW=6', 3), 'N = 0': (_set('N', 0), 'N=0', 3),
    'two of one kind': (_second_gamma, 'two element-wise operands of kind 3', 3),
    'kind DEMOSAIC_NEAREST': (_at('kind', 3, 1), 'operand 3: kind 1', 3), 'null block': (_at('ptr', 0, None), 'operand 0: null pointer', 3),
    'tensor offset by 4 bytes': (_offset_tensor, 'operand 1 unaligned', 3), 'x == NULL': (_set('x', None), 'need the slot input x', 3),
    'gx == NULL': ('gx', 'null or unaligned argument', 2), 'null y': (_set('y', None), 'null output', 1),
}


@pytest.mark.parametrize('name', ['null descriptor'] + list(SLOT_REFUSED))
def test_slot_refused_arguments_return_before_any_launch(name):
    case = R.build('refusal', R._case((2, 4, 4), ['gamma', T, 'wb_quadratic', 'skip'], 120))
    run = Runner(case)
    run.alloc()
    F, lib = run.F, run.L.load()
    d = run.desc()
    gx = F._p(run.gx.t)
    if name == 'null descriptor':
        status = (lib.risp_slot_mix_fwd(None, F._stream()), lib.risp_slot_mix_bwd(None, F._p(run.gy), gx, F._p(run.gw.t), F._p(run.scratch.t), F._stream()))
        needle, which = 'null descriptor', 3
    else:
        edit, needle, which = SLOT_REFUSED[name]
        if edit == 'gx':
            gx = None
        else:
            edit(d, run)
        status = (lib.risp_slot_mix_fwd(C.byref(d), F._stream()) if which & 1 else 0,
                  lib.risp_slot_mix_bwd(C.byref(d), F._p(run.gy), gx, F._p(run.gw.t), F._p(run.scratch.t), F._stream()) if which & 2 else 0)
    message = lib.risp_last_error().decode()
    torch.cuda.synchronize()
    assert [bool(s) for s in status] == [bool(which & 1), bool(which & 2)], '%s: status %s' % (name, status)
    assert 'risp_slot_mix_' in message and needle in message, '%s: "%s" does not name the cause' % (name, message)
    outputs = [run.y, run.gx, run.gw, run.scratch] + [g for g, _ in run.go.values()] + [g for g, _ in run.gp.values()]
    assert all(g.untouched() for g in outputs), '%s: an output was written' % name
    _budget('after a refusal', run.run(), *R.reference_pair(case))     # and a valid call still goes through
