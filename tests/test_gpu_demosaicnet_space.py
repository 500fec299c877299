"""GPU: DemosaicNet (convnets._DemosaicNet, risp_dmnet.hip, demosaicnet.fold) against float64 over the case table of
tests/demosaicnet_reference.py, at random weights - the fifth network under the rule of tests/test_gpu_net_space.py: the float64
referee takes the DEVICE'S OWN ReLU decisions (its saved activations > 0) for the backward pass and checks separately that they are
legitimate (the output, every saved activation and ``up`` against plain float64).  The head's hidden ReLU is the one decision the
device does not save; the referee takes it in float64 from the device's saved ``up``, and a unit within TAU_HEAD of zero is
enumerated - either side is legitimate, at most MAX_UNDECIDED per case (``demosaicnet_reference.judge``).  Nothing is blanked.

Per 'grad' row: the launches are the ones ``expected_entries`` names (``lib.CALLS``); every compared tensor is held to
max|got - ref64| / max|ref64| <= 1e-4, the bar of BASELINE.json; no NaN; a second forward + backward gives the same bits; image k
alone gives the bits of image k in the batch.  'infer' rows save nothing: the output against float64, repeated and per image.  (The
bits of an inference output are NOT compared with the 'grad' form's: no test of the project promises that.)  'reuse' rows: the second
forward with a filled record launches nothing and returns the same bits, and so do both backward passes.  Every row also holds the
output to the released network ``reference`` in float64 (cfa='grbg': on the x-mirrored mosaic, mirrored back, as
tests/test_demosaicnet_cpu.py states the fold).  Kernel rows: the four risp_dmnet_* launches on their own at the bar
tests/test_gpu_demosaicnet.py holds them to, 1e-5 of the reference's RMS, every pixel compared.

With RISP_BUDGET_REPORT=1 one line per row and tensor: the device's error, the error of the fp32 CPU restatement with the same
decisions (the yardstick, never the code under test), the decisions that differ from float64's own, the undecided head units
(pytest -s; tools/demosaicnet_budget_report.py condenses them into profiles/demosaicnet_space_budget.txt)."""
import ctypes as C
import os

import pytest
import torch

import demosaicnet_reference as R

pytestmark = pytest.mark.gpu

REPORT = os.environ.get('RISP_BUDGET_REPORT') == '1'
KERNEL_BAR = 1e-5                                    # of the reference's RMS (tests/test_gpu_demosaicnet.py)


def _counted(fn):
    from reconfigisp_amd import lib as L
    L.CALLS = {}
    try:
        out = fn()
        return out, dict(L.CALLS)
    finally:
        L.CALLS = None


def _convs(calls):
    """the risp_conv2d* launches, the two entries of the vector kernel under one name"""
    out = {}
    for k, v in calls.items():
        if k.startswith('risp_conv2d'):
            k = 'risp_conv2d_small' if k == 'risp_conv2d_small_split' else k
            out[k] = out.get(k, 0) + v
    return out


def _others(calls):
    """the launches of risp_dmnet.hip (a first forward also builds weight packs)"""
    return {k: v for k, v in calls.items() if k.startswith('risp_dmnet')}


def _same_bits(a, b, what):
    assert len(a) == len(b), what
    for j, (p, q) in enumerate(zip(a, b)):
        assert torch.equal(p, q), '%s: tensor %d differs in %d elements' % (what, j, int((p != q).sum()))


class _Ledger:
    def __init__(self, case):
        self.cid, self.rows, self.flips, self.undecided, self.entries = R.case_id(case), [], 0, 0, set()

    def take(self, res, tag=''):
        self.rows += [(tag + what, e, e32) for what, e, e32 in res['rows']]
        self.flips, self.undecided = max(self.flips, res['flips']), max(self.undecided, res['undecided'])

    def finish(self, bar=R.BAR):
        if REPORT:
            ent = ','.join(sorted(e[len('risp_conv2d'):].lstrip('_') or 'direct' for e in self.entries)) or '-'
            for what, e, e32 in self.rows:
                print('DMSPACE %s | %s dev %.2e fp32 %s flips %d undecided %d entries %s' % (
                    self.cid, what.replace(' ', '_'), e, '%.2e' % e32 if e32 is not None else '-', self.flips, self.undecided, ent))
        bad = ['%s %.3e' % (what, e) for what, e, _ in self.rows if not e <= bar]
        assert not bad, '%s: over %.0e against float64 (%d decisions differ from float64\'s own, %d head units undecided): %s' % (
            self.cid, bar, self.flips, self.undecided, '; '.join(bad))


def _released(x, sd, cfa, dtype=torch.float64):
    """the released network on the fp32 mosaic: what ``load_demosaicnet(sd, cfa)`` computes"""
    x, sd = x.to(dtype), R.as_dtype(sd, dtype)
    return R.reference(x, sd) if cfa == 'rggb' else R.reference(x.flip(3), sd, 'grbg').flip(3)


@pytest.mark.parametrize('case', R.CASES, ids=R.case_id)
def test_network_against_float64(case, monkeypatch):
    import reconfigisp_amd.functional as F
    from reconfigisp_amd import convnets as CN
    from reconfigisp_amd import demosaicnet as DN
    monkeypatch.setattr(CN, 'CONV_ARITH', case['arith'])
    form, n = case['form'], case['n']
    sd, fd, x, gy = R.case_inputs(case)
    net = DN.load_demosaicnet(sd, case['cfa'])
    assert net.cfa == case['cfa'] and all(torch.equal(net.folded[k].double(), v) for k, v in fd.items())
    led = _Ledger(case)

    def forward(xs, record=None):
        xd = xs.cuda().requires_grad_(form != 'infer')
        if form == 'infer':
            with torch.no_grad():
                y, fc = _counted(lambda: F.demosaicnet(xd, net))
            assert y.grad_fn is None and not y.requires_grad
        else:
            y, fc = _counted(lambda: F.demosaicnet(xd, net, record))
        return xd, y, fc

    def backward(xd, y, g):
        saved = tuple(t.detach().clone() for t in y.grad_fn.saved_tensors)
        (gx,), bc = _counted(lambda: torch.autograd.grad(y, xd, g.cuda()))
        return saved, gx, bc

    def launches(fc, bc=None):
        led.entries.update(_convs(fc), _convs(bc or {}))
        assert _convs(fc) == R.expected_calls(case), (fc, R.expected_entries(case))
        assert _others(fc) == {'risp_dmnet_tail_fwd': 1, 'risp_dmnet_head_fwd': 1}, fc
        if bc is not None:
            assert _convs(bc) == R.expected_calls(case, backward=True), (bc, R.expected_entries(case))
            assert _others(bc) == {'risp_dmnet_head_bwd': 1, 'risp_dmnet_tail_bwd': 1}, bc

    def clean(*ts):
        for t in ts:
            assert not torch.isnan(t).any(), '%s: NaN' % led.cid

    if form == 'infer':
        _, y, fc = forward(x)
        launches(fc)
        clean(y)
        led.take(R.judge(x, fd, {'y': y}, yardstick=REPORT))
        assert torch.equal(y, forward(x)[1]), 'a second forward gives other bits'
        for k in range(n):
            assert torch.equal(y[k:k + 1], forward(x[k:k + 1].clone())[1]), 'image %d alone gives other bits' % k
    elif form == 'grad':
        def once(xs, gs):
            xd, y, fc = forward(xs)
            saved, gx, bc = backward(xd, y, gs)
            return (y.detach(), gx) + saved, fc, bc
        out, fc, bc = once(x, gy)
        launches(fc, bc)
        y, gx, saved = out[0], out[1], out[2:]
        clean(*out)
        assert len(saved) == 18 and torch.equal(saved[0].cpu(), x)
        led.take(R.judge(x, fd, {'y': y, 'saved': saved, 'gx': gx}, gy, yardstick=REPORT))
        _same_bits(out, once(x, gy)[0], 'a second forward + backward')
        for k in range(n if n > 1 else 0):
            alone = once(x[k:k + 1].clone(), gy[k:k + 1].clone())[0]
            _same_bits([t[k:k + 1] for t in out], alone, 'image %d alone' % k)
    else:
        rec = {}
        xa, ya, fca = forward(x, rec)
        assert 'y' in rec and len(rec['saved']) == 18
        xb, yb, fcb = forward(x, rec)
        launches(fca)
        assert fcb == {}, 'the second forward launched %s' % fcb
        assert torch.equal(ya, yb) and ya.grad_fn is not yb.grad_fn
        sa, ga, bca = backward(xa, ya, gy)
        sb, gb, bcb = backward(xb, yb, gy)
        launches(fca, bca)
        launches(fca, bcb)
        clean(ya, ga, *sa)
        _same_bits((ga,) + sa, (gb,) + sb, 'the two nodes of one record')
        _same_bits(sa, tuple(rec['saved']), 'the record')
        xc, yc, _ = forward(x)                                         # ... and without a record
        sc, gc, _ = backward(xc, yc, gy)
        _same_bits((ya.detach(), ga) + sa, (yc.detach(), gc) + sc, 'with and without a record')
        y = ya.detach()
        led.take(R.judge(x, fd, {'y': y, 'saved': sa, 'gx': ga}, gy, yardstick=REPORT))
    released = _released(x, sd, case['cfa'])
    led.rows.append(('y against the released network', R.rel_err(y, released),
                     R.rel_err(_released(x, sd, case['cfa'], torch.float32), released) if REPORT else None))
    led.finish()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _rms_err(got, ref):
    """max|got - ref| relative to the RMS of ref"""
    got, ref = got.detach().double().cpu(), ref.detach().double()
    assert tuple(got.shape) == tuple(ref.shape) and not torch.isnan(got).any()
    return float((got - ref).abs().max() / ref.pow(2).mean().sqrt())


def _kernel_refs(k, dtype):
    """the four stages in ``dtype`` on the CPU (autograd through ``relu``: no hidden unit of these inputs is undecided)"""
    fd = R.as_dtype(k['fd'], dtype)
    fa, fb = (k[name].to(dtype).requires_grad_(True) for name in ('fa', 'fb'))
    up_t = R.tail(fa, fb, fd)
    ra, rb = torch.autograd.grad(up_t, (fa, fb), k['gup'].to(dtype))
    x, up = (k[name].to(dtype).requires_grad_(True) for name in ('x', 'up'))
    y = R.head(x, up, fd)
    rx, rup = torch.autograd.grad(y, (x, up), k['gy'].to(dtype))
    return {'tail up': up_t.detach(), 'tail g_filt': ra * (fa > 0), 'tail g_mask': rb * (fb > 0), 'head y': y.detach(),
            'head g_up': rup, 'head g_x': rx}


@pytest.mark.parametrize('case', R.KERNEL_CASES, ids=R.case_id)
def test_kernels_against_float64(case):
    from reconfigisp_amd import lib as L
    from reconfigisp_amd.functional import _stream
    n, (h, w) = case['n'], case['hw']
    k = R.kernel_inputs(case)
    cuda = lambda t: t.float().contiguous().cuda()
    d = {name: cuda(v) for name, v in k['fd'].items()}
    fa, fb, x, up, gy, gup, add = (cuda(k[name]) for name in ('fa', 'fb', 'x', 'up', 'gy', 'gup', 'add'))
    got = {'tail up': torch.empty(n, 3, h, w, device='cuda'), 'tail g_filt': torch.empty_like(fa), 'tail g_mask': torch.empty_like(fb),
           'head y': torch.empty(n, 3, h, w, device='cuda'), 'head g_up': torch.empty_like(up), 'head g_x': torch.empty_like(x)}
    L.call('risp_dmnet_tail_fwd', _p(fa), _p(fb), _p(d['rp.weight']), _p(d['rp.bias']), _p(d['up.weight']), _p(d['up.bias']),
           _p(got['tail up']), n, h, w, _stream())
    L.call('risp_dmnet_tail_bwd', _p(gup), _p(fa), _p(fb), _p(d['rp.weight']), _p(d['up.weight']), _p(got['tail g_filt']),
           _p(got['tail g_mask']), n, h, w, _stream())
    L.call('risp_dmnet_head_fwd', _p(x), _p(up), _p(d['post.weight']), _p(d['post.bias']), _p(d['out.weight']), _p(d['out.bias']),
           _p(got['head y']), n, h, w, _stream())
    g_up2, g_x2 = torch.empty_like(up), torch.empty_like(x)
    for a, gu, gxo in ((None, got['head g_up'], got['head g_x']), (add, g_up2, g_x2)):
        L.call('risp_dmnet_head_bwd', _p(gy), _p(x), _p(up), _p(d['post.weight']), _p(d['post.bias']), _p(d['out.weight']), _p(a),
               _p(gu), _p(gxo), n, h, w, _stream())
    ref = _kernel_refs(k, torch.float64)
    r32 = _kernel_refs(k, torch.float32) if REPORT else None
    led = _Ledger(case)
    for name in got:
        led.rows.append((name, _rms_err(got[name], ref[name]), _rms_err(r32[name], ref[name]) if REPORT else None))
    led.rows.append(('head g_x with add', _rms_err(g_x2, k['add'] + ref['head g_x']),
                     _rms_err(k['add'].float() + r32['head g_x'], k['add'] + ref['head g_x']) if REPORT else None))
    assert torch.equal(g_x2, add + got['head g_x']), 'add + the direct term, in that order'
    assert torch.equal(g_up2, got['head g_up']), 'g_up depends on add'
    led.finish(KERNEL_BAR)
