"""GPU: the autograd Functions of reconfigisp_amd/convnets.py - the four proxy families in every form they take - against float64 over
the case table of tests/net_reference.py, at random weights.  The rule that makes a network gradient testable is stated there: the
float64 referee takes the DEVICE'S OWN ReLU decisions (its saved activations > 0) and statistics indices for the backward pass, and
checks separately that those decisions are legitimate (the forward, every saved activation included, against plain float64; the
indices against their contract, exactly).  Nothing is blanked and no footprint is excluded.

Per case: the launches show the form the row names (``lib.CALLS``); every compared tensor is held to max|got - ref64| / max|ref64| <=
1e-4, the parity bar of BASELINE.json; no NaN; a second forward + backward gives the same bits.  With RISP_BUDGET_REPORT=1 one line
per case and tensor: the device's error, the error of the fp32 CPU restatement of the same graph with the same decisions (the
yardstick - net_reference in float32, never the code under test), the decisions that differ from float64's own, the conv entries
that ran (pytest -s; tools/net_space_budget_report.py condenses them into profiles/net_space_budget.txt)."""
import os

import pytest
import torch

import net_reference as R

pytestmark = pytest.mark.gpu

REPORT = os.environ.get('RISP_BUDGET_REPORT') == '1'
MATRIX_F16 = ('risp_conv2d_f16x2', 'risp_conv2d_thin5', 'risp_conv2d_toep_first', 'risp_conv2d_toep_first_exact', 'risp_conv2d_toep',
              'risp_conv2d_toep_sums', 'risp_conv2d_tapout', 'risp_conv2d_tapout_sums', 'risp_conv2d_narrow3')


def _counted(fn):
    from reconfigisp_amd import lib as L
    L.CALLS = {}
    try:
        out = fn()
        return out, dict(L.CALLS)
    finally:
        L.CALLS = None


def _convs(calls):
    return sum(v for k, v in calls.items() if k.startswith('risp_conv2d') and k != 'risp_conv2d_wgrad')


def _module(kind, wts, P=0):
    from reconfigisp_amd.codes.models.modules import tools_proxy as TP
    cls = {'srcnn_res': TP.ProxyNet, 'srcnn_demosaic': TP.ProxyDemosaicNet, 'path14l_bayer': TP.PathRestore14lBayer,
           'path14l_bgr': TP.PathRestore14lBgr}[kind]
    m = cls(P, None)
    m.load_state_dict(wts)
    return m.cuda()


class _Ledger:
    """the compared tensors of one case: (tensor, device error, fp32 yardstick or None); ``finish`` prints and asserts"""

    def __init__(self, case):
        self.cid, self.rows, self.flips, self.entries = R.case_id(case), [], 0, set()

    def add(self, what, got, ref64, ref32=None):
        assert not torch.isnan(got).any(), '%s: %s holds NaN' % (self.cid, what)
        self.rows.append((what, R.rel_err(got, ref64), R.rel_err(ref32, ref64) if ref32 is not None else None))

    def ran(self, *calls):
        for c in calls:
            self.entries.update(k for k in c if k.startswith('risp_conv2d'))

    def finish(self):
        if REPORT:
            ent = ','.join(sorted(e[len('risp_conv2d'):].lstrip('_') or 'direct' for e in self.entries))
            for what, e, e32 in self.rows:
                print('NETSPACE %s | %s dev %.2e fp32 %s flips %d entries %s' % (
                    self.cid, what.replace(' ', '_'), e, '%.2e' % e32 if e32 is not None else '-', self.flips, ent))
        bad = ['%s %.3e' % (what, e) for what, e, _ in self.rows if not e <= R.BAR]
        assert not bad, '%s: over %.0e of the tensor\'s magnitude against float64 (%d decisions differ from float64\'s own): %s' % (
            self.cid, R.BAR, self.flips, '; '.join(bad))


def _forward_rule(led, tag, kind, x, pv, wts, y, saved):
    """rule 1: ``y`` and every saved post-ReLU activation against the plain float64 evaluation; returns the device's masks"""
    plain = R.evaluate(kind, x, pv, wts)
    p32 = R.evaluate(kind, x, pv, wts, dtype=torch.float32) if REPORT else None
    led.add(tag + 'y', y, plain['y'], p32['y'] if REPORT else None)
    assert len(saved) in (0, R.RELUS[kind]), '%d activations saved for %d ReLUs' % (len(saved), R.RELUS[kind])
    for k, act in enumerate(saved):
        led.add(tag + 'act%d' % k, act, torch.relu(plain['pre'][k]), torch.relu(p32['pre'][k]) if REPORT else None)
    masks = R.masks_of(saved)
    led.flips += R.flips(masks, plain['pre'])
    return masks


def _backward_ref(kind, x, pv, wts, gy, masks, arg=None, weight_grads=False):
    """rule 2: float64 autograd through the network with the device's decisions as constants (and the fp32 yardstick of the same)"""
    ref = R.evaluate(kind, x, pv, wts, gy, masks=masks, arg=arg, weight_grads=weight_grads)
    r32 = R.evaluate(kind, x, pv, wts, gy, masks=masks, arg=arg, weight_grads=weight_grads, dtype=torch.float32) if REPORT else None
    return ref, r32


def _stats_rule(x, arg):
    """rule 3: the saved indices against ``x``, exactly"""
    bad = R.check_arg(x, arg)
    assert not bad, 'saved statistics indices: ' + '; '.join(bad)
    return arg.detach().cpu()


def _same_bits(a, b, what):
    for j, (p, q) in enumerate(zip(a, b)):
        assert (p is None) == (q is None), '%s: tensor %d' % (what, j)
        if p is not None:
            assert torch.equal(p, q), '%s: tensor %d differs in %d elements' % (what, j, int((p != q).sum()))


# ------------------------------------------------------------------------------------------------ SRCNNRes, one member
def _srcnn_res_single(case, led):
    import reconfigisp_amd.functional as F
    from reconfigisp_amd import convnets as CN
    x, (pv,), (wts,), (gy,) = R.case_inputs(case)
    form, P, (h, w) = case['form'], case['P'][0], case['hw']
    m = _module('srcnn_res', wts, P)
    if form == 'train':
        m.train_weights = True
    names = sorted(wts) if form == 'train' else []

    def once():
        xd = x.cuda().requires_grad_(form != 'folded-infer')
        pd = pv.cuda().requires_grad_(form != 'folded-infer') if P else None
        if form == 'plain' and not R.plain_by_dispatch(case):      # the dispatch folds at this size: the Function itself
            packs = F._packs(m, lambda: CN.build_srcnn_packs(m.srcnn, residual=True))
            y, fc = _counted(lambda: CN._SrcnnRes.apply(xd, pd, packs))
        elif form == 'folded-infer':
            with torch.no_grad():
                y, fc = _counted(lambda: m(xd, pd))
            assert y.grad_fn is None and not y.requires_grad
            return y, fc, (), {}, ()
        else:
            y, fc = _counted(lambda: m(xd, pd))
        saved = tuple(t.detach().clone() for t in y.grad_fn.saved_tensors)
        params = dict(m.named_parameters())
        leaves = [xd] + ([pd] if P else []) + [params[k] for k in names]
        grads, bc = _counted(lambda: torch.autograd.grad(y, leaves, gy.cuda()))
        return y.detach(), fc, saved, bc, grads

    y, fc, saved, bc, grads = once()
    led.ran(fc, bc)
    # ---- the form
    if form in ('plain', 'train'):
        assert fc.get('risp_srcnn_cvals') == 1 and 'risp_srcnn_case_table' not in fc, fc
        assert bc.get('risp_stats_bwd') == 1 and 'risp_stats_bwd_rows' not in bc and 'risp_srcnn_const_grad' not in bc, bc
        assert bc.get('risp_conv2d_wgrad', 0) == (3 if form == 'train' else 0), bc
    else:
        assert fc.get('risp_srcnn_case_table') == 1 and 'risp_srcnn_cvals' not in fc, fc
        if form == 'folded':
            assert sum(v for k, v in bc.items() if k.startswith('risp_rect_sums')) == 1 and bc.get('risp_srcnn_const_grad') == 1, bc
            assert bc.get('risp_stats_bwd_rows') == 1 and 'risp_stats_bwd' not in bc and 'risp_conv2d_wgrad' not in bc, bc
    assert _convs(fc) == 3, fc
    if form == 'folded-infer':
        _forward_rule(led, '', 'srcnn_res', x, pv, wts, y, ())
        y2 = once()[0]
        assert torch.equal(y, y2), 'a second forward gives other bits'
        return
    t1, t2, arg = saved[-3:]                                       # (the train form also keeps x and the constants)
    masks = _forward_rule(led, '', 'srcnn_res', x, pv, wts, y, (t1, t2))
    arg = _stats_rule(x, arg)
    ref, r32 = _backward_ref('srcnn_res', x, pv, wts, gy, masks, arg, form == 'train')
    rest = list(grads)
    led.add('gx', rest.pop(0), ref['gx'], r32['gx'] if REPORT else None)
    if P:
        led.add('gpv', rest.pop(0), ref['gpv'], r32['gpv'] if REPORT else None)
    for k, g in zip(names, rest):
        led.add('g ' + k, g, ref['gw'][k], r32['gw'][k] if REPORT else None)
    again = once()
    _same_bits((y,) + tuple(saved) + tuple(grads), (again[0],) + tuple(again[2]) + tuple(again[4]), 'a second forward + backward')


# ------------------------------------------------------------------------------------------------ SRCNNRes groups
def _srcnn_res_group(case, led):
    import reconfigisp_amd.functional as F
    from reconfigisp_amd import convnets as CN
    x, pvs, wts, gys = R.case_inputs(case)
    n, G = case['n'], case['members']
    mods = [_module('srcnn_res', wts[j], p) for j, p in enumerate(case['P'])]
    assert F.can_group(mods, x.cuda())

    def run(grouped, flags=None, leave_out=None):
        CN.GROUP_LAUNCH = grouped
        try:
            xd = x.cuda().requires_grad_(True)
            pd = [p.cuda().requires_grad_(True) for p in pvs]
            outs, fc = _counted(lambda: F.srcnn_res_group(xd, pd, mods, dict(flags or {})))
            saved = tuple(t.detach().clone() for t in outs[0].grad_fn.saved_tensors)
            use = [j for j in range(G) if j != leave_out]
            grads, bc = _counted(lambda: torch.autograd.grad([outs[j] for j in use], [xd] + pd, [gys[j].cuda() for j in use], allow_unused=True))
            return [o.detach() for o in outs], saved, grads, fc, bc
        finally:
            CN.GROUP_LAUNCH = True

    outs, saved, grads, fc, bc = run(True)
    led.ran(fc, bc)
    assert fc.get('risp_srcnn_case_table_group') == 1 and fc.get('risp_channel_stats') == 1 and _convs(fc) == 3, fc
    assert bc.get('risp_srcnn_const_grad_group') == 1 and bc.get('risp_group_sum') == 1 and _convs(bc) == 3, bc
    assert 'risp_stats_bwd' not in bc and 'risp_stats_bwd_rows' not in bc, bc
    t1, t2, arg, xs = saved
    assert torch.equal(xs.cpu(), x)
    arg = _stats_rule(x, arg)                           # of the shared input: once for the whole group
    refs = []
    for j in range(G):
        s = slice(j * n, (j + 1) * n)
        masks = _forward_rule(led, 'm%d ' % j, 'srcnn_res', x, pvs[j], wts[j], outs[j], (t1[s], t2[s]))
        ref, r32 = _backward_ref('srcnn_res', x, pvs[j], wts[j], gys[j], masks, arg)
        refs.append((ref, r32))
        led.add('m%d gpv' % j, grads[1 + j], ref['gpv'], r32['gpv'] if REPORT else None)
    total = lambda k, skip=None: sum(r[k]['gx'] for j, r in enumerate(refs) if j != skip)
    led.add('gx', grads[0], total(0), total(1) if REPORT else None)
    # ---- the members launched one by one: the bits are pinned equal, so the comparison above covers them
    o2, s2, g2, fc2, bc2 = run(False)
    assert _convs(fc2) == 3 * G and _convs(bc2) == 3 * G and bc2.get('risp_group_sum') == 1, (fc2, bc2)
    _same_bits(outs + list(saved) + list(grads), o2 + list(s2) + list(g2), 'GROUP_LAUNCH off')
    _same_bits(outs + list(grads), (lambda r: r[0] + list(r[2]))(run(True)), 'a second forward + backward')
    # ---- nobody consumes the input gradient: none is computed, every parameter gradient keeps its bits (the member-by-member form
    #      is a diagnostic and keeps computing it: only its parameter gradients are held)
    _, _, g3, _, bc3 = run(True, flags={'skip_gx': True})
    assert g3[0] is None and 'risp_group_sum' not in bc3 and _convs(bc3) == 2, bc3
    _same_bits(grads[1:], g3[1:], 'skip_gx')
    _same_bits(grads[1:], run(False, flags={'skip_gx': True})[2][1:], 'skip_gx, GROUP_LAUNCH off')
    # ---- one member outside the loss: zeros upstream, exactly zero parameter gradient, gx = the sum of the others
    out = G // 2
    _, _, g4, _, _ = run(True, leave_out=out)
    assert g4[1 + out] is not None and not g4[1 + out].any(), 'the member outside the loss has a parameter gradient'
    for j in range(G):
        if j != out:
            led.add('without m%d: m%d gpv' % (out, j), g4[1 + j], refs[j][0]['gpv'], refs[j][1]['gpv'] if REPORT else None)
    led.add('without m%d: gx' % out, g4[0], total(0, out), total(1, out) if REPORT else None)


# ------------------------------------------------------------------------------------------------ SRCNNDemosaic
def _srcnn_demosaic(case, led):
    import reconfigisp_amd.functional as F
    from reconfigisp_amd import convnets as CN
    x, _, wts, gys = R.case_inputs(case)
    n, G, form = case['n'], case['members'], case['form']
    infer, group = form.endswith('infer'), form.startswith('group')
    mods = [_module('srcnn_demosaic', w) for w in wts]
    assert not group or F.can_group(mods, x.cuda())

    def run(grouped=True):
        CN.GROUP_LAUNCH = grouped
        try:
            xd = x.cuda().requires_grad_(not infer)
            fwd = (lambda: F.srcnn_demosaic_group(xd, mods, {})) if group else (lambda: [mods[0](xd, None)])
            if infer:
                with torch.no_grad():
                    outs, fc = _counted(fwd)
                assert all(o.grad_fn is None and not o.requires_grad for o in outs)
                return [o.detach() for o in outs], (), None, fc, {}
            outs, fc = _counted(fwd)
            saved = tuple(t.detach().clone() for t in outs[0].grad_fn.saved_tensors)
            (gx,), bc = _counted(lambda: torch.autograd.grad(outs, xd, [g.cuda() for g in gys]))
            return [o.detach() for o in outs], saved, gx, fc, bc
        finally:
            CN.GROUP_LAUNCH = True

    outs, saved, gx, fc, bc = run()
    led.ran(fc, bc)
    assert _convs(fc) == 3, fc
    if not infer:
        assert _convs(bc) == 3 and bc.get('risp_group_sum', 0) == (1 if group else 0), bc
    total = [0, 0]
    for j in range(G):
        s = slice(j * n, (j + 1) * n)
        masks = _forward_rule(led, 'm%d ' % j if group else '', 'srcnn_demosaic', x, None, wts[j], outs[j],
                              () if infer else (saved[0][s], saved[1][s]))
        if not infer:
            ref, r32 = _backward_ref('srcnn_demosaic', x, None, wts[j], gys[j], masks)
            total = [total[0] + ref['gx'], total[1] + r32['gx'] if REPORT else None]
    if not infer:
        if group:
            assert torch.equal(saved[2].cpu(), x)
        led.add('gx', gx, total[0], total[1])
    again = run()
    _same_bits(outs + [gx], again[0] + [again[2]], 'a second forward + backward')
    if group:
        o2, s2, gx2, fc2, bc2 = run(False)
        assert _convs(fc2) == 3 * G and (infer or _convs(bc2) == 3 * G), (fc2, bc2)
        _same_bits(outs + list(saved) + [gx], o2 + list(s2) + [gx2], 'GROUP_LAUNCH off')


# ------------------------------------------------------------------------------------------------ Path-Restore 14l
def _path14l(case, led, monkeypatch):
    from reconfigisp_amd import convnets as CN
    monkeypatch.setattr(CN, 'CONV_ARITH', case['arith'])
    kind, form = case['kind'], case['form']
    x, _, (wts,), (gy,) = R.case_inputs(case)
    h, w = case['hw'] if kind == 'path14l_bgr' else (case['hw'][0] // 2, case['hw'][1] // 2)
    m = _module(kind, wts)

    def arith_rule(calls, n_wide):
        assert _convs(calls) == n_wide + 2, calls
        if case['arith'] == 'f32':
            assert not any(k in calls for k in MATRIX_F16), calls
        elif w % 4 == 0:
            assert calls.get('risp_conv2d_f16x2') == n_wide, calls
        else:
            assert 'risp_conv2d_f16x2' not in calls, calls

    def once(record=None):
        if record is not None:
            m.__dict__['_risp_reuse'] = record
        try:
            xd = x.cuda().requires_grad_(form != 'infer')
            if form == 'infer':
                with torch.no_grad():
                    y, fc = _counted(lambda: m(xd, None))
                assert y.grad_fn is None and not y.requires_grad
                return xd, y, fc
            y, fc = _counted(lambda: m(xd, None))
            return xd, y, fc
        finally:
            m.__dict__.pop('_risp_reuse', None)

    def back(xd, y, g):
        saved = tuple(t.detach().clone() for t in y.grad_fn.saved_tensors)
        (gx,), bc = _counted(lambda: torch.autograd.grad(y, xd, g.cuda()))
        return saved, gx, bc

    if form == 'infer':
        _, y, fc = once()
        led.ran(fc)
        arith_rule(fc, 12)
        _forward_rule(led, '', kind, x, None, wts, y, ())
        assert torch.equal(y, once()[1]), 'a second forward gives other bits'
        return
    if form == 'grad':
        xd, y, fc = once()
        saved, gx, bc = back(xd, y, gy)
        led.ran(fc, bc)
        arith_rule(fc, 12)
        arith_rule(bc, 12)
        masks = _forward_rule(led, '', kind, x, None, wts, y.detach(), saved)
        ref, r32 = _backward_ref(kind, x, None, wts, gy, masks)
        led.add('gx', gx, ref['gx'], r32['gx'] if REPORT else None)
        xd2, y2, _ = once()
        s2, gx2, _ = back(xd2, y2, gy)
        _same_bits((y.detach(), gx) + saved, (y2.detach(), gx2) + s2, 'a second forward + backward')
        return
    # ---- 'reuse': the second forward with the record filled launches nothing and returns the same bits; each of the two nodes
    #      differentiates with its own upstream gradient
    rec = {}
    xa, ya, fca = once(rec)
    assert 'y' in rec and len(rec['saved']) == 13
    xb, yb, fcb = once(rec)
    led.ran(fca)
    arith_rule(fca, 12)
    assert fcb == {}, 'the second forward launched %s' % fcb
    assert torch.equal(ya, yb) and ya.grad_fn is not yb.grad_fn
    masks = _forward_rule(led, '', kind, x, None, wts, ya.detach(), tuple(rec['saved']))
    gy2 = R.make_gy(gy.shape, 77)
    for tag, xd, y, g in (('node 1 ', xa, ya, gy), ('node 2 ', xb, yb, gy2)):
        saved, gx, bc = back(xd, y, g)
        _same_bits(saved, tuple(rec['saved']), tag + 'saved activations')
        arith_rule(bc, 12)
        ref, r32 = _backward_ref(kind, x, None, wts, g, masks)
        led.add(tag + 'gx', gx, ref['gx'], r32['gx'] if REPORT else None)


@pytest.mark.parametrize('hw', [153, 1001, 70003, 1024, 70004])
@pytest.mark.parametrize('rows', [False, True])
def test_stats_bwd_both_forms(hw, rows):
    """risp_stats_bwd / risp_stats_bwd_rows on planes of any size: the element-wise form (H W % 4 != 0, or a gradient that does not
    start on 16 bytes) beside the vector one - one block, a ragged last block, more than the 64 blocks of a plane's grid.  Both
    do the same three fp32 additions per element in the same order, so they are held to the fp32 restatement bit for bit, and at
    H W % 4 == 0 to each other through an unaligned view."""
    import ctypes as C
    from reconfigisp_amd import lib as L
    from reconfigisp_amd.functional import _p, _stream
    n, c, row = 2, 3, 11
    g = torch.Generator().manual_seed(hw)
    gx = torch.randn((n * c, hw), generator=g)
    gstat = torch.randn((n, row), generator=g)           # columns 0-2 / 3-5 / 6-8: min, mean, max (the folded backward's layout)
    arg = torch.stack([torch.randint(0, hw, (n * c,), generator=g), torch.randint(0, hw, (n * c,), generator=g)], dim=1).to(torch.int32)
    arg[0] = torch.tensor([hw - 1, hw - 1])             # the last element, min and max on one pixel
    arg[1] = torch.tensor([0, hw - 1])
    col = lambda k: gstat[:, k:k + c].reshape(-1).contiguous()       # plane n * C + c reads gstat[n, k + c]
    inv_hw = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(hw), dtype=torch.float32)
    want = gx + (col(3) * inv_hw)[:, None]
    idx = torch.arange(n * c)
    want[idx, arg[:, 0].long()] += col(0)
    want[idx, arg[:, 1].long()] += col(6)

    def run(offset):
        buf = torch.zeros(n * c * hw + 4, device='cuda')
        view = buf[offset:offset + n * c * hw].view(n * c, hw)
        view.copy_(gx)
        argd = arg.cuda()
        if rows:
            gs = gstat.cuda()
            base = gs.data_ptr()
            L.call('risp_stats_bwd_rows', _p(view), C.c_void_p(base), C.c_void_p(base + 12), C.c_void_p(base + 24), _p(argd), n, c, hw,
                   row, _stream())
        else:
            cols = [col(k).cuda() for k in (0, 3, 6)]
            L.call('risp_stats_bwd', _p(view), _p(cols[0]), _p(cols[1]), _p(cols[2]), _p(argd), n * c, hw, _stream())
        torch.cuda.synchronize()
        assert not buf[:offset].any() and not buf[offset + n * c * hw:].any(), 'a write outside the planes'
        return view.cpu()

    got = run(0)
    assert torch.equal(got, want), '%d elements differ, max %g' % (int((got != want).sum()), float((got - want).abs().max()))
    assert torch.equal(run(1), want), 'the unaligned view'


@pytest.mark.parametrize('case', R.CASES, ids=R.case_id)
def test_network_against_float64(case, monkeypatch):
    led = _Ledger(case)
    if case['kind'] == 'srcnn_res':
        (_srcnn_res_group if case['form'] == 'group' else _srcnn_res_single)(case, led)
    elif case['kind'] == 'srcnn_demosaic':
        _srcnn_demosaic(case, led)
    else:
        _path14l(case, led, monkeypatch)
    led.finish()
