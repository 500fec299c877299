"""GPU: ``convnets.conv`` - the dispatch every wide layer of the four proxy families goes through, forward and backward-data - over its
argument space, against float64.

The table, the seeded walk, the float64 restatement, the float32 yardstick and what each of the eight entry points accepts are
tests/conv_reference.py (plain CPU code, checked by tests/test_conv_reference_cpu.py).  Every case goes through ``CN.conv`` into ``out=``,
a view inside a NaN-filled buffer between guard bands (tests/guarded.py), with ``L.call`` recorded, and is held to

  1. entry: exactly one risp_conv2d* launch, the case's literal expectation and what ``route`` names; that entry's own conditions
     (``ENTRY_ACCEPTS``) accept the launch; the descriptor carries the case's epilogue; ``_have`` is ``pack_kinds``;
  2. writes: every output element written, both guard bands untouched (PixelShuffle stores into the (N, cout / 4, 2 H, 2 W) shape);
  3. accuracy, relative to max|ref64|: the split-precision entries to the bar of their own file (f16x2 5e-6, thin5 2e-6, the two first-layer
     entries 3e-6); the fp32 entries, which have no bar of their own, to conftest.ErrorBudget's rule against the CPU float32 yardstick of
     their algorithm class, e_gpu <= min(2 * E32, 1e-4) + 4e-6; and ``assert_close`` with conftest's defaults;
  4. exact zeros: 0.0 wherever mask <= 0; under a ReLU nothing negative, and no -0.0 where float64 is clearly negative;
  5. determinism: a second call gives the same bits.

Contracts, one test each: a grouped launch equals its per-member launches bit for bit and launches the same entry; an inference result
does not depend on the batch; ``add=`` without EPI_ADD is refused; a NaN in x stays within the reach of the filter; refused arguments
raise on the host and write nothing.  RISP_BUDGET_REPORT=1 prints one line per case (tools/conv_budget_report.py)."""
import os

import pytest
import torch

import conv_reference as R
from conftest import assert_close
from conv_reference import ADD, MASK, RELU, TF1, TF1X, THIN5, W43, W45
from guarded import Guarded, off16

pytestmark = pytest.mark.gpu

REPORT = os.environ.get('RISP_BUDGET_REPORT') == '1'


@pytest.fixture
def calls(monkeypatch):
    """the conv launches of ``conv``, as tests/test_gpu_conv_modes.py::test_conv_launches_what_route_says records them"""
    from reconfigisp_amd import convnets as CN, lib as L
    rec, real = [], L.call

    def spy(name, *a):
        if name.startswith('risp_conv2d'):
            rec.append((name, a))
        return real(name, *a)
    monkeypatch.setattr(CN.L, 'call', spy)
    return rec


def switches(monkeypatch, case):
    from reconfigisp_amd import convnets as CN
    monkeypatch.setattr(CN, 'CONV_ARITH', case['arith'])
    monkeypatch.setattr(CN, 'TOEP_FIRST', case['toep'])


def packs(case):
    """the members' ``PackedConv`` objects of a case (the FORWARD layer: a backward-data case hands its weight over as it is)"""
    from reconfigisp_amd import convnets as CN
    d = R.inputs(case)
    return [CN.PackedConv(w.cuda(), b.cuda()) for w, b in zip(d['weights'], d['bias'])]


def device_inputs(case):
    """x, cvals, add, mask on the device; the tensor the case names as a view 4 bytes off 16"""
    d = R.inputs(case)
    t = {k: d[k].cuda() if d[k] is not None else None for k in ('x', 'cvals', 'add', 'mask')}
    if case['misalign'] in t:
        t[case['misalign']] = off16(t[case['misalign']])
        assert t[case['misalign']].data_ptr() % 16 == 4
    return t


def launch(case, pc, t, out=None, n=None, group=None):
    from reconfigisp_amd import convnets as CN
    if out is None:
        out = Guarded(*R.out_shape(case), off=1 if case['misalign'] == 'out' else 0)
    CN.conv(t['x'], pc, case['n'] if n is None else n, case['h'], case['w'], transpose=case['transpose'], load=case['load'],
            cin_img=case['cin_img'], cvals=t['cvals'], epi=case['epi'], add=t['add'], add_c=case['add_c'], mask=t['mask'],
            out=out.t if isinstance(out, Guarded) else out, infer=case['infer'], group=group)
    torch.cuda.synchronize()
    return out


def errors(y, ref):
    m = ref.abs().max().item() or 1.0
    e = y.double().cpu() - ref
    return e.pow(2).mean().sqrt().item() / m, e.abs().max().item() / m


def check_entry(case, rec, pc):
    """the entry of the one conv launch recorded, held to the route, the expectation, the entry's own conditions and the descriptor"""
    from reconfigisp_amd import convnets as CN
    assert len(rec) == 1, [r[0] for r in rec]
    entry, args = rec[0]
    d = args[0]._obj                                                  # the ConvDesc behind byref
    assert entry == R.routed(case), (case['name'], entry, R.routed(case))
    if case['expect'] is not None:
        assert entry == case['expect'], (case['name'], entry, case['expect'])
    assert R.ENTRY_ACCEPTS[entry](R.launch_of(case, wpack_gs=d.wpack_gs)), (case['name'], entry)
    G = case['group'] or 1
    assert (d.N, d.H, d.W, d.cin, d.cout, d.ksize) == (G * case['n'], case['h'], case['w'], case['cin'], case['cout'], case['k'])
    assert (d.epilogue, d.add_c, d.load_mode, d.cin_img) == (R.launch_epi(case), case['add_c'], case['load'], case['cin_img'])
    assert (d.group_n, d.group_flags) == ((case['n'], case['gflags']) if case['group'] else (0, 0))
    if not case['group']:
        assert CN._have(pc, case['transpose']) == CN.pack_kinds(*R.layer_of(case), case['transpose'])
    return entry


def check_output(case, entry, out, tag='CONVSPACE'):
    """writes, accuracy and exact zeros of a launch"""
    name = case['name']
    assert tuple(out.t.shape) == R.out_shape(case)
    assert out.bands_intact(), '%s: the guard bands were written' % name
    assert not torch.isnan(out.t).any().item(), '%s: output elements left unwritten' % name
    ref = R.ref64(case)
    rms, mx = errors(out.t, ref)
    e32 = R.E32(case, entry)
    bound = R.bound(entry, e32)
    if REPORT:
        print('%s %-72s | %-28s rms %.3e max %.3e E32 %.3e bound %.3e ratio %.2f' % (tag, name, entry, rms, mx, e32, bound, mx / e32))
    assert mx <= bound, '%s on %s: max error %.3e of max|ref| (rms %.3e), bound %.3e (float32 yardstick %.3e)' % (name, entry, mx, rms, bound, e32)
    assert_close(out.t, ref, what=name)
    y = out.t.cpu()
    if case['epi'] & MASK:
        dead = R.inputs(case)['mask'] <= 0
        assert dead.any() and (y[dead] == 0).all() and not torch.signbit(y[dead]).any(), '%s: not exactly 0.0 where mask <= 0' % name
    if case['epi'] & RELU:
        assert not (y < 0).any(), '%s: negative outputs after the ReLU' % name
        clearly = R.pre64(case) < -bound * (ref.abs().max().item() or 1.0)
        assert clearly.any() and (y[clearly] == 0).all() and not torch.signbit(y[clearly]).any(), '%s: -0.0 or more where float64 is negative' % name


@pytest.mark.parametrize('name', sorted(R.ALL))
def test_case(name, calls, monkeypatch):
    case = R.ALL[name]
    switches(monkeypatch, case)
    pc, t = packs(case)[0], device_inputs(case)
    out = launch(case, pc, t)
    entry = check_entry(case, calls, pc)
    check_output(case, entry, out)
    again = launch(case, pc, t)
    assert calls[1][0] == entry and again.bands_intact() and torch.equal(out.t, again.t), '%s: a second call gives other bits' % name


@pytest.mark.parametrize('name', sorted(R.GROUPED))
def test_grouped_launch_equals_its_per_member_launches(name, calls, monkeypatch):
    """conv(..., group=(G, flags)) on ``stack_packed`` layers against the members' own calls: the same entry point, the same bits, and
    the float64 restatement within the entry's bound"""
    from reconfigisp_amd import convnets as CN
    case = R.GROUPED[name]
    switches(monkeypatch, case)
    G, n, fl = case['group'], case['n'], case['gflags']
    pcs, t = packs(case), device_inputs(case)
    stacked = CN.stack_packed(pcs)
    out = launch(case, stacked, t, group=(G, fl))
    entry = check_entry(case, calls, stacked)
    check_output(case, entry, out, tag='CONVSPACE')
    again = launch(case, stacked, t, group=(G, fl))
    assert torch.equal(out.t, again.t), '%s: a second call gives other bits' % name
    del calls[:]
    members = Guarded(*R.out_shape(case))
    for g in range(G):
        s = slice(g * n, (g + 1) * n)
        tm = dict(x=t['x'] if fl & R.SHARED_X else t['x'][s], cvals=t['cvals'][s] if t['cvals'] is not None else None,
                  add=None if t['add'] is None else t['add'] if fl & R.SHARED_ADD else t['add'][s], mask=t['mask'][s] if t['mask'] is not None else None)
        launch(case, pcs[g], tm, out=members.t[s])
    assert [c[0] for c in calls] == [entry] * G, '%s: the grouped launch runs %s, its members %s' % (name, entry, [c[0] for c in calls])
    assert members.bands_intact() and torch.equal(out.t, members.t), '%s: the per-member launches give other bits' % name


@pytest.mark.parametrize('name', sorted(R.BATCH))
def test_inference_does_not_depend_on_the_batch(name, calls, monkeypatch):
    """conv(x, infer=True)[i] == conv(x[i:i+1], infer=True), bit for bit, on every entry an inference launch reaches"""
    case = R.BATCH[name]
    switches(monkeypatch, case)
    pc, t = packs(case)[0], device_inputs(case)
    out = launch(case, pc, t)
    entry = check_entry(case, calls, pc)
    check_output(case, entry, out, tag='CONVBATCH')
    for i in range(case['n']):
        one = Guarded(1, *R.out_shape(case)[1:])
        launch(case, pc, {k: v[i:i + 1] if v is not None else None for k, v in t.items()}, out=one, n=1)
        assert calls[-1][0] == entry and one.bands_intact()
        assert torch.equal(out.t[i:i + 1], one.t), '%s: image %d alone gives other bits than in a batch of %d' % (name, i, case['n'])


def nan_reach(entry, k, y0, x0, h, w):
    """(must, may): the outputs a NaN at (y0, x0) must reach - its k x k footprint - and those it may.  The direct fp32 kernels and
    risp_conv2d_f16x2 (whose tile scale ignores a NaN: test_gpu_f16x2.py) reach the footprint and nothing else.  The Winograd kernels
    transform 6 (F(4,3)) or 8 (F(4,5)) input columns into the four outputs of a quad, so whole quads whose window holds the column are
    reached, on the footprint's rows.  risp_conv2d_thin5 has one scale per work item (128 columns x 32 rows: test_gpu_thin5.py lets the
    NaN's own item go); the first-layer kernels one per strip of the image, so the NaN's image is theirs."""
    P = k // 2
    must = torch.zeros(h, w, dtype=torch.bool)
    must[max(0, y0 - P):y0 + P + 1, max(0, x0 - P):x0 + P + 1] = True
    may = must.clone()
    if entry in (W43, W45):
        lo, hi = (1, 4) if entry == W43 else (2, 5)                       # quad q reads the columns 4 q - lo .. 4 q + hi
        for q in range((w + 3) // 4):
            if 4 * q - lo <= x0 <= 4 * q + hi:
                may[max(0, y0 - P):y0 + P + 1, 4 * q:4 * q + 4] = True
    elif entry == THIN5:
        may[32 * (y0 // 32):32 * (y0 // 32) + 32, 128 * (x0 // 128):128 * (x0 // 128) + 128] = True
    elif entry in (TF1, TF1X):
        may[:] = True
    return must, may


@pytest.mark.parametrize('name', sorted(R.NANLOC))
def test_a_nan_stays_within_the_reach_of_the_filter(name, calls, monkeypatch):
    case = R.NANLOC[name]
    switches(monkeypatch, case)
    pc, t = packs(case)[0], device_inputs(case)
    i, y0, x0 = R.NAN_AT
    t['x'] = t['x'].clone()
    t['x'][i, case['cin'] // 2, y0, x0] = float('nan')
    out = launch(case, pc, t)
    entry = check_entry(case, calls, pc)
    assert out.bands_intact()
    bad = torch.isnan(out.t).cpu()
    must, may = nan_reach(entry, case['k'], y0, x0, case['h'], case['w'])
    assert not bad[:i].any() and not bad[i + 1:].any(), '%s: the NaN reaches another image' % name
    assert bad[i][:, must].all(), '%s: outputs under the footprint are not NaN' % name
    assert not bad[i][:, ~may].any(), '%s: %d outputs outside the reach of the filter are NaN' % (name, bad[i][:, ~may].sum().item())
    clean = R.ref64(case)
    ok = ~bad
    m = clean.abs().max().item()
    assert ((out.t.cpu().double() - clean)[ok].abs().max().item() <= R.bound(entry, R.E32(case, entry)) * m), '%s: the clean outputs moved' % name


def test_add_without_the_flag_is_refused(calls, monkeypatch):
    """``conv`` used to route on epi | EPI_ADD whenever ``add`` was given and to write the caller's epilogue into the descriptor: a route
    chosen for a residual that the kernel then never added.  Now a ValueError, before anything is launched"""
    from reconfigisp_amd import convnets as CN
    case = R.CASES['wino43 epi add+mask 3x3_17to33 2x50x68']
    switches(monkeypatch, case)
    pc, t = packs(case)[0], device_inputs(case)
    out = Guarded(*R.out_shape(case))
    for epi in (0, RELU, MASK):
        with pytest.raises(ValueError, match='EPI_ADD'):
            CN.conv(t['x'], pc, case['n'], case['h'], case['w'], epi=epi, add=t['add'], add_c=case['add_c'], mask=t['mask'] if epi & MASK else None,
                    out=out.t)
    torch.cuda.synchronize()
    assert not calls and out.untouched()
    launch(case, pc, t, out=out)                                       # ... and with the flag the same arguments run
    assert [c[0] for c in calls] == [W43] and not torch.isnan(out.t).any().item()


def test_refused_arguments_raise_on_the_host_and_write_nothing(calls, monkeypatch):
    """a grouped 3x3 layer, stacked packs of another member count, a CPU tensor: raised by ``conv`` itself, nothing launched, the NaN fill
    and the guard bands intact"""
    from reconfigisp_amd import convnets as CN
    c3, c5 = R.CASES['wino43 epi relu 3x3_17to33 2x50x68'], R.GROUPED['grouped wino45 5x5_12to40 G=2 flags=0 2x13x68']
    switches(monkeypatch, c5)
    p3, t3 = packs(c3)[0], device_inputs(c3)
    out = Guarded(2 * c3['n'], c3['cout'], c3['h'], c3['w'])
    with pytest.raises(ValueError, match='3x3'):
        CN.conv(t3['x'].repeat(2, 1, 1, 1), CN.stack_packed([p3, p3]), c3['n'], c3['h'], c3['w'], epi=RELU, out=out.t, group=(2, 0))
    torch.cuda.synchronize()
    assert not calls and out.untouched()
    p5, t5 = packs(c5), device_inputs(c5)
    out = Guarded(3 * c5['n'], c5['cout'], c5['h'], c5['w'])
    with pytest.raises(ValueError, match='members'):
        CN.conv(t5['x'], CN.stack_packed(p5), c5['n'], c5['h'], c5['w'], epi=c5['epi'], add=t5['add'], add_c=c5['add_c'], out=out.t, group=(3, 0))
    with pytest.raises(ValueError, match='disagree'):
        CN.stack_packed([p5[0], p3])
    torch.cuda.synchronize()
    assert not calls and out.untouched()
    out = Guarded(*R.out_shape(c3))
    for which in ('x', 'add', 'mask', 'out'):
        kw = dict(x=t3['x'], add=torch.zeros(R.out_shape(c3), device='cuda'), mask=torch.ones(R.out_shape(c3), device='cuda'), out=out.t)
        kw[which] = kw[which].cpu()
        with pytest.raises(RuntimeError, match='must be a CUDA/HIP tensor'):
            CN.conv(kw['x'], p3, c3['n'], c3['h'], c3['w'], epi=RELU | ADD | MASK, add=kw['add'], add_c=c3['cout'], mask=kw['mask'], out=kw['out'])
    torch.cuda.synchronize()
    assert not calls and out.untouched()
