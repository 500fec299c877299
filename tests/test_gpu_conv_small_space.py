"""GPU: ``convnets.conv_small`` - the dispatch the models call for layers with few output channels - over its argument space, against
float64.

The table, the seeded walk, the float64 restatement and what each entry point accepts are tests/conv_small_reference.py (plain CPU
code, checked by tests/test_conv_small_reference_cpu.py).  Every case goes through ``CN.conv_small`` into ``out=``, a 16-byte-aligned
view inside a NaN-filled buffer between guard bands, with ``L.call`` recorded, and is held to

  1. entry: the launched entry point is the case's literal expectation and what ``route_small`` names (``_split`` only where the case
     expects a channel split: small training grids, and 9x9 layers with 32 channels or more always), and that entry's own conditions (``ENTRY_ACCEPTS``) accept the launch with the segment height / split passed;
  2. writes: every output element written, the guard bands untouched;
  3. accuracy: max error relative to max|ref| below the bar of the kernel's own file (tap-row, band 5e-6: test_gpu_tapout.py,
     test_gpu_toep.py; narrow3 2e-6: test_gpu_narrow3.py; vector 3e-6: test_gpu_toep.py), and ``assert_close`` with conftest's defaults;
  4. determinism: a second call gives the same bits.

Contracts, one test each: an inference result does not depend on the batch; a grouped launch equals its per-member form bit for bit
and launches the same entry; the tile sums of the backward-data launches finish into the float64 rectangle sums; refused arguments
raise on the host and write nothing.  RISP_BUDGET_REPORT=1 prints one line per case (tools/conv_small_budget_report.py)."""
import os
import types

import numpy as np
import pytest
import torch

import conv_small_reference as R
from conftest import assert_close
from conv_small_reference import ADD, NOBIAS, SHUFFLE2, NARROW3, SMALL, SPLIT, TAPOUT, TOEP
from guarded import Guarded

pytestmark = pytest.mark.gpu

REPORT = os.environ.get('RISP_BUDGET_REPORT') == '1'


@pytest.fixture
def calls(monkeypatch):
    """the conv launches of ``conv_small``, as tests/test_gpu_conv_modes.py::test_conv_launches_what_route_says records them"""
    from reconfigisp_amd import convnets as CN, lib as L
    rec, real = [], L.call

    def spy(name, *a):
        if name.startswith('risp_conv2d'):
            rec.append((name, a))
        return real(name, *a)
    monkeypatch.setattr(CN.L, 'call', spy)
    return rec


def packs(case):
    """the members' ``SmallConv`` objects of a case"""
    from reconfigisp_amd import convnets as CN
    d = R.inputs(case)
    return [CN.SmallConv(w.cuda(), b.cuda() if b is not None else None, transpose=case['transpose'], keep=R.keep_of(case))
            for w, b in zip(d['weights'], d['bias'])]


def device_inputs(case):
    d = R.inputs(case)
    return tuple(d[k].cuda() if d[k] is not None else None for k in ('x', 'add', 'mask'))


def launch(case, sc, x, add, mask, n=None, out=None, **kw):
    from reconfigisp_amd import convnets as CN
    out = out if out is not None else Guarded(*R.out_shape(case))
    CN.conv_small(x, sc, case['n'] if n is None else n, case['h'], case['w'], epi=case['epi'], add=add, add_c=case['add_c'], mask=mask,
                  infer=case['infer'], out=out.t if isinstance(out, Guarded) else out, **kw)
    torch.cuda.synchronize()
    return out


def errors(y, ref):
    m = ref.abs().max().item() or 1.0
    e = y.double().cpu() - ref
    return e.pow(2).mean().sqrt().item() / m, e.abs().max().item() / m


def CN_chain(case, n_all):
    from reconfigisp_amd import convnets as CN
    return CN.small_chain_groups(case['k'], case['cin'], n_all)


def check_entry(case, rec, lib):
    """(entry, base entry) of the one conv launch recorded, held to the route, the expectation and the entry's own conditions"""
    assert len(rec) == 1, [r[0] for r in rec]
    entry, args = rec[0]
    base = SMALL if entry == SPLIT else entry
    n_all = case['n'] * (case['group'] or 1)
    assert base == R.routed(case), (case['name'], entry, R.routed(case))
    groups = args[2] if entry == SPLIT else 1
    want_groups = 1
    if base == SMALL:                           # the grid's split (the library's choice, training only), else the fixed split of long chains
        by_grid = 1 if case['infer'] else lib.risp_conv_small_groups(args[0])
        assert by_grid == (1 if case['infer'] else R.small_groups(case['cin'], n_all, case['h'], case['w']))
        want_groups = R.vector_groups(case)
        assert want_groups == (by_grid if by_grid > 1 else CN_chain(case, n_all))
    assert (entry == SPLIT) == (want_groups > 1) and groups == want_groups, (case['name'], entry, groups, want_groups)
    if case['expect'] is not None:
        assert entry == case['expect'] and (entry == SPLIT) == bool(case['split']), (case['name'], entry, case['expect'])
    over = dict(groups=groups)
    if entry == TAPOUT:
        over['seg_rows'] = args[1]
        if not case['infer']:                   # the library's half of the segment height: a multiple of 4, or the image whole
            assert args[1] == lib.risp_conv_tapout_seg_rows(n_all, case['h'], case['w'])
    assert R.ENTRY_ACCEPTS[entry](R.launch_of(case, **over)), (case['name'], entry, over)
    return entry


@pytest.mark.parametrize('name', sorted(R.ALL))
def test_case(name, calls, monkeypatch):
    from reconfigisp_amd import convnets as CN, lib as L
    case = R.ALL[name]
    monkeypatch.setattr(CN, 'CONV_ARITH', case['arith'])
    sc, (x, add, mask) = packs(case)[0], device_inputs(case)
    out = launch(case, sc, x, add, mask)
    entry = check_entry(case, calls, L.load())
    assert out.bands_intact(), '%s: the guard bands were written' % name
    assert not torch.isnan(out.t).any().item(), '%s: output elements left unwritten' % name
    ref = R.ref64(case)
    rms, mx = errors(out.t, ref)
    if REPORT:
        print('CONVSMALL %-70s | %-24s rms %.3e max %.3e bar %.1e' % (name, entry, rms, mx, R.BAR[entry]))
    assert mx < R.BAR[entry], '%s on %s: max error %.3e of max|ref| (rms %.3e), bar %.1e' % (name, entry, mx, rms, R.BAR[entry])
    assert_close(out.t, ref, what=name)
    again = launch(case, sc, x, add, mask)
    assert calls[1][0] == entry and torch.equal(out.t, again.t), '%s: a second call gives other bits' % name


INFER_LAYERS = {'taprow 5x5_32to3': (5, 32, 3, TAPOUT), 'taprow 9x9_64to3': (9, 64, 3, TAPOUT), 'band 9x9_64to4': (9, 64, 4, TOEP),
                'band 5x5_32to12': (5, 32, 12, TOEP), 'narrow3 3x3_64to4': (3, 64, 4, NARROW3), 'vector 3x3_24to3': (3, 24, 3, SMALL),
                'vector 9x9_64to3 f32 (channel groups)': (9, 64, 3, SPLIT), 'vector 9x9_64to4 f32 (channel groups)': (9, 64, 4, SPLIT)}


@pytest.mark.parametrize('h', [50, 66, 130])
@pytest.mark.parametrize('layer', sorted(INFER_LAYERS))
def test_inference_does_not_depend_on_the_batch(layer, h, calls, monkeypatch):
    """conv_small(x, infer=True)[i] == conv_small(x[i:i+1], infer=True), bit for bit: below one 64-row segment with H % 4 = 2, one segment
    plus two rows, two segments plus two rows"""
    from reconfigisp_amd import convnets as CN
    monkeypatch.setattr(CN, 'CONV_ARITH', 'f32' if 'f32' in layer else 'f16x2')
    k, cin, cout, entry = INFER_LAYERS[layer]
    n, w = 3, 68
    rng = np.random.default_rng(700 + h)
    rnd = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).cuda()
    sc = CN.SmallConv(rnd(cout, cin, k, k) * 0.05, rnd(cout) * 0.1)
    x, add = rnd(n, cin, h, w), rnd(n, cout, h, w)
    kw = dict(epi=CN.EPI_ADD, add=add, add_c=cout) if entry in (TAPOUT, TOEP) else dict(epi=CN.EPI_RELU)
    y = CN.conv_small(x, sc, n, h, w, infer=True, **kw)
    assert calls[-1][0] == entry and not torch.isnan(y).any().item()
    for i in range(n):
        if 'add' in kw:
            kw['add'] = add[i:i + 1].contiguous()
        yi = CN.conv_small(x[i:i + 1].contiguous(), sc, 1, h, w, infer=True, **kw)
        assert calls[-1][0] == entry
        assert torch.equal(y[i:i + 1], yi), '%s H=%d: image %d alone gives other bits than in a batch of %d' % (layer, h, i, n)


@pytest.mark.parametrize('name', sorted(R.GROUPED))
def test_grouped_launch_equals_its_per_member_form(name, calls, monkeypatch):
    """conv_small(..., group=(G, 0)) on stack_small packs against the per-member calls as the models make them: split=_small_split(...) and
    seg_rows=tapout_seg(G * n, h, w, False) - the same entry point, the same bits, and the float64 restatement within the entry's bar"""
    from reconfigisp_amd import convnets as CN, lib as L
    case = R.GROUPED[name]
    monkeypatch.setattr(CN, 'CONV_ARITH', case['arith'])
    G, n, h, w = case['group'], case['n'], case['h'], case['w']
    scs, (x, add, mask) = packs(case), device_inputs(case)
    stacked = CN.stack_small(scs)
    out = launch(case, stacked, x, add, mask, group=(G, 0))
    entry = check_entry(case, calls, L.load())
    assert out.bands_intact() and not torch.isnan(out.t).any().item(), name
    rms, mx = errors(out.t, R.ref64(case))
    if REPORT:
        print('CONVSMALL %-70s | %-24s rms %.3e max %.3e bar %.1e' % (name, entry, rms, mx, R.BAR[entry]))
    assert mx < R.BAR[entry], (name, entry, mx)
    assert_close(out.t, R.ref64(case), what=name)
    del calls[:]
    split = CN._small_split(x, stacked, G * n, h, w, case['epi'], case['add_c'])
    seg = CN.tapout_seg(G * n, h, w, False)
    members = Guarded(*R.out_shape(case))
    for g in range(G):
        s = slice(g * n, (g + 1) * n)
        launch(case, scs[g], x[s], add[s] if add is not None else None, None, out=members.t[s], split=split, seg_rows=seg)
    assert [c[0] for c in calls] == [entry] * G, '%s: the grouped launch runs %s, its members %s' % (name, entry, [c[0] for c in calls])
    assert members.bands_intact() and torch.equal(out.t, members.t), '%s: the per-member form gives other bits' % name


@pytest.mark.parametrize('hw', [(64, 68), (66, 132), (128, 260), (50, 8)])
@pytest.mark.parametrize('cout', [3, 4])
def test_tile_sums_finish_into_the_rectangle_sums(cout, hw, calls, monkeypatch):
    """conv_small(..., tile_sums=[]) on the 9x9 64 -> 3 (tap-row) and 64 -> 4 (band) backward-data packs, then CN.rect_sums: float64 rectangle
    sums and the whole-plane risp_rect_sums, at heights that are a multiple of the segment (64 rows) / tile and heights that are not"""
    from reconfigisp_amd import convnets as CN
    monkeypatch.setattr(CN, 'CONV_ARITH', 'f16x2')
    h, w = hw
    n = 2
    rng = np.random.default_rng(900 + h + cout)
    rnd = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).cuda()
    w1 = rnd(64, 12 if cout == 3 else 4, 9, 9) * 0.05
    sc = CN.SmallConv(w1, None, transpose=True, keep=cout)
    g1 = rnd(n, 64, h, w)
    ts = []
    y = CN.conv_small(g1, sc, n, h, w, infer=True, tile_sums=ts)
    plain = CN.conv_small(g1, sc, n, h, w, infer=True)
    want = ['risp_conv2d_tapout_sums', 'risp_conv2d_tapout'] if cout == 3 else ['risp_conv2d_toep_sums', 'risp_conv2d_toep']
    assert [c[0] for c in calls] == want
    assert len(ts) == 1 and not torch.isnan(ts[0]).any().item() and torch.equal(y, plain)
    rs, rs0 = Guarded(n, 64 * 81), Guarded(n, 64 * 81)
    CN.rect_sums(g1, rs.t, n, 64, h, w, 9, ts)
    CN.rect_sums(g1, rs0.t, n, 64, h, w, 9, None)
    torch.cuda.synchronize()
    assert rs.bands_intact() and rs0.bands_intact() and not torch.isnan(rs.t).any().item()
    ref = R.rect_sums64(g1.cpu(), 9)
    assert_close(rs.t, ref, what='tile sums against float64')
    assert_close(rs0.t, ref, what='whole planes against float64')
    assert_close(rs.t, rs0.t, what='tile sums against the whole planes')


def test_refused_arguments_raise_on_the_host_and_write_nothing(calls, monkeypatch):
    """cout = 13, k = 7, SHUFFLE2 with 3 couts, ADD without its tensor: RuntimeError from the entry point's own argument check (nothing
    is launched), the NaN fill and the guard bands intact"""
    from reconfigisp_amd import convnets as CN
    monkeypatch.setattr(CN, 'CONV_ARITH', 'f16x2')
    n, h, w = 2, 16, 68
    rng = np.random.default_rng(77)
    rnd = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).cuda()
    sc12 = CN.SmallConv(rnd(12, 32, 5, 5) * 0.05, rnd(12) * 0.1)
    sc13 = types.SimpleNamespace(wpack=sc12.wpack, bias=rnd(13), cin=32, cout=13, k=5)       # (SmallConv itself refuses to pack 13 couts)
    with pytest.raises(ValueError):
        CN.SmallConv(rnd(13, 32, 5, 5))
    sc7 = CN.SmallConv(rnd(3, 32, 7, 7) * 0.05, rnd(3) * 0.1)
    sc3 = CN.SmallConv(rnd(3, 32, 5, 5) * 0.05, rnd(3) * 0.1)
    x = rnd(n, 32, h, w)
    for what, sc, cout, kw in (('cout 13', sc13, 13, {}), ('k 7', sc7, 3, {}), ('shuffle2 with 3 couts', sc3, 3, dict(epi=CN.EPI_SHUFFLE2)),
                               ('add without its tensor', sc3, 3, dict(epi=CN.EPI_ADD, add_c=3))):
        for infer in (True, False):
            out = Guarded(n, cout, h, w)
            with pytest.raises(RuntimeError, match='risp_conv2d'):
                CN.conv_small(x, sc, n, h, w, infer=infer, out=out.t, **kw)
            torch.cuda.synchronize()
            assert out.untouched(), '%s (infer=%s): refused, and the output was written' % (what, infer)
