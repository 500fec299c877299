"""GPU: the device-side auto white balance / auto exposure - the two launches (risp_control_solve, risp_gain_map) through the
C ABI and ``functional.gain_control`` / ``control_update`` on synthetic statistics.  No frames are needed.

The definition is integers (include/risp.h), so every comparison is ``torch.equal`` / ``array_equal`` against
tests/control_reference.py (numpy int64) and nothing here has a tolerance.  The inputs are ``SOLVE_CASES``, ``SPECIAL_CASES``
and ``MAP_CASES`` of that file; tests/test_control_reference_cpu.py asserts that they tell every wrong variant of the definition
apart.  State, zones, hist, scratch and the maps lie inside allocations of a pattern, so a write outside shows; the inputs are
compared after the call; behind every call the scratch is all zero, and the same call from the same state gives the same
sixteen words - which it could not with anything left in the scratch."""
import ctypes as C

import numpy as np
import pytest
import torch

import control_reference as CR

pytestmark = pytest.mark.gpu

PATTERN = {torch.int64: 0x5A5A5A5A5A5A5A5A, torch.int32: 0x5A5A5A5A, torch.uint16: 0x5A5A}


def _guarded(x, fill=None):
    """the numpy array (or, with ``fill``, that value) as a contiguous device view 8 elements into an allocation of a pattern
    with 8 more behind it -> (view, allocation)"""
    t = torch.from_numpy(np.ascontiguousarray(x))
    big = torch.full((t.numel() + 16,), PATTERN[t.dtype], dtype=t.dtype).cuda()
    view = big[8:8 + t.numel()].view(t.shape)
    view.copy_(t) if fill is None else view.fill_(fill)
    assert view.is_contiguous() and view.data_ptr() % 8 == 0
    return view, big


def _assert_guards(*allocations):
    for big in allocations:
        assert (big[:8] == PATTERN[big.dtype]).all() and (big[-8:] == PATTERN[big.dtype]).all(), 'written outside (%s)' % big.dtype


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _solve_call(zones, hist, state, scratch, spec, geometry):
    import reconfigisp_amd.functional as F
    from reconfigisp_amd import lib as L
    n, gh, gw = zones.shape[:3]
    h, w, zone_h, zone_w, shift, cfa = geometry
    return L.load().risp_control_solve(_p(zones), _p(hist), _p(state), _p(scratch), (C.c_int * len(spec))(*spec), n, gh, gw, h, w,
                                       zone_h, zone_w, hist.shape[2], shift, cfa, F._stream())


def _check_solve(zones, hist, state, spec, geometry, what):
    from reconfigisp_amd import lib as L
    want = CR.solve_ref(zones, hist, state, spec, geometry)
    dz, big_z = _guarded(zones)
    dh, big_h = _guarded(hist)
    ds, big_s = _guarded(state)
    scratch, big_x = _guarded(np.zeros(5 + hist.shape[2], dtype=np.int64))
    for again in (False, True):                             # the same call twice from the same state
        ds.copy_(torch.from_numpy(state))
        assert _solve_call(dz, dh, ds, scratch, spec, geometry) == 0, L.load().risp_last_error()
        torch.cuda.synchronize()
        got = ds.cpu().numpy()
        assert np.array_equal(got, want), '%s%s: state %s, reference %s' % (what, ', called again' if again else '', got.tolist(),
                                                                           want.tolist())
        assert not scratch.any().item(), '%s: the scratch is not zero behind the call: %s' % (what, scratch.cpu().tolist()[:8])
    _assert_guards(big_z, big_h, big_s, big_x)
    assert torch.equal(dz.cpu(), torch.from_numpy(zones)) and torch.equal(dh.cpu(), torch.from_numpy(hist)), '%s: the inputs changed' % what
    return want


# ---------------------------------------------------------------- 1. the solve launch
@pytest.mark.parametrize('case', range(len(CR.SOLVE_CASES)), ids=[c[0] for c in CR.SOLVE_CASES])
def test_control_solve_equals_the_reference(case):
    zones, hist, state, spec, geometry = CR.solve_case(case)
    want = _check_solve(zones, hist, state, spec, geometry, CR.SOLVE_CASES[case][0])
    assert want[7] & 3 == 3


@pytest.mark.parametrize('name', CR.SPECIAL_CASES)
def test_control_solve_on_the_cases_built_by_hand(name):
    zones, hist, state, spec, geometry = CR.special_case(name)
    want = _check_solve(zones, hist, state, spec, geometry, name)
    flags = {'no-candidate': 2, 'all-empty': 0, 'hist-empty': 1, 'green-empty': 1, 'ceiling': 7, 'speeds-0': 3, 'deadband': 3}
    if name in flags:
        assert want[7] == flags[name], (name, want[7])


def test_updates_chain_from_one_state_to_the_next():
    """four updates in a row on one stream, no host work between them: the state of one launch is the next one's input, and the
    scratch one launch leaves is the next one's start"""
    from reconfigisp_amd import lib as L
    zones, hist, state, spec, geometry = CR.solve_case(2)
    dz, dh, ds = (torch.from_numpy(a).cuda() for a in (zones, hist, state))
    scratch = torch.zeros(5 + hist.shape[2], dtype=torch.int64, device='cuda')
    want = state
    for _ in range(4):
        assert _solve_call(dz, dh, ds, scratch, spec, geometry) == 0, L.load().risp_last_error()
        want = CR.solve_ref(zones, hist, want, spec, geometry)
    torch.cuda.synchronize()
    assert np.array_equal(ds.cpu().numpy(), want) and not scratch.any().item()


# ---------------------------------------------------------------- 2. the map launch
@pytest.mark.parametrize('case', range(len(CR.MAP_CASES)), ids=['%dx%d-%s' % (c[0], c[1], 'base' if c[2] else 'flat') for c in CR.MAP_CASES])
def test_gain_map_equals_the_reference(case):
    import reconfigisp_amd.functional as F
    from reconfigisp_amd import lib as L
    base, state, (gh, gw) = CR.map_case(case)
    want = CR.gain_map_ref(base, state, (gh, gw))
    db, big_b = _guarded(base) if base is not None else (None, None)
    ds, big_s = _guarded(state)
    out, big_o = _guarded(np.zeros((gh, gw, 4), dtype=np.uint16), fill=0x1234)
    assert L.load().risp_gain_map(_p(db), _p(ds), _p(out), gh, gw, F._stream()) == 0, L.load().risp_last_error()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got, want), '%d words differ, first at %s' % ((got != want).sum(), np.argwhere(got != want)[:1].tolist())
    _assert_guards(big_s, big_o, *([big_b] if base is not None else []))
    assert torch.equal(ds.cpu(), torch.from_numpy(state)) and (base is None or torch.equal(db.cpu(), torch.from_numpy(base)))


# ---------------------------------------------------------------- 3. functional.gain_control on synthetic statistics
def _stats_of(zones, hist, geometry):
    import reconfigisp_amd.functional as F
    h, w, zone_h, zone_w, shift, _ = geometry
    st = F.raw_statistics(zones.shape[0], h, w, zone=(zone_h, zone_w), bins=hist.shape[2], hist_shift=shift)
    st.zones.copy_(torch.from_numpy(zones)), st.hist.copy_(torch.from_numpy(hist))
    return st


@pytest.mark.parametrize('with_base', [False, True], ids=['flat', 'base'])
def test_gain_control_owns_state_and_map_and_update_is_two_launches(with_base):
    import lens_shading_reference as LS
    import reconfigisp_amd.functional as F
    from reconfigisp_amd import lib as L
    zones, hist, _, _, geometry = CR.solve_case(3)          # (3,34,156), grbg
    h, w, cfa, cell = geometry[0], geometry[1], geometry[5], 16
    fields = dict(fill=230, target=400)
    st = _stats_of(zones, hist, geometry)
    base = LS.random_map(h, w, 4, seed=5) if with_base else None
    dbase = torch.from_numpy(base).cuda() if with_base else None
    ctl = F.gain_control(st, cell=cell, base=dbase, cfa='grbg', **fields)
    shape = LS.map_shape(h, w, 4)
    assert tuple(ctl.gains.shape) == shape + (4,) and ctl.gains.dtype == torch.uint16 and ctl.state.dtype == torch.int32
    assert ctl.shading[0] is ctl.gains and ctl.shading[1] == cell and F.shading_check(ctl.shading, h, w)[1:] == (4,) + shape
    state = CR.new_state(cfa=cfa)
    assert np.array_equal(ctl.state.cpu().numpy(), state) and np.array_equal(ctl.gains.cpu().numpy(), CR.gain_map_ref(base, state, shape))
    spec = CR.spec_tuple(**fields)
    assert ctl.spec == spec
    for step in range(3):
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        L.CALLS = {}
        try:
            assert ctl.update(st) is ctl
            calls = dict(L.CALLS)
        finally:
            L.CALLS = None
        assert calls == {'risp_control_solve': 1, 'risp_gain_map': 1} and torch.cuda.memory_allocated() == before
        state = CR.solve_ref(zones, hist, state, spec, geometry)
        assert np.array_equal(ctl.state.cpu().numpy(), state), step
        assert np.array_equal(ctl.gains.cpu().numpy(), CR.gain_map_ref(base, state, shape)), step
        assert not ctl._scratch.any().item()
    if with_base:
        assert torch.equal(dbase.cpu(), torch.from_numpy(base)) and ctl.base is dbase       # kept, never written
    # reset: other gains, the map made at once
    assert ctl.reset(exposure=8192, wb=(6000, 5000)) is ctl
    state = CR.new_state(8192, (6000, 5000), cfa)
    assert np.array_equal(ctl.state.cpu().numpy(), state) and np.array_equal(ctl.gains.cpu().numpy(), CR.gain_map_ref(base, state, shape))
    for bad, word in ((dict(exposure=100), 'exposure 100'), (dict(wb=(4096, 70000)), 'wb blue 70000'), (dict(wb=4096), 'red, blue')):
        with pytest.raises(ValueError, match=word):
            ctl.reset(**bad)


def test_update_refuses_other_statistics_before_a_launch():
    import reconfigisp_amd.functional as F
    from reconfigisp_amd import lib as L
    st = F.raw_statistics(2, 12, 24, zone=(4, 8), bins=16, hist_shift=6)
    ctl = F.gain_control(st, cell=8)
    held = ctl.state.clone()
    others = ((F.raw_statistics(3, 12, 24, zone=(4, 8), bins=16, hist_shift=6), 'zones for 2 frames'),
              (F.raw_statistics(2, 12, 24, zone=(4, 8), bins=32, hist_shift=6), '32 bins'),
              (F.raw_statistics(2, 12, 24, zone=(2, 8), bins=16, hist_shift=6), 'zones of 2 x 8'),
              (F.raw_statistics(2, 12, 24, zone=(4, 8), bins=16, hist_shift=5), 'hist_shift 5'),
              (F.raw_statistics(2, 12, 24, zone=(4, 8), bins=16, hist_shift=6, device='cpu'), 'lives on cpu'), ('zones', 'RawStatistics'))
    L.CALLS = {}
    try:
        for other, word in others:
            with pytest.raises(ValueError, match=word):
                ctl.update(other)
        assert L.CALLS == {}, 'launched before the refusal: %s' % L.CALLS
    finally:
        L.CALLS = None
    assert torch.equal(ctl.state, held)
    with pytest.raises(ValueError, match='lens shading gains'):         # a base of another cell's shape
        F.gain_control(st, cell=8, base=torch.zeros((2, 2, 4), dtype=torch.uint16, device='cuda'))


# ---------------------------------------------------------------- 4. refusals through the C ABI
def test_refusals_through_the_c_abi_leave_state_and_map_alone():
    import reconfigisp_amd.functional as F
    from reconfigisp_amd import lib as L
    lib = L.load()
    zones, hist, state, spec, geometry = CR.special_case('ceiling')       # (2,12,24), zones of 4 x 8, 16 bins, shift 6, grbg
    n, (gh, gw), bins = zones.shape[0], zones.shape[1:3], hist.shape[2]
    dz, dh = torch.from_numpy(zones).cuda(), torch.from_numpy(hist).cuda()
    ds, big_s = _guarded(state, fill=PATTERN[torch.int32])
    scratch, big_x = _guarded(np.zeros(5 + bins, dtype=np.int64))
    spec_of = lambda **f: (C.c_int * len(spec))(*CR.spec_tuple(**dict(dict(zip(CR.FIELDS, spec)), **f)))

    def solve(zones=_p(dz), hist=_p(dh), state=_p(ds), scratch=_p(scratch), spec=spec_of(), N=n, ZH=gh, ZW=gw, H=12, W=24, zh=4, zw=8,
              bins=bins, shift=6, cfa=1):
        return lib.risp_control_solve(zones, hist, state, scratch, spec, N, ZH, ZW, H, W, zh, zw, bins, shift, cfa, F._stream())

    def raw_spec(**f):                                      # out of range: not through spec_tuple's ints alone
        values = dict(zip(CR.FIELDS, spec))
        values.update(f)
        return (C.c_int * len(spec))(*[values[k] for k in CR.FIELDS])

    off = lambda t, d: C.c_void_p(t.data_ptr() + d)
    refused = {'null zones': (dict(zones=None), b'null'), 'null hist': (dict(hist=None), b'null'), 'null state': (dict(state=None), b'null'),
               'null scratch': (dict(scratch=None), b'null'), 'null spec': (dict(spec=None), b'null'),
               'N 0': (dict(N=0), b'N=0'), 'H 11': (dict(H=11), b'H=11'), 'W 22': (dict(W=22), b'W 22'), 'W 0': (dict(W=0), b'W 0'),
               'zone_h 3': (dict(zh=3), b'zone_h 3'), 'zone_w 6': (dict(zw=6), b'zone_w 6'), 'zone_w 0': (dict(zw=0), b'zone_w 0'),
               'ZH 4': (dict(ZH=4), b'ZH 4'), 'ZW 2': (dict(ZW=2), b'ZW 2'),
               'too many zones': (dict(N=(1 << 24) // 9 + 1), b'2^24'),
               'too many samples': (dict(N=1, H=1 << 20, W=1 << 21, zh=1 << 20, zw=1 << 21, ZH=1, ZW=1), b'2^40'),
               'bins 0': (dict(bins=0), b'bins 0'), 'bins 1025': (dict(bins=1025), b'bins 1025'),
               'shift 17': (dict(shift=17), b'hist_shift 17'), 'shift -1': (dict(shift=-1), b'hist_shift -1'),
               'cfa 4': (dict(cfa=4), b'cfa 4'), 'cfa -1': (dict(cfa=-1), b'cfa -1'),
               'zones 4-byte aligned': (dict(zones=off(dz, 4)), b'aligned'), 'scratch 4-byte aligned': (dict(scratch=off(scratch, 4)), b'aligned'),
               'hist 2-byte aligned': (dict(hist=off(dh, 2)), b'aligned'), 'state 2-byte aligned': (dict(state=off(ds, 2)), b'aligned')}
    for name, (lo, hi) in CR.RANGES.items():
        refused['%s below' % name] = (dict(spec=raw_spec(**{name: lo - 1})), ('%s %d outside' % (name, lo - 1)).encode())
        refused['%s above' % name] = (dict(spec=raw_spec(**{name: hi + 1})), ('%s %d outside' % (name, hi + 1)).encode())
    for low, high in CR.PAIRS:
        lo = CR.RANGES[low][0]
        refused['%s above %s' % (low, high)] = (dict(spec=raw_spec(**{low: lo + 2, high: lo + 1})),
                                                ('%s %d above %s %d' % (low, lo + 2, high, lo + 1)).encode())
    for what, (kw, word) in refused.items():
        assert solve(**kw) != 0, '%s was accepted' % what
        err = lib.risp_last_error()
        assert b'risp_control_solve' in err and word in err, (what, err)

    base, _, (mh, mw) = CR.map_case(2)
    db = torch.from_numpy(base).cuda()
    out, big_o = _guarded(np.zeros((mh, mw, 4), dtype=np.uint16), fill=PATTERN[torch.uint16])
    both = torch.zeros((2 * mh * mw * 4,), dtype=torch.uint16, device='cuda')

    def gain_map(base=_p(db), state=_p(ds), out=_p(out), GH=mh, GW=mw):
        return lib.risp_gain_map(base, state, out, GH, GW, F._stream())

    refused = {'null state': (dict(state=None), b'null'), 'null out': (dict(out=None), b'null'), 'GH 1': (dict(GH=1), b'1 x 5'),
               'GW 0': (dict(GW=0), b'3 x 0'), 'too many nodes': (dict(GH=1 << 16, GW=(1 << 14) + 1), b'2^30'),
               'out 4-byte aligned': (dict(out=off(out, 4)), b'aligned'), 'base 2-byte aligned': (dict(base=off(db, 2)), b'aligned'),
               'state 2-byte aligned': (dict(state=off(ds, 2)), b'aligned'),
               'out inside base': (dict(base=_p(both), out=off(both, 8 * (mh * mw - 1))), b'overlaps'),
               'base inside out': (dict(out=_p(both), base=off(both, 8)), b'overlaps')}
    for what, (kw, word) in refused.items():
        assert gain_map(**kw) != 0, '%s was accepted' % what
        err = lib.risp_last_error()
        assert b'risp_gain_map' in err and word in err, (what, err)
    torch.cuda.synchronize()
    assert (big_s == PATTERN[torch.int32]).all().item() and (big_o == PATTERN[torch.uint16]).all().item(), 'a refused call wrote'
    assert not scratch.any().item() and (both == 0).all().item()
    _assert_guards(big_x)
    # the accepted calls: out right behind base is no overlap
    ds.copy_(torch.from_numpy(state))
    assert solve() == 0, lib.risp_last_error()
    both[:mh * mw * 4].copy_(torch.from_numpy(base).flatten())
    assert gain_map(base=_p(both), out=off(both, 8 * mh * mw)) == 0, lib.risp_last_error()
    torch.cuda.synchronize()
    want = CR.solve_ref(zones, hist, state, spec, geometry)
    assert np.array_equal(ds.cpu().numpy(), want)
    assert np.array_equal(both[mh * mw * 4:].view(mh, mw, 4).cpu().numpy(), CR.gain_map_ref(base, want))
    _assert_guards(big_s)
