"""Without a GPU: the case table of tests/conv_small_reference.py reaches what it claims to reach, ``convnets.route_small`` only ever
names an entry point whose own argument checks (``ENTRY_ACCEPTS``, restated from the library) accept the launch, the per-member form of a
grouped launch is sent where the grouped launch goes, and the float64 restatement tells wrong operations apart."""
import itertools

import pytest
import torch

import conv_small_reference as R
from conv_small_reference import ADD, MASK, NOBIAS, RELU, SHUFFLE2, NARROW3, SMALL, SPLIT, TAPOUT, TOEP
from reconfigisp_amd import convnets as CN


routed = R.routed


def test_the_bits_are_the_library_s():
    assert (RELU, ADD, MASK, SHUFFLE2, NOBIAS) == (CN.EPI_RELU, CN.EPI_ADD, CN.EPI_MASK, CN.EPI_SHUFFLE2, CN.EPI_NOBIAS)


def test_table_reaches_every_entry_epilogue_direction_arithmetic_threshold_and_row_phase():
    cases = list(R.CASES.values())
    assert {c['expect'] for c in cases} == {TAPOUT, TOEP, NARROW3, SMALL, SPLIT}
    by = lambda e: [c for c in cases if c['expect'] == e]
    for entry, bits in ((TAPOUT, (RELU, ADD)), (TOEP, (RELU, ADD, SHUFFLE2)), (NARROW3, (RELU, SHUFFLE2)), (SMALL, (RELU, ADD, MASK, SHUFFLE2)),
                        (SPLIT, (ADD, MASK, SHUFFLE2))):
        got = by(entry)
        for bit in bits:
            assert any(c['epi'] & bit for c in got), (entry, bit)
        assert any(c['epi'] == 0 and c['bias'] for c in got) and any(not c['bias'] for c in got), entry
        assert {c['transpose'] for c in got} == {False, True}, entry
        if ADD in bits:
            assert any(c['epi'] & ADD and c['add_c'] == c['cout'] for c in got) and (entry == SPLIT or any(c['epi'] & ADD and c['add_c'] < c['cout'] for c in got))
    assert any((c['epi'] & (ADD | RELU)) == (ADD | RELU) for e in (TAPOUT, TOEP, SMALL) for c in by(e))
    assert {c['cout'] for c in cases if c['epi'] & SHUFFLE2} == {4, 8, 12}
    assert {c['arith'] for c in cases} == {'f16x2', 'f32'}
    layers = {(c['k'], c['cin'], c['cout']) for c in cases}
    assert layers >= set(R.ALL_LAYERS)
    for k, cin, cout in R.ALL_LAYERS:                          # every layer under the fp32 arithmetic and with a mask: the vector kernel
        assert any((c['k'], c['cin'], c['cout'], c['arith']) == (k, cin, cout, 'f32') and c['expect'] in (SMALL, SPLIT) for c in cases)
        assert any((c['k'], c['cin'], c['cout']) == (k, cin, cout) and c['mask'] and c['expect'] in (SMALL, SPLIT) for c in cases)
    # a combination the preferred kernel of a layer does not have lands on the vector kernel
    refused = [c for c in cases if 'not the kernel' in c['name']]
    assert {c['k'] for c in refused} == {3, 5, 9} and all(c['expect'] == R._vec(c['k'], c['cin'], c['cout']) for c in refused)
    # shapes: every H and W of the list; W % 4 != 0; H % 4 in {0, 1, 2, 3} and the three segment edges under inference, per matrix-pipe route
    assert {c['h'] for c in cases} >= {1, 2, 3, 5, 13, 31, 50, 63, 66, 130} and {c['w'] for c in cases} >= {4, 8, 68, 132, 260, 6, 30}
    for entry in (TAPOUT, TOEP, NARROW3, SMALL):
        hs = {c['h'] for c in by(entry) if c['infer']}
        assert {h % 4 for h in hs} == {0, 1, 2, 3} and hs >= {50, 66, 130}, entry
    # both sides of both grid thresholds, exactly, in training launches
    train = {(c['expect'], c['n']) for c in cases if not c['infer'] and (c['h'], c['w']) == (12, 8)}
    assert train >= {(SPLIT, CN.TAPOUT_MIN_ITEMS - 1), (TAPOUT, CN.TAPOUT_MIN_ITEMS), (SPLIT, CN.TOEP_MIN_TILES - 1), (TOEP, CN.TOEP_MIN_TILES),
                     (SMALL, CN.TOEP_MIN_TILES - 1)}
    for c in cases:
        if not c['infer'] and (c['h'], c['w']) == (12, 8):
            assert CN.tapout_grid_ok(c['n'], 12, 8) == (c['n'] >= CN.TAPOUT_MIN_ITEMS) and CN.toep_grid_ok(c['n'], 12, 8) == (c['n'] >= CN.TOEP_MIN_TILES)
    # the tap-row grid fails where the band grid holds; a channel split of more than 1; an image the launch keeps whole with H % 4 != 0
    both = [c for c in list(cases) + list(R.GROUPED.values()) if not c['infer'] and CN.small_has_tapout(c['k'], c['cin'], c['cout'])
            and not CN.tapout_grid_ok(c['n'] * (c['group'] or 1), c['h'], c['w']) and CN.toep_grid_ok(c['n'] * (c['group'] or 1), c['h'], c['w'])]
    assert {bool(c['group']) for c in both} == {False, True} and all(c['expect'] == TOEP for c in both)
    assert any(c['split'] and R.small_groups(c['cin'], c['n'], c['h'], c['w']) == 8 for c in cases)
    assert any(c['expect'] == TAPOUT and not c['infer'] and c['h'] % 4 for c in cases)
    g = list(R.GROUPED.values())
    assert {c['expect'] for c in g} == {TAPOUT, TOEP, SPLIT} and any(c['h'] % 4 and c['expect'] == TAPOUT for c in g)
    assert len(R.WALK) >= 12 and len({(c['k'], c['cin'], c['cout']) for c in R.WALK.values()}) >= 6


@pytest.mark.parametrize('table', ['cases', 'grouped'])
def test_every_literal_expectation_is_what_route_small_says_and_what_its_entry_accepts(table, monkeypatch):
    for c in (R.CASES if table == 'cases' else R.GROUPED).values():
        monkeypatch.setattr(CN, 'CONV_ARITH', c['arith'])
        groups = R.vector_groups(c)
        want = c['expect'] if c['expect'] != SPLIT else SMALL
        assert routed(c) == want, c['name']
        assert (c['expect'] == SPLIT) == bool(c['split']) == (want == SMALL and groups > 1), (c['name'], groups)
        assert R.ENTRY_ACCEPTS[c['expect']](R.launch_of(c, groups=groups)), c['name']
        if 'not the kernel' in c['name']:                      # ... and the kernel the layer would otherwise take refuses the epilogue
            assert not any(R.ENTRY_ACCEPTS[e](R.launch_of(c)) for e in (TAPOUT, TOEP, NARROW3)), c['name']


# the dense grid: every layer family and its neighbours, planes from one row to untiled 12 and 24 MPix frames and the powers of two at
# which the kernels' size bounds sit (4096 x 4096 = 2^24 pixels; x 16 / 32 / 64 channels = 2^28 .. 2^30 elements)
GRID_K, GRID_CIN, GRID_COUT = (3, 5, 9), (1, 7, 16, 17, 24, 32, 48, 64, 80), (1, 2, 3, 4, 8, 12)
GRID_HW = [(1, 4), (12, 8), (50, 64), (50, 68), (63, 260), (30, 30), (256, 256), (2048, 2048), (3000, 4000), (4000, 6000), (4096, 4096), (4092, 4096),
           (4100, 4096)]
GRID_IMAGES = (1, 2, 32, 127, 128, 255, 256)


def _epilogues(cout):
    e = [(0, 0), (RELU, 0), (NOBIAS, 0), (ADD, cout), (ADD, max(1, cout - 1)), (ADD | RELU | NOBIAS, cout)]
    return e + ([(SHUFFLE2, 0), (SHUFFLE2 | NOBIAS, 0)] if cout % 4 == 0 else [])


def grid():
    for k, cin, cout in itertools.product(GRID_K, GRID_CIN, GRID_COUT):
        if k == 9 and cout > 4:
            continue
        for (h, w), images, infer, mask, (epi, add_c) in itertools.product(GRID_HW, GRID_IMAGES, (False, True), (False, True), _epilogues(cout)):
            if mask and epi & SHUFFLE2:
                continue
            yield dict(k=k, cin=cin, cout=cout, h=h, w=w, n=images, infer=infer, mask=mask, epi=epi & ~NOBIAS | (MASK if mask else 0), add_c=add_c,
                       bias=not (epi & NOBIAS), group=None)


@pytest.mark.parametrize('arith', ['f16x2', 'f32'])
def test_route_small_names_an_entry_that_accepts_the_launch(arith, monkeypatch):
    """over the grid: whatever the vector kernel - the catch-all - accepts is sent to an entry point that accepts it too (the 3x3 tail's
    bound of 2^31 bytes per image side among the conditions: 64 channels of an untiled 3000 x 4000 frame are past it).  The segment height of
    an inference launch is the value ``tapout_seg`` passes, before the library clamps it; a training launch's comes from the library (GPU)."""
    monkeypatch.setattr(CN, 'CONV_ARITH', arith)
    bad, seen = [], set()
    for c in grid():
        launch = R.launch_of(c)
        assert R.accepts_small(launch), c
        entry = routed(c)
        if entry == TAPOUT:
            launch['seg_rows'] = CN.tapout_seg(c['n'], c['h'], c['w'], True) if c['infer'] else 0
        seen.add(entry)
        if not R.ENTRY_ACCEPTS[entry](launch):
            bad.append((entry, c))
    assert not bad, '%d launches are routed to an entry that refuses them, first: %s' % (len(bad), bad[:3])
    assert seen == ({TAPOUT, TOEP, NARROW3, SMALL} if arith == 'f16x2' else {SMALL})


def test_inference_segment_height_does_not_depend_on_the_image():
    """a fixed 64 rows for every inference launch, whatever H (an image of fewer rows is kept whole by the library's clamp): the entry point
    takes 50-row images - H % 4 = 2 - at that value, and would not at min(64, H)"""
    for h in (1, 2, 3, 5, 13, 31, 50, 63, 64, 66, 130):
        seg = CN.tapout_seg(3, h, 68, True)
        assert seg == CN.TAPOUT_INFER_SEG == 64
        assert R.accepts_tapout(dict(k=5, cin=32, cout=3, n=3, h=h, w=68, epi=0, add_c=0, has_add=False, has_mask=False, has_bias=True, seg_rows=seg))
    assert not R.accepts_tapout(dict(k=5, cin=32, cout=3, n=3, h=50, w=68, epi=0, add_c=0, has_add=False, has_mask=False, has_bias=True, seg_rows=6))


def test_per_member_split_follows_route_small(monkeypatch):
    """``small_group_split`` - the decision inside ``_small_split`` - against ``route_small(..., split=None)`` on the grouped grid: a
    matrix-pipe kernel there <=> a code here, and a member launched with that code (one image of the group, the code as ``split``) is sent
    to the very entry the grouped launch takes - the tap-row layers whose grid has band tiles enough and too few tap-row items included"""
    fell = 0
    for arith in ('f16x2', 'f32'):
        monkeypatch.setattr(CN, 'CONV_ARITH', arith)
        for c in grid():
            if c['infer'] or c['mask']:
                continue
            epi = c['epi'] | (0 if c['bias'] else NOBIAS)
            assert CN.small_packs(c['k'], c['cin'], c['cout'], epi, bool(epi & ADD)) == R.pack_flags(CN, c['k'], c['cin'], c['cout'], epi, bool(epi & ADD))
            grouped = routed(c)
            code = CN.small_group_split(c['k'], c['cin'], c['cout'], c['h'], c['w'], c['n'], epi, bool(epi & ADD))
            assert (code is not None) == (grouped != SMALL), (arith, c, grouped, code)
            member = routed(c, images=1, split=code if code is not None else 1)
            assert member == grouped, (arith, c, grouped, member, code)
            fell += grouped == TOEP and CN.small_has_tapout(c['k'], c['cin'], c['cout']) and not (epi & SHUFFLE2)
    assert fell > 0


MOVED = 1e-3          # 200 x the widest bar of the GPU test (5e-6 of max|ref|)


@pytest.mark.parametrize('wrong', sorted(R.WRONG))
def test_reference_tells_wrong_operations_apart(wrong):
    cases = [c for c in R.ALL.values() if R.WRONG[wrong](c)]
    assert len(cases) >= 8, wrong
    if wrong == 'flip':                                         # (every case has taps: every layer, direction and epilogue once is enough)
        seen, few = set(), []
        for c in sorted(cases, key=lambda c: c['n'] * c['h'] * c['w']):
            key = (c['k'], c['cin'], c['cout'], c['transpose'], c['epi'])
            if key not in seen:
                seen.add(key)
                few.append(c)
        cases = few
    for c in cases:
        ref, bad = R.ref64(c), R.reference(c, torch.float64, wrong=wrong)
        moved = (ref - bad).abs().max().item() / ref.abs().max().item()
        assert moved > MOVED, (wrong, c['name'], moved)


def test_reference_in_float32_is_within_the_bars_of_float64_and_shapes_hold():
    """the restatement itself: its float32 evaluation is a valid fp32 implementation, so it sits inside the vector kernel's bar"""
    for c in list(R.WALK.values()) + [c for c in R.CASES.values() if c['n'] <= 3 and c['h'] <= 50][::7]:
        ref = R.ref64(c)
        assert tuple(ref.shape) == R.out_shape(c) and torch.isfinite(ref).all()
        e = (R.reference(c, torch.float32).double() - ref).abs().max().item() / ref.abs().max().item()
        assert e < R.BAR[SMALL], (c['name'], e)


def test_long_chains_split_whatever_the_grid_and_the_mode():
    """``small_chain_groups`` is a function of the layer: 9x9 with 32 channels or more in groups of 16 (at most 8), nothing else - and the
    table holds such layers on the vector kernel in inference, with a mask, under the fp32 arithmetic and with W % 4 != 0"""
    for k, cin in itertools.product((3, 5, 9), (1, 7, 16, 17, 24, 31, 32, 48, 64, 80, 128, 256)):
        for n in (1, 3, 256, 8191, 8192):
            want = min(8, cin // 16) if k == 9 and cin >= 32 else 1
            assert CN.small_chain_groups(k, cin, n) == R.chain_groups(k, cin, n) == (want if n * want <= 65535 else 1), (k, cin, n)
    long_ = [c for c in R.CASES.values() if c['infer'] and c['expect'] == SPLIT]
    assert long_ and all(c['k'] == 9 and c['cin'] == 64 for c in long_)
    assert any(c['mask'] for c in long_) and any(c['arith'] == 'f32' for c in long_) and any(c['w'] % 4 for c in long_)
    assert not any(c['infer'] and c['expect'] == SMALL and c['k'] == 9 and c['cin'] >= 32 for c in R.CASES.values())


def test_small_groups_restatement():
    assert R.small_groups(64, 2, 24, 64) == 8 and R.small_groups(32, 127, 12, 8) == 4 and R.small_groups(16, 2, 24, 64) == 1
    assert R.small_groups(64, 255, 12, 8) == 4 and R.small_groups(64, 768, 12, 8) == 1 and R.small_groups(64, 600, 12, 8) == 1
