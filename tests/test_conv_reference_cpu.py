"""Without a GPU: the case table of tests/conv_reference.py reaches what it claims to reach, every literal expectation is what
``convnets.route`` names and what that entry's own argument checks (``ENTRY_ACCEPTS``, restated from the library) accept, the size
boundaries of the split-precision entries hold as pure functions of large planes, the float64 restatement agrees with autograd and
with torch's PixelShuffle / PixelUnshuffle and tells wrong operations apart, and the float32 yardstick of every case stays far
below the cap of the accuracy rule."""
import pytest
import torch
import torch.nn.functional as TF

import conv_reference as R
from conv_reference import (ADD, CASEBIAS, CONSTCH, F16X2, GEN, K3, MASK, NOBIAS, PLAIN, RELU, SHUFFLE2, TF1, TF1X, THIN5, UNSHUFFLE2, W43,
                            W45)
from reconfigisp_amd import convnets as CN


def switches(monkeypatch, c):
    monkeypatch.setattr(CN, 'CONV_ARITH', c['arith'])
    monkeypatch.setattr(CN, 'TOEP_FIRST', c['toep'])


def test_the_bits_are_the_library_s():
    assert (RELU, ADD, MASK, SHUFFLE2, NOBIAS, CASEBIAS) == (CN.EPI_RELU, CN.EPI_ADD, CN.EPI_MASK, CN.EPI_SHUFFLE2, CN.EPI_NOBIAS, CN.EPI_CASEBIAS)
    assert (PLAIN, UNSHUFFLE2, CONSTCH) == (CN.LOAD_PLAIN, CN.LOAD_UNSHUFFLE2, CN.LOAD_CONSTCH)
    from reconfigisp_amd import lib as L
    assert (R.SHARED_X, R.SHARED_ADD) == (L.GROUP_SHARED_X, L.GROUP_SHARED_ADD)


@pytest.mark.parametrize('table', ['cases', 'grouped'])
def test_every_literal_expectation_is_what_route_says_and_what_its_entry_accepts(table, monkeypatch):
    """... and nothing is left out: a case may be omitted only when the expected entry's own checks reject it, at most 2 % of the table"""
    cases = list((R.CASES if table == 'cases' else R.GROUPED).values())
    omitted = 0
    for c in cases:
        switches(monkeypatch, c)
        assert R.routed(c) == c['expect'], (c['name'], R.routed(c))
        if not R.ENTRY_ACCEPTS[c['expect']](R.launch_of(c)):
            omitted += 1
        if 'not the' in c['name']:                            # the kernel the layer would otherwise take refuses the epilogue
            pref = R.routed(dict(c, epi=c['epi'] & ~(ADD | MASK)))
            assert pref != c['expect'] and not R.ENTRY_ACCEPTS[pref](R.launch_of(c)), c['name']
    print('%s: %d cases, %d left out by ENTRY_ACCEPTS' % (table, len(cases), omitted))
    assert omitted == 0 and omitted <= 0.02 * len(cases)


def test_walk_is_routed_to_entries_that_accept_it(monkeypatch):
    seen = set()
    for c in R.WALK.values():
        switches(monkeypatch, c)
        entry = R.routed(c)
        seen.add(entry)
        assert R.ENTRY_ACCEPTS[entry](R.launch_of(c)), (c['name'], entry)
    assert len(R.WALK) >= 4 * R.SEEDS and len(seen) >= 4


def test_table_reaches_every_entry_instance_form_epilogue_and_boundary(monkeypatch):
    cases = list(R.CASES.values())
    by = lambda e: [c for c in cases if c['expect'] == e]
    entries = {c['expect'] for c in cases}
    inst = {R.gen_instance(c) for c in by(GEN)}
    print('coverage: entries %d/%d, risp_conv2d instances %d/%d' % (len(entries & set(R.ENTRIES)), len(R.ENTRIES), len(inst & R.GEN_INSTANCES),
                                                                   len(R.GEN_INSTANCES)))
    assert entries == set(R.ENTRIES) and inst == R.GEN_INSTANCES
    assert {c['expect'] for c in R.GROUPED.values()} == {W45, F16X2, THIN5, K3, TF1, TF1X, GEN}
    # the general kernel's two switches, independently: staging by x, stores by y | add | mask
    assert {(R.gen_instance(c)[3], R.gen_vector_stores(c)) for c in by(GEN)} == {(True, True), (True, False), (False, True), (False, False)}
    assert {c['misalign'] for c in by(GEN)} == {None, 'x', 'out', 'add', 'mask'}
    assert {c['cin'] % R.gen_instance(c)[1] for c in by(GEN)} > {0} and {c['cin'] for c in by(GEN)} >= {5, 13, 17}
    assert {c['cout'] for c in by(GEN)} >= {13, 31, 33, 48, 64}
    assert {c['w'] % 4 for c in by(GEN)} == {0, 2} and {(c['n'], c['h'], c['w']) for c in by(GEN)} >= set(R.ODD + R.GEOMS + R.TINY)
    assert {c['cout'] for c in by(GEN) if c['epi'] & SHUFFLE2} >= {16, 64}
    assert {c['cin'] for c in by(GEN) if c['load'] == UNSHUFFLE2} >= {8, 64}
    assert {c['cin'] - 12 for c in by(GEN) if c['load'] == CONSTCH and c['k'] == 9 and c['cin_img'] == 3} == {0, 1, 5}
    srcnn = [c for c in by(GEN) if c['transpose'] and c['k'] == 9 and c['cin'] == 64 and c['epi'] == ADD and c['add_c'] == 3]
    assert {c['cout'] - 12 for c in srcnn} == {0, 1, 5}
    # border-case tables on the general kernel: tiles that see one case only, tiles at the edge, and the element form where H != W
    cb = [c for c in by(GEN) if c['epi'] & CASEBIAS]
    interior = lambda c: any(x0 >= c['k'] // 2 and y0 >= c['k'] // 2 and x0 + 32 <= c['w'] - c['k'] // 2 and y0 + 16 <= c['h'] - c['k'] // 2
                             for x0 in range(0, c['w'], 32) for y0 in range(0, c['h'], 16))
    assert any(interior(c) and R.gen_vector_stores(c) for c in cb) and any(not interior(c) and R.gen_vector_stores(c) for c in cb)
    assert any(not R.gen_vector_stores(c) and c['h'] != c['w'] for c in cb) and any(c['epi'] & RELU for c in cb) and any(not c['epi'] & RELU for c in cb)
    # Winograd: both cout-block forms of F(4,3) and its two single-block forms; the channel counts of the issue
    assert {R.wino43_form(c) for c in by(W43)} == {'b2', 'glds', 'plain'}
    assert any(R.wino43_form(c) == 'plain' and c['cout'] > 32 for c in by(W43))
    assert {c['cin'] for c in by(W43)} >= {64, 17, 4} and {c['cout'] for c in by(W43)} >= {64, 33, 32, 20}
    assert {c['cin'] for c in by(W45)} >= {64, 12, 3, 1} and {c['cout'] for c in by(W45)} >= {64, 40, 32}
    assert {(c['k'], c['cin'], c['cout']) for c in by(F16X2)} >= {(k, ci, co) for k in (3, 5) for ci in (16, 32, 64) for co in (32, 64)
                                                                  if (k, ci, co) not in ((5, 16, 64), (3, 32, 32), (5, 32, 32))}
    assert {(c['k'], c['cin'], c['cout']) for c in by(F16X2)} >= {(3, 32, 32), (5, 32, 32)} and all(c['scale'] for c in by(F16X2))
    assert {(c['cin'], c['cout']) for c in by(THIN5)} == {(ci, co) for ci in (1, 2, 3) for co in (32, 64)}
    # every subset of RELU / ADD / MASK the entry takes; a residual narrower than the layer leaves the split-precision kernel
    for entry, bits in ((GEN, R.SUBSETS), (W43, R.SUBSETS), (W45, R.SUBSETS), (F16X2, R.SUBSETS), (THIN5, (0, RELU, MASK, RELU | MASK))):
        got = {c['epi'] & (RELU | ADD | MASK) for c in by(entry)}
        assert got >= set(bits), (entry, got)
        assert any(c['epi'] & NOBIAS for c in by(entry)) and {c['transpose'] for c in by(entry)} == {False, True}, entry
    for entry in (GEN, W43, W45):
        assert any(c['epi'] & ADD and c['add_c'] < c['cout'] for c in by(entry)), entry
    assert any(c['epi'] & ADD and c['add_c'] < c['cout'] and 'f16x2' in CN.pack_kinds(*R.layer_of(c), c['transpose']) and c['arith'] == 'f16x2'
               for c in by(W43) + by(W45))
    # first layers: both kernel forms, both loads and taps, the three widths, and rule 1 under every switch
    first = by(K3) + by(TF1) + by(TF1X)
    forms = {CN.first_layer_form(c['cin'], c['cout'], c['h'], c['w'], c['load'] == UNSHUFFLE2) for c in by(TF1) + by(TF1X)}
    assert forms == {'xwin', 'band'}
    assert {(c['k'], c['cin'], c['load']) for c in first} == {(3, 3, PLAIN), (9, 3, PLAIN), (3, 4, UNSHUFFLE2), (9, 4, UNSHUFFLE2)}
    assert {c['cout'] for c in first} == {20, 40, 64}
    want = {(k, ld, ar, tp, inf) for k in (3, 9) for ld in (PLAIN, UNSHUFFLE2) for ar in ('f16x2', 'f32') for tp in ('0', 'infer', 'train', 'plain')
            for inf in (False, True)}
    assert {(c['k'], c['load'], c['arith'], c['toep'], c['infer']) for c in first} == want
    for entry in (K3, TF1, TF1X):
        assert {c['epi'] & (CASEBIAS | RELU) for c in by(entry)} >= {0, RELU, CASEBIAS, CASEBIAS | RELU} and any(c['epi'] & NOBIAS for c in by(entry))
    assert any((c['h'], c['w']) == (8, 8) for c in by(TF1)) and any((c['h'], c['w']) == (8, 8) for c in by(K3))
    assert any((c['k'], c['h'], c['w']) == (3, 2, 4) for c in by(K3))
    # geometry: the siblings' list and the smallest planes on every entry that has no halo condition; many work items per workgroup
    for entry in (GEN, W43, W45, F16X2, THIN5):
        assert {(c['n'], c['h'], c['w']) for c in by(entry)} >= set(R.GEOMS + R.TINY), entry
    for entry in (K3, TF1):
        assert {(c['n'], c['h'], c['w']) for c in by(entry)} >= set(R.GEOMS), entry
    assert {c['expect'] for c in cases if c['n'] >= 150} == {F16X2, THIN5, TF1, TF1X}
    # grouped launches: 2 and 3 members, with and without a shared input, a shared residual wherever the entry takes one
    for entry in {c['expect'] for c in R.GROUPED.values()}:
        g = [c for c in R.GROUPED.values() if c['expect'] == entry]
        assert {c['group'] for c in g} == {2, 3} and {c['gflags'] & R.SHARED_X for c in g} == {0, R.SHARED_X}, entry
        assert any(c['gflags'] & R.SHARED_ADD for c in g) == (entry in (GEN, W45, F16X2)), entry
    assert not any(c['k'] == 3 for c in R.GROUPED.values())


def _probe(k, cin, cout, h, w, **kw):
    c = dict(name='probe', k=k, cin=cin, cout=cout, n=1, h=h, w=w, expect=None, epi=0, add_c=0, load=PLAIN, cin_img=0, transpose=False, infer=True,
             arith='f16x2', toep='train', misalign=None, group=None, gflags=0, scale=False)
    c.update(kw)
    return c


def test_both_sides_of_every_boundary_of_route(monkeypatch):
    """the boundaries a small shape reaches are in the table (W % 4, the halo of the first layers, cin % 16, cout 32 | 64, cin <= 3,
    cin % 4, add_c == cout, alignment, the direction, the switches); the three size bounds are checked here only, through ``route`` and
    ``ENTRY_ACCEPTS`` as pure functions of large planes - they are never launched"""
    monkeypatch.setattr(CN, 'CONV_ARITH', 'f16x2')
    monkeypatch.setattr(CN, 'TOEP_FIRST', 'train')
    # small shapes, one step either side
    for a, b, kw_a, kw_b in (
            (F16X2, W43, dict(cin=16), dict(cin=12)), (F16X2, W43, dict(cout=32), dict(cout=33)), (F16X2, W43, dict(cout=64), dict(cout=63)),
            (F16X2, GEN, dict(w=68), dict(w=66)), (F16X2, W43, dict(epi=ADD, add_c=32), dict(epi=ADD, add_c=31)),
            (F16X2, GEN, {}, dict(misalign='mask')), (F16X2, GEN, {}, dict(epi=SHUFFLE2)), (F16X2, GEN, {}, dict(load=CONSTCH, cin_img=3))):
        base = dict(k=3, cin=32, cout=32, h=13, w=68)
        assert R.routed(_probe(**dict(base, **kw_a))) == a and R.routed(_probe(**dict(base, **kw_b))) == b, (kw_a, kw_b)
    for a, b, kw_a, kw_b in ((THIN5, W45, dict(cin=3), dict(cin=4)), (THIN5, W45, dict(cout=32), dict(cout=40)), (THIN5, W45, {}, dict(epi=ADD, add_c=32)),
                             (THIN5, GEN, dict(w=68), dict(w=70)), (W45, GEN, dict(cin=4, cout=40), dict(cin=5, cout=40)), (THIN5, GEN, {}, dict(misalign='x'))):
        base = dict(k=5, cin=3, cout=32, h=13, w=68)
        assert R.routed(_probe(**dict(base, **kw_a))) == a and R.routed(_probe(**dict(base, **kw_b))) == b, (kw_a, kw_b)
    for a, b, kw_a, kw_b in ((TF1, GEN, dict(h=8), dict(h=7)), (TF1, GEN, dict(w=8), dict(w=4)), (TF1, GEN, dict(cin=3), dict(cin=5)),
                             (TF1, GEN, {}, dict(epi=MASK)), (TF1, TF1X, {}, dict(infer=False)), (TF1, GEN, {}, dict(load=UNSHUFFLE2, cin=8)),
                             (TF1, GEN, dict(load=UNSHUFFLE2, cin=4), dict(cin=4)), (TF1, GEN, {}, dict(misalign='out'))):
        base = dict(k=9, cin=3, cout=20, h=8, w=8)
        assert R.routed(_probe(**dict(base, **kw_a))) == a and R.routed(_probe(**dict(base, **kw_b))) == b, (kw_a, kw_b)
    assert R.routed(_probe(3, 3, 20, 2, 4)) == K3 and R.routed(_probe(3, 3, 20, 1, 4)) == W43
    # 2^31 bytes per image side: risp_conv2d_f16x2 (max(cin, cout) planes), risp_conv2d_thin5 (cout planes)
    for k, cin, cout, entry, below in ((3, 64, 64, F16X2, W43), (5, 64, 32, F16X2, W45), (5, 3, 32, THIN5, W45), (5, 3, 64, THIN5, W45)):
        planes = max(cin, cout) if entry == F16X2 else cout
        h = 2048
        w = 2 ** 29 // (planes * h)                                                # planes * h * w * 4 == 2^31 exactly
        inside, outside = _probe(k, cin, cout, h, w - 4), _probe(k, cin, cout, h, w)
        assert R.routed(inside) == entry and R.ENTRY_ACCEPTS[entry](R.launch_of(inside)), (k, cin, cout)
        assert R.routed(outside) == below and not R.ENTRY_ACCEPTS[entry](R.launch_of(outside)), (k, cin, cout)
        assert R.ENTRY_ACCEPTS[below](R.launch_of(outside))
        if entry == F16X2:
            assert CN.f16x2_addressable(cin, cout, h, w - 4) and not CN.f16x2_addressable(cin, cout, h, w)
    # 2^30 input elements per image: risp_conv2d_toep_first; beyond, the fp32 first-layer kernel
    for cin, load in ((3, PLAIN), (4, UNSHUFFLE2)):
        h = 4096
        w = (2 ** 30 // (cin * h) + 3) // 4 * 4                                     # the first W % 4 == 0 with cin * h * w >= 2^30
        inside, outside = _probe(9, cin, 20, h, w - 4, load=load), _probe(9, cin, 20, h, w, load=load)
        assert cin * h * (w - 4) < 2 ** 30 <= cin * h * w
        assert R.routed(inside) == TF1 and R.ENTRY_ACCEPTS[TF1](R.launch_of(inside))
        assert R.routed(outside) == K3 and not R.ENTRY_ACCEPTS[TF1](R.launch_of(outside)) and R.ENTRY_ACCEPTS[K3](R.launch_of(outside))
    # ... whose exact form counts its outputs in 32 bits: ``conv`` itself falls back to the plain form
    big = _probe(9, 3, 64, 4096, 4096, infer=False, n=4)
    assert CN.route(9, 3, 64, 4096, 4096, False, PLAIN, 0, 0, False, True, R.have_of(big)) == TF1X and R.routed(big) == TF1
    assert not R.ENTRY_ACCEPTS[TF1X](R.launch_of(big)) and R.ENTRY_ACCEPTS[TF1](R.launch_of(big))
    # inference launches never take the exact form: batch independence is asked of the seven entries an inference launch reaches
    for tp in ('0', 'infer', 'train', 'plain'):
        monkeypatch.setattr(CN, 'TOEP_FIRST', tp)
        assert R.routed(_probe(9, 3, 20, 13, 68)) != TF1X


def test_route_only_names_entries_that_accept_the_launch(monkeypatch):
    """over a dense grid of layers, planes, loads, epilogues, directions and switches: whatever the general kernel - the catch-all -
    accepts is sent to an entry point that accepts it too"""
    seen, bad = set(), []
    for arith, toep in (('f16x2', 'train'), ('f16x2', 'infer'), ('f16x2', '0'), ('f32', 'plain')):
        monkeypatch.setattr(CN, 'CONV_ARITH', arith)
        monkeypatch.setattr(CN, 'TOEP_FIRST', toep)
        for k in (1, 3, 5, 9):
            for cin in (1, 3, 4, 5, 12, 16, 17, 64):
                for cout in (13, 20, 32, 33, 64):
                    for (h, w) in ((1, 4), (2, 4), (7, 8), (8, 8), (13, 68), (9, 10), (2048, 4096), (4096, 8192)):
                        for load in (PLAIN, UNSHUFFLE2, CONSTCH):
                            if (load == UNSHUFFLE2 and cin % 4) or (load == CONSTCH and cin < 4):
                                continue
                            for epi, add_c in ((0, 0), (RELU | NOBIAS, 0), (ADD, cout), (ADD | MASK, cout - 1), (CASEBIAS | RELU, 0), (SHUFFLE2, 0)):
                                if epi & SHUFFLE2 and cout % 4:
                                    continue
                                for transpose, infer, mis in ((False, True, None), (False, False, None), (True, False, None), (False, True, 'x')):
                                    c = _probe(k, cin, cout, h, w, load=load, cin_img=3 if load == CONSTCH else 0, epi=epi, add_c=add_c,
                                               transpose=transpose, infer=infer, misalign=mis, arith=arith, toep=toep)
                                    if not R.accepts_gen(R.launch_of(c)):
                                        continue
                                    entry = R.routed(c)
                                    seen.add(entry)
                                    if not R.ENTRY_ACCEPTS[entry](R.launch_of(c)):
                                        bad.append((entry, {f: c[f] for f in ('k', 'cin', 'cout', 'h', 'w', 'load', 'epi', 'transpose', 'infer', 'misalign')}))
    assert not bad, '%d launches are routed to an entry that refuses them, first: %s' % (len(bad), bad[:3])
    assert seen == set(R.ENTRIES)


def test_restatement_agrees_with_autograd_and_with_torch_s_shuffles():
    g = torch.Generator().manual_seed(5)
    z = torch.randn(2, 8, 3, 5, generator=g, dtype=torch.float64)
    assert torch.equal(R.shuffle2(z), TF.pixel_shuffle(z, 2)) and not torch.equal(R.shuffle2(z, swapped=True), TF.pixel_shuffle(z, 2))
    x = torch.randn(2, 3, 6, 10, generator=g, dtype=torch.float64)
    assert torch.equal(R.unshuffle2(x), TF.pixel_unshuffle(x, 2)) and torch.equal(R.shuffle2(R.unshuffle2(x)), x)
    assert [R.border_case(v, 10, 2) for v in range(10)] == [0, 1, 2, 2, 2, 2, 2, 2, 3, 4] and [R.border_case(v, 2, 1) for v in range(2)] == [0, 2]
    for name in ('wino43 backward-data 3x3_33to17 3x13x68', 'gen srcnn backward-data P=1 9x9_64to13 2x13x68', 'thin5 backward-data 5x5_1to64 3x13x68'):
        c = R.CASES[name]                                   # backward-data = the gradient of the forward layer with respect to its input
        d = R.inputs(c)
        xin = torch.zeros(c['n'], c['cout'], c['h'], c['w'], dtype=torch.float64, requires_grad=True)
        y = TF.conv2d(xin, d['weights'][0].double(), padding=c['k'] // 2)
        gx, = torch.autograd.grad(y, xin, d['x'].double())
        got = R.reference(dict(c, epi=0), torch.float64)
        assert torch.allclose(got, gx, rtol=1e-12, atol=1e-12), name
    # the border-case table is what the constant planes of a CONSTCH load contribute (convnets.srcnn_fold_tables builds it so)
    c = R.CASES['gen constch srcnn P=1 9x9_13to64 2x13x68']
    d = R.inputs(c)
    rcase, _ = CN.srcnn_fold_tables(d['weights'][0].double())
    table = (d['cvals'].double() @ rcase).view(c['n'], c['cout'], 9, 9)
    iy = torch.tensor([R.border_case(v, c['h'], 4) for v in range(c['h'])])
    ix = torch.tensor([R.border_case(v, c['w'], 4) for v in range(c['w'])])
    folded = torch.relu(TF.conv2d(d['x'].double(), d['weights'][0][:, :3].double(), d['bias'][0].double(), padding=4) + table[:, :, iy][:, :, :, ix])
    assert torch.allclose(folded, R.ref64(c), rtol=1e-10, atol=1e-10)


MOVED = 1e-3          # 10 x the cap of the accuracy rule (1e-4 of max|ref|), 200 x the widest split-precision bar


@pytest.mark.parametrize('wrong', sorted(R.WRONG))
def test_reference_tells_wrong_operations_apart(wrong):
    cases = [c for c in R.EVERY.values() if R.WRONG[wrong](c) and c['n'] * c['h'] * c['w'] <= 8000]
    seen, few = set(), []
    for c in sorted(cases, key=lambda c: c['n'] * c['h'] * c['w'] * c['cin'] * c['cout']):
        key = (c['k'], c['transpose'], c['epi'], c['load'], bool(c['group'])) if wrong in ('flip', 'bias') else c['name']
        if key not in seen:
            seen.add(key)
            few.append(c)
    assert len(few) >= 6, wrong
    for c in few[:40]:
        ref, bad = R.ref64(c), R.reference(c, torch.float64, wrong=wrong)
        moved = (ref - bad).abs().max().item() / ref.abs().max().item()
        assert moved > MOVED, (wrong, c['name'], moved)


def test_float32_yardstick_stays_far_below_the_cap(monkeypatch):
    """E32 <= 2.5e-5 on every case, so that min(2 * E32, 1e-4) never binds at the cap; shapes hold; the yardstick of the Winograd entries is
    the emulation of their kernels on float32 tensors (printed beside torch's direct float32 convolution)"""
    worst, ratio = {}, []
    for c in R.EVERY.values():
        switches(monkeypatch, c)
        entry = c['expect'] or R.routed(c)
        ref = R.ref64(c)
        assert tuple(ref.shape) == R.out_shape(c) and torch.isfinite(ref).all(), c['name']
        e = R.E32(c, entry)
        assert 0 < e <= 2.5e-5, (c['name'], entry, e)
        worst[entry] = max(worst.get(entry, 0.0), e)
        if entry in (W43, W45) and c['n'] * c['h'] * c['w'] <= 3000:
            ratio.append(e / R.E32(c, GEN))
    print('largest E32 per entry: ' + ', '.join('%s %.2e' % (e.replace('risp_conv2d', '') or 'general', v) for e, v in sorted(worst.items())))
    print('Winograd emulation in float32 against the direct float32 convolution, E32 ratio: median %.2f over %d cases' % (
        sorted(ratio)[len(ratio) // 2], len(ratio)))
    assert set(worst) == set(R.ENTRIES) and len(ratio) >= 20
