"""The float64 statement of the scene route (tests/serve_scene_reference.py) and its case table (tests/serve_scene_cases.py),
checked without a GPU: the table covers its axes, every input stays under the tie caps, the three scene stages agree with
the oracle, the recorded E32 / CONST_E32 are what the float32 evaluation costs, that evaluation passes the comparison rule,
``scene_plan`` names the route for the right module lists and leaves ``serve_route`` / ``serve_plan`` alone, and the rule
tells wrong variants of the scene stages apart."""
import numpy as np
import pytest
import torch

import isp_oracle as O
import serve_reference as S
import serve_scene_cases as T
import serve_scene_reference as SC
import test_serve_route_cpu as ROUTE

ALL = [('sweep', i) for i in range(len(T.CASES))] + [('walk', s) for s in range(T.WALK)]


def _case(kind, i):
    return T.sweep_case(i) if kind == 'sweep' else T.walk_case(i)


def test_tables_agree_with_the_package():
    import reconfigisp_amd.functional as F
    assert (SC.SCENE_STAT[SC.GRAYWORLD], SC.SCENE_STAT[SC.WHITEWORLD], SC.SCENE_STAT[SC.REINHARD]) == (
        F.SCENE_MEAN3, F.SCENE_MAX3, F.SCENE_LOGLUM)
    assert (SC.SCENE_OP[SC.GRAYWORLD], SC.SCENE_OP[SC.WHITEWORLD], SC.SCENE_OP[SC.REINHARD]) == (
        F.OP_GAIN3, F.OP_GAIN3_Q8, F.OP_TONE_REINHARD)


def test_table_covers_its_axes():
    assert 60 <= len(T.CASES) <= 90 and T.WALK == 8
    black = lambda c: c[1].split('/')[1] != '0'
    assert {(c[2], c[3], black(c)) for c in T.CASES} == {(p, k, b) for p in S.SITES for k in S.DEMOSAIC for b in (False, True)}
    assert {c[0] for c in T.CASES} == set(T.SHAPES) and {c[1] for c in T.CASES} == set(T.DEPTHS) and {c[5] for c in T.CASES} == {0, 1}
    assert {c[4] for c in T.CASES} == set(T.PIPES)
    scene_of = lambda ops: [op for op in ops if op in SC.SCENE]
    for stage in SC.SCENE:
        pipes = [p for p in T.PIPES.values() if stage in p]
        assert any(p == [stage] for p in pipes), 'directly behind the demosaic'
        assert any(T.WQ in p[:p.index(stage)] for p in pipes), 'behind a prefix with WbQuadratic'
        assert any(p[-1] != stage for p in pipes), 'followed by a tail'
        # every shape and every demosaic kind meets every statistic
        assert {c[0] for c in T.CASES if stage in T.PIPES[c[4]]} == set(T.SHAPES)
        assert {c[3] for c in T.CASES if stage in T.PIPES[c[4]]} == set(S.DEMOSAIC)
    pairs = {tuple(scene_of(p)) for p in T.PIPES.values()}
    assert (SC.GRAYWORLD, SC.REINHARD) in pairs and (SC.WHITEWORLD, SC.GRAYWORLD) in pairs
    assert all(1 <= len(scene_of(p)) <= 2 and len(p) <= 8 for p in T.PIPES.values())
    raw = T.T.make_raw(3, 4, 8, 1023, 64, 1)
    assert (raw[1] == 0).all() and len(np.unique(raw[2])) == 1


@pytest.mark.parametrize('kind,i', ALL)
def test_inputs_stay_under_the_caps_and_fp32_passes_the_rule(kind, i):
    case = _case(kind, i)
    inner, loose = S.tie_shares(case['ref'], T.TAU)
    assert inner <= S.TIE_CAP and loose <= S.FINAL_CAP, case['what']
    bad, rep = S.check(T.reference(case, np.float32).bytes, case['ref'], T.TAU)
    assert not bad, '%s: the float32 evaluation breaks the rule: %s' % (case['what'], '; '.join(bad))


def measure(case, worst, worst_const):
    """serve_space's measure_e32 over the main world's points, and the relative error of every scene stage's float32
    constants (every segment, statistics included, started from the float64 run's codes)"""
    r64 = case['ref']
    r32 = T.reference(case, np.float32, sync=r64)
    for k, (kind, unq, _) in enumerate(r64.points[:r64.n_points]):
        e = np.where((unq >= -0.5) & (unq <= 255.5), np.abs(r32.points[k][1].astype(np.float64) - unq), 0.0)
        worst[kind] = max(worst.get(kind, 0.0), e.max())
    if r64.final_kind:
        m = ~np.isnan(r64.final_t) & ~np.isnan(r32.final_t) & (r64.final_t >= 0) & (r64.final_t <= 256)
        if m.any():
            key = 'final/' + r64.final_kind
            worst[key] = max(worst.get(key, 0.0), np.abs(r32.final_t - r64.final_t)[m].max())
    stages = [op for op in case['ops'] if op in SC.SCENE]
    for stage, c64, c32 in zip(stages, r64.consts, r32.consts):
        rel = np.abs(c32.astype(np.float64) - c64) / np.maximum(np.abs(c64), 1e-30)
        worst_const[SC.SCENE_STAT[stage]] = max(worst_const.get(SC.SCENE_STAT[stage], 0.0), rel.max())


def test_recorded_e32_is_the_fp32_references_error():
    assert all(T.TAU[k] == 2.0 * T.E32[k] for k in T.E32) and all(T.CONST_TAU[k] == 2.0 * T.CONST_E32[k] for k in T.CONST_E32)
    worst, worst_const = {}, {}
    for kind, i in ALL:
        measure(_case(kind, i), worst, worst_const)
    print({k: '%.3e' % v for k, v in sorted(worst.items())}, {k: '%.3e' % v for k, v in sorted(worst_const.items())})
    assert set(worst) == set(T.E32) and set(worst_const) == set(T.CONST_E32)
    for rec, got in ((T.E32, worst), (T.CONST_E32, worst_const)):
        for k, e in got.items():
            assert e <= rec[k], '%s: measured %.3e, recorded %.3e' % (k, e, rec[k])
            assert e >= rec[k] / 1.25, '%s: recorded %.3e is wider than the measured %.3e' % (k, rec[k], e)


# ---------------------------------------------------------------------------------------------------- agreement
def test_scene_stages_are_the_oracles():
    n = 4
    x = np.random.default_rng(7).uniform(0.0, 1.3, size=(n, 3, 6, 8))
    x[1] = 0.0
    xt = torch.from_numpy(x)
    g = SC.grayworld_gains(x)
    assert np.abs(np.clip(x * g[:, :, None, None], 0, 1) - O.grayworld(xt).numpy()).max() <= 1e-12
    ratio = np.array([0.0, 1.0, 0.3, 0.7])
    wp, mg = np.array([0.0, 0.005, 1.0, 0.4]), np.array([0.18, 0.005, 1.0, 0.5])
    with O.unquantized():
        ww = O.origin_whiteworld(xt * 255.0, ratio).numpy()
        rh = O.origin_tonemap(xt * 255.0, 'reinhard', {'white_point': wp, 'middle_grey': mg}).numpy()
    assert np.abs(x * SC.whiteworld_gains(x, ratio)[:, :, None, None] * 255.0 - ww).max() <= 1e-9
    p0, p1 = SC.reinhard_constants(x, wp, mg)
    assert np.abs(SC.reinhard_raw(x, p0, p1) - rh).max() <= 1e-9 * max(1.0, np.abs(rh).max())


# ---------------------------------------------------------------------------------------------------- scene_plan
NAMES = {'wb': 'wbmanual', 'gtm': 'gtmmanual', 'wbq': 'wbquadratic', 'gw': 'grayworld', 'ww': 'whiteworld', 'rh': 'reinhard',
         'crysis': 'crysisengine'}


def _mods(names):
    return ROUTE.modules(*[NAMES.get(n, n) for n in names])


PLANS = [
    (['bilinear', 'gw', 'gamma'], ('bilinear', [1, 2], [True, False])),
    (['skip', 'laplacian', 'ww', 'rh', 'gamma'], ('laplacian', [2, 3, 4], [True, True, False])),
    (['nearest', 'skip', 'gw'], ('nearest', [2], [True])),
    (['nearest', 'wb', 'wbq', 'crysis', 'filmic', 'rh'], ('nearest', [1, 2, 3, 4, 5], [False, False, False, False, True])),
    (['bilinear', 'gamma'], None),                                    # no scene stage: serve_route's business
    (['nearest', 'gw', 'ww', 'rh'], None),                            # three scene stages
    (['gw', 'nearest'], None),                                        # no demosaic in front
    (['bilinear', 'bilateral', 'gw'], None),                          # a stage the launch cannot hold
    (['nearest', 'median', 'rh'], None),
    (['bilinear'] + ['gamma'] * 8 + ['gw'], None),                    # more than MAX_CHAIN stages
    (['bilinear'] + ['gamma'] * 7 + ['gw'], ('bilinear', list(range(1, 9)), [False] * 7 + [True])),
    ([], None),
]


@pytest.mark.parametrize('names,want', PLANS, ids=lambda v: '-'.join(v) if isinstance(v, list) else None)
def test_scene_plan(names, want):
    from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF
    got = PF.scene_plan(_mods(names))
    assert got == want if want is None else (got[0], list(got[1]), list(got[2])) == want


def test_scene_plan_leaves_the_existing_routes_alone():
    """every COMPOSED list of tests/test_serve_route_cpu.py without a scene stage has no scene plan; with one,
    serve_route / serve_plan still say 'composed': the route is opt-in"""
    from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF
    scene = {'grayworld', 'whiteworld', 'reinhard'}
    plain = [names for names in ROUTE.COMPOSED if not scene & set(names)]
    assert len(plain) >= 20 and len(plain) < len(ROUTE.COMPOSED)
    for names in plain:
        assert PF.scene_plan(ROUTE.modules(*names)) is None, names
    for names in ROUTE.FUSED + ROUTE.CLASSICAL:
        assert PF.scene_plan(ROUTE.modules(*names)) is None, names
    for names in ROUTE.COMPOSED:                       # the lists with a scene stage: still composed by default
        assert PF.serve_route(ROUTE.modules(*names)) == 'composed' and PF.serve_plan(ROUTE.modules(*names)) == 'composed'
    for names, want in PLANS:
        if want is not None:
            assert PF.serve_route(_mods(names)) == 'composed' and PF.serve_plan(_mods(names)) == 'composed'


# ---------------------------------------------------------------------------------------------------- wrong variants
def _padded_count(x):
    return (x.shape[2] + 31) // 32 * 32 * ((x.shape[3] + 63) // 64 * 64)


# variant -> (how it is put into the reference, the table case that must tell it apart)
VARIANTS = {
    'a mean taken over a padded count': (lambda m: m.setattr(SC, 'pixel_count', _padded_count), 2),
    'luminance weights in RGB order': (lambda m: m.setattr(SC, 'lum_weights', lambda: (0.299, 0.587, 0.114)), 2),
    'a statistic taken before the prefix stages': (
        lambda m: m.setattr(SC, 'scene_stat_input', lambda v, first, x, phase, kind, d: S.demosaic_nearest(x, phase)), 3),
    'the log floor left out': (lambda m: m.setattr(SC, 'log_floor', lambda: 1e-300), 23),
    'the second scene stage fed the first one\'s input': (
        lambda m: m.setattr(SC, 'scene_stat_input', lambda v, first, x, phase, kind, d: first), 26),
}


@pytest.mark.parametrize('name', list(VARIANTS))
def test_wrong_variant_is_told_apart(name, monkeypatch):
    patch, index = VARIANTS[name]
    case = T.sweep_case(index)
    true = case['ref']
    with monkeypatch.context() as m:
        patch(m)
        wrong = T.reference(case, single=True).bytes
    bad, rep = S.check(wrong, true, T.TAU)
    assert bad and rep['decided_share'] > max(S.TIE_CAP, S.FINAL_CAP), '%s on %s: only %d decided bytes differ (%.3e of the case)' % (
        name, case['what'], rep['decided_differ'], rep['decided_share'])


def test_a_maximum_with_identity_zero_shows_in_the_partial_rows_only(monkeypatch):
    """'a maximum with identity 0 behind a negative prefix': WbManual does not clamp, so a negative gain through the C ABI puts
    all-negative channels in front of white-world.  The constants cannot tell the variant apart - max(255 max_c, 1e-3) is the
    floor for a negative maximum and for 0 alike, so no byte of any case moves - but the partial rows can: a tile's row is the
    negative maximum, and the variant reports 0.  tests/test_gpu_serve_scene.py compares the kernel's rows with tile_partials
    on such an input; here the reference itself is shown to separate the two"""
    x = -np.random.default_rng(3).uniform(0.1, 1.0, size=(2, 3, 34, 68))
    ratio = np.array([1.0, 0.5])
    true_rows, true_gains = SC.tile_partials(x, 1), SC.whiteworld_gains(x, ratio)
    assert true_rows.shape == (2, 4, 4) and (true_rows[:, :, :3] < 0).all() and (true_rows[:, :, 3] == 0).all()
    assert np.array_equal(true_rows[:, :, :3].max(axis=1), x.reshape(2, 3, -1).max(axis=2))
    monkeypatch.setattr(SC, 'max_identity', lambda: 0.0)
    assert (SC.tile_partials(x, 1)[:, :, :3] == 0).all()                 # told apart, row by row
    assert np.array_equal(SC.whiteworld_gains(x, ratio), true_gains)      # ... and invisible behind the 1e-3 floor
