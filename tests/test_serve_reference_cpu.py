"""The float64 statement of the serving path (tests/serve_reference.py) and the case table of tests/serve_space_cases.py,
checked without a GPU: the table covers its axes, every input stays under the tie caps, the reference agrees with the
statements the project already trusts, "phase by mirror" holds for the stencil demosaics, the recorded E32 is what the
float32 evaluation costs, that evaluation itself passes the comparison rule, and the rule tells wrong variants apart."""
import numpy as np
import pytest
import torch

import fused_segment_reference as R
import isp_oracle as O
import serve_reference as S
import serve_space_cases as T
import test_serve_cfa_cpu as CFA_CPU

ALL = [('sweep', i) for i in range(len(T.CASES))] + [('walk', s) for s in range(T.WALK)]


def _case(kind, i):
    return T.sweep_case(i) if kind == 'sweep' else T.walk_case(i)


def test_tables_agree_with_the_package():
    import reconfigisp_amd.functional as F
    assert S.CFA == F.CFA and S.DEMOSAIC == F.DEMOSAIC and S.SITES == CFA_CPU.SITES
    assert (S.OP_SKIP, S.OP_DEMOSAIC_NEAREST, S.OP_WB_MANUAL, S.OP_GAMMA, S.OP_GTM_MANUAL, S.OP_WB_QUADRATIC, S.OP_GAIN3,
            S.OP_TONE_CRYSIS, S.OP_TONE_FILMIC) == (F.OP_SKIP, F.OP_DEMOSAIC_NEAREST, F.OP_WB_MANUAL, F.OP_GAMMA, F.OP_GTM_MANUAL,
                                                   F.OP_WB_QUADRATIC, F.OP_GAIN3, F.OP_TONE_CRYSIS, F.OP_TONE_FILMIC)


def test_table_covers_its_axes():
    cl = [c for c in T.CASES if c[0] == 'c']
    sv = [c for c in T.CASES if c[0] == 's']
    assert 140 <= len(T.CASES) <= 160 and T.WALK == 16
    black = lambda c: c[2].split('/')[1] != '0'
    assert {(c[3], c[4], black(c)) for c in cl} == {(p, k, b) for p in S.SITES for k in S.DEMOSAIC for b in (False, True)}
    assert {(c[3], c[4], black(c)) for c in sv} == {(p, f, b) for p in S.SITES for f in T.WINDOWS for b in (False, True)}
    assert {c[1] for c in cl} == set(T.SHAPES_CLASSICAL) and {c[1] for c in sv} == set(T.SHAPES_SERVE)
    assert {c[2] for c in cl} == {c[2] for c in sv} == set(T.DEPTHS)
    assert {c[6] for c in cl} == {c[6] for c in sv} == {0, 1}
    ops_cl = {op for c in cl for op in T.TAILS[c[5]]}
    assert ops_cl == set(range(9)) - {S.OP_DEMOSAIC_NEAREST}
    assert {op for c in sv if c[4] != 'none' for op in T.TAILS[c[5]]} == set(S.ELEMENTWISE)
    assert all(op in S.ELEMENTWISE for c in sv for op in T.TAILS[c[5]])
    for tone in (S.OP_TONE_CRYSIS, S.OP_TONE_FILMIC):       # first, middle and last stage
        tails = [T.TAILS[c[5]] for c in cl if tone in T.TAILS[c[5]]]
        assert any(t[0] == tone and len(t) > 1 for t in tails) and any(t[-1] == tone and len(t) > 1 for t in tails)
        assert any(tone in t[1:-1] for t in tails)
    assert all(len(t) <= 8 for t in T.TAILS.values()) and any(len(t) == 8 for t in T.TAILS.values())
    # the depths' samples: above the white level where the type allows, below and at the black level, a zero and a constant image
    raw = T.make_raw(3, 4, 8, 1023, 64, 1)
    assert raw.max() > 1023 and (raw == 64).any() and (raw < 64).any() and (raw[1] == 0).all() and len(np.unique(raw[2])) == 1
    assert T.make_raw(1, 4, 4, 65535, 0, 1).max() == 65535
    # 10-bit lattice: (a + b) / 2 * 255 / 1023 is a half-integer when a + b is an odd multiple of 341, and the constant 341 of
    # tests/test_gpu_serve_cfa._raw is an exact integer code (a boundary of the final truncation); this constant is neither
    assert (170 + 171) * 255 % 2046 == 1023 and 341 * 255 % 1023 == 0
    assert (int(raw[2, 0, 0]) - 64) * 255 % 959 not in (0, 959 // 2, 959 // 2 + 1)


@pytest.mark.parametrize('kind,i', ALL)
def test_inputs_stay_under_the_caps_and_fp32_passes_the_rule(kind, i):
    """properties of the input and the reference alone - and the float32 evaluation of the reference itself, free-running,
    passes the comparison rule with the recorded TAU"""
    case = _case(kind, i)
    inner, loose = S.tie_shares(case['ref'], T.TAU)
    assert inner <= S.TIE_CAP and loose <= S.FINAL_CAP, case['what']
    bad, rep = S.check(T.reference(case, np.float32).bytes, case['ref'], T.TAU)
    assert not bad, '%s: the float32 evaluation breaks the rule: %s' % (case['what'], '; '.join(bad))


def measure_e32(case, worst):
    """the largest |v32 - v64| in codes per kind of quantisation point, every float32 segment started from the float64 codes.
    Only values whose float64 side lies in [-0.5, 255.5] (inner points) / [0, 256] (truncation) count: every decision boundary
    lies inside, and far above the clip a tone curve's error is large and decides nothing"""
    r64 = case['ref']
    r32 = T.reference(case, np.float32, sync=r64)
    for k, (kind, unq, _) in enumerate(r64.points):
        e = np.where((unq >= -0.5) & (unq <= 255.5), np.abs(r32.points[k][1].astype(np.float64) - unq), 0.0)
        if kind == 'bilateral':
            for img, wd in enumerate(r64.bilateral_windows):
                worst['bilateral%d' % wd] = max(worst.get('bilateral%d' % wd, 0.0), e[img].max())
        else:
            worst[kind] = max(worst.get(kind, 0.0), e.max())
    if r64.final_kind:
        m = ~np.isnan(r64.final_t) & ~np.isnan(r32.final_t) & (r64.final_t >= 0) & (r64.final_t <= 256)
        if m.any():
            key = 'final/' + r64.final_kind
            worst[key] = max(worst.get(key, 0.0), np.abs(r32.final_t - r64.final_t)[m].max())


def test_recorded_e32_is_the_fp32_references_error():
    assert all(T.TAU[k] == 2.0 * T.E32[k] for k in T.E32)
    worst = {}
    for kind, i in ALL:
        measure_e32(_case(kind, i), worst)
    print({k: '%.3e' % v for k, v in sorted(worst.items())})
    assert set(worst) == set(T.E32)
    for k, e in worst.items():
        assert e <= T.E32[k], '%s: measured %.3e, recorded %.3e' % (k, e, T.E32[k])
        assert e >= T.E32[k] / 1.25, '%s: recorded %.3e is wider than the measured %.3e' % (k, T.E32[k], e)


# ---------------------------------------------------------------------------------------------------- agreement
def _flip(a, code):
    return CFA_CPU._flip(a, code)


@pytest.mark.parametrize('kind', ['bilinear', 'laplacian'])
def test_rggb_demosaic_is_the_oracles(kind):
    x = np.random.default_rng(3).uniform(-0.1, 1.2, size=(2, 10, 12))
    with O.unquantized():
        want = O.origin_demosaic(torch.from_numpy(x)[:, None] * 255.0, kind).numpy()
    assert np.abs(S.demosaic_stencil(x, 'rggb', kind) - want).max() <= 1e-9


@pytest.mark.parametrize('phase', list(S.SITES))
def test_nearest_is_the_natural_map(phase):
    m = np.random.default_rng(5).uniform(size=(10, 12))
    assert np.array_equal(S.demosaic_nearest(m[None], phase)[0], CFA_CPU._natural_map(m, phase))


def test_tone_curves_are_the_oracles():
    n = 4
    x = torch.from_numpy(np.random.default_rng(7).uniform(-0.2, 1.5, size=(n, 3, 6, 8)))
    lum, wp, bias = np.array([0.0, 1.0, 0.3, 0.7]), np.array([0.0, 0.005, 1.0, 0.4]), np.array([1.0, 10.0, 3.0, 7.0])
    with O.unquantized():
        cr = O.origin_tonemap(x * 255.0, 'crysisengine', {'lum_adapted': lum}).numpy()
        fi = O.origin_tonemap(x * 255.0, 'filmic', {'white_point': wp, 'exposure_bias': bias}).numpy()
    assert np.abs(S.tone_raw(S.OP_TONE_CRYSIS, x.numpy(), lum[:, None]) - cr).max() <= 1e-9
    assert np.abs(S.tone_raw(S.OP_TONE_FILMIC, x.numpy(), np.stack([wp, bias], 1)) - fi).max() <= 1e-9 * np.abs(fi).max()


@pytest.mark.parametrize('i', [i for i, c in enumerate(T.CASES) if c[0] == 's' and c[2].endswith('/0') and c[3] == 'rggb'])
def test_serve_u8_reference_is_the_segment_restatement(i):
    case = T.sweep_case(i)
    x = torch.from_numpy(case['raw'] / float(case['white']))[:, None]
    if case['bilateral'] is None:
        cur = R.demosaic(x)
        for op, par in zip(case['ops'], case['params']):
            cur = R.elementwise(op, cur, None if par is None else torch.from_numpy(par))
    else:
        stages, _ = R.segment(x, True, *[torch.from_numpy(a) for a in case['bilateral']], case['ops'],
                              [None if p is None else torch.from_numpy(p) for p in case['params']])
        cur = stages[-1]
    want = torch.floor((cur * 255.0).clamp(0.0, 255.0)).numpy()[:, [2, 1, 0] if case['reverse'] else [0, 1, 2]].transpose(0, 2, 3, 1)
    assert np.array_equal(want, case['ref'].bytes)


@pytest.mark.parametrize('size', [(4, 4), (4, 8), (6, 12), (10, 12)], ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('kind', ['bilinear', 'laplacian'])
@pytest.mark.parametrize('phase', list(S.SITES))
def test_mirror_premise_for_the_stencil_demosaics(phase, kind, size):
    """the sentence the kernels rest on: the per-phase demosaic is unflip(rggb_demosaic(flip(mosaic))), exactly"""
    code = S.CFA[phase]
    # samples k / 1024: every product, sum and division by 2, 4, 8 below is exact in float64, so the order of a sum is no excuse
    m = np.random.default_rng(11 + code + size[1]).integers(0, 1126, size=(2,) + size).astype(np.float64) / 1024.0
    direct = S.demosaic_stencil(m, phase, kind)
    mirrored = _flip(S.demosaic_stencil(_flip(m, code), 'rggb', kind), code)
    assert np.array_equal(direct, mirrored)


# ---------------------------------------------------------------------------------------------------- wrong variants
def _swap_sites(m):
    m.setattr(S, 'SITES', dict(S.SITES, grbg=S.SITES['gbrg'], gbrg=S.SITES['grbg']))


def _edge_repeat(i, n):
    i = np.where(i < 0, -i - 1, i)
    return np.where(i >= n, 2 * n - 1 - i, i)


def _drop_far(tap, inside):
    t = lambda dy, dx: tap(dy, dx) * inside(dy, dx)
    return t(0, -2) + t(0, 2), t(-2, 0) + t(2, 0)


def _norm(f):
    def normalise(raw, white, black, dtype=np.float64):
        x = f(np.asarray(raw).astype(np.int64), int(white), int(black)).astype(dtype)
        return x, np.zeros(x.shape, np.int8)
    return normalise


_malvar = S.malvar_terms
# variant -> (how it is put into the reference, the table case that must tell it apart)
VARIANTS = {
    'x and y mirror bits exchanged': (_swap_sites, 3),
    'G from the other row of the quad': (lambda m: m.setattr(S, 'green_row', lambda y: 1 - y % 2), 0),
    'Malvar rb_hor / rb_ver exchanged': (lambda m: m.setattr(S, 'malvar_terms', lambda *a: (lambda g, h, v, d: (g, v, h, d))(*_malvar(*a))), 2),
    'edge-repeating reflect': (lambda m: m.setattr(S, 'reflect101', _edge_repeat), 1),
    'far ring of Malvar dropped at a border': (lambda m: m.setattr(S, 'far_ring', _drop_far), 2),
    'truncation at an inner code': (lambda m: m.setattr(S, 'code', lambda v: np.floor(np.clip(v, 0.0, 255.0))), 1),
    'rounding at the final conversion': (lambda m: m.setattr(S, 'final_byte', lambda v: np.floor(np.clip(v * 255, 0.0, 255.0) + 0.5)), 0),
    'black level subtracted after the division': (lambda m: m.setattr(S, 'normalise', _norm(lambda s, w, b: np.maximum(s / (w - b) - b / w, 0.0))), 1),
    'black level not clamped at 0': (lambda m: m.setattr(S, 'normalise', _norm(lambda s, w, b: (s - b) / (w - b))), 4),
    'divisor white': (lambda m: m.setattr(S, 'normalise', _norm(lambda s, w, b: np.maximum(s - b, 0) / w)), 1),
    'channels not reversed': (lambda m: m.setattr(S, 'store_order', lambda reverse: [0, 1, 2]), 3),
    'Filmic parameters exchanged': (lambda m: m.setattr(S, 'filmic_block', lambda p: (p[:, 1], p[:, 0])), 2),
    'Crysis without the 0.05': (lambda m: m.setattr(S, 'crysis_scale', lambda lum, d: d(0.5) / np.maximum(lum, d(1e-30))), 1),
    'parameters of image 0 for every image': (lambda m: m.setattr(S, 'image_params', lambda par, i: par[0]), 12),
}


@pytest.mark.parametrize('name', list(VARIANTS))
def test_wrong_variant_is_told_apart(name, monkeypatch):
    patch, index = VARIANTS[name]
    case = T.sweep_case(index)
    true = case['ref']
    with monkeypatch.context() as m:
        patch(m)
        wrong = T.reference(case).bytes
    bad, rep = S.check(wrong, true, T.TAU)
    # more than the caps allow: the DECIDED bytes that differ (no tie excuses them) are a larger share of the case than both caps
    assert bad and rep['decided_share'] > max(S.TIE_CAP, S.FINAL_CAP), '%s on %s: only %d decided bytes differ (%.3e of the case)' % (
        name, case['what'], rep['decided_differ'], rep['decided_share'])
