"""pipeline_fusion.denoise_scene_plan: the module lists ``serve(fast_denoise_scene=True)`` serves without fp32 planes
(risp_serve_scene_stats / risp_serve_denoise_stats + risp_serve_scene_finish per scene stage, then
risp_serve_denoise_scene_u8) - Skips stripped, a classical demosaic, at most MAX_CHAIN stages around exactly ONE classical
bilateral / median / non-local means, one or two of them Grayworld / OriginWbWhiteworld at any position relative to the
denoiser, every other stage element-wise or a Crysis / Filmic curve - a pure function of the list, no GPU needed.  The route is
opt-in and the plan disjoint from every other: denoise_plan, scene_plan, cond_plan, serve_plan and serve_route answer for every
list here what they answered before the plan existed."""
import pytest
import torch

import reconfigisp_amd.functional as F
from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF
from test_serve_denoise_plan_cpu import COND, DEMOSAICS, DENOISERS, modules

# (names, plan): plan = (demosaic, indices of the stages around the denoiser, index of the denoiser, scene flags of the stages)
PLANNED, DROPPED = [], []
for dm in DEMOSAICS:
    for dn in DENOISERS:
        PLANNED.append(((dm, 'grayworld', dn, 'gamma'), (dm, [1, 3], 2, [True, False])))           # scene stage in front
        # behind, and one each side: measured slower than the default call for non-local means (test_the_dropped_combinations)
        (DROPPED if dn == 'fastnlm' else PLANNED).extend([
            ((dm, 'wbmanual', dn, 'whiteworld', 'crysisengine'), (dm, [1, 3, 4], 2, [False, True, False])),
            ((dm, 'grayworld', 'gamma', dn, 'whiteworld'), (dm, [1, 2, 4], 3, [True, False, True]))])
PLANNED += [
    # two on one side
    (('bilinear', 'grayworld', 'whiteworld', 'median'), ('bilinear', [1, 2], 3, [True, True])),
    (('nearest', 'bilateral', 'whiteworld', 'gamma', 'grayworld', 'filmic'), ('nearest', [2, 3, 4, 5], 1, [True, False, True, False])),
    (('laplacian', 'median', 'grayworld', 'grayworld'), ('laplacian', [2, 3], 1, [True, True])),
    (('laplacian', 'whiteworld', 'grayworld', 'fastnlm', 'gamma'), ('laplacian', [1, 2, 4], 3, [True, True, False])),
    # the bilateral directly behind the nearest demosaic is the fused kernel's only without a scene stage
    (('nearest', 'bilateral', 'grayworld'), ('nearest', [2], 1, [True])),
    # Skips in between: the indices are those of the whole list
    (('skip', 'bilinear', 'skip', 'grayworld', 'skip', 'bilateral', 'skip', 'gamma', 'skip', 'crysisengine', 'skip'),
     ('bilinear', [3, 7, 9], 5, [True, False, False])),
    (('skip', 'laplacian', 'median', 'skip', 'skip', 'whiteworld'), ('laplacian', [5], 2, [True])),
    # MAX_CHAIN stages around the denoiser
    (('bilinear',) + ('gamma',) * 7 + ('bilateral', 'grayworld'), ('bilinear', list(range(1, 8)) + [9], 8, [False] * 7 + [True])),
    (('bilinear', 'grayworld') + ('gamma',) * 7 + ('fastnlm',), ('bilinear', list(range(1, 9)), 9, [True] + [False] * 7)),
    (('nearest', 'whiteworld', 'median') + ('wbmanual', 'skip') * 7, ('nearest', [1, 3, 5, 7, 9, 11, 13, 15], 2, [True] + [False] * 7)),
]

NOT_PLANNED = [
    # Reinhard anywhere, with or without another scene stage
    ('bilinear', 'reinhard', 'median'), ('laplacian', 'bilateral', 'reinhard'), ('nearest', 'grayworld', 'fastnlm', 'reinhard'),
    ('bilinear', 'reinhard', 'bilateral', 'whiteworld'),
    # two denoisers
    ('bilinear', 'grayworld', 'bilateral', 'median'), ('laplacian', 'median', 'whiteworld', 'median'), ('nearest', 'fastnlm', 'grayworld', 'bilateral'),
    # three scene stages
    ('bilinear', 'grayworld', 'median', 'whiteworld', 'grayworld'), ('nearest', 'whiteworld', 'whiteworld', 'grayworld', 'fastnlm'),
    # nine stages
    ('bilinear',) + ('gamma',) * 8 + ('median', 'grayworld'), ('laplacian', 'grayworld', 'fastnlm') + ('filmic',) * 8,
    ('nearest',) + ('gamma',) * 4 + ('bilateral', 'whiteworld') + ('gamma',) * 4,
    # CNN stages, no demosaic
    ('bilinear', 'grayworld', 'median', 'path_bgr'), ('path_bayer', 'bilinear', 'grayworld', 'median'), ('demosaicnet', 'grayworld', 'median'),
    ('bilinear', 'bm3d', 'grayworld', 'median'), ('grayworld', 'median'), ('median', 'grayworld', 'gamma'), (),
    # no scene stage: denoise_plan's lists (or the fused kernel's)
    ('bilinear', 'median'), ('laplacian', 'gamma', 'fastnlm', 'filmic'), ('nearest', 'gamma', 'bilateral'), ('nearest', 'bilateral'),
    # no denoiser: scene_plan's lists
    ('bilinear', 'grayworld'), ('laplacian', 'whiteworld', 'gamma', 'grayworld'), ('nearest', 'gamma', 'reinhard'),
    # neither
    ('bilinear', 'gamma'), ('laplacian',),
    # the 'fused' list
    ('nearest', 'bilateral', 'wbmanual', 'gamma', 'gtmmanual'),
]


def _ids(v):
    return '-'.join(v) if isinstance(v, tuple) and all(isinstance(s, str) for s in v) else None


def _todays_answers(mods):
    """what the plans and routes that existed before say for a list, by their own documented rules (the plan under test
    takes no part): a scene stage or a denoiser beside the other takes a list out of both older plans"""
    fused = PF._serve_split(mods) is not None
    assert PF.serve_plan(mods) == ('fused' if fused else 'composed')
    assert PF.serve_route(mods) == ('fused' if fused else 'classical' if PF._classical_split(mods) is not None else 'composed')
    kinds = [type(m) for m in mods]
    has_scene = any(t in PF._SCENE_STAT for t in kinds)
    has_denoiser = any(t in PF._DENOISER for t in kinds)
    if has_scene:
        assert PF.denoise_plan(mods) is None
    if has_denoiser:
        assert PF.scene_plan(mods) is None
    if has_scene or has_denoiser:
        assert PF.cond_plan(mods) is None


@pytest.mark.parametrize('names,plan', PLANNED, ids=_ids)
def test_planned_lists(names, plan):
    mods = modules(*names)
    assert PF.denoise_scene_plan(mods) == plan
    # disjoint from every other plan, and the default call's answers stay what they are
    assert PF.denoise_plan(mods) is None and PF.scene_plan(mods) is None and PF.cond_plan(mods) is None
    assert PF.serve_route(mods) == 'composed' and PF.serve_plan(mods) == 'composed'


@pytest.mark.parametrize('names', NOT_PLANNED, ids=lambda v: '-'.join(v) or 'empty')
def test_lists_without_a_plan(names):
    mods = modules(*names)
    assert PF.denoise_scene_plan(mods) is None
    _todays_answers(mods)


def test_the_neighbouring_plans_keep_their_lists():
    """the lists one keyword away keep the plan they have"""
    assert PF.denoise_plan(modules('bilinear', 'gamma', 'median')) == ('bilinear', [1], 2, [])
    assert PF.scene_plan(modules('bilinear', 'grayworld', 'gamma')) == ('bilinear', [1, 2], [True, False])
    assert PF.cond_plan(modules('bilinear', 'conditional_gamma')) == ('bilinear', [1], [True])
    assert PF.serve_plan(modules('nearest', 'bilateral', 'gamma')) == 'fused'
    assert PF.serve_route(modules('laplacian', 'gamma', 'filmic')) == 'classical'


def test_classical_bm3d_has_no_plan():
    for names in (('bilinear', 'bm3d', 'grayworld'), ('bilinear', 'grayworld', 'bm3d', 'median'), ('nearest', 'whiteworld', 'bilateral', 'bm3d')):
        mods = modules(*names, classical_bm3d=True)
        assert PF.denoise_scene_plan(mods) is None
        _todays_answers(mods)


@pytest.mark.parametrize('head', sorted(COND))
def test_a_head_has_no_plan(head):
    """(heads exist only in IspUniversal, whose denoisers are proxies; a list built by hand is refused all the same)"""
    for names in (('bilinear', head, 'grayworld', 'median'), ('nearest', 'grayworld', 'bilateral', head)):
        mods = modules(*names)
        assert PF.denoise_scene_plan(mods) is None
        _todays_answers(mods)


def test_proxies_have_no_plan():
    """the differentiable proxies of the same names are CNNs: IspUniversal's lists keep the composed route"""
    for names in (('bilinear', 'grayworld', 'median'), ('nearest', 'bilateral', 'grayworld'), ('laplacian', 'whiteworld', 'fastnlm', 'gamma')):
        mods = modules(*names, origin=False)
        assert PF.denoise_scene_plan(mods) is None
        assert PF.serve_route(mods) == 'composed' and PF.serve_plan(mods) == 'composed'
        assert PF.denoise_plan(mods) is None and PF.scene_plan(mods) is None


@pytest.mark.parametrize('names,plan', DROPPED, ids=_ids)
def test_the_dropped_combinations(names, plan, monkeypatch):
    """profiles/serve_denoise_scene.txt, net.serve(out=) medians over 7 interleaved rounds: a scene stage behind non-local
    means costs a second run of the denoiser and lost to the default call at 64 x 256 x 256 - gray-world behind 193.1 us
    against 161.6 us composed, one scene stage each side 213.1 against 192.1 (spreads 0.5 and 1.7 us) - while winning at
    1 x 3000 x 4000 (522.7 against 753.9, 582.2 against 811.9).  The rule asks for both sizes, so the plan has no answer for
    the two combinations; every other (denoiser, position) cleared it at both sizes and stays.  The lists are well formed:
    with the measured verdict taken away the plan is the one the kernels serve"""
    mods = modules(*names)
    assert PF._DENOISE_SCENE_SLOWER == frozenset({('fastnlm', 'behind'), ('fastnlm', 'both')})
    assert PF.denoise_scene_plan(mods) is None
    _todays_answers(mods)
    monkeypatch.setattr(PF, '_DENOISE_SCENE_SLOWER', frozenset())
    assert PF.denoise_scene_plan(mods) == plan


def test_the_keyword_exists_on_every_serve():
    import inspect
    from reconfigisp_amd.codes.models.isp_model import IspModel
    from reconfigisp_amd.codes.models.modules.isp_universal import IspUniversal
    from reconfigisp_amd.codes.models.modules.origin_universal import OriginUniversal
    for fn in (PF.serve, IspUniversal.serve, OriginUniversal.serve, IspModel.serve):
        par = inspect.signature(fn).parameters
        assert par['fast_denoise_scene'].default is False, fn
        assert list(par)[-1] == 'fast_denoise_scene', 'the keyword comes last: positional callers keep their meaning'


def test_cpu_tensors_are_refused():
    raw = torch.zeros(1, 4, 4, dtype=torch.uint16)
    with pytest.raises(RuntimeError, match='GPU-only'):
        F.serve_denoise_scene_u8(raw, 1023.0, 'bilinear', [], [], 'median', (3,), [], [])
    with pytest.raises(RuntimeError, match='GPU-only'):
        F.serve_denoise_stats(raw, 1023.0, 'bilinear', [], [], 'median', (3,), [], [], F.SCENE_MAX3)
