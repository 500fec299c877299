"""pipeline_fusion.serve_route: which of the three routes the serving path takes for a module list - 'fused'
(risp_serve_u8), 'classical' (risp_serve_classical_u8: the nearest or a classical stencil demosaic, element-wise stages and
the Crysis / Filmic tone curves, still one launch) or 'composed' - a pure function of the list, no GPU needed.  The lists
are those of tests/test_serve_plan_cpu.py plus the ones the classical route is about; everywhere serve_route is 'fused'
exactly where serve_plan is."""
import pytest
import torch

import reconfigisp_amd.functional as F
from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF
from reconfigisp_amd.codes.models.modules import registry as R

COND = {'conditional_gamma': (12, 8), 'conditional_wb_manual': (12, 8), 'conditional_wb_quadratic': (24, 8)}


def modules(*names, origin=True):
    return [R.make_op(n, None, origin=origin, conditional_channels=COND.get(n)) for n in names]


FUSED = [
    ('nearest', 'bilateral', 'wbmanual', 'gamma', 'gtmmanual'), ('nearest', 'wbmanual', 'gamma', 'gtmmanual'), ('nearest',),
    ('nearest', 'bilateral'), ('nearest', 'wbquadratic', 'gamma'),
    ('skip', 'nearest', 'bilateral', 'wbmanual', 'gamma', 'gtmmanual'),
    ('skip', 'nearest', 'skip', 'bilateral', 'skip', 'wbmanual', 'skip', 'gamma', 'gtmmanual', 'skip'),
    ('skip', 'nearest', 'skip', 'wbmanual', 'skip'), ('nearest', 'bilateral') + ('gamma', 'skip') * 8, ('nearest',) + ('gamma',) * 8,
]
CLASSICAL = [
    ('bilinear', 'gamma'), ('bilinear',), ('laplacian',), ('bilinear', 'wbmanual', 'gamma', 'gtmmanual'),
    ('laplacian', 'wbmanual', 'filmic', 'gamma'), ('laplacian', 'wbquadratic', 'skip', 'crysisengine', 'gamma'),
    ('nearest', 'crysisengine', 'gamma'), ('nearest', 'filmic'), ('nearest', 'gamma', 'filmic', 'crysisengine'),
    ('skip', 'laplacian', 'skip', 'filmic', 'skip'), ('bilinear',) + ('gamma', 'skip') * 8, ('laplacian',) + ('filmic',) * 8,
    ('nearest',) + ('gamma',) * 7 + ('crysisengine',),
]
COMPOSED = [
    ('nearest', 'grayworld', 'gamma'), ('nearest', 'bilateral', 'grayworld'), ('nearest', 'bilateral', 'wbmanual', 'gamma', 'grayworld'),
    ('nearest', 'grayworld'), ('nearest', 'median', 'gamma'), ('nearest', 'bilateral', 'median'), ('nearest', 'fastnlm', 'gamma'),
    ('nearest', 'bilateral', 'fastnlm'), ('path_bayer', 'nearest', 'gamma'), ('nearest', 'gamma', 'path_bgr'),
    ('nearest', 'gamma', 'bilateral'), ('nearest', 'bilateral', 'bilateral'), ('gamma', 'wbmanual'), (),
    ('nearest',) + ('gamma',) * 9, ('nearest', 'bilateral') + ('wbmanual', 'gamma', 'gtmmanual') * 3,
    # the stencil demosaics and the tone curves outside what the classical launch takes
    ('bilinear', 'bilateral', 'gamma'), ('laplacian', 'bilateral'),        # a bilateral behind a stencil demosaic
    ('nearest', 'bilateral', 'filmic'), ('nearest', 'bilateral', 'crysisengine', 'gamma'),      # no bilateral in the classical launch
    ('bilinear', 'reinhard', 'gamma'), ('nearest', 'reinhard'), ('laplacian', 'whiteworld'), ('bilinear', 'grayworld'),
    ('bilinear', 'median'), ('laplacian', 'fastnlm'), ('bilinear', 'gamma', 'path_bgr'), ('path_bayer', 'bilinear', 'gamma'),
    ('demosaicnet', 'gamma'), ('bilinear', 'bilinear'), ('filmic', 'gamma'),
    ('bilinear',) + ('gamma',) * 9, ('laplacian',) + ('filmic',) * 9, ('nearest',) + ('gamma',) * 8 + ('filmic',),
]


@pytest.mark.parametrize('names', FUSED, ids=lambda v: '-'.join(v))
def test_fused_lists(names):
    assert PF.serve_route(modules(*names)) == 'fused' and PF.serve_plan(modules(*names)) == 'fused'


@pytest.mark.parametrize('names', CLASSICAL, ids=lambda v: '-'.join(v))
def test_classical_lists(names):
    assert PF.serve_route(modules(*names)) == 'classical' and PF.serve_plan(modules(*names)) == 'composed'


@pytest.mark.parametrize('names', COMPOSED, ids=lambda v: '-'.join(v) or 'empty')
def test_composed_lists(names):
    assert PF.serve_route(modules(*names)) == 'composed' and PF.serve_plan(modules(*names)) == 'composed'


@pytest.mark.parametrize('head', sorted(COND))
def test_conditional_heads_compose(head):
    for names in (('nearest', head, 'gamma'), ('nearest', 'bilateral', 'gamma', head), ('bilinear', head), ('laplacian', 'filmic', head)):
        assert PF.serve_route(modules(*names)) == 'composed' and PF.serve_plan(modules(*names)) == 'composed'


def test_proxies_compose():
    """the differentiable proxies of the same names are CNNs: IspUniversal's lists keep the composed route"""
    for names in (('nearest', 'bilateral', 'gamma'), ('laplacian', 'gamma'), ('bilinear', 'gamma'), ('nearest', 'filmic'),
                  ('nearest', 'crysisengine', 'gamma')):
        assert PF.serve_route(modules(*names, origin=False)) == 'composed'
        assert PF.serve_plan(modules(*names, origin=False)) == 'composed'


def test_the_stage_codes_and_the_demosaic_kinds():
    assert (F.OP_TONE_CRYSIS, F.OP_TONE_FILMIC) == (7, 8) and F.OP_GAIN3 == 6
    assert F.DEMOSAIC == {'nearest': 0, 'bilinear': 1, 'laplacian': 2}
    assert PF.MAX_CHAIN == 8
    kind, stages = PF._classical_split(modules('skip', 'laplacian', 'wbmanual', 'skip', 'filmic', 'gamma'))
    assert kind == 'laplacian' and stages == [2, 4, 5]


def test_cpu_tensors_are_refused():
    with pytest.raises(RuntimeError, match='GPU-only'):
        F.serve_classical_u8(torch.zeros(1, 4, 4, dtype=torch.uint16), 1023.0, 'bilinear', [], [])
