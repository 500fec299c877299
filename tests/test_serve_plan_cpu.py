"""pipeline_fusion.serve_plan: which pipelines the serving path runs as ONE launch (uint16 frames in, packed bytes out) and
which it composes from the existing kernels - a pure function of the module list, no GPU needed.  And the two new
functional ops refuse CPU tensors like every other op."""
import pytest
import torch

import reconfigisp_amd.functional as F
from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF
from reconfigisp_amd.codes.models.modules import registry as R

COND = {'conditional_gamma': (12, 8), 'conditional_wb_manual': (12, 8), 'conditional_wb_quadratic': (24, 8)}


def modules(*names, origin=True):
    return [R.make_op(n, None, origin=origin, conditional_channels=COND.get(n)) for n in names]


def test_headline_pipeline_is_one_launch():
    assert PF.serve_plan(modules('nearest', 'bilateral', 'wbmanual', 'gamma', 'gtmmanual')) == 'fused'


def test_chain_only_is_one_launch():
    assert PF.serve_plan(modules('nearest', 'wbmanual', 'gamma', 'gtmmanual')) == 'fused'
    assert PF.serve_plan(modules('nearest')) == 'fused'
    assert PF.serve_plan(modules('nearest', 'bilateral')) == 'fused'
    assert PF.serve_plan(modules('nearest', 'wbquadratic', 'gamma')) == 'fused'


def test_skips_are_stripped():
    assert PF.serve_plan(modules('skip', 'nearest', 'bilateral', 'wbmanual', 'gamma', 'gtmmanual')) == 'fused'
    assert PF.serve_plan(modules('skip', 'nearest', 'skip', 'bilateral', 'skip', 'wbmanual', 'skip', 'gamma', 'gtmmanual', 'skip')) == 'fused'
    assert PF.serve_plan(modules('skip', 'nearest', 'skip', 'wbmanual', 'skip')) == 'fused'
    # eight chain stages and any number of Skips still fit
    assert PF.serve_plan(modules('nearest', 'bilateral', *(['gamma', 'skip'] * 8))) == 'fused'


@pytest.mark.parametrize('names', [
    ('nearest', 'grayworld', 'gamma'), ('nearest', 'bilateral', 'grayworld'), ('nearest', 'bilateral', 'wbmanual', 'gamma', 'grayworld'),
    ('nearest', 'grayworld')])
def test_grayworld_anywhere_composes(names):
    assert PF.serve_plan(modules(*names)) == 'composed'


@pytest.mark.parametrize('head', sorted(COND))
def test_conditional_head_composes(head):
    assert PF.serve_plan(modules('nearest', head, 'gamma')) == 'composed'
    assert PF.serve_plan(modules('nearest', 'bilateral', 'gamma', head)) == 'composed'


@pytest.mark.parametrize('stencil', ['median', 'fastnlm'])
def test_other_classical_stencils_compose(stencil):
    assert PF.serve_plan(modules('nearest', stencil, 'gamma')) == 'composed'
    assert PF.serve_plan(modules('nearest', 'bilateral', stencil)) == 'composed'


def test_cnn_stages_compose():
    assert PF.serve_plan(modules('nearest', 'bilateral', 'gamma', origin=False)) == 'composed'      # the bilateral PROXY net
    assert PF.serve_plan(modules('path_bayer', 'nearest', 'gamma')) == 'composed'                   # Path-Restore on the mosaic
    assert PF.serve_plan(modules('nearest', 'gamma', 'path_bgr')) == 'composed'
    assert PF.serve_plan(modules('laplacian', 'gamma', origin=False)) == 'composed'                 # a proxy demosaic
    assert PF.serve_plan(modules('bilinear', 'gamma')) == 'composed'                                # a classical one


def test_other_orders_compose():
    assert PF.serve_plan(modules('nearest', 'gamma', 'bilateral')) == 'composed'        # the bilateral must follow the demosaic
    assert PF.serve_plan(modules('nearest', 'bilateral', 'bilateral')) == 'composed'
    assert PF.serve_plan(modules('gamma', 'wbmanual')) == 'composed'                    # no demosaic
    assert PF.serve_plan(modules()) == 'composed'


def test_nine_chain_ops_compose():
    assert PF.MAX_CHAIN == 8
    assert PF.serve_plan(modules('nearest', *(['gamma'] * 8))) == 'fused'
    assert PF.serve_plan(modules('nearest', *(['gamma'] * 9))) == 'composed'
    assert PF.serve_plan(modules('nearest', 'bilateral', *(['wbmanual', 'gamma', 'gtmmanual'] * 3))) == 'composed'


def test_cpu_tensors_are_refused():
    with pytest.raises(RuntimeError, match='GPU-only'):
        F.quantise_u8(torch.rand(1, 3, 4, 4))
    with pytest.raises(RuntimeError, match='GPU-only'):
        F.serve_u8(torch.zeros(1, 4, 4, dtype=torch.uint16), 1023.0, [], [])
    from reconfigisp_amd.codes.utils import util
    with pytest.raises(RuntimeError, match='GPU-only'):
        util.tensor2bgr_device(torch.rand(3, 4, 4))
