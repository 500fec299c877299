"""``serve(fast_median=True)``: what is decided on the host - the size OriginNoiseMedian's rule gives
(pipeline_fusion._median_args), the keyword on every ``serve``, the table of sizes the measurement left on the launch
(pipeline_fusion._MEDIAN_SIZES against profiles/serve_median.txt) and the declaration of the entry point.  No GPU needed."""
import inspect
import os
import re

import pytest
import torch

import reconfigisp_amd.functional as F
from reconfigisp_amd import lib as L
from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF
from reconfigisp_amd.codes.models.modules import registry as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {5, 7, 9, 11, 13, 15}


@pytest.mark.parametrize('p,size', [(0.0, 3), (0.1, 3), (0.142, 3), (0.143, 5), (0.2, 5), (0.3, 7), (0.5, 9), (0.6, 11), (0.75, 13),
                                    (0.86, 15), (0.99, 15), (1.0, 17)])
def test_median_size_follows_the_rule(p, size):
    med = R.make_op('median', None, origin=True)
    assert PF._median_args(med, torch.full((3, 1), p)) == size == 2 * int(p * 7) + 3


def test_median_size_is_image_0s_and_follows_the_version():
    med = R.make_op('median', None, origin=True)
    q = torch.tensor([[0.5], [0.1], [1.0]])
    assert PF._median_args(med, q) == 9, 'image 0 alone decides'
    cached = med.__dict__['_risp_median_size']
    assert PF._median_args(med, q) == 9 and med.__dict__['_risp_median_size'] is cached, 'derived again for the same version'
    q[1, 0] = 0.9                                          # in place, another image: a new version, the same size
    assert PF._median_args(med, q) == 9 and med.__dict__['_risp_median_size'] is not cached
    q[0, 0] = 0.2
    assert PF._median_args(med, q) == 5
    assert PF._median_args(med, torch.full((2, 1), 0.99)) == 15, 'another tensor'
    # the 3 x 3 route's answer is untouched: size 5 is not its to serve
    assert PF._denoise_args(med, q) is None
    q[0, 0] = 0.1
    assert PF._denoise_args(med, q) == ('median', (3,)) and PF._median_args(med, q) == 3


def test_the_keyword_exists_on_every_serve():
    from reconfigisp_amd.codes.models.isp_model import IspModel
    from reconfigisp_amd.codes.models.modules.isp_universal import IspUniversal
    from reconfigisp_amd.codes.models.modules.origin_universal import OriginUniversal
    for fn in (PF.serve, IspUniversal.serve, OriginUniversal.serve, IspModel.serve):
        par = inspect.signature(fn).parameters
        assert par['fast_median'].default is False and par['fast_median'].kind is inspect.Parameter.KEYWORD_ONLY, fn
        assert list(par)[-2:] == ['fast_median', 'fast_denoise_scene'], 'in front of fast_denoise_scene, which stays last'
        assert par['fast_denoise'].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD, 'the positional list is unchanged'


def test_the_table_is_what_the_measurement_shows():
    """the rule: a size is sent to the launch only where profiles/serve_median.txt has ``fast_median=True`` beat the default
    call by more than the larger spread of the two legs at both benchmark sizes, for both demosaics"""
    assert PF._MEDIAN_SIZES <= SIZES and isinstance(PF._MEDIAN_SIZES, frozenset)
    lines = open(os.path.join(ROOT, 'profiles', 'serve_median.txt')).read().splitlines()
    sizes = lambda text: {int(k) for k in re.findall(r'\d+', text)}
    won = [ln.split('for:')[1] for ln in lines if 'beats the default call by more than the spread at both sizes for:' in ln]
    lost = [ln.split('for:')[1] for ln in lines if 'and does not for:' in ln]
    assert len(won) == 1 and len(lost) == 1
    assert sizes(won[0]) | sizes(lost[0]) == SIZES and not sizes(won[0]) & sizes(lost[0])
    assert PF._MEDIAN_SIZES == sizes(won[0])
    # and the summary follows from the rows above it: route, default and their spreads per (size, demosaic, frames)
    rows = {}
    for ln in lines:
        m = re.match(r'\s*K=(\d+)\s+(bilinear|laplacian)\s+(\d+x\d+x\d+)\s+route\s+([\d.]+)\s+\+-\s+([\d.]+)\s+us\s+default\s+([\d.]+)\s+\+-\s+([\d.]+)\s+us', ln)
        if m:
            route, rs, default, ds = (float(v) for v in m.groups()[3:])
            rows.setdefault(int(m.group(1)), []).append(default - route > max(rs, ds))
    assert set(rows) == SIZES and all(len(v) == 4 for v in rows.values()), rows
    assert {k for k, v in rows.items() if all(v)} == sizes(won[0])


def test_the_wrapper_serves_every_size():
    assert set(F.MEDIAN_SIZES) == SIZES


def test_cpu_tensors_are_refused():
    with pytest.raises(RuntimeError, match='GPU-only'):
        F.serve_median_u8(torch.zeros(1, 8, 8, dtype=torch.uint16), 1023.0, 'bilinear', [], [], 9, [], [])
    with pytest.raises(RuntimeError, match='GPU-only'):
        PF.serve([], [], torch.zeros(1, 8, 8, dtype=torch.uint16), 1023.0, fast_median=True)


def test_the_entry_point_is_declared():
    header = open(os.path.join(ROOT, 'include', 'risp.h')).read()
    m = re.search(r'int risp_serve_median_u8\(([^;]*)\);', header)
    assert m, 'include/risp.h does not declare risp_serve_median_u8'
    args = [a.strip() for a in m.group(1).replace('\n', ' ').split(',')]
    assert [a.split()[-1].lstrip('*') for a in args] == [
        'raw', 'divisor', 'demosaic', 'n_pre', 'pre_ops', 'pre_params', 'size', 'n_post', 'post_ops', 'post_params', 'out',
        'reverse_channels', 'N', 'H', 'W', 'black_level', 'cfa', 'stream']
    res, sig = L.SIGNATURES['risp_serve_median_u8']
    assert len(sig) == len(args) == 18
