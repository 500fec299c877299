"""Classical BM3D without a GPU: the parameter mapping, the float64 OPSPEC's own properties (tests/bm3d_reference.py),
the C ABI declarations and exports, and the two opt-in option keys on the CPU seam."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import bm3d_reference as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('risp_origin_bm3d_scratch_bytes', 'risp_origin_bm3d')


def test_parameter_mapping_reproduces_initial_values():
    from reconfigisp_amd.codes.models.modules import registry as R
    from reconfigisp_amd.codes.models.modules.tools_origin import OriginNoiseBm3d
    p = torch.sigmoid(torch.tensor([R.PARAM_INIT['bm3d']]))
    d = OriginNoiseBm3d()._params(p, {})
    assert abs(float(d['cff'][0]) - 1.5) < 1e-3
    assert (int(d['n1'][0]), int(d['cspace'][0]), int(d['wtransform'][0]), int(d['neighborhood'][0])) == (8, 0, 0, 8)
    edges = OriginNoiseBm3d()._params(torch.tensor([[0., 0.49, 0.5, 0.49, 0.], [1., 0.5, 0.49, 0.5, 1.]]), {})
    assert edges['n1'].tolist() == [4, 8] and edges['cspace'].tolist() == [1, 0]
    assert edges['wtransform'].tolist() == [0, 1] and edges['neighborhood'].tolist() == [1, 9]
    assert edges['cff'].tolist() == [0., 12.]


def test_sigma_zero_returns_codes():
    x = torch.rand(2, 3, 12, 10) * 300 - 20
    y, _ = B.bm3d(x, 0.0, [4, 8], 0, 0, 2)
    assert torch.equal(y, torch.from_numpy(B.codes(x)).float())


@pytest.mark.parametrize('cspace,wtransform,n1', [(0, 0, 8), (1, 1, 4), (0, 1, 8), (1, 0, 4)])
def test_constant_image_stays_constant(cspace, wtransform, n1):
    x = torch.empty(1, 3, 21, 19)
    x[:, 0], x[:, 1], x[:, 2] = 120., 80., 200.
    y, _ = B.bm3d(x, 2.55 * 12, n1, cspace, wtransform, 3)
    assert torch.equal(y, x)


@pytest.mark.parametrize('n1', [4, 8])
@pytest.mark.parametrize('h,w', [(8, 8), (13, 29), (31, 17), (40, 41)])
def test_reference_blocks_cover_every_pixel(n1, h, w):
    gy, gx = B.grid(h, n1), B.grid(w, n1)
    cover = np.zeros((h, w), bool)
    for y in gy:
        for x in gx:
            cover[y:y + n1, x:x + n1] = True
    assert cover.all() and gy[-1] == h - n1 and gx[-1] == w - n1
    assert B.refs(h, w, n1) == len(gy) * len(gx) <= B.table_rows(h, w)


def _strip(cols, h=4):
    """codes whose matching plane S repeats ``cols`` on every row (all of S in channel 0)"""
    q = np.zeros((3, h, len(cols)))
    q[0] = np.asarray(cols, float)[None, :]
    return q


def test_group_order_and_size_on_known_distances():
    """4 x 4 blocks on a 4-row strip: the reference at (0, 0) sees candidates x = 1..R only, with
    D(x) = 4 * sum_j (S[x + j] - S[j])^2 known by hand"""
    cols = [0, 0, 0, 0, 30, 0, 20, 0, 0, 0, 0, 0]
    # D(1) = 4 * 30^2 = 3600, D(2) = 3600, D(3) = 4 * (30^2 + 20^2) = 5200: ordered by D, then x; 4 kept -> N2 = 4
    assert B.match(_strip(cols), 4, 3)[0] == [(0, 0), (0, 1), (0, 2), (0, 3)]
    assert B.match(_strip(cols), 4, 1)[0] == [(0, 0), (0, 1)]          # R = 1: 2 kept
    cols2 = [0, 0, 0, 0, 0, 0, 25, 0, 0, 0, 0, 0]
    # D(1) = D(2) = 0 (ties broken by x), D(3) = 2500: 4 kept; R = 2 -> 3 kept -> N2 = 2
    assert B.match(_strip(cols2), 4, 3)[0] == [(0, 0), (0, 1), (0, 2), (0, 3)]
    assert B.match(_strip(cols2), 4, 2)[0] == [(0, 0), (0, 1)]
    # the keep bound D <= 22500 n1^2 = 360000 is inclusive: 4 * 300^2 = 360000 kept, 4 * 301^2 not
    three = lambda v: [0, 0, 0, 0, v, 0, 0, 0]
    assert B.match(_strip(three(300)), 4, 1)[0] == [(0, 0), (0, 1)]
    assert B.match(_strip(three(301)), 4, 1)[0] == [(0, 0)]
    # the reference stays rank 0 even when a candidate ties it at D = 0 with a smaller corner: reference (0, 3)
    flat = B.match(_strip([7] * 12), 4, 3)
    assert flat[1] == [(0, 3), (0, 0), (0, 1), (0, 2)] and len(flat[1]) == 4   # 7 kept -> N2 = 4


def test_header_and_signatures_declare_the_entry_points():
    from reconfigisp_amd import lib as L
    header = open(os.path.join(ROOT, 'include', 'risp.h')).read()
    for name in NEW_SYMBOLS:
        assert re.search(r'\b%s\(' % name, header), name
        assert name in L.SIGNATURES, name
    assert len(L.SIGNATURES['risp_origin_bm3d'][1]) == 16


def test_library_exports_the_entry_points():
    from reconfigisp_amd import lib as L
    assert os.path.exists(L.LIB_PATH), 'build the library first (__graft_entry__.build())'
    so = ctypes.CDLL(L.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(so, name), name
    so.risp_origin_bm3d_scratch_bytes.restype = ctypes.c_size_t
    one = so.risp_origin_bm3d_scratch_bytes(1, 256, 256)
    assert one > 7056 * 16 * 3 * 64 * 4 and so.risp_origin_bm3d_scratch_bytes(3, 256, 256) == 3 * one
    assert so.risp_origin_bm3d_scratch_bytes(1, 3, 256) == 0
    # packed corners hold 16 bits each, the kernels index 3 H W with int arithmetic: both limits refused
    assert so.risp_origin_bm3d_scratch_bytes(1, 65535, 8) > 0 and so.risp_origin_bm3d_scratch_bytes(1, 65536, 8) == 0
    assert so.risp_origin_bm3d_scratch_bytes(1, 30000, 30000) == 0


# ------------------------------------------------------------------ opt-in keys on the CPU seam
class _Bm3dOracle:
    """the test backend plus origin_denoise('bm3d') from the float64 reference"""
    @staticmethod
    def origin_denoise(x, option, params, scales=(1.0, 1.0)):
        if option != 'bm3d':
            from oracle_backend import OracleImpl
            return OracleImpl.origin_denoise(x, option, params, scales)
        y, _ = B.bm3d(x, 2.55 * torch.as_tensor(params['cff']).float(), params['n1'], params['cspace'],
                      params['wtransform'], params['neighborhood'], scales[0], scales[1])
        return y


@pytest.fixture
def seam(monkeypatch):
    import reconfigisp_amd.functional as F
    from oracle_backend import OracleImpl
    impl = type('Bm3dOracleImpl', (OracleImpl,), {'origin_denoise': _Bm3dOracle.origin_denoise})
    monkeypatch.setattr(F, '_IMPL', impl)


def test_define_g_classical_bm3d_key():
    from reconfigisp_amd.codes.models import networks
    from reconfigisp_amd.codes.models.modules.srcnn_res_arch import SRCNNRes
    from reconfigisp_amd.codes.models.modules.tools_origin import OriginNoiseBm3d
    net = dict(which_model_G='OriginUniversal', architecture='Demosaic_02_sRGB_15_01', module_path=None)
    plain = networks.define_G(dict(network_G=net))
    assert isinstance(plain.all_modules[1], SRCNNRes)                           # default off: the proxy
    classical = networks.define_G(dict(network_G=dict(net, classical_bm3d=True)))
    assert isinstance(classical.all_modules[1], OriginNoiseBm3d)
    off = networks.define_G(dict(network_G=dict(net, classical_bm3d=False)))
    assert isinstance(off.all_modules[1], SRCNNRes)


def test_origin_universal_bm3d_on_cpu_seam(seam):
    from reconfigisp_amd.codes.models.modules.origin_universal import OriginUniversal
    model = OriginUniversal(None, 'sRGB_15', classical_bm3d=True)
    x = torch.rand(1, 3, 16, 20)
    y = model(x)
    ref, _ = B.bm3d(x * 255., 2.55 * 12 * torch.sigmoid(torch.tensor(-1.946)), 8, 0, 0, 8)
    assert torch.allclose(y, ref / 255., atol=1.5 / 255.)


@pytest.mark.filterwarnings('ignore:Detected call of')
def test_darts_ft_bm3d_teacher_key(seam):
    """proxy_ft_params.bm3d_teacher: off by default (today's fine-tuned set), on: bm3d appended last with its
    classical teacher; finetune_proxies() on the CPU seam changes the bm3d proxy and gives finite losses"""
    import random
    from collections import OrderedDict
    from reconfigisp_amd.codes.models import create_model
    from reconfigisp_amd.codes.models.modules.tools_origin import OriginNoiseBm3d

    def opt(teacher):
        ft = dict(memory_size=2, ft_interval=1, ft_steps=1)
        if teacher is not None:
            ft['bm3d_teacher'] = teacher
        return OrderedDict(model='darts_ft', gpu_ids=None, dist=False, is_train=True,
                           network_G=dict(which_model_G='SuperPruneFifteenDemosFourBayerTwoFt', n_step=1, n_modules=15,
                                          prune_threshold=0.2, module_path=None),
                           path=dict(pretrain_model_G=None, strict_load=True), proxy_ft_params=ft,
                           train=dict(lr_G=1e-3, momentum_G=0.9, lr_meta=1e-2, beta1=0.9, beta2=0.99,
                                      pixel_criterion='l2', lr_scheme='MultiStepLR', lr_steps=[1000], restarts=None,
                                      restart_weights=None, lr_gamma=0.5, clear_state=False))
    base = ['crysisengine', 'whiteworld', 'bilateral', 'median', 'fastnlm']
    assert [n for n, *_ in create_model(opt(None)).ft_nets] == base
    assert [n for n, *_ in create_model(opt(False)).ft_nets] == base
    model = create_model(opt(True))
    assert [n for n, *_ in model.ft_nets] == base + ['bm3d']
    assert isinstance(model.ft_nets[-1][3], OriginNoiseBm3d)
    model.ft_nets = model.ft_nets[-1:]                      # the bm3d entry alone: the other teachers are not under test
    model.ft_data = [torch.rand(1, 3, 16, 16)]
    idx = [n for n, _ in model.netG.proxy_ft_flag].index('bm3d')
    before = {k: v.clone() for k, v in model.netG.all_modules[-1][idx].state_dict().items()}
    random.seed(2)
    torch.manual_seed(2)
    model.finetune_proxies()
    assert np.isfinite(model.log_dict['ft_loss_bm3d'])
    after = model.netG.all_modules[-1][idx].state_dict()
    assert any(not torch.equal(after[k], before[k]) for k in before)
