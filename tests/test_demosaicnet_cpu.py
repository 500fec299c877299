"""DemosaicNet on the CPU: the loader's key / shape table, the three load-time folds in float64, the option keys of define_G, and
the unavailable state (raise / masked in the super-net) that stays exactly as before without weights."""
import functools

import pytest
import torch
import torch.nn.functional as Fn

import demosaicnet_reference as R
from reconfigisp_amd import demosaicnet as DN
from reconfigisp_amd.isp_kernels import demosaic as dm


@pytest.fixture
def unregister():
    """registration is process-global and the other tests rely on the masked state: always undo it"""
    yield
    dm.unregister_demosaicnet()


def _x(seed, n=2, h=12, w=20):
    return torch.rand(n, 1, h, w, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))


def test_loader_accepts_the_table(tmp_path):
    sd = R.random_state_dict(0)
    assert DN.check_state_dict(sd) is sd
    path = tmp_path / 'dmnet.pth'
    torch.save({k: v.float() for k, v in sd.items()}, str(path))
    net = DN.load_demosaicnet(str(path))
    assert net.cfa == 'rggb' and net.folded['conv1.weight'].shape == (64, 4, 3, 3)
    assert net.folded['conv1.weight'].dtype == torch.float32
    net = DN.load_demosaicnet(sd, cfa='grbg')
    assert net.cfa == 'grbg'
    assert len(DN.LAYOUT) == 2 + 30 + 8


def test_loader_rejects_missing_extra_and_misshapen_keys():
    sd = R.random_state_dict(0)
    bad = dict(sd)
    del bad['main_processor.conv7.bias']
    with pytest.raises(ValueError, match=r"missing key 'main_processor\.conv7\.bias'"):
        DN.load_demosaicnet(bad)
    bad = dict(sd, **{'main_processor.conv16.weight': torch.zeros(64, 64, 3, 3)})
    with pytest.raises(ValueError, match=r"unexpected key 'main_processor\.conv16\.weight'"):
        DN.load_demosaicnet(bad)
    bad = dict(sd, **{'upsampler.weight': torch.zeros(12, 1, 3, 3)})
    with pytest.raises(ValueError, match=r"'upsampler\.weight' has shape \(12, 1, 3, 3\)"):
        DN.load_demosaicnet(bad)
    with pytest.raises(ValueError, match='cfa'):
        DN.load_demosaicnet(sd, cfa='bggr')


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_rggb_fold_equals_the_released_network(seed):
    sd = R.random_state_dict(seed)
    x = _x(seed)
    ref = R.reference(x, sd)                                   # the released network on the RGB masked mosaic, BGR order
    got = R.folded_forward(x, DN.fold(sd))
    assert (got - ref).abs().max() <= 1e-12 * ref.abs().max()


@pytest.mark.parametrize('seed', [0, 1])
def test_grbg_fold_equals_the_mirrored_network(seed):
    sd = R.random_state_dict(seed)
    x = _x(seed, w=24)
    ref = R.reference(x.flip(3), sd, cfa='grbg').flip(3)       # G R / B G weights on the x-mirrored mosaic, mirrored back
    got = R.folded_forward(x, DN.fold(sd, 'grbg'))
    assert (got - ref).abs().max() <= 1e-12 * ref.abs().max()
    assert (got - R.folded_forward(x, DN.fold(sd))).abs().max() > 1e-3     # the phase matters


@pytest.mark.parametrize('h,w', [(4, 4), (6, 10), (16, 12)])
def test_pack_fold_into_conv1(h, w):
    sd = R.random_state_dict(3)
    x = _x(h * w, h=h, w=w)
    mp = 'main_processor.'
    p = Fn.conv2d(R.masked_mosaic(x), sd[mp + 'pack_mosaic.weight'], sd[mp + 'pack_mosaic.bias'], stride=2)
    ref = Fn.conv2d(p, sd[mp + 'conv1.weight'], sd[mp + 'conv1.bias'], padding=1)
    got = R.folded_first(x, DN.fold(sd))
    assert (got - ref).abs().max() <= 1e-12 * ref.abs().max()


def _nets(tmp_path):
    sd = R.random_state_dict(0)
    path = str(tmp_path / 'w.pth')
    torch.save(sd, path)
    return path, [dict(which_model_G='SuperPruneFifteenDemosFourBayerTwo', n_step=1, n_modules=15, prune_threshold=0.2,
                       module_path=None),
                  dict(which_model_G='OriginUniversal', architecture='Bayer_02_Demosaic_04_sRGB_01', module_path=None),
                  dict(which_model_G='IspUniversal', architecture='Bayer_02_Demosaic_04_sRGB_01', module_path=None,
                       individual_module_paths=None)]


def test_option_keys_for_every_network_kind(tmp_path, unregister):
    from reconfigisp_amd.codes.models import networks
    path, nets = _nets(tmp_path)
    assert networks.demosaicnet_options({}) == (None, 'rggb')
    assert networks.demosaicnet_options({'demosaicnet_weights': path, 'demosaicnet_cfa': 'grbg'}) == (path, 'grbg')
    assert networks.demosaicnet_options({'demosaicnet_weights': None, 'demosaicnet_cfa': None}) == (None, 'rggb')
    for net in nets:
        dm.unregister_demosaicnet()
        networks.define_G(dict(network_G=dict(net)))
        assert not dm.demosaicnet_available(), net['which_model_G']
        networks.define_G(dict(network_G=dict(net, demosaicnet_weights=path, demosaicnet_cfa='grbg')))
        assert dm.demosaicnet_available(), net['which_model_G']
        assert dm._BUILTIN is not None and dm._BUILTIN.cfa == 'grbg'
    with pytest.raises(ValueError, match='cfa'):
        networks.define_G(dict(network_G=dict(nets[1], demosaicnet_weights=path, demosaicnet_cfa='xyz')))


def _demosaic_slot(net):
    from reconfigisp_amd.codes.models.modules import tools_origin as T
    for mods in net.all_modules:
        if any(isinstance(m, T.DemosaicNet) for m in mods):
            return mods
    raise AssertionError('no DemosaicNet in the super-net')


def test_without_weights_the_op_stays_unavailable(tmp_path, unregister):
    from reconfigisp_amd.codes.models.modules.super_prune_fifteen_demos_four_bayer_two import SuperPruneFifteenDemosFourBayerTwo
    with pytest.raises(NotImplementedError):
        dm.Demosaic().run(torch.rand(1, 1, 8, 8), 'demosaicnet', {})
    net = SuperPruneFifteenDemosFourBayerTwo(n_step=1, threshold=0.2, module_path=None)
    mods = _demosaic_slot(net)
    mask = net._unavailable(mods, torch.device('cpu'))
    assert mask is not None and mask.tolist() == [0, 0, 0, 1]

    dm.load_demosaicnet(R.random_state_dict(0))
    assert net._unavailable(mods, torch.device('cpu')) is None          # with weights: the reference behaviour, no mask
    dm.unregister_demosaicnet()                                          # ... and back
    assert net._unavailable(mods, torch.device('cpu')).tolist() == [0, 0, 0, 1]
    with pytest.raises(NotImplementedError):
        dm.Demosaic().run(torch.rand(1, 1, 8, 8), 'demosaicnet', {})


def test_user_registration_still_wins(unregister):
    dm.load_demosaicnet(R.random_state_dict(0))
    seen = []
    dm.register_demosaicnet(lambda img: seen.append(img.shape) or img.repeat(1, 3, 1, 1))
    y = dm.Demosaic().run(torch.rand(1, 1, 8, 8), 'demosaicnet', {})
    assert seen == [(1, 1, 8, 8)] and y.shape == (1, 3, 8, 8)
    dm.unregister_demosaicnet()
    assert not dm.demosaicnet_available()


def test_builtin_refuses_cpu_tensors(unregister):
    dm.load_demosaicnet(R.random_state_dict(0))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        dm.Demosaic().run(torch.rand(1, 1, 8, 8), 'demosaicnet', {})


# ------------------------------------------------------------------------------------------------ the referee of the network-level test
# (tests/test_gpu_demosaicnet_space.py): checked on its own, as tests/test_net_reference_cpu.py does for the four proxy networks
@pytest.mark.parametrize('cfa', DN.CFA_PHASES)
def test_hooked_network_is_the_folded_forward(cfa):
    sd = R.random_state_dict(6)
    x = _x(6, h=12, w=20)
    fd = DN.fold(sd, cfa)
    y, up = R.network(x, fd)
    assert torch.equal(y, R.folded_forward(x, fd)) and torch.equal(up, R.tail(*R.body(x, fd), fd))
    ref = R.reference(x, sd) if cfa == 'rggb' else R.reference(x.flip(3), sd, 'grbg').flip(3)
    assert R.rel_err(y, ref) <= 1e-12
    fd32 = R.as_dtype(fd, torch.float32)                               # fp32 too: the yardstick of the budget report is the same code
    assert torch.equal(R.evaluate(x, fd, dtype=torch.float32)['y'], R.folded_forward(x.float(), fd32))
    # own masks reproduce autograd through relu; every hook is live; a wrong number of masks is refused
    gy = torch.randn(y.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    xg = x.clone().requires_grad_(True)
    want, = torch.autograd.grad(R.folded_forward(xg, fd), xg, gy)
    plain = R.evaluate(x, fd, gy)
    assert len(plain['pre']) == R.RELUS and plain['pre'][14].shape[1] == 128 and R.rel_err(plain['gx'], want) <= 1e-12
    masks = [p > 0 for p in plain['pre']]
    assert R.rel_err(R.evaluate(x, fd, gy, masks)['gx'], want) <= 1e-12
    for k in range(R.RELUS):
        flipped = [m.clone() for m in masks]
        # (conv15: a filter whose gate is live too - the product hides the other ones)
        live = (masks[k][:, :64] & masks[k][:, 64:] if k == 14 else masks[k]).nonzero()
        flipped[k][tuple(live[len(live) // 2].tolist())] = False
        assert R.rel_err(R.evaluate(x, fd, gy, flipped)['gx'], want) > 1e-9, 'mask %d is dead' % k
    for bad in (masks[:-1], masks + masks[-1:], masks[1:2] + masks[:1] + masks[2:]):
        if bad[0].shape != masks[0].shape or len(bad) != R.RELUS:
            with pytest.raises(ValueError):
                R.evaluate(x, fd, gy, bad)
    # saved_masks reads [x, conv1 .. conv14, fa, fb, up]
    acts = [torch.relu(p) for p in plain['pre'][:15]]
    saved = [x] + acts[:14] + [acts[14][:, :64], acts[14][:, 64:], plain['up']]
    assert all(torch.equal(a, b) for a, b in zip(R.saved_masks(saved), masks[:15]))
    with pytest.raises(ValueError):
        R.saved_masks(saved[:-1])


def test_space_table_reaches_every_branch():
    rows = R.CASES + R.KERNEL_CASES
    ids = [R.case_id(c) for c in rows]
    assert len(set(ids)) == len(ids), 'two rows are one case'
    for name, pred in R.BRANCHES.items():
        assert any(pred(c) for c in rows), 'no row reaches: ' + name
    sizes = {(4, 4), (4, 8), (8, 12), (36, 20), (32, 32), (34, 66), (66, 34), (40, 72), (64, 96)}
    grad = [c for c in R.CASES if c['form'] == 'grad']
    assert {c['hw'] for c in grad} == sizes and {c['hw'] for c in R.KERNEL_CASES} == sizes
    assert {c['form'] for c in R.CASES} == {'grad', 'infer', 'reuse'}
    for c in rows:
        h, w = c['hw']
        assert h % 2 == 0 and w % 2 == 0 and h >= 4 and w >= 4 and c['cfa'] in DN.CFA_PHASES and c['arith'] in ('f16x2', 'f32'), R.case_id(c)
        if c['form'] != 'infer':
            assert c['n'] * h * w <= R.MAX_PIXELS, R.case_id(c)
    assert sum(c['n'] == 3 for c in grad) >= 2 and all(c['n'] == 1 for c in grad if c['hw'] == (64, 96))
    for hw in sizes:                                               # both arithmetics wherever the plane takes a matrix kernel
        if (hw[1] // 2) % 4 == 0:
            assert {c['arith'] for c in grad if c['hw'] == hw} == {'f16x2', 'f32'}, hw
    grbg = lambda form: sum(c['cfa'] == 'grbg' for c in R.CASES if c['form'] == form)
    assert grbg('grad') >= 3 and grbg('infer') >= 1 and grbg('reuse') >= 1
    assert {c['input'] for c in grad} == {'smooth', 'quantised', 'constant'}
    sd, fd, x, gy = R.case_inputs(R.CASES[4])
    assert x.dtype == torch.float32 and float(x[0].min()) == float(x[0].max()) == 0.5 and float(x[1].min()) < float(x[1].max())
    assert all(torch.equal(a, b) for a, b in zip(R.case_inputs(R.CASES[4])[2:], (x, gy)))
    assert all(torch.equal(v, v.float().double()) for v in fd.values())        # the fold as the device holds it


@pytest.mark.parametrize('arith', ['f16x2', 'f32'])
def test_expected_entries_against_the_route(arith, monkeypatch):
    from reconfigisp_amd import convnets as CN
    monkeypatch.setattr(CN, 'CONV_ARITH', arith)
    body_f, body_b = CN.pack_kinds(3, 64, 64, False), CN.pack_kinds(3, 64, 64, True)
    for c in R.CASES:
        if c['arith'] != arith:
            continue
        h, w = c['hw'][0] // 2, c['hw'][1] // 2
        infer = c['form'] == 'infer'
        e = R.expected_entries(c)
        assert e['conv1'] == CN.route(3, 4, 64, h, w, load=CN.LOAD_UNSHUFFLE2, epi=CN.EPI_RELU | CN.EPI_CASEBIAS, infer=infer,
                                      have=CN.pack_kinds(3, 4, 64)), R.case_id(c)
        assert e['body'] == CN.route(3, 64, 64, h, w, epi=CN.EPI_RELU, infer=infer, have=body_f), R.case_id(c)
        assert e['body_bwd'] == CN.route(3, 64, 64, h, w, transpose=True, epi=CN.EPI_MASK | CN.EPI_NOBIAS, have=body_b), R.case_id(c)
        assert e['body_bwd'] == CN.route(3, 64, 64, h, w, transpose=True, epi=CN.EPI_NOBIAS, have=body_b), R.case_id(c)
        assert e['join_bwd'] == CN.route(3, 64, 64, h, w, transpose=True, epi=CN.EPI_ADD | CN.EPI_MASK | CN.EPI_NOBIAS, add_c=64,
                                         have=body_b), R.case_id(c)
        toep, tapout, narrow3 = CN.small_packs(3, 64, 4, CN.EPI_SHUFFLE2 | CN.EPI_NOBIAS, False)
        assert e['conv1_bwd'] == CN.route_small(3, 64, 4, h, w, c['n'], infer=False, has_mask=False, has_toep=toep, has_tapout=tapout,
                                                has_narrow3=narrow3), R.case_id(c)
        assert sum(R.expected_calls(c).values()) == 16 and sum(R.expected_calls(c, True).values()) == 16


@functools.lru_cache(maxsize=None)
def _head_survey():
    """per row of CASES: (id, form, [head_pre_error, undecided units] with float64's own ``up`` and with the fp32 restatement's)"""
    out = []
    for c in R.CASES:
        sd, fd, x, gy = R.case_inputs(c)
        per = []
        for dt in (torch.float64, torch.float32):
            up = R.evaluate(x, fd, dtype=dt)['up'].float()
            per.append((R.head_pre_error(x, up, fd), int(R.head_decisions(x, up, fd)[1].sum())))
        out.append((R.case_id(c), c['form'], per))
    return out


def test_tau_head_is_the_measured_error():
    """TAU_HEAD = 4 x the largest error of the fp32 restatement of the head's hidden pre-activation over all rows, re-measured"""
    errs = [per[0][0] for _, _, per in _head_survey()]                 # (float64's own ``up``: the same bits on every machine)
    errs += [R.head_pre_error(k['x'], k['up'], k['fd']) for k in map(R.kernel_inputs, R.KERNEL_CASES)]
    assert 1e-7 < min(errs) and 0.9 * R.HEAD_PRE_FP32_ERR <= max(errs) <= R.HEAD_PRE_FP32_ERR, (min(errs), max(errs))
    assert R.TAU_HEAD == 4 * R.HEAD_PRE_FP32_ERR and R.MAX_UNDECIDED == 4 and R.MAX_UNDECIDED_CPU == 2


def test_undecided_head_units_stay_under_the_cap():
    """every row that differentiates: at most MAX_UNDECIDED_CPU undecided units, with float64's own ``up`` and with the fp32
    restatement's standing in for the device's; every kernel row: none after at most REDRAWS draws"""
    for cid, form, per in _head_survey():
        if form != 'infer':
            assert max(u for _, u in per) <= R.MAX_UNDECIDED_CPU, (cid, per)
    for c in R.KERNEL_CASES:
        k = R.kernel_inputs(c)
        assert 1 <= k['draws'] <= R.REDRAWS and not R.head_decisions(k['x'], k['up'], k['fd'])[1].any(), R.case_id(c)
        assert all(torch.equal(v, v.float().double()) for v in (k['x'], k['up'], k['fa'], k['fb'], k['gy'], k['gup'], k['add']))


_GRAD_ROWS = sorted((c for c in R.CASES if c['form'] == 'grad'), key=lambda c: c['n'] * c['hw'][0] * c['hw'][1])


def _worst(case, name):
    dev = R.wrong_device(case, name)
    if dev is None:
        return None
    sd, fd, x, gy = R.case_inputs(case)
    res = R.judge(x, fd, dev, gy)
    return max(res['rows'], key=lambda r: r[1]), res


def test_the_rule_passes_the_network_itself():
    """float64 standing in for the device: every tensor of every size at rounding, with the undecided units enumerated"""
    seen = set()
    for c in _GRAD_ROWS:
        if (c['hw'], c['cfa']) in seen:
            continue
        seen.add((c['hw'], c['cfa']))
        (what, e, _), res = _worst(c, None)
        assert e <= 1e-11 and res['flips'] == 0 and len(res['rows']) == 18, (R.case_id(c), what, e, res['flips'])


def test_an_undecided_unit_is_enumerated_not_blanked():
    """a device that takes the other side of an undecided unit passes; one that takes the other side of a DECIDED unit does not"""
    c = next(c for c in _GRAD_ROWS if c['hw'] == (40, 72) and c['cfa'] == 'grbg')
    sd, fd, x, gy = R.case_inputs(c)
    dev = R.wrong_device(c, None)
    hmask, und = R.head_decisions(x, dev['saved'][17], fd)
    assert 1 <= int(und.sum()) <= R.MAX_UNDECIDED_CPU
    masks = R.saved_masks(dev['saved'])
    gx_other = R.evaluate(x, fd, gy, masks + [hmask ^ und])['gx']
    assert R.rel_err(gx_other, dev['gx']) > R.BAR                      # the flip is far above the bar ...
    res = R.judge(x, fd, dict(dev, gx=gx_other), gy)
    assert res['undecided'] == int(und.sum()) and res['rows'][-1][0] == 'gx' and res['rows'][-1][1] <= 1e-11     # ... and legitimate
    decided = (~und).nonzero()[12345]
    wrong = hmask.clone()
    wrong[tuple(decided.tolist())] ^= True
    res = R.judge(x, fd, dict(dev, gx=R.evaluate(x, fd, gy, masks + [wrong])['gx']), gy)
    assert res['rows'][-1][1] > R.BAR


@pytest.mark.parametrize('name', R.WRONG)
def test_the_rule_tells_a_wrong_variant_apart(name):
    """each defect, run through the same comparison in float64 at the table's sizes, breaks the bar on some row"""
    assert len(R.WRONG) >= 12
    tried = []
    for c in _GRAD_ROWS:
        got = _worst(c, name)
        if got is None:
            continue
        (what, e, _), _ = got
        tried.append((R.case_id(c), what, e))
        if e > R.BAR:
            return
    raise AssertionError('%s stays within %.0e on every row: %s' % (name, R.BAR, tried))
