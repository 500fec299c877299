"""GPU: ``convnets.conv_wgrad`` - the weight gradient of one conv layer, risp_conv2d_wgrad behind it - over its argument space, against
float64.

The table, the seeded walk, the float64 restatement, the form of each launch and what the entry point refuses are tests/wgrad_reference.py
(plain CPU code, checked by tests/test_wgrad_reference_cpu.py, which also shows that a float32 restatement of every table case stays within
a quarter of the bar used here).  Every case goes through ``CN.conv_wgrad`` with ``L.call`` recorded, and is held to

  1. entry: one risp_conv2d_wgrad launch and one risp_plane_sums; the first-layer shortcut additionally one risp_rect_sums, its wgrad launch
     on the image channels alone; risp_conv_wgrad_scratch_floats equals the restated slot count;
  2. accuracy: max |dW - ref| / max|ref| <= 3e-6, the bar of the fp32-accumulating conv kernels (test_gpu_toep.py, vector kernel) - seven times
     the 4.3e-7 recorded for this kernel at 32 x 256 x 256 pixels (profiles/r06_wgrad_ft.txt), a reduction far longer than any here -,
     ``assert_close`` with conftest's defaults for dW and db, and exactly 0.0 for taps that never land inside the image;
  3. determinism: a second call gives the same bits;
  4. scratch independence: with the stream's cached scratch filled with NaN a third call gives the same bits again - every slot the
     finishing kernel reads was written by this launch.

Contracts, one test each: the result does not depend on what earlier calls left in the scratch; scaling the operands by powers of two
scales the result bit for bit; a NaN in one channel stays in that channel's slice of dW; the gradient of a batch is the float64 sum of its
images'; refused arguments return or raise on the host and write nothing; the SRCNNRes training chain against float64 autograd of the oracle.
RISP_BUDGET_REPORT=1 prints one line per case (tools/wgrad_budget_report.py)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import wgrad_reference as R
from conftest import assert_close
from wgrad_reference import BAR, CONSTCH, PLAIN

pytestmark = pytest.mark.gpu

NAN, GUARD, BAND = float('nan'), 12345.0, 64
REPORT = os.environ.get('RISP_BUDGET_REPORT') == '1'
WGRAD, PLANE, RECT = 'risp_conv2d_wgrad', 'risp_plane_sums', 'risp_rect_sums'


@pytest.fixture
def calls(monkeypatch):
    """every C-ABI call ``conv_wgrad`` makes: (name, arguments)"""
    from reconfigisp_amd import convnets as CN, lib as L
    rec, real = [], L.call

    def spy(name, *a):
        rec.append((name, a))
        return real(name, *a)
    monkeypatch.setattr(CN.L, 'call', spy)
    return rec


def dev(case, x=None, gy=None, cv=None):
    x0, gy0, cv0 = R.inputs(case)
    pick = lambda a, b: (b if a is None else a)
    x, gy, cv = pick(x, x0), pick(gy, gy0), pick(cv, cv0)
    return x.cuda(), gy.cuda(), (cv.cuda() if cv is not None else None)


def wgrad(case, x, gy, cv):
    from reconfigisp_amd import convnets as CN
    n = gy.shape[0]
    dw, db = CN.conv_wgrad(x, gy, case['cin'], case['cout'], case['k'], n, case['h'], case['w'], load=case['load'], cin_img=case['cin_img'], cvals=cv)
    torch.cuda.synchronize()
    return dw, db


def scratch():
    """the cached scratch of the current stream, or None"""
    from reconfigisp_amd import convnets as CN
    d = torch.device('cuda', torch.cuda.current_device())
    for key, t in CN._WGRAD_SCRATCH.items():
        if key[1] == torch.cuda.current_stream(d).cuda_stream and torch.device(key[0]).index in (None, d.index):
            return key, t
    return None, None


def drop_scratch():
    from reconfigisp_amd import convnets as CN
    key, _ = scratch()
    if key is not None:
        del CN._WGRAD_SCRATCH[key]


def check_entry(case, rec, lib):
    names = [r[0] for r in rec]
    short = R.shortcut(case)
    assert names == ([WGRAD, PLANE, RECT] if short else [WGRAD, PLANE]), (case['name'], names)
    if case['shortcut'] is not None:
        assert short == case['shortcut'], case['name']
    d = rec[0][1][0]._obj                                    # the descriptor behind byref
    cin, cout, k = R.launched(case)
    assert (d.cin, d.cout, d.ksize) == (cin, cout, k) and d.load_mode == (PLAIN if short else case['load']), case['name']
    frm = R.form(cin, cout, k)
    assert case['form'] in (None, frm), (case['name'], frm)
    assert lib.risp_conv_wgrad_scratch_floats(cin, cout, k) == R.scratch_floats(cin, cout, k) <= rec[0][1][4]
    return frm


@pytest.mark.parametrize('name', sorted(R.ALL))
def test_case(name, calls):
    from reconfigisp_amd import lib as L
    case = R.ALL[name]
    x, gy, cv = dev(case)
    dw, db = wgrad(case, x, gy, cv)
    frm = check_entry(case, calls, L.load())
    ref, refb = R.ref64(case)
    rms, mx = R.errors(dw, ref)
    if REPORT:
        print('WGRAD %-56s | %-17s rms %.3e max %.3e bar %.1e ratio %.2f' % (name, ('shortcut+' if R.shortcut(case) else '') + frm, rms, mx, BAR, mx / BAR))
    assert tuple(dw.shape) == tuple(ref.shape) and torch.isfinite(dw).all().item()
    assert mx <= BAR, '%s (%s): max error %.3e of max|ref| (rms %.3e), bar %.1e' % (name, frm, mx, rms, BAR)
    assert_close(dw, ref, what=name + ' dW')
    assert_close(db, refb, what=name + ' db')
    zero = (ref == 0)
    assert zero[:, :, R.never_lands(case['k'], case['h'], case['w'])].all()
    assert (dw.cpu()[zero] == 0).all().item(), '%s: taps that never land inside the image are not exactly 0' % name
    dw2, db2 = wgrad(case, x, gy, cv)
    assert torch.equal(dw, dw2) and torch.equal(db, db2), '%s: a second call gives other bits' % name
    _, ws = scratch()
    assert ws is not None and ws.numel() >= R.scratch_floats(*R.launched(case))
    ws.fill_(NAN)
    dw3, _ = wgrad(case, x, gy, cv)
    assert not torch.isnan(dw3).any().item() and torch.equal(dw, dw3), '%s: the finishing kernel read a slot this launch did not write' % name


def test_result_does_not_depend_on_the_calls_before():
    """the largest scratch (9x9 plain), then a one-tile thin layer, then 1x1 - each against the same case run first in a fresh scratch"""
    order = ['9x9_17to64 plain 2x20x36', '5x5_32to3 thin_out 1x8x16', '1x1_64to32 k1 3x7x15', '3x3_3to64 thin_in 1x8x16']
    fresh = {}
    for name in order:
        drop_scratch()
        fresh[name] = wgrad(R.CASES[name], *dev(R.CASES[name]))[0]
    drop_scratch()
    for name in order + order[::-1]:
        got = wgrad(R.CASES[name], *dev(R.CASES[name]))[0]
        assert torch.equal(got, fresh[name]), '%s: other bits after other launches on the same scratch' % name
    _, ws = scratch()
    assert ws.numel() == R.scratch_floats(17, 64, 9)


FORM_CASES = ['1x1_64to32 k1 3x7x15', '3x3_33to40 plain 1x9x17', '9x9_17to64 plain 2x20x36', '3x3_10to33 thin_in 3x7x15', '9x9_3to64 thin_in 1x9x17',
              '3x3_64to3 thin_out 1x9x17', '5x5_40to6 thin_out 3x7x15', '9x9_17to64 plain 2x9x17 constch 4', '5x5_40to6 thin_out 2x9x17 constch 11',
              '9x9_13to64 thin_in 3x20x36 constch 3']


@pytest.mark.parametrize('name', FORM_CASES)
def test_powers_of_two_scale_the_result_bit_for_bit(name):
    """dW(2^-40 x, 2^20 gy) == 2^-20 dW(x, gy), dW(2^12 x, 2^3 gy) == 2^15 dW(x, gy): standard normals, nothing under- or overflows (the
    constants of a CONSTCH layer are input channels: scaled with x)"""
    case = R.CASES[name]
    x, gy, cv = dev(case)
    dw, db = wgrad(case, x, gy, cv)
    for ex, eg in ((-40, 20), (12, 3)):
        dws, dbs = wgrad(case, x * 2.0 ** ex, gy * 2.0 ** eg, cv * 2.0 ** ex if cv is not None else None)
        assert torch.equal(dws, dw * 2.0 ** (ex + eg)), '%s: x * 2^%d, gy * 2^%d' % (name, ex, eg)
        assert torch.equal(dbs, db * 2.0 ** eg), name


# (case, input channel that gets the NaN, gy channel that gets the NaN): channels in the second 32-channel block among them
LOCAL = [('1x1_64to32 k1 3x7x15', 35, 17), ('3x3_33to40 plain 1x9x17', 32, 39), ('9x9_17to64 plain 2x20x36', 16, 33), ('3x3_10to33 thin_in 3x7x15', 9, 32),
         ('9x9_3to64 thin_in 1x9x17', 1, 63), ('3x3_64to3 thin_out 1x9x17', 63, 2), ('5x5_40to6 thin_out 3x7x15', 35, 5),
         ('9x9_17to64 plain 2x9x17 constch 4', 3, 0), ('9x9_17to64 plain 2x9x17 constch 4', 16, 40), ('5x5_40to6 thin_out 2x9x17 constch 11', 35, 0),
         ('5x5_40to6 thin_out 2x1x17 constch 3', 35, 3), ('9x9_13to64 thin_in 3x20x36 constch 3', 7, 20), ('9x9_13to64 thin_in 3x20x36 constch 3', 2, 63)]


@pytest.mark.parametrize('name,ci,co', LOCAL)
def test_a_nan_stays_in_its_channel(name, ci, co):
    """a NaN in one input channel (of one image: a pixel of an image channel, the constant of a constant plane) leaves every other dW[:, ci']
    with the bits of the clean run and makes dW[:, ci] NaN wherever the float64 restatement is; the same for one gy channel and the rows of
    dW.  Nothing finer than the channel is asserted (the thin-out form multiplies halo columns by zero rows)."""
    case = R.CASES[name]
    x0, gy0, cv0 = R.inputs(case)
    clean, _ = wgrad(case, *dev(case))
    # the input channel
    x, cv = x0.clone(), (cv0.clone() if cv0 is not None else None)
    if case['load'] == CONSTCH and ci >= case['cin_img']:
        cv[case['n'] - 1, ci - case['cin_img']] = NAN
    else:
        x[case['n'] - 1, ci, case['h'] // 2, case['w'] // 3] = NAN
    dw, _ = wgrad(case, *dev(case, x=x, cv=cv))
    ref, _ = R.restate(x, gy0, case['k'], cv, case['cin_img'])
    others = [c for c in range(case['cin']) if c != ci]
    assert torch.isnan(ref[:, ci]).any() and not torch.isnan(ref[:, others]).any()
    assert torch.equal(dw[:, others], clean[:, others]), '%s: a NaN in input channel %d reaches other channels of dW' % (name, ci)
    assert torch.isnan(dw[:, ci].cpu())[torch.isnan(ref[:, ci])].all().item(), '%s: the NaN of input channel %d is lost' % (name, ci)
    # the gradient channel
    gy = gy0.clone()
    gy[0, co, case['h'] // 2, case['w'] // 2] = NAN
    dw, db = wgrad(case, *dev(case, gy=gy))
    ref, refb = R.restate(x0, gy, case['k'], cv0, case['cin_img'])
    others = [c for c in range(case['cout']) if c != co]
    assert torch.isnan(ref[co]).any() and not torch.isnan(ref[others]).any()
    assert torch.equal(dw[others], clean[others]), '%s: a NaN in gy channel %d reaches other rows of dW' % (name, co)
    assert torch.isnan(dw[co].cpu())[torch.isnan(ref[co])].all().item(), '%s: the NaN of gy channel %d is lost' % (name, co)
    assert torch.isnan(db[co]).item() and not torch.isnan(db[others]).any().item() and torch.isnan(refb[co]).item()


BATCH = ['1x1_33to1 k1 3x7x15', '3x3_64to64 plain 3x7x15', '5x5_6to40 thin_in 5x2x70', '5x5_40to6 thin_out 3x7x15', '9x9_31to64 plain 3x7x15',
         '9x9_17to64 plain 3x7x15 constch 4', '9x9_17to64 thin_in 3x20x36 constch 3']


@pytest.mark.parametrize('name', BATCH)
def test_batch_is_the_sum_of_its_images(name):
    """dW of n images against the float64 sum of the single-image float64 restatements, within the bar; db likewise within assert_close"""
    case = R.CASES[name]
    x, gy, cv = R.inputs(case)
    assert case['n'] > 1
    parts = [R.restate(x[i:i + 1], gy[i:i + 1], case['k'], cv[i:i + 1] if cv is not None else None, case['cin_img']) for i in range(case['n'])]
    ref, refb = sum(p[0] for p in parts), sum(p[1] for p in parts)
    dw, db = wgrad(case, *dev(case))
    mx = R.errors(dw, ref)[1]
    assert mx <= BAR, (name, mx)
    assert_close(dw, ref, what=name + ' dW')
    assert_close(db, refb, what=name + ' db')


class Guarded:
    """a device buffer between two bands of BAND sentinel floats, NaN inside"""

    def __init__(self, *shape):
        numel = int(np.prod(shape))
        self.raw = torch.full((numel + 2 * BAND,), GUARD, device='cuda')
        self.t = self.raw[BAND: BAND + numel].view(*shape)
        self.t.fill_(NAN)

    def untouched(self):
        return (self.raw[:BAND] == GUARD).all().item() and (self.raw[-BAND:] == GUARD).all().item() and torch.isnan(self.t).all().item()


def test_refused_arguments_return_on_the_host_and_write_nothing():
    """through the C ABI: a scratch one float short, a grouped descriptor, cin = 65, k = 7, null pointers, the UNSHUFFLE load, CONSTCH without its
    constants, and the two 9x9 layers the LDS check refuses (32 input channels and more: 32 x 129 + 32 x 385 floats are 65 792 bytes) -
    a non-zero status, the NaN fill of dw and its guard bands intact.  Through ``conv_wgrad``: RuntimeError for the same layers, and from
    risp_plane_sums for N x cout = 65536"""
    from reconfigisp_amd import convnets as CN, lib as L
    lib = L.load()
    n, h, w = 2, 9, 17
    rng = np.random.Generator(np.random.PCG64(77))
    x, gy, cv = R.rnd(rng, n, 65, h, w).cuda(), R.rnd(rng, n, 64, h, w).cuda(), R.rnd(rng, n, 64).cuda()
    ws = torch.zeros(R.scratch_floats(17, 64, 9) + 1, device='cuda')
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def desc(cin, cout, k, load=PLAIN, cin_img=0, cvals=None, group_n=0, xt=x):
        return L.ConvDesc(N=n, H=h, W=w, cin=cin, cout=cout, ksize=k, load_mode=load, cin_img=cin_img, epilogue=0, add_c=0, x=p(xt), wpack=None,
                          bias=None, cvals=p(cvals), add=None, mask=None, y=None, group_n=group_n)

    ok = lambda d: lib.risp_conv_wgrad_scratch_floats(d.cin, d.cout, d.ksize)
    refused = [('scratch one float short', desc(11, 11, 3), gy, True, ws, lambda d: ok(d) - 1),
               ('grouped descriptor', desc(11, 11, 3, group_n=1), gy, True, ws, ok),
               ('cin 65', desc(65, 8, 3), gy, True, ws, ok), ('cout 65', desc(8, 65, 3), gy, True, ws, ok), ('k 7', desc(17, 64, 7), gy, True, ws, lambda d: ws.numel()),
               ('null gy', desc(11, 11, 3), None, True, ws, ok), ('null dw', desc(11, 11, 3), gy, False, ws, ok), ('null scratch', desc(11, 11, 3), gy, True, None, ok),
               ('null x', desc(11, 11, 3, xt=None), gy, True, ws, ok),
               ('unshuffle load', desc(4, 11, 3, load=R.UNSHUFFLE), gy, True, ws, ok),
               ('constch without its constants', desc(17, 64, 9, load=CONSTCH, cin_img=4), gy, True, ws, ok),
               ('constch without image channels', desc(17, 64, 9, load=CONSTCH, cin_img=0, cvals=cv), gy, True, ws, ok),
               ('9x9 32 -> 64: LDS', desc(32, 64, 9), gy, True, ws, ok), ('9x9 64 -> 3: LDS', desc(64, 3, 9), gy, True, ws, ok)]
    for what, d, g, has_dw, scr, floats in refused:
        out = Guarded(d.cout, d.cin, d.ksize, d.ksize)
        status = lib.risp_conv2d_wgrad(C.byref(d), p(g), p(out.t) if has_dw else None, p(scr), floats(d), None)
        torch.cuda.synchronize()
        assert status != 0 and b'risp_conv2d_wgrad' in lib.risp_last_error(), what
        assert out.untouched(), '%s: refused, and dw was written' % what
        with pytest.raises(RuntimeError, match='risp_conv2d_wgrad'):
            L.call(WGRAD, C.byref(d), p(g), p(out.t) if has_dw else None, p(scr), floats(d), None)
    assert b'tile too large for LDS' in lib.risp_last_error()
    # the same descriptor with everything in order is taken
    out = Guarded(11, 11, 3, 3)
    d = desc(11, 11, 3)
    assert lib.risp_conv2d_wgrad(C.byref(d), p(gy), p(out.t), p(ws), ok(d), None) == 0
    torch.cuda.synchronize()
    assert not torch.isnan(out.t).any().item() and (out.raw[:BAND] == GUARD).all().item() and (out.raw[-BAND:] == GUARD).all().item()
    for cin, cout, k, kw in ((65, 8, 3, {}), (17, 64, 7, {}), (32, 64, 9, {}), (64, 3, 9, {}), (4, 11, 3, dict(load=CN.LOAD_UNSHUFFLE2)),
                             (17, 64, 9, dict(load=CN.LOAD_CONSTCH, cin_img=4))):
        with pytest.raises(RuntimeError, match='risp_conv2d_wgrad'):
            CN.conv_wgrad(x, gy, cin, cout, k, n, h, w, **kw)
    big = 65536 // 64                                          # 1 x 1 pixels: N x cout = 65536 planes cost nothing
    xb, gb = torch.ones(big, 1, 1, 1, device='cuda'), torch.ones(big, 64, 1, 1, device='cuda')
    with pytest.raises(RuntimeError, match='risp_plane_sums'):
        CN.conv_wgrad(xb, gb, 1, 64, 1, big, 1, 1)
    dw, db = CN.conv_wgrad(xb[:-1], gb[:-1], 1, 64, 1, big - 1, 1, 1)                 # one image fewer: taken
    torch.cuda.synchronize()
    assert (dw == big - 1).all().item() and (db == big - 1).all().item()


@pytest.mark.parametrize('P', [0, 2])
@pytest.mark.parametrize('nhw', [(2, 9, 17), (1, 24, 40)])
def test_srcnn_res_training_chain_against_float64(P, nhw):
    """``_SrcnnResTrain`` through ProxyNet with kink-free weights (tests/test_gpu_conv_modes.py::test_srcnn_res_weight_gradients_vs_oracle): all
    six gradients against float64 autograd of the oracle fed doubles, conftest's defaults"""
    import isp_oracle as O
    from reconfigisp_amd.codes.models.modules.tools_proxy import ProxyNet
    n, h, w = nhw
    wts = O.make_weights('srcnn_res', 55, P)
    for k in list(wts):
        if k.endswith('.bias') and not k.startswith('srcnn.4'):
            s = torch.ones_like(wts[k])
            s[1::2] = -1.0
            wts[k] = s
        elif k.endswith('.weight'):
            wts[k] = wts[k] * 0.02
    rng = np.random.Generator(np.random.PCG64(900 + 10 * P + h))
    x, pv, gy = R.rnd(rng, n, 3, h, w).abs().clamp(0, 1), R.rnd(rng, n, P).abs().clamp(0, 1), R.rnd(rng, n, 3, h, w)
    leaf = {k: v.double().requires_grad_(True) for k, v in wts.items()}
    keys = sorted(leaf)
    yc = O.srcnn_res(x.double(), pv.double(), leaf)
    gref = torch.autograd.grad(yc, [leaf[k] for k in keys], gy.double())
    m = ProxyNet(P, None)
    m.load_state_dict(wts)
    m = m.cuda()
    m.train_weights = True
    yg = m(x.cuda(), pv.cuda() if P else None)
    assert_close(yg, yc, what='y')
    params = dict(m.named_parameters())
    ggot = torch.autograd.grad(yg, [params[k] for k in keys], gy.cuda())
    for k, a, b in zip(keys, ggot, gref):
        assert b.abs().max().item() > 0
        assert_close(a, b, what='grad ' + k)
