"""GPU: the per-image reduction kernels over their argument space - risp_reduce.hip (risp_channel_stats, risp_stats_bwd /
_rows, risp_grayworld_gains_fwd / _bwd, risp_srcnn_cvals, risp_srcnn_case_table, risp_histc, risp_mix_fwd / _bwd,
risp_plane_sums, risp_sse_uint8), risp_condfc.hip (risp_cond_fc_fwd / _bwd) and the two losses of risp_step.hip
(risp_pixel_loss, risp_local_global_l2) - against the float64 restatement of tests/reduce_reference.py.

The table, the grid mirror, the inputs and the bounds are plain CPU code in tests/reduce_space_cases.py (checked without
a GPU by tests/test_reduce_reference_cpu.py).  Every case is launched through the C ABI (lib.call) and held to:

  1. exact where the operation is exact: minimum, maximum and both first indices; histogram counts; the cvals copies
     and mean = fp32(sum) x fp32(1 / HW); the mixture's go_k = fp32(w_k gy); the statistics gradient's three fp32
     additions per element; the zero tail of the conditional head's gradient; the 12 zero gradient positions of each
     4 x 4 cell of the global branch (the buffer is handed over full of NaN);
  2. coverage, exactly, at every size: each summing kernel also runs on integer-valued inputs whose every fp32 partial
     sum is an integer below 2^24 (values 0..3 for the statistics and the plane sums; gy, o_k in {-1, 0, 1}; y - gt in
     {-1, 0, 1}; codes that differ by 0 or 255; the local branch with the gain pinned at 0.5 (b = 0) and at 2 (b = 4 a);
     integer cell centres for the global branch).  The result equals the integer sum: one dropped, repeated or
     misplaced element fails at any size.  (a = b does NOT give a gain of 1: mean / (mean + 1e-6) is below 1 in any
     arithmetic; that input runs too, test_local_global_l2_equal_planes, held to the bound, not to zero.)  The local / global partial slots
     plane x bx + block are read back and add up to each plane's integer sum;
  3. rounded quantities: |got - float64| <= MARGIN x depth x 2^-24 x sum |term|, depth the longest chain of roundings a
     term passes through (its products, the per-thread trips, 6 shuffle steps, the additions across the waves, the
     finishing trips and shuffles) from the grid mirror, MARGIN = 2 for the second-order terms; derived quantities
     (gains, gradients) by the first-order propagation written out beside each bound in reduce_space_cases.py.  The
     conditional head passes through __expf: there the yardstick is the fp32 restatement of the same formula against
     float64 through conftest.ErrorBudget with its stock settings;
  4. gates decided in fp32 (the ReLU of the head, the gain clamp at 0.5 / 2, the gray-world m >= eps, the mean clamp at
     0, the truncation to 8 bits): the inputs keep the float64 value away from every gate by more than the bound
     (asserted on the CPU), or sit exactly on it where fp32 and float64 agree by construction (a black plane, codes
     whose fp32 product v x 255 is the operation's own definition).  No case is excused after the fact;
  5. the same bits twice (every case runs twice into fresh buffers), and minimum, maximum, indices and counts the same
     in the aligned form and with the base moved by one float; the sums of the two forms are added in different orders
     and each is held to its own bound;
  6. guard bands: outputs and scratch sit between sentinel bands (tests/guarded.py), intact after every call, the scratch
     sized by risp_*_scratch_floats() / risp_sse_uint8_doubles() exactly;
  7. the REFUSED table: raised before a launch, every output untouched;
  8. the reconfigisp_amd.functional wrappers (and util.psnr_tensors) give the bits of the direct call.

RISP_BUDGET_REPORT=1 prints per entry point the number of cases, the largest error, its bound and the largest ratio
of an error to its bound (profiles/reduce_space_budget.txt).
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import reduce_reference as R
import reduce_space_cases as S
from conftest import ErrorBudget
from guarded import Guarded, off16

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
BUDGET = {}                      # entry -> [cases, largest error, its bound, largest ratio]


@pytest.fixture(scope='module', autouse=True)
def _budget_report():
    yield
    if os.environ.get('RISP_BUDGET_REPORT') == '1':
        print('\nBUDGET %-34s %6s %12s %12s %8s' % ('entry point: quantity', 'cases', 'err', 'bound', 'ratio'))
        for key in sorted(BUDGET):
            n, err, bound, ratio = BUDGET[key]
            print('BUDGET %-34s %6d %12.3e %12.3e %8.3f' % (key, n, err, bound, ratio))


class Checks(list):
    """collects the failures of a case; ``hold`` records the ratio of an error to its bound under ``key``"""

    def hold(self, key, what, got, ref, bound):
        got, ref, bound = np.asarray(got, F64), np.asarray(ref, F64), np.broadcast_to(np.asarray(bound, F64), np.shape(ref))
        err = np.abs(got - ref)
        bad = ~(err <= bound)                                  # NaN fails
        ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0))) if err.size else 0.0
        at = int(np.argmax(np.where(bound > 0, err / np.where(bound > 0, bound, 1), err > 0)))
        b = BUDGET.setdefault(key, [0, 0.0, 0.0, 0.0])
        b[0] += 1
        if ratio > b[3]:
            b[1], b[2], b[3] = float(err.reshape(-1)[at]), float(bound.reshape(-1)[at]), ratio
        print('%s: %s: largest error / bound %.3f' % (key, what, ratio))
        if bad.any():
            self.append('%s: %s: %d of %d beyond the bound, worst %.3e against %.3e' % (key, what, int(bad.sum()), bad.size, float(err.reshape(-1)[at]),
                                                                                      float(bound.reshape(-1)[at])))

    def exact(self, what, got, ref):
        got, ref = np.asarray(got), np.asarray(ref)
        if got.shape != ref.shape or not np.array_equal(got, ref):
            self.append('%s: not exact (%s)' % (what, 'shape' if got.shape != ref.shape else '%d of %d differ' % (int((got != ref).sum()), got.size)))

    def finish(self):
        assert not self, '%d checks failed:\n  %s' % (len(self), '\n  '.join(self))


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _st():
    import reconfigisp_amd.functional as F
    return F._stream()


def call(name, *args):
    from reconfigisp_amd import lib as L
    L.call(name, *args)


def dev(a, off=0):
    """a numpy array on the device: a fresh allocation, or a contiguous view ``off`` floats off a 16-byte boundary"""
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    assert t.data_ptr() % 16 == 0
    return off16(t, off) if off else t


def settle(failed, what, *guards):
    torch.cuda.synchronize()
    for g in guards:
        if g is not None and not g.bands_intact():
            failed.append('%s: wrote outside a buffer of %d floats' % (what, g.t.numel()))


def twice(failed, what, run):
    """the case run twice into fresh buffers: the same bits"""
    first, second = run(), run()
    for k in first:
        for a, b in zip(first[k] if isinstance(first[k], list) else [first[k]], second[k] if isinstance(second[k], list) else [second[k]]):
            if a is not None and a.tobytes() != b.tobytes():
                failed.append('%s: %s differs between two calls' % (what, k))
    return first


# ---------------------------------------------------------------------------------------------------- statistics
def stats_call(failed, x, off, what):
    from reconfigisp_amd import lib as L
    P, HW = x.shape
    n = L.load().risp_channel_stats_scratch_floats(P, HW)
    assert n == P * S.stat_blocks(HW) * 5
    xd, stats, arg, ws = dev(x, off), Guarded(P, 4), Guarded(P, 2), Guarded(n)
    call('risp_channel_stats', _p(xd), _p(stats.t), _p(arg.t), _p(ws.t), P, HW, _st())
    settle(failed, what, stats, arg, ws)
    return dict(stats=stats.t.cpu().numpy(), arg=arg.t.view(torch.int32).cpu().numpy())


def judge_stats(failed, x, got, off, what, integer):
    r, w = R.channel_stats(x), S.stats_walk(x.shape[1], off)
    s = got['stats']
    failed.exact(what + ' minimum', s[:, 0].astype(F64), r['mn'])
    failed.exact(what + ' maximum', s[:, 2].astype(F64), r['mx'])
    failed.exact(what + ' fourth word', s[:, 3], np.zeros(len(s), F32))
    failed.exact(what + ' first argmin / argmax', got['arg'], np.stack([r['imn'], r['imx']], 1))
    if integer:
        failed.exact(what + ' integer sum', s[:, 1].astype(F64), r['sum'])
    else:
        failed.hold('risp_channel_stats: sum', what, s[:, 1], r['sum'], S.sum_bound(w['depth'], np.abs(x.astype(F64)).sum(1)))


@pytest.mark.parametrize('hw,n,c', S.stats_cases(), ids=lambda v: str(v))
def test_channel_stats(hw, n, c):
    failed = Checks()
    for integer in (False, True):
        x = S.stats_input(hw, n, c, integer)
        forms = {}
        for off in (0, 1):
            what = 'HW %d (%s) %d x %d %s %s' % (hw, S.STATS_BRANCH[hw], n, c, 'integers' if integer else 'reals', 'moved by one float' if off else 'aligned')
            forms[off] = twice(failed, what, lambda: stats_call(failed, x, off, what))
            judge_stats(failed, x, forms[off], off, what, integer)
        failed.exact('across forms: min, max', forms[0]['stats'][:, [0, 2, 3]], forms[1]['stats'][:, [0, 2, 3]])
        failed.exact('across forms: indices', forms[0]['arg'], forms[1]['arg'])
    failed.finish()


@pytest.mark.parametrize('hw,kind', S.tie_cases())
def test_channel_stats_ties(hw, kind):
    failed, ran = Checks(), 0
    for off in (0, 1):
        made = S.tie_input(hw, kind, off)
        if made is None:
            continue                                           # the element form of this size has no unrolled trip
        x, want = made
        what = 'HW %d tie %s %s' % (hw, kind, 'moved by one float' if off else 'aligned')
        got = twice(failed, what, lambda: stats_call(failed, x, off, what))
        judge_stats(failed, x, got, off, what, False)
        failed.exact(what + ' the index the table names', got['arg'], want)
        ran += 1
    assert ran
    failed.finish()


@pytest.mark.parametrize('constant', [False, True], ids=['reals', 'constant'])
@pytest.mark.parametrize('row', S.STATS_BWD, ids=lambda r: r[5])
def test_stats_bwd(row, constant):
    hw, n, c, gs, which, branch = row
    x, gx, grads = S.stats_bwd_input(row, constant)
    r = R.channel_stats(x)
    arg = np.stack([r['imn'], r['imx']], 1).astype(np.int32)
    if constant:
        assert (arg == 0).all()                                # argmin == argmax
    use_arg = 'min' in which or 'max' in which
    failed, P = Checks(), n * c
    for off in (0, 1):
        what = 'HW %d %s %s' % (hw, branch, 'moved by one float' if off else 'aligned')

        def run():
            g = Guarded(P, hw, off=off)
            g.t.copy_(torch.from_numpy(gx))
            d = {k: (dev(v) if v is not None else None) for k, v in grads.items()}
            a = dev(arg) if use_arg else None
            if gs is None:
                call('risp_stats_bwd', _p(g.t), _p(d['min']), _p(d['mean']), _p(d['max']), _p(a), P, hw, _st())
            else:
                call('risp_stats_bwd_rows', _p(g.t), _p(d['min']), _p(d['mean']), _p(d['max']), _p(a), n, c, hw, gs, _st())
            settle(failed, what, g)
            return dict(gx=g.t.cpu().numpy())
        got = twice(failed, what, run)['gx']
        failed.exact(what + ' three fp32 additions per element', got, R.stats_bwd(gx, grads['min'], grads['mean'], grads['max'], arg, c, gs or 1, dtype=F32))
        ref = R.stats_bwd(gx, grads['min'], grads['mean'], grads['max'], arg, c, gs or 1)
        # the rounded 1 / HW and the product with it, then three additions, each of at most the sum of the magnitudes
        mags = R.stats_bwd(np.abs(gx), *[np.abs(grads[k]) if grads[k] is not None else None for k in ('min', 'mean', 'max')], arg, c, gs or 1)
        failed.hold('risp_stats_bwd: gx', what, got, ref, S.MARGIN * 5 * S.U * mags)
    failed.finish()


def test_grayworld_gains_and_gradient():
    sums, gk, hw = S.gray_case()
    n = len(sums)
    stats = np.zeros((n, 3, 4), F32)
    stats[:, :, 1] = sums
    failed = Checks()

    def run():
        gains, gm = Guarded(n, 3), Guarded(n, 3)
        sd, gd = dev(stats), dev(gk)
        call('risp_grayworld_gains_fwd', _p(sd), _p(gains.t), n, hw, _st())
        call('risp_grayworld_gains_bwd', _p(sd), _p(gd), _p(gm.t), n, hw, _st())
        settle(failed, 'gray-world', gains, gm)
        return dict(gains=gains.t.cpu().numpy(), gm=gm.t.cpu().numpy())
    got = twice(failed, 'gray-world', run)
    fwd, bwd = S.gray_bounds(sums, gk, hw)
    failed.hold('risp_grayworld_gains_fwd', 'ordinary, black, negative-mean planes', got['gains'], R.grayworld_gains(sums, hw), fwd)
    failed.hold('risp_grayworld_gains_bwd', 'ordinary, black, negative-mean planes', got['gm'], R.grayworld_gains_bwd(sums, gk, hw), bwd)
    failed.finish()


@pytest.mark.parametrize('hw,n,P,M', [(5, 1, 0, 1), (4096, 2, 5, 300), (129 * 129, 3, 2, 257)])
def test_srcnn_cvals_and_case_table(hw, n, P, M):
    failed = Checks()
    x = S.stats_input(hw, n, 3, False) / F32(300)
    g = S.rng(22, hw, P, M)
    pv, rcase = g.uniform(0, 1, size=(n, max(P, 1))).astype(F32)[:, :P], g.uniform(-1, 1, size=(9 + P, M)).astype(F32)
    st = stats_call(failed, x, 0, 'statistics')['stats'].reshape(n, 3, 4)

    def run():
        cv, tb = Guarded(n, 9 + P), Guarded(n, M)
        sd, pd, rd = dev(st), (dev(pv) if P else None), dev(rcase)
        call('risp_srcnn_cvals', _p(sd), _p(pd), _p(cv.t), n, P, hw, _st())
        call('risp_srcnn_case_table', _p(sd), _p(pd), _p(rd), _p(tb.t), n, P, hw, M, _st())
        settle(failed, 'cvals', cv, tb)
        return dict(cvals=cv.t.cpu().numpy(), table=tb.t.cpu().numpy())
    got = twice(failed, 'cvals HW %d' % hw, run)
    want = R.srcnn_cvals(st[:, :, 0], st[:, :, 1], st[:, :, 2], pv, hw)
    failed.exact('cvals [min | mean | max | params]', got['cvals'], want)
    mags = np.abs(want.astype(F64)) @ np.abs(rcase.astype(F64))
    failed.hold('risp_srcnn_case_table', 'HW %d P %d M %d' % (hw, P, M), got['table'], R.srcnn_case_table(want, rcase), S.sum_bound(9 + P, mags))
    failed.finish()


# ---------------------------------------------------------------------------------------------------- histogram
@pytest.mark.parametrize('hw', S.HIST_HW)
@pytest.mark.parametrize('bins', S.HIST_BINS)
def test_histc(bins, hw):
    failed = Checks()
    x = S.hist_input(bins, hw)
    want, forms = R.histc(x, bins), {}
    for off in (0, 1):
        what = 'bins %d HW %d %s (%s)' % (bins, hw, 'moved by one float' if off else 'aligned', S.histc_walk(hw, bins, off))

        def run():
            h, xd = Guarded(2, bins), dev(x, off)
            call('risp_histc', _p(xd), _p(h.t), 2, hw, bins, _st())
            settle(failed, what, h)
            return dict(hist=h.t.cpu().numpy())
        forms[off] = twice(failed, what, run)['hist']
        failed.exact(what + ' counts', forms[off].astype(F64), want)
    failed.exact('across forms', forms[0], forms[1])
    failed.finish()


# ---------------------------------------------------------------------------------------------------- mixture
def mix_call(failed, outs, w, gy, go_mode, what):
    from reconfigisp_amd import lib as L
    K, numel = len(outs), gy.size
    od, gd = [dev(o) for o in outs], dev(gy)
    y, gw, scratch = Guarded(numel), Guarded(K), Guarded(L.load().risp_mix_scratch_floats())
    want = [go_mode == 'all' or (go_mode == 'alternate' and k % 2 == 0) for k in range(K)]
    go = [Guarded(numel) if want[k] else None for k in range(K)]
    ptrs, cw = L.ptr_array([o.data_ptr() for o in od]), (C.c_float * K)(*[float(v) for v in w])
    call('risp_mix_fwd', ptrs, cw, K, _p(y.t), numel, _st())
    call('risp_mix_bwd', ptrs, cw, K, _p(gd), L.ptr_array([g.t.data_ptr() if g else None for g in go]), _p(gw.t), _p(scratch.t), numel, _st())
    settle(failed, what, y, gw, scratch, *go)
    return dict(y=y.t.cpu().numpy(), gw=gw.t.cpu().numpy(), go=[g.t.cpu().numpy() if g else None for g in go])


@pytest.mark.parametrize('K,numel', S.mix_cases())
def test_mix(K, numel):
    failed, w_ = Checks(), S.mix_walk(numel, K)
    for integer in (False, True):
        outs, w, gy = S.mix_input(K, numel, integer)
        ref = R.mix(outs, w, gy)
        modes = S.MIX_GO if numel <= S.MIX_NUMEL[-1] else ['alternate']
        for mode in modes if not integer else modes[-1:]:
            what = 'K %d numel %d go %s %s (%s)' % (K, numel, mode, 'integers' if integer else 'reals', w_)
            got = twice(failed, what, lambda: mix_call(failed, outs, w, gy, mode, what))
            for k, g in enumerate(got['go']):
                if g is not None:
                    failed.exact(what + ' go %d = fp32(w gy)' % k, g, gy * w[k])
            if integer:
                failed.exact(what + ' y', got['y'].astype(F64), ref['y'])
                failed.exact(what + ' gw', got['gw'].astype(F64), ref['gw'])
            else:
                mags = sum(np.abs(o.astype(F64) * F64(w[k])) for k, o in enumerate(outs))
                failed.hold('risp_mix_fwd: y', what, got['y'], ref['y'], S.sum_bound(w_['y_depth'], mags))
                gmag = np.array([np.abs(gy.astype(F64) * o).sum() for o in outs])
                failed.hold('risp_mix_bwd: gw', what, got['gw'], ref['gw'], S.sum_bound(w_['gw_depth'], gmag))
    failed.finish()


# ---------------------------------------------------------------------------------------------------- plane sums
@pytest.mark.parametrize('n', S.PLANE_N)
@pytest.mark.parametrize('hw', S.PLANE_HW)
def test_plane_sums(hw, n):
    failed = Checks()
    for integer in (False, True):
        x = S.plane_input(hw, n, integer)
        for c0, nc in S.PLANE_SEL:
            ref = R.plane_sums(x, c0, nc)
            mags = np.abs(x.astype(F64))[:, c0: c0 + nc].sum(2)
            for off in (0, 1):
                what = 'HW %d N %d planes %d..%d %s %s' % (hw, n, c0, c0 + nc - 1, 'integers' if integer else 'reals', 'moved by one float' if off else 'aligned')

                def run():
                    out, xd = Guarded(n, nc), dev(x, off)
                    call('risp_plane_sums', _p(xd), _p(out.t), n, S.PLANE_C, c0, nc, hw, _st())
                    settle(failed, what, out)
                    return dict(sums=out.t.cpu().numpy())
                got = twice(failed, what, run)['sums']
                if integer:
                    failed.exact(what, got.astype(F64), ref)
                else:
                    failed.hold('risp_plane_sums', what, got, ref, S.sum_bound(S.plane_walk(hw, off)['depth'], mags))
    failed.finish()


# ---------------------------------------------------------------------------------------------------- squared error
def sse_call(failed, a, b, off, what):
    from reconfigisp_amd import lib as L
    n = L.load().risp_sse_uint8_doubles()
    assert n == 1 + 1024
    g, ad, bd = Guarded(2 * n), dev(a, off), dev(b, off)          # the operands stay alive until the call has run
    call('risp_sse_uint8', _p(ad), _p(bd), _p(g.t), n, a.size, _st())
    settle(failed, what, g)
    return dict(sse=g.t.view(torch.float64).cpu().numpy())


@pytest.mark.parametrize('numel', S.SSE_NUMEL)
def test_sse_uint8(numel):
    import reconfigisp_amd.codes.utils.util as util
    failed, w = Checks(), S.sse_walk(numel)
    for integer in (False, True):
        a, b = S.sse_input(numel, integer)
        ref, forms = R.sse_uint8(a, b), {}
        for off in (0, 1):
            what = 'numel %d %s %s (%s)' % (numel, 'codes 0 / 255' if integer else 'reals', 'moved by one float' if off else 'aligned', w)
            forms[off] = twice(failed, what, lambda: sse_call(failed, a, b, off, what))['sse']
            got = forms[off]
            if integer:
                failed.exact(what + ' the count of differing codes', got[0], ref)
            else:
                failed.hold('risp_sse_uint8', what, got[0], ref, S.sse_bound(a, b))
            fill = np.full(2, np.nan, F32).view(np.uint64)[0]              # an unwritten double: two of the buffer's NaN floats
            if not (got[1 + w['grid']:].view(np.uint64) == fill).all() or (got[: 1 + w['grid']].view(np.uint64) == fill).any():
                failed.append(what + ': the partial slots written are not 1 .. %d' % w['grid'])
        failed.exact('across forms (element loads in both)', forms[0][0], forms[1][0])
        psnr = util.psnr_tensors(dev(a).view(1, 1, 1, -1), dev(b).view(1, 1, 1, -1))
        failed.exact('util.psnr_tensors', psnr, R.psnr_from_sse(float(forms[0][0]), numel))
    failed.finish()


# ---------------------------------------------------------------------------------------------------- conditional head
def fc_call(failed, hist, flat, gout, widths, what):
    from reconfigisp_amd import lib as L
    N, nl = len(hist), len(widths) - 1
    cw = (C.c_int * len(widths))(*widths)
    row = L.load().risp_cond_fc_row_floats(cw, nl)
    assert row == sum(widths)
    acts, out, deltas, dflat = Guarded(N, row), Guarded(N, widths[-1]), Guarded(N, row), Guarded(flat.size)
    hd, fd, gd = dev(hist), dev(flat), dev(gout)
    call('risp_cond_fc_fwd', _p(hd), _p(fd), cw, nl, _p(acts.t), _p(out.t), N, _st())
    call('risp_cond_fc_bwd', _p(fd), cw, nl, _p(acts.t), _p(out.t), _p(gd), _p(deltas.t), _p(dflat.t), flat.size, N, _st())
    settle(failed, what, acts, out, deltas, dflat)
    return dict(acts=acts.t.cpu().numpy(), out=out.t.cpu().numpy(), dflat=dflat.t.cpu().numpy())


@pytest.mark.parametrize('N', S.FC_N)
@pytest.mark.parametrize('index', range(len(S.FC_WIDTHS)), ids=lambda i: '-'.join(map(str, S.FC_WIDTHS[i][0])) + '+%d' % S.FC_WIDTHS[i][1])
def test_cond_fc(index, N):
    (widths, extra), failed = S.FC_WIDTHS[index], Checks()
    hist, flat, gout = S.fc_input(widths, extra, N)
    what = 'widths %s N %d (%s)' % (widths, N, S.FC_BRANCH[index])
    got = twice(failed, what, lambda: fc_call(failed, hist, flat, gout, widths, what))
    o32, a32, d32 = R.cond_fc(hist, flat, widths, gout, dtype=F32)
    o64, a64, d64 = R.cond_fc(hist, flat, widths, gout)
    offs, gofs = R.fc_layout(widths)
    failed.exact('the histogram row of acts', got['acts'][:, : widths[0]], hist)
    failed.exact('the zero tail of the gradient', got['dflat'][gofs + 1:], np.zeros(extra, F32))
    for l in range(1, len(widths) - 1):                        # no ReLU decided the other way (the gate margin is asserted on the CPU)
        at = sum(widths[:l])
        failed.exact('the ReLU pattern of layer %d' % l, got['acts'][:, at: at + widths[l]] > 0, a64[l] > 0)
    budget = ErrorBudget()
    budget(got['out'], o32, o64, what + ' out', family='out')
    for l, (wo, bo) in enumerate(offs):
        budget(got['dflat'][wo: bo], d32[wo: bo], d64[wo: bo], what + ' dW%d' % l, family='dflat')
        budget(got['dflat'][bo: bo + widths[l + 1]], d32[bo: bo + widths[l + 1]], d64[bo: bo + widths[l + 1]], what + ' db%d' % l, family='dflat')
    budget(got['dflat'][gofs: gofs + 1], d32[gofs: gofs + 1], d64[gofs: gofs + 1], what + ' d global', family='dflat')
    for name, e_got, e_ref, _, _ in budget.rows:
        b = BUDGET.setdefault('risp_cond_fc: ' + ('out' if name.endswith('out') else 'dflat') + ' (ErrorBudget)', [0, 0.0, 0.0, 0.0])
        bound = min(2 * e_ref, 1e-4) + 4e-6
        b[0] += 1
        if e_got / bound > b[3]:
            b[1], b[2], b[3] = e_got, bound, e_got / bound
    budget.finish()
    failed.finish()


# ---------------------------------------------------------------------------------------------------- pixel loss
@pytest.mark.parametrize('with_g', [True, False], ids=['gradient', 'no-gradient'])
@pytest.mark.parametrize('kind', [0, 1], ids=['l2', 'l1'])
@pytest.mark.parametrize('numel', S.LOSS_NUMEL)
def test_pixel_loss(numel, kind, with_g):
    from reconfigisp_amd import lib as L
    failed, w = Checks(), S.loss_walk(numel)
    ns = L.load().risp_loss_scratch_floats()
    assert ns >= w['blocks']
    for integer in (False, True):
        y, gt = S.loss_input(numel, integer)
        what = 'numel %d kind %d %s %s (%s)' % (numel, kind, 'integers' if integer else 'reals', 'g' if with_g else 'g NULL', w)

        def run():
            g, loss, scratch, yd, td = (Guarded(numel) if with_g else None), Guarded(1), Guarded(ns), dev(y), dev(gt)
            call('risp_pixel_loss', _p(yd), _p(td), _p(g.t) if g else None, _p(loss.t), _p(scratch.t), numel, kind, _st())
            settle(failed, what, g, loss, scratch)
            return dict(loss=loss.t.cpu().numpy(), g=g.t.cpu().numpy() if g else None)
        got = twice(failed, what, run)
        ref, gref = R.pixel_loss(y, gt, kind)
        if integer:
            total = (np.abs(y.astype(F64) - gt) ** (2 - kind)).sum()
            failed.exact(what + ' loss = fp32(integer sum) x fp32(1 / numel)', got['loss'][0], F32(total) * (F32(1) / F32(numel)))
        else:
            failed.hold('risp_pixel_loss: loss', what, got['loss'][0], ref, S.sum_bound(w['depth'], ref))
        if with_g:
            # the difference, the rounded 2 / numel (or 1 / numel) and the product: 3 roundings of the value itself
            failed.hold('risp_pixel_loss: gradient', what, got['g'], gref, S.MARGIN * 3 * S.U * np.abs(gref))
            failed.exact(what + ' zero gradient where y == gt', got['g'][y == gt], np.zeros(int((y == gt).sum()), F32))
    failed.finish()


# ---------------------------------------------------------------------------------------------------- local / global loss
def lg_call(failed, a, b, flag, what, with_g=True):
    from reconfigisp_amd import lib as L
    N, Cc, H, W = a.shape
    ns = L.load().risp_local_global_scratch_floats(N, Cc)
    assert ns == N * Cc * 66
    g, loss, scratch = (Guarded(N, Cc, H, W) if with_g else None), Guarded(1), Guarded(ns)        # g full of NaN
    ad, bd, fd = dev(a), dev(b), dev(flag)
    call('risp_local_global_l2', _p(ad), _p(bd), _p(fd), _p(g.t) if g else None, _p(loss.t), _p(scratch.t), N, Cc, H, W, _st())
    settle(failed, what, g, loss, scratch)
    return dict(loss=loss.t.cpu().numpy(), g=g.t.cpu().numpy() if g else None, scratch=scratch.t.cpu().numpy())


@pytest.mark.parametrize('flags', S.LG_FLAGS)
@pytest.mark.parametrize('shape', S.LG_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_local_global_l2(shape, flags):
    failed, w = Checks(), S.lg_walk(*shape)
    N, Cc, H, W = shape
    flag = S.lg_flags(flags, N, S.LG_ROTATE[S.LG_SHAPES.index(shape)])        # 'values': 0, 0.5, 1, 2 dealt over the shapes
    a, b = S.lg_input(shape)
    what = '%s flags %s (%s)' % (shape, flag.tolist(), w)
    got = twice(failed, what, lambda: lg_call(failed, a, b, flag, what))
    ref, gref = R.local_global_l2(a, b, flag)
    lb, gb = S.lg_bounds(a, b, flag)
    failed.hold('risp_local_global_l2: loss', what, got['loss'][0], ref, lb)
    failed.hold('risp_local_global_l2: gradient', what, got['g'], gref, gb)
    glob = ~(flag < 1)
    if glob.any():
        z = np.ones((H, W), bool)
        z[1::4, 1::4] = z[1::4, 2::4] = z[2::4, 1::4] = z[2::4, 2::4] = False
        failed.exact(what + ' the 12 zero positions of every cell', got['g'][glob][:, :, z], np.zeros((int(glob.sum()), Cc, int(z.sum())), F32))
    none = lg_call(failed, a, b, flag, what + ' g NULL', with_g=False)
    failed.exact(what + ' the loss without a gradient buffer', none['loss'], got['loss'])
    failed.finish()


@pytest.mark.parametrize('shape', S.LG_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_local_global_l2_equal_planes(shape):
    """a = b: the gain is mean / (mean + 1e-6), just below 1 and inside the clamp, and every difference a gain - b is a
    cancellation down to about 1e-6 of the values - held to the bound of reduce_space_cases.lg_bounds, not to zero"""
    failed, w = Checks(), S.lg_walk(*shape)
    a, b = S.lg_input(shape, 'equal')
    flag = S.lg_flags('local', shape[0])
    what = '%s a = b (%s)' % (shape, w)
    got = twice(failed, what, lambda: lg_call(failed, a, b, flag, what))
    ref, gref = R.local_global_l2(a, b, flag)
    lb, gb = S.lg_bounds(a, b, flag)
    failed.hold('risp_local_global_l2: loss, a = b', what, got['loss'][0], ref, lb)
    failed.hold('risp_local_global_l2: gradient, a = b', what, got['g'], gref, gb)
    failed.exact(what + ' zero gradient where a = b = 0', got['g'][a == 0], np.zeros(int((a == 0).sum()), F32))
    failed.finish()


@pytest.mark.parametrize('kind', ['half', 'two', 'centres'])
@pytest.mark.parametrize('shape', S.LG_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_local_global_l2_integer_coverage(shape, kind):
    failed, w = Checks(), S.lg_walk(*shape)
    N, Cc, H, W = shape
    a, b = S.lg_input(shape, kind)
    flag = S.lg_flags('global' if kind == 'centres' else 'local', N)
    what = '%s %s (%s)' % (shape, kind, w)
    got = twice(failed, what, lambda: lg_call(failed, a, b, flag, what))
    if kind == 'centres':
        d = R.lg_centres(a) - R.lg_centres(b)
        den = F32(N) * F32(Cc) * (F32(H) * F32(W) / F32(16))
    else:
        d = a.astype(F64) * (0.5 if kind == 'half' else 2.0) - b
        den = F32(N) * F32(Cc) * (F32(H) * F32(W))
    per_plane = (d * d).sum((2, 3)).reshape(-1)
    failed.exact(what + ' loss = fp32(integer sum) / fp32(count)', got['loss'][0], F32(per_plane.sum()) / den + F32(0))
    nc = N * Cc
    failed.exact(what + ' plane sums of a and b', got['scratch'][: 2 * nc].astype(F64), np.concatenate([a.astype(F64).sum((2, 3)).reshape(-1), b.astype(F64).sum((2, 3)).reshape(-1)]))
    slots = got['scratch'][2 * nc: 2 * nc + nc * w['bx']].astype(F64).reshape(nc, w['bx'])
    failed.exact(what + ' the partial slots plane x bx + block add up to each plane', slots.sum(1), per_plane)
    if not np.isnan(got['scratch'][2 * nc + nc * w['bx']:]).all():
        failed.append(what + ': partial slots beyond N x C x bx were written')
    failed.finish()


# ---------------------------------------------------------------------------------------------------- refusals
def _refused(entry, ov):
    """a valid small call of ``entry`` with the named arguments replaced -> (the call, its guarded outputs)"""
    from reconfigisp_amd import lib as L
    lib, st = L.load(), _st()
    ones = lambda *s: torch.full(s, 0.5, device='cuda')
    mv = lambda t, k: off16(t, ov.get(k, 0)) if ov.get(k) else t
    if entry == 'channel_stats':
        NC = ov.get('NC', 2)
        outs = [Guarded(NC, 4), Guarded(NC, 2), Guarded(NC * 5)]
        x = ones(NC, 4)
        return (lambda: call('risp_channel_stats', _p(x), _p(outs[0].t), _p(outs[1].t), _p(outs[2].t), NC, 4, st)), outs
    if entry == 'histc':
        NC, bins = ov.get('NC', 2), ov.get('bins', 8)
        outs, x = [Guarded(min(NC, 4), max(bins, 1))], ones(NC, 4)
        return (lambda: call('risp_histc', _p(x), _p(outs[0].t), NC, 4, bins, st)), outs
    if entry in ('mix_fwd', 'mix_bwd'):                        # one entry point a row: nothing launched, nothing written
        K, numel = ov.get('K', 2), ov.get('numel', 8)
        o = [ones(8) for _ in range(16)]
        o[1] = mv(o[1], 'off_o')
        ptrs, cw = (C.c_void_p * 17)(*[t.data_ptr() for t in o], o[0].data_ptr()), (C.c_float * 17)(*([0.5] * 17))
        if entry == 'mix_fwd':
            y = Guarded(8, off=ov.get('off_y', 0))
            return (lambda: call('risp_mix_fwd', ptrs, cw, K, _p(y.t), numel, st)), [y]
        gy = mv(ones(8), 'off_gy')
        gw, sc, go = Guarded(16), Guarded(lib.risp_mix_scratch_floats()), [Guarded(8, off=ov.get('off_go', 0)), Guarded(8)]
        gop = (C.c_void_p * 17)(go[0].t.data_ptr(), go[1].t.data_ptr(), *([None] * 15))
        return (lambda: call('risp_mix_bwd', ptrs, cw, K, _p(gy), gop, _p(gw.t), _p(sc.t), numel, st)), [gw, sc] + go
    if entry == 'pixel_loss':
        numel = ov.get('numel', 8)
        y, gt = mv(ones(8), 'off_y'), ones(8)
        outs = [Guarded(8, off=ov.get('off_g', 0)), Guarded(1), Guarded(lib.risp_loss_scratch_floats())]
        return (lambda: call('risp_pixel_loss', _p(y), _p(gt), _p(outs[0].t), _p(outs[1].t), _p(outs[2].t), numel, 0, st)), outs
    if entry == 'local_global':
        N, Cc, H, W = ov.get('N', 1), ov.get('C', 2), ov.get('H', 4), ov.get('W', 8)
        a, b, flag = mv(ones(N, Cc, 8, 8), 'off_a'), ones(N, Cc, 8, 8), torch.zeros(N, device='cuda')
        outs = [Guarded(min(N, 2), min(Cc, 2), 8, 8, off=ov.get('off_g', 0)), Guarded(1), Guarded(min(N * Cc, 4) * 66)]
        return (lambda: call('risp_local_global_l2', _p(a), _p(b), _p(flag), _p(outs[0].t), _p(outs[1].t), _p(outs[2].t), N, Cc, H, W, st)), outs
    if entry in ('cond_fc', 'cond_fc_bwd'):
        widths = ov.get('widths', (3, 2, 1))
        cw, nl = (C.c_int * len(widths))(*widths), len(widths) - 1
        hist, flat, gout = ones(2, 3), ones(4096), ones(2, 1)
        acts, out, deltas, dflat = Guarded(2, 64), Guarded(2, 8), Guarded(2, 64), Guarded(4096)

        def both():
            errs = []
            for fn in ([lambda: call('risp_cond_fc_fwd', _p(hist), _p(flat), cw, nl, _p(acts.t), _p(out.t), 2, st)] if entry == 'cond_fc' else []) + [
                    lambda: call('risp_cond_fc_bwd', _p(flat), cw, nl, _p(acts.t), _p(out.t), _p(gout), _p(deltas.t), _p(dflat.t), ov.get('total', 4096), 2, st)]:
                try:
                    fn()
                except RuntimeError as e:
                    errs.append(str(e))
            assert len(errs) == (2 if entry == 'cond_fc' else 1)
            raise RuntimeError(' | '.join(errs))
        return both, [acts, out, deltas, dflat]
    if entry == 'sse':
        outs, a = [Guarded(2 * 1025)], ones(8)
        return (lambda: call('risp_sse_uint8', _p(a), _p(a), _p(outs[0].t), ov['doubles'], 8, st)), outs
    if entry == 'plane_sums':
        outs, x = [Guarded(2, 3)], ones(2, 3, 4)
        return (lambda: call('risp_plane_sums', _p(x), _p(outs[0].t), 2, 3, ov['c0'], ov['nc'], 4, st)), outs
    outs, g, arg = [Guarded(2, 3, 4)], ones(6), torch.zeros(6, 2, dtype=torch.int32, device='cuda')
    if entry == 'stats_bwd_rows':
        return (lambda: call('risp_stats_bwd_rows', _p(outs[0].t), _p(g), _p(g), _p(g), _p(arg), 2, 3, 4, ov['row_stride'], st)), outs
    return (lambda: call('risp_stats_bwd', _p(outs[0].t), _p(g), None, _p(g), None, 6, 4, st)), outs


@pytest.mark.parametrize('row', range(len(S.REFUSED)), ids=lambda i: '%s-%s' % (S.REFUSED[i][0], '_'.join('%s=%s' % (k, v if not isinstance(v, tuple) else 'x'.join(
    map(str, v[:4]))) for k, v in S.REFUSED[i][1].items())))
def test_refused_arguments_raise_before_any_launch(row):
    entry, ov, needle = S.REFUSED[row]
    fn, outs = _refused(entry, ov)
    with pytest.raises(RuntimeError, match=needle):
        fn()
    torch.cuda.synchronize()
    assert all(g.untouched() for g in outs), 'the refused call wrote an output'


# ---------------------------------------------------------------------------------------------------- the wrappers
def test_wrappers_give_the_bits_of_the_direct_call():
    import reconfigisp_amd.functional as F
    failed = Checks()
    for hw, n, c in [(5, 2, 3), (4096, 1, 5), (129 * 129, 2, 3)]:
        x = S.stats_input(hw, n, c, False)
        for off in (0, 1):
            direct = stats_call(failed, x, off, 'stats')
            stats, arg = F.channel_stats(dev(x.reshape(n, c, 1, hw), off))
            failed.exact('channel_stats', stats.cpu().numpy().reshape(-1, 4), direct['stats'])
            failed.exact('channel_stats arg', arg.cpu().numpy().reshape(-1, 2), direct['arg'])
    for bins, hw in [(30, 4100), (256, 5), (4096, 4096)]:
        x = S.hist_input(bins, hw)
        failed.exact('hist_features', F.hist_features(dev(x.reshape(1, 2, 1, hw)), bins).cpu().numpy().reshape(2, bins).astype(F64), R.histc(x, bins))
    # conditional_fc = the histogram, then the head: the bits of the two direct calls
    bins, hw = 4, 64
    widths = (12, 8, 1)
    img = S.rng(23).uniform(-0.1, 1.1, size=(3, 3, 8, 8)).astype(F32)
    _, flat, gout = S.fc_input(widths, 0, 3)
    hist = R.histc(img.reshape(9, hw), bins).reshape(3, 12).astype(F32)
    direct = fc_call(failed, hist, flat, gout, widths, 'cond_fc')
    tf = dev(flat).requires_grad_()
    out = F.conditional_fc(dev(img), tf, widths)
    out.backward(dev(gout))
    failed.exact('conditional_fc', out.detach().cpu().numpy(), direct['out'])
    failed.exact('conditional_fc gradient', tf.grad.cpu().numpy(), direct['dflat'])
    # grayworld: statistics, gains, the gain applied
    x = S.rng(24).uniform(0.01, 1, size=(2, 3, 8, 12)).astype(F32)
    st = stats_call(failed, x.reshape(6, 96), 0, 'stats')['stats']
    gains, y = Guarded(2, 3), Guarded(2, 3, 8, 12)
    sd, xd = dev(st), dev(x)
    call('risp_grayworld_gains_fwd', _p(sd), _p(gains.t), 2, 96, _st())
    call('risp_gain3_fwd', _p(xd), _p(gains.t), _p(y.t), 2, 96, _st())
    settle(failed, 'grayworld', gains, y)
    failed.exact('grayworld', F.grayworld(dev(x)).cpu().numpy(), y.t.cpu().numpy())
    failed.exact('grayworld_gains', F.grayworld_gains(dev(x)).cpu().numpy(), gains.t.cpu().numpy())
    # mix, forward and backward, and a view off a 16-byte boundary (copied by the wrapper, refused by the C ABI)
    for K, numel, off in [(2, 1020, 0), (5, 262148, 0), (16, 4, 0), (3, 1020, 1)]:
        outs, w, gy = S.mix_input(K, numel, False)
        direct = mix_call(failed, outs, w, gy, 'all', 'mix')
        to = [dev(o, off if k == 1 else 0).requires_grad_() for k, o in enumerate(outs)]
        tw = dev(w).requires_grad_()
        y = F.mix(tw, to)
        y.backward(dev(gy, off))
        failed.exact('mix y', y.detach().cpu().numpy(), direct['y'])
        failed.exact('mix gw', tw.grad.cpu().numpy(), direct['gw'])
        for k in range(K):
            failed.exact('mix go %d' % k, to[k].grad.cpu().numpy(), direct['go'][k])
    for numel, kind in [(1020, 'l2'), (262148, 'l1')]:
        y, gt = S.loss_input(numel, False)
        ty = dev(y).requires_grad_()
        loss = F.pixel_loss(ty, dev(gt), kind)
        loss.backward()
        g, l, sc, yd, td = Guarded(numel), Guarded(1), Guarded(256), dev(y), dev(gt)
        call('risp_pixel_loss', _p(yd), _p(td), _p(g.t), _p(l.t), _p(sc.t), numel, {'l2': 0, 'l1': 1}[kind], _st())
        settle(failed, 'pixel_loss', g, l, sc)
        failed.exact('pixel_loss', loss.detach().cpu().numpy().reshape(1), l.t.cpu().numpy())
        failed.exact('pixel_loss gradient', ty.grad.cpu().numpy(), g.t.cpu().numpy())
    for shape, flags in [((2, 3, 8, 12), 'mixed'), ((3, 2, 128, 128), 'values'), ((2, 3, 128, 132), 'values')]:
        a, b = S.lg_input(shape)
        flag = S.lg_flags(flags, shape[0], S.LG_ROTATE[S.LG_SHAPES.index(shape)])
        direct = lg_call(failed, a, b, flag, 'local_global')
        ta = dev(a).requires_grad_()
        loss = F.local_global_l2(ta, dev(b), dev(flag))
        loss.backward()
        failed.exact('local_global_l2', loss.detach().cpu().numpy().reshape(1), direct['loss'])
        failed.exact('local_global_l2 gradient', ta.grad.cpu().numpy(), direct['g'])
    failed.finish()
