"""No GPU: the float64 restatement of the per-image reductions (tests/reduce_reference.py) against independent
implementations (torch.histc, torch.min / max with the first index built by comparison, torch's losses in float64,
the oracle's gray-world, conditional head and PSNR, the committed goldens), and the case table of
tests/reduce_space_cases.py: every case reaches the branch it names, the gate margins hold, the integer inputs stay exact."""
import numpy as np
import pytest
import torch

import isp_oracle as O
import reduce_reference as R
import reduce_space_cases as S

F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------ the restatement
def _first(flat, m):
    return (flat == m.unsqueeze(-1)).int().argmax(dim=1)


@pytest.mark.parametrize('hw', [1, 5, 4096, 129 * 129])
def test_statistics_against_torch_with_first_indices(hw):
    x = S.stats_input(hw, 2, 3, True if hw == 4096 else False)               # the integer planes are full of ties
    r, t = R.channel_stats(x), torch.from_numpy(x).double()
    assert np.array_equal(r['mn'], t.min(1).values.numpy()) and np.array_equal(r['mx'], t.max(1).values.numpy())
    assert np.array_equal(r['imn'], _first(t, t.min(1).values).numpy()) and np.array_equal(r['imx'], _first(t, t.max(1).values).numpy())
    assert np.allclose(r['sum'], t.sum(1).numpy(), rtol=1e-13)


def test_statistics_ties_name_the_first_index():
    for hw in S.TIE_HW:
        for kind in S.TIE_KINDS:
            for off in (0, 1):
                made = S.tie_input(hw, kind, off)
                if made is None:
                    continue
                x, want = made
                r = R.channel_stats(x)
                assert np.array_equal(np.stack([r['imn'], r['imx']], 1), want), (hw, kind, off)


def test_statistics_gradient_against_autograd_without_ties_and_by_hand_with_them():
    x, gx, grads = S.stats_bwd_input(S.STATS_BWD[2], False)
    hw, n, c, gs = S.STATS_BWD[2][:4]
    r = R.channel_stats(x)
    arg = np.stack([r['imn'], r['imx']], 1)
    got = R.stats_bwd(gx, grads['min'], grads['mean'], grads['max'], arg, c, gs)
    t = torch.from_numpy(x).double().requires_grad_()
    pick = lambda v: torch.from_numpy(v.astype(F64)).view(n, gs)[:, :c].reshape(-1)
    (t.min(1).values * pick(grads['min']) + t.mean(1) * pick(grads['mean']) + t.max(1).values * pick(grads['max'])).sum().backward()
    assert np.allclose(got, gx.astype(F64) + t.grad.numpy(), rtol=1e-13, atol=1e-15)
    # a constant plane: everything on index 0, nothing split
    got = R.stats_bwd(np.zeros((1, 8)), [3.0], [8.0], [5.0], np.zeros((1, 2), np.int64))
    assert np.array_equal(got, np.array([[9.0, 1, 1, 1, 1, 1, 1, 1]]))
    # the fp32 form is the float64 one rounded where the arithmetic is exact
    assert np.array_equal(R.stats_bwd(np.zeros((1, 8), F32), [3.0], [8.0], [5.0], np.zeros((1, 2), np.int64), dtype=F32), got.astype(F32))


def test_grayworld_gains_and_gradient_against_the_oracle():
    g = S.rng(1)
    x = torch.from_numpy(g.uniform(0.01, 1, size=(3, 3, 8, 8))).double()
    x[1, 0] = 0.0                                              # a black plane: the clamp gate
    x[2, 1] = -x[2, 1]                                         # a negative mean
    sums = x.sum((2, 3)).numpy()
    gains = R.grayworld_gains(sums, 64)
    assert np.allclose(np.clip(x.numpy() * gains[:, :, None, None], 0, 1), O.grayworld(x).numpy(), rtol=1e-12, atol=1e-15)
    m = (x.sum((2, 3)) / 64).requires_grad_()
    gk = torch.from_numpy(g.uniform(-1, 1, size=(3, 3)))
    ((m.mean(1, keepdim=True) / m.clamp_min(O.GRAY_EPS)) * gk).sum().backward()
    assert np.allclose(R.grayworld_gains_bwd(sums, gk.numpy(), 64), m.grad.numpy(), rtol=1e-12, atol=1e-12)


def test_grayworld_on_the_pointwise_fixture_input_against_the_oracle(golden):
    x = golden('pointwise')['x']
    gains = R.grayworld_gains(x.astype(F64).sum((2, 3)), x.shape[2] * x.shape[3])
    want = O.grayworld(torch.from_numpy(x).double()).numpy()
    assert np.allclose(np.clip(x * gains[:, :, None, None], 0, 1), want, rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize('bins', S.HIST_BINS)
def test_histogram_against_torch_histc(bins):
    for hw in (5, 4100):
        x = S.hist_input(bins, hw)
        want = np.stack([torch.histc(torch.from_numpy(p), bins=bins, min=0, max=1).numpy() for p in x])
        assert np.array_equal(R.histc(x, bins), want), 'bins %d hw %d' % (bins, hw)
        assert R.histc(x, bins)[1].max() == hw                 # the constant plane: one bin


def test_mixture_and_plane_sums():
    outs, w, gy = S.mix_input(5, 1020, False)
    r = R.mix(outs, w, gy)
    o, tw, tg = torch.tensor(np.stack(outs)).double().requires_grad_(), torch.tensor(w).double().requires_grad_(), torch.tensor(gy).double()
    y = (o * tw[:, None]).sum(0)
    y.backward(tg)
    assert np.allclose(r['y'], y.detach().numpy(), atol=1e-15) and np.allclose(r['gw'], tw.grad.numpy(), rtol=1e-12)
    assert np.allclose(np.stack(r['go']), o.grad.numpy(), atol=1e-15)
    x = S.plane_input(1023, 3, False)
    assert np.allclose(R.plane_sums(x, 2, 3), torch.from_numpy(x).double()[:, 2:5].sum(2).numpy(), rtol=1e-13)


def test_squared_error_against_the_oracle_psnr():
    a, b = S.sse_input(4097, False)
    ca, cb = R.u8_code(a), R.u8_code(b)
    assert ca.min() == 0 and ca.max() == 255
    # numpy's own truncation of the fp32 product (tensor2bgr): the same codes
    with np.errstate(invalid='ignore'):
        assert np.array_equal(ca, np.clip(a * F32(255), 0, 255).astype(np.uint8))
    want = O.psnr_uint8(ca.astype(np.uint8), cb.astype(np.uint8))
    assert abs(R.psnr_from_sse(R.sse_uint8(a, b), a.size) - want) < 1e-4 * want       # the oracle squares and averages in fp32
    k = (np.arange(256) / 255).astype(F32)
    assert np.array_equal(R.u8_code(np.array([-1.0, 2.0, 1.0, 0.0], F32)), [0, 255, 255, 0]) and np.abs(R.u8_code(k) - np.arange(256)).max() <= 1


def test_conditional_head_against_the_oracle_and_the_golden(golden):
    z = golden('conditional')
    x = torch.from_numpy(z['x'])
    for name in ('gamma', 'wbm', 'wbq'):
        flat, inch, want = z[name + '_flat'], [int(v) for v in z[name + '_inch']], z[name + '_fc']
        widths = tuple(inch) + (want.shape[1],)
        hist = R.histc(z['x'].reshape(-1, 256), widths[0] // 3).reshape(x.shape[0], -1)
        out, _ = R.cond_fc(hist, flat, widths)
        assert np.allclose(out, want, rtol=2e-5, atol=1e-6), name                      # the golden is fp32
        ref = O.conditional_fc(x.double(), torch.from_numpy(flat).double(), inch, want.shape[1]).numpy()
        assert np.allclose(out, ref, rtol=1e-12, atol=1e-14), name
    widths, extra = S.FC_WIDTHS[1]
    hist, flat, gout = S.fc_input(widths, 7, 3)
    out, _, dflat = R.cond_fc(hist, flat, widths, gout)
    tf = torch.from_numpy(flat).double().requires_grad_()
    offs, gofs = R.fc_layout(widths)
    a = torch.from_numpy(hist).double()
    for l, (wo, bo) in enumerate(offs):
        a = a @ tf[wo: bo].view(widths[l], widths[l + 1]) + tf[bo: bo + widths[l + 1]]
        a = torch.relu(a) if l < len(offs) - 1 else a
    torch.sigmoid(a + tf[gofs]).backward(torch.from_numpy(gout).double())
    assert np.allclose(dflat, tf.grad.numpy(), rtol=1e-11, atol=1e-15) and not dflat[gofs + 1:].any() and dflat[gofs] != 0


@pytest.mark.parametrize('kind', [0, 1])
def test_pixel_loss_against_torch(kind):
    y, gt = S.loss_input(1020, False)
    ty, tg = torch.from_numpy(y).double().requires_grad_(), torch.from_numpy(gt).double()
    loss = (torch.nn.functional.mse_loss if kind == 0 else torch.nn.functional.l1_loss)(ty, tg)
    loss.backward()
    got, g = R.pixel_loss(y, gt, kind)
    assert abs(got - loss.item()) <= 1e-14 and np.allclose(g, ty.grad.numpy(), atol=1e-18)
    assert (g[::3] == 0).all()                                 # sign(0) = 0


def test_local_global_loss_against_the_golden(golden):
    z = golden('losses')
    for name in ('mixed', 'local', 'global'):
        loss, g = R.local_global_l2(z['lg_in'], z['lg_gt'], z['lg_%s_flags' % name])
        assert abs(loss - z['lg_%s_loss' % name]) <= 2e-6 * abs(loss), name
        assert np.abs(g - z['lg_%s_grad' % name]).max() <= 2e-6 * np.abs(g).max(), name
    loss, g = R.local_global_l2(z['lg_clamp_in'], z['lg_gt'][:2], np.zeros(2, F32))      # the gain clamp
    assert abs(loss - z['lg_clamp_loss']) <= 2e-6 * abs(loss) and np.abs(g - z['lg_clamp_grad']).max() <= 2e-6 * np.abs(g).max()


def test_local_global_loss_against_torch_interpolate():
    a, b = S.lg_input((2, 3, 8, 12))
    ta, tb = torch.from_numpy(a).double().requires_grad_(), torch.from_numpy(b).double()
    down = lambda t: torch.nn.functional.interpolate(t, scale_factor=0.25, mode='bilinear', align_corners=False)
    torch.nn.functional.mse_loss(down(ta), down(tb)).backward()
    loss, g = R.local_global_l2(a, b, np.ones(2, F32))
    assert np.allclose(g, ta.grad.numpy(), rtol=1e-12, atol=1e-18)
    assert (g[..., 0::4, :] == 0).all() and (g[..., 3::4, :] == 0).all() and (g[..., :, 0::4] == 0).all() and (g[..., :, 3::4] == 0).all()


# ------------------------------------------------------------------------------------------------ the table
def test_every_statistics_size_reaches_the_branch_it_names():
    w = lambda hw, off=0: S.stats_walk(hw, off)
    assert set(S.STATS_BRANCH) == set(S.STATS_HW)
    for hw in (1, 2, 3, 5, 129 * 129):
        assert not w(hw)['vec']
    for hw in (4, 4092, 4096, 16380, 16384, 524288, 524292):
        assert w(hw)['vec'] and not w(hw, 1)['vec']            # moved by one float: the element route by design
    assert w(4)['n'] == 1 and not w(4)['unrolled']
    assert w(4092)['unrolled'] and w(4092)['n'] % 1024 == 1023 and w(4096)['unrolled'] and w(4096)['n'] == 4 * w(4096)['step']
    assert w(16380)['nb'] == 1 and w(16384)['nb'] == 2 and w(129 * 129)['nb'] == 2 and w(16384, 1)['nb'] == 2
    assert w(524288 - 8192)['nb'] == 63 and w(524288)['nb'] == 64 and w(524288)['capped'] and w(524292)['nb'] == 64
    assert w(524288)['n'] == 8 * w(524288)['step'] and w(524292)['trips'] == w(524288)['trips'] + 1
    assert S.stat_blocks(8191) == 1 and S.stat_blocks(10 ** 7) == 64


def test_every_tie_sits_on_the_boundary_it_names():
    for hw in S.TIE_HW:
        for off in (0, 1):
            w, pos = S.stats_walk(hw, off), S.tie_positions(hw, off)
            e = 4 if w['vec'] else 1
            assert w['nb'] == 2
            unit = lambda p: p // e                            # the load an element belongs to
            p, q = pos["either side of a thread's load"]
            assert unit(p) + 1 == unit(q)
            p, q = pos['either side of a wave (lane 63 / 64)']
            assert unit(p) % 256 == 63 and unit(q) % 256 == 64
            p, q = pos["either side of a workgroup's walk"]
            assert unit(p) // 256 == 0 and unit(q) // 256 == 1 and unit(q) < w['step']
            p, q = pos['either side of a trip']
            assert unit(p) == w['step'] - 1 and unit(q) == w['step']
            if w['vec']:
                p, q = pos['either side of an unrolled trip']
                assert unit(q) == 4 * w['step'] and unit(q) + 3 * w['step'] < w['n']      # the second unrolled trip runs
    assert S.stats_walk(S.TIE_HW[2], 0)['n'] > 2 * 4 * S.stats_walk(S.TIE_HW[2], 0)['step']       # the unrolled trip twice, then a tail


def test_statistics_gradient_cases_reach_their_branches():
    rows = {r[5]: r for r in S.STATS_BWD}
    assert not S.stats_bwd_walk(5, 0)['vec'] and S.stats_bwd_walk(4096, 0)['vec'] and not S.stats_bwd_walk(4096, 1)['vec']
    hw = rows['more than 64 x 256 vectors: the grid-stride trip'][0]
    assert S.stats_bwd_walk(hw, 0) == dict(vec=True, bx=64, trips=2) and S.stats_bwd_walk(hw - 4, 0)['trips'] == 1
    hw = rows['element form past 64 x 256 elements'][0]
    assert S.stats_bwd_walk(hw, 0) == dict(vec=False, bx=64, trips=2)
    assert S.stats_bwd_walk(129 * 129, 0)['trips'] == 2 and rows['gstride > C'][3] > rows['gstride > C'][2]


def test_histogram_cases_reach_their_branches():
    for bins in S.HIST_BINS:
        assert S.histc_walk(4096, bins, 0)['copies'] == S.HIST_COPIES[bins] and bins * S.HIST_COPIES[bins] <= 4096
    assert sorted(set(S.HIST_COPIES.values())) == [1, 4, 8, 16] and S.histc_walk(1, 2048, 0)['copies'] == 2
    assert S.histc_walk(4096, 30, 0)['bx'] == 1 and S.histc_walk(4100, 30, 0)['bx'] == 2
    assert not S.histc_walk(262144, 30, 0)['capped'] and S.histc_walk(262148, 30, 0)['capped'] and S.histc_walk(262148, 30, 0)['trips'] == 5
    assert not S.histc_walk(5, 30, 0)['vec'] and not S.histc_walk(4096, 30, 1)['vec']
    # every edge with both neighbours is in the plane once it is long enough; the specials always
    x = S.hist_input(30, 4096)[0]
    e = (np.arange(31) / 30).astype(F32)
    for v in (e, np.nextafter(e, F32(-1)), np.nextafter(e, F32(2))):
        assert np.isin(v, x).all()
    assert np.isnan(x).any() and np.isinf(x).sum() == 2 and (x < 0).any() and np.signbit(x[x == 0]).any()


def test_mixture_cases_reach_their_branches():
    w = S.mix_walk
    assert w(4, 1)['bwd_grid'] == 1 and w(262144, 2)['bwd_grid'] == 64 and w(262144, 2)['finish_trips'] == 1
    assert w(262148, 2)['bwd_grid'] == 65 and w(262148, 2)['finish_trips'] == 2                 # mix_finish_kernel's loop
    assert not w(2 * 1024 * 1024, 2)['fwd_capped'] and w(S.MIX_LARGE[0], 2)['fwd_capped'] and w(S.MIX_LARGE[0], 2)['fwd_trips'] == 2
    assert not w(4 * 1024 * 1024, 2)['bwd_capped'] and w(S.MIX_LARGE[1], 2)['bwd_capped'] and w(S.MIX_LARGE[1], 2)['bwd_trips'] == 5
    assert max(S.MIX_K) == S.MAX_MIX and all(n % 4 == 0 for _, n in S.mix_cases())
    assert S.mix_input(5, 8, False)[1][2] == 0


def test_plane_sum_and_squared_error_and_loss_cases_reach_their_branches():
    assert not S.plane_walk(3, 0)['vec'] and S.plane_walk(1024, 0) == dict(vec=True, trips=1, depth=13) and S.plane_walk(1028, 0)['trips'] == 2
    assert S.plane_walk(1023, 0)['trips'] == 4 and not S.plane_walk(1024, 1)['vec'] and S.plane_walk(16384, 0)['trips'] == 16
    s = S.sse_walk
    assert s(4096)['grid'] == 1 and s(4097)['grid'] == 2 and s(262144)['grid'] == 64 and s(262145)['finish_trips'] == 2
    assert not s(4 * 1024 * 1024)['capped'] and s(S.SSE_NUMEL[-1])['capped'] and s(S.SSE_NUMEL[-1])['trips'] == 17
    w = S.loss_walk
    assert w(1020)['blocks'] == 1 and w(1024)['blocks'] == 1 and w(1028)['blocks'] == 2 and w(262144)['blocks'] == 256
    assert not w(262144)['capped'] and w(262148)['capped'] and w(262148)['trips'] == 2 and w(262144)['finish_trips'] == 4
    y, gt = S.loss_input(1020, False)
    assert (y[::3] == gt[::3]).all()


def test_conditional_head_cases_reach_their_branches_and_clear_the_relu_gate():
    ws = [w for w, _ in S.FC_WIDTHS]
    assert len(ws) == len(S.FC_BRANCH) and len(ws[0]) == 2 and ws[2][0] == 768 > 256 and ws[2][1] > 256 and 257 in ws[3] and 256 in ws[3]
    assert max(ws[4]) == S.FC_MAXW and len(ws[5]) - 1 == S.FC_MAXL and S.FC_WIDTHS[6][1] > 2 * 256
    for widths, extra in S.FC_WIDTHS:
        for n in S.FC_N:
            hist, flat, _ = S.fc_input(widths, extra, n)
            assert flat.size == R.fc_layout(widths)[1] + 1 + extra
            assert S.fc_gate_margin(hist, flat, widths) > 4, (widths, n)
            if len(widths) > 2:                                # both sides of every ReLU layer are exercised
                _, acts = R.cond_fc(hist, flat, widths)
                assert all((a > 0).any() for a in acts[1:-1]) and any((a == 0).any() for a in acts[1:-1])


def test_local_global_cases_reach_their_branches_and_clear_their_gates():
    walks = [S.lg_walk(*s) for s in S.LG_SHAPES]
    assert [w['bx'] for w in walks] == [1, 1, 2, 3, 64] and S.lg_walk(1, 1, 64, 64)['bx'] == 1 and S.lg_walk(1, 1, 128, 64)['bx'] == 1
    assert not walks[4]['capped'] and S.lg_walk(1, 3, 728, 724)['capped'] and walks[4]['local_trips'] == 8
    assert walks[2]['finish_trips'] == 1 and walks[4]['finish_trips'] == 3
    for shape in S.LG_SHAPES:
        a, b = S.lg_input(shape)
        w = S.lg_walk(*shape)
        gain_margin, mean_margin = S.lg_gate_margin(a, b)
        # the fp32 gain errs by (2 plane_depth + LG_GAIN_BOUND) u relative; the mean of a by plane_depth u of mean |a|
        assert gain_margin > 100 * (2 * w['plane_depth'] + S.LG_GAIN_BOUND) * S.U and mean_margin > 0.5, shape
        raw = R.lg_gain(a, b).reshape(-1)
        if raw.size >= 4:
            assert (raw == 0.5).any() and (raw == 2.0).any() and ((raw > 0.5) & (raw < 2)).any() and (a.mean((2, 3)) < 0).any()
    launched = S.lg_value_flags()                              # the flags the GPU test hands over, shape by shape
    assert [len(f) for f in launched] == [s[0] for s in S.LG_SHAPES]
    assert {float(v) for f in launched for v in f} == {0.0, 0.5, 1.0, 2.0}
    assert any((f < 1).any() and (f >= 1).any() for f in launched)             # a batch with both branches among them
    assert (launched[4] == 2.0).all()                          # the cap of 64 workgroups with a flag of 2: all global
    assert (S.lg_flags('mixed', 1) < 1).all()
    for shape in S.LG_SHAPES:                                  # a = b: the gain just below 1, inside the clamp by far
        a, b = S.lg_input(shape, 'equal')
        gain = R.lg_gain(a, b)
        assert np.array_equal(a, b) and (gain < 1).all() and (gain > 0.99).all() and S.lg_gate_margin(a, b)[0] > 0.4
    for kind in ('half', 'two'):
        a, b = S.lg_input((2, 3, 8, 12), kind)
        assert (R.lg_gain(a, b) == (0.5 if kind == 'half' else 2.0)).all()
        d = a * R.lg_gain(a, b)[:, :, None, None] - b
        assert np.array_equal(d, np.round(d))
    a, b = S.lg_input((2, 3, 8, 12), 'centres')
    assert np.array_equal(R.lg_centres(a), np.round(R.lg_centres(a)))


def test_gray_world_gate_margins():
    sums, gk, hw = S.gray_case()
    margin = S.gray_gate_margin(sums, hw)
    m = sums.astype(F64) / hw
    assert (margin > 100).all()                                # no fp32 mean decides the gate the other way
    assert (m == 0).any() and (m < 0).any() and ((m > 0) & (m < R.GRAY_EPS)).any() and ((m > R.GRAY_EPS) & (m < 1e-5)).any()
    fwd, bwd = S.gray_bounds(sums, gk, hw)
    assert np.isfinite(fwd).all() and np.isfinite(bwd).all()


def test_integer_inputs_stay_below_2_to_the_24():
    ok, worst = S.integer_range_ok()
    assert all(ok.values()), worst
    x = S.stats_input(524292, 1, 1, True)
    assert set(np.unique(x)) <= {0.0, 1.0, 2.0, 3.0}
    outs, w, gy = S.mix_input(16, 1020, True)
    assert all(set(np.unique(o)) <= {-1.0, 0.0, 1.0} for o in outs + [gy]) and np.abs(w).max() <= 2
    a, b = S.sse_input(4097, True)
    assert set(np.unique(np.abs(R.u8_code(a) - R.u8_code(b)))) <= {0, 255}
    y, gt = S.loss_input(1020, True)
    assert set(np.unique(y - gt)) <= {-1.0, 0.0, 1.0}


def test_squared_error_inputs_cover_the_truncation():
    a, b = S.sse_input(4097, False)
    k = (np.arange(256) / 255).astype(F32)
    for v in (k, np.nextafter(k, F32(-1)), np.nextafter(k, F32(2))):
        assert np.isin(v, a).all()
    assert (a < 0).any() and (a > 1).any()


def test_refused_table_names_every_entry():
    assert {r[0] for r in S.REFUSED} == {'channel_stats', 'histc', 'mix_fwd', 'mix_bwd', 'pixel_loss', 'local_global', 'cond_fc', 'cond_fc_bwd', 'sse',
                                         'plane_sums', 'stats_bwd_rows', 'stats_bwd'}
