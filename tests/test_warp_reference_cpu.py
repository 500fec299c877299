"""The mesh warp without a GPU: the per-pixel coordinate against hand-worked values, the Catmull-Rom table's facts, the overflow
bound, the properties the definition promises (identity, flips, transpose, the affine bound), the radial builder against its own
per-pixel evaluation, what each deliberate mistake of the reference (tests/warp_reference.py) changes on the GPU tests' own
inputs, and the plumbing - builders, host refusals, keywords, header, verdict table."""
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import warp_reference as WR  # noqa: E402
from serve_verdicts import read_verdict  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the definition
def test_hand_worked_coordinates():
    """worked on paper: k = 2 (cell 4, shift 4, rounding term 8), a 2 x 2 node mesh, a 3 x 3 output of a 10 x 20 image"""
    mesh = np.array([[[0, -100], [400, 300]], [[800, 700], [1200, 1100]]], dtype=np.int32)
    uy, ux = WR.coords(mesh, 2, (3, 3), 10, 20, clamp=False)
    # y: rows are 0 -> 400 and 800 -> 1200 along x.  pixel (0,0): 4 * 4 * 0 + 8 >> 4 = 0; pixel (1,2): top = 2*0 + 2*400 = 800,
    # bot = 2*800 + 2*1200 = 4000, 3*800 + 1*4000 + 8 = 6408 >> 4 = 400; pixel (2,1): top = 3*0 + 400 = 400, bot = 3*800 + 1200 =
    # 3600, 2*400 + 2*3600 + 8 = 8008 >> 4 = 500
    assert uy[0, 0] == 0 and uy[1, 2] == 400 and uy[2, 1] == 500
    # x: rows are -100 -> 300 and 700 -> 1100.  pixel (0,0): 16 * -100 + 8 = -1592 >> 4 = -100 (floor of -99.5); pixel (0,1):
    # top = 3 * -100 + 300 = 0 -> 8 >> 4 = 0; pixel (1,0): top = -400, bot = 2800, 3 * -400 + 2800 + 8 = 1608 >> 4 = 100; and a
    # negative one that does not fall on an integer: nodes -101 instead of -100 give 16 * -101 + 8 = -1608 >> 4 = -101 (-100.5 floors)
    assert ux[0, 0] == -100 and ux[0, 1] == 0 and ux[1, 0] == 100
    mesh[0, 0, 1] = -101
    assert WR.coords(mesh, 2, (3, 3), 10, 20, clamp=False)[1][0, 0] == -101
    mesh[0, 0, 1] = -7                                  # pixel (0,1): top = 3 * -7 + 300 = 279, 4 * 279 + 8 = 1124 >> 4 = 70
    got = WR.coords(mesh, 2, (3, 3), 10, 20, clamp=False)[1]
    assert got[0, 1] == 70 and got[0, 0] == -7
    mesh[0, 1, 1] = -9                                  # pixel (0,1): top = 3 * -7 - 9 = -30, 4 * -30 + 8 = -112 >> 4 = -7 exactly;
    assert WR.coords(mesh, 2, (3, 3), 10, 20, clamp=False)[1][0, 1] == -7
    mesh[0, 1, 1] = -10                                 # top = -31, -124 + 8 = -116 >> 4 = -8 (floor of -7.25)
    assert WR.coords(mesh, 2, (3, 3), 10, 20, clamp=False)[1][0, 1] == -8
    # the replicate border: clamped to 0 .. (S-1) << 8 after the interpolation
    uy, ux = WR.coords(mesh, 2, (3, 3), 2, 2)
    assert uy.max() == 256 and ux.min() == 0 and ux.max() == 256 and uy[1, 2] == 256 and ux[0, 0] == 0
    # the largest mesh: no sum passes 2^48 (the reference asserts it) and the result is the node value itself
    big = np.full((2, 2, 2), 2 ** 31 - 1, dtype=np.int32)
    for k in (2, 8):
        assert (WR.coords(big, k, (1 << k, 1 << k), 5, 5, clamp=False)[0] == 2 ** 31 - 1).all()
        assert (WR.coords(-big - 1, k, (1 << k, 1 << k), 5, 5, clamp=False)[1] == -2 ** 31).all()


def test_the_cubic_table():
    import reconfigisp_amd.functional as F
    q = WR.cubic_table()
    assert q.shape == (256, 4) and (q.sum(axis=1) == 2048).all()
    assert q[0].tolist() == [0, 2048, 0, 0] and q[128].tolist() == [-128, 1152, 1152, -128]
    raw = WR.cubic_table(fixup=False)
    assert int((raw.sum(axis=1) != 2048).sum()) == 68
    got = F.warp_cubic_table()
    assert got.dtype == np.int16 and np.array_equal(got, q)
    # the float construction: floor(w * 2048 + 0.5) of the resize's bicubic kernel at the four tap distances, the same fix-up
    for f in range(256):
        t = f / 256.0
        row = [int(np.floor(F._resample_weight('bicubic', d) * 2048 + 0.5)) for d in (t + 1.0, t, 1.0 - t, 2.0 - t)]
        row[row.index(max(row))] += 2048 - sum(row)
        assert row == q[f].tolist(), f


def test_the_bicubic_sum_stays_inside_int32():
    """|v| + 2^21 < 2^31 over all 256 x 256 phase pairs on 0 / 255 images: the worst image puts 255 under every weight of one sign"""
    q = WR.cubic_table()
    outer = q[:, None, :, None] * q[None, :, None, :]                   # (ty, tx, r, c)
    hi = 255 * np.where(outer > 0, outer, 0).sum(axis=(2, 3))
    lo = 255 * np.where(outer < 0, outer, 0).sum(axis=(2, 3))
    worst = max(int(hi.max()), int(-lo.min()))
    assert worst == 1370357760 and worst + (1 << 21) < 1 << 31
    q12 = 4 * worst                                                     # Q12 weights: twice each factor
    assert q12 + (1 << 23) >= 1 << 31


@pytest.mark.parametrize('kernel', WR.KERNELS)
@pytest.mark.parametrize('k', (2, 4, 8))
def test_identity_double_flip_and_transpose_are_exact(k, kernel):
    h, w = 21, 35
    img = WR.make_image(2, h, w, seed=k)
    assert np.array_equal(WR.warp(img, WR.make_mesh('identity', (h, w), (h, w), k), k, (h, w), kernel), img)
    assert np.array_equal(WR.warp(img, WR.make_mesh('flip', (h, w), (h, w), k), k, (h, w), kernel), img[:, ::-1, ::-1])
    assert np.array_equal(WR.warp(img, WR.make_mesh('transpose', (h, w), (w, h), k), k, (w, h), kernel), img.transpose(0, 2, 1, 3))


def test_an_affine_map_is_within_one_q8_unit():
    """node rounding contributes 1/2 (a convex combination of errors <= 1/2), the final rounding 1/2"""
    import reconfigisp_amd.functional as F
    a = np.deg2rad(7.0)
    m = np.array([[0.93 * np.cos(a), -0.93 * np.sin(a), 11.3], [0.93 * np.sin(a), 0.93 * np.cos(a), -4.6], [0.0, 0.0, 1.0]])
    size = (70, 90)
    y, x = np.arange(size[0], dtype=np.float64)[:, None], np.arange(size[1], dtype=np.float64)[None, :]
    exact = (256.0 * (m[1, 0] * x + m[1, 1] * y + m[1, 2]), 256.0 * (m[0, 0] * x + m[0, 1] * y + m[0, 2]))
    worst = 0.0
    for cell in (4, 16, 256):
        mesh = F.warp_homography(m, size, cell).numpy()
        got = WR.coords(mesh, cell.bit_length() - 1, size, 1000, 1000, clamp=False)
        worst = max(worst, max(np.abs(g - e).max() for g, e in zip(got, exact)))
    print('affine: largest per-pixel coordinate error %.3f Q8 units' % worst)
    assert worst <= 1.0


def test_warp_radial_against_its_own_per_pixel_evaluation():
    import reconfigisp_amd.functional as F
    H, W, size = 96, 128, (96, 128)
    args = dict(k1=-0.18, k2=0.03, zoom=0.95)
    fn = F.warp_radial_source(H, W, size, **args)
    y, x = np.arange(size[0], dtype=np.float64)[:, None], np.arange(size[1], dtype=np.float64)[None, :]
    exact = [256.0 * v for v in fn(y, x)]
    err = {}
    for cell in (16, 64):
        mesh = F.warp_radial(H, W, size, cell, **args)
        assert mesh.dtype == torch.int32 and tuple(mesh.shape) == ((size[0] - 1) // cell + 2, (size[1] - 1) // cell + 2, 2)
        got = WR.coords(mesh.numpy(), cell.bit_length() - 1, size, H, W, clamp=False)
        err[cell] = max(np.abs(g - e).max() for g, e in zip(got, exact))
        print('warp_radial 96 x 128, k1 -0.18, k2 0.03, zoom 0.95, cell %d: largest coordinate error %.2f Q8 units' % (cell, err[cell]))
    assert err[16] <= err[64]
    # a node IS the model: floor(v * 256 + 0.5) there
    mesh = F.warp_radial(H, W, size, 16, **args).numpy()
    sy, sx = fn(np.array([[32.0]]), np.array([[48.0]]))
    assert mesh[2, 3].tolist() == [int(np.floor(sy[0, 0] * 256 + 0.5)), int(np.floor(sx[0, 0] * 256 + 0.5))]
    # no distortion, same size: the identity
    assert np.array_equal(F.warp_radial(H, W, size, 16, 0.0).numpy(), WR.make_mesh('identity', (H, W), size, 4))


@pytest.mark.parametrize('name', list(WR.WRONG))
def test_every_wrong_variant_changes_a_byte_on_the_cases(name):
    fn, kernels = WR.WRONG[name]
    for kernel in kernels:
        changed = sum(int((fn(ci, kernel) != WR.want(ci, kernel)).sum()) for ci in range(len(WR.CASES)))
        assert changed > 0, (name, kernel)


@pytest.mark.parametrize('name', list(WR.HARMLESS))
def test_two_mistakes_cannot_change_a_byte(name):
    """truncation at the per-pixel shift differs from floor only below zero, where the clamp to 0 follows - the unclamped
    coordinates do differ -; the tap past the last column has weight 0 (the clamp keeps the read inside the image)"""
    fn, kernels = WR.HARMLESS[name]
    for kernel in kernels:
        for ci in range(len(WR.CASES)):
            assert np.array_equal(fn(ci, kernel), WR.want(ci, kernel)), (name, kernel, ci)
    img, mesh, k, size = WR.case_inputs(5)
    a = WR.coords(mesh, k, size, *img.shape[1:3], clamp=False)
    b = WR.coords(mesh, k, size, *img.shape[1:3], clamp=False, truncate=True)
    assert (a[0] != b[0]).any() and (a[0][a[0] >= 0] == b[0][a[0] >= 0]).all() and (b[0][a[0] < 0] <= 0).all()


def test_the_cases_are_the_ones_the_launch_can_go_wrong_at():
    """which tiles stage: from the coordinates, the box of each 64 x 16 tile as the kernel forms it"""
    import reconfigisp_amd.functional as F

    def staged(ci, cubic):
        img, mesh, k, size = WR.case_inputs(ci)
        H, W = img.shape[1:3]
        uy, ux = WR.coords(mesh, k, size, H, W)
        res = []
        for i0 in range(0, size[0], F.WARP_TILE_H):
            for j0 in range(0, size[1], F.WARP_TILE_W):
                ty, tx = uy[i0:i0 + F.WARP_TILE_H, j0:j0 + F.WARP_TILE_W] >> 8, ux[i0:i0 + F.WARP_TILE_H, j0:j0 + F.WARP_TILE_W] >> 8
                rows = min(ty.max() + (2 if cubic else 1), H - 1) - max(ty.min() - (1 if cubic else 0), 0) + 1
                cols = min(tx.max() + (2 if cubic else 1), W - 1) - max(tx.min() - (1 if cubic else 0), 0) + 1
                res.append(rows * ((cols * 3 + 6) & ~3) <= F.WARP_LDS_BYTES - 5136)
        return res
    for cubic in (False, True):
        assert all(staged(0, cubic)) and all(staged(1, cubic)) and len(staged(1, cubic)) == 16
        assert not staged(2, cubic)[0], 'the 8:1 tile of 64 columns passes the LDS budget'
        s = staged(3, cubic)
        assert any(s) and not all(s), 'staged and global tiles in one launch'


# ---------------------------------------------------------------- builders and refusals on the host
def test_builders():
    import reconfigisp_amd.functional as F
    for k in (2, 4, 8):
        cell = 1 << k
        ident = F.warp_homography(np.eye(3), (21, 35), cell)
        assert ident.dtype == torch.int32 and ident.is_contiguous() and not ident.is_cuda
        assert np.array_equal(ident.numpy(), WR.make_mesh('identity', (21, 35), (21, 35), k))
        flip = F.warp_homography([[-1, 0, 34], [0, -1, 20], [0, 0, 1]], (21, 35), cell)
        assert np.array_equal(flip.numpy(), WR.make_mesh('flip', (21, 35), (21, 35), k))
        turn = F.warp_homography(torch.tensor([[0.0, 1, 0], [1, 0, 0], [0, 0, 1]]), (35, 21), cell)
        assert np.array_equal(turn.numpy(), WR.make_mesh('transpose', (21, 35), (35, 21), k))
    # warp_mesh: fn sees the node coordinates once, floor(v * 256 + 0.5), saturation
    seen = []

    def fn(y, x):
        seen.append((y.shape, x.shape, y[-1, 0], x[0, -1]))
        return y * 0.5 - 0.001, x * 1e9
    mesh = F.warp_mesh(fn, (9, 10), 4).numpy()
    assert seen == [((4, 1), (1, 4), 12.0, 12.0)] and mesh.shape == (4, 4, 2)
    assert mesh[1, 0].tolist() == [int(np.floor((2.0 - 0.001) * 256 + 0.5)), 0] and mesh[0, 0, 0] == int(np.floor(-0.256 + 0.5))
    assert mesh[0, 1, 1] == 2 ** 31 - 1 and F.warp_mesh(lambda y, x: (y, -x * 1e9), (9, 10), 4).numpy()[0, 1, 1] == -2 ** 31
    # keystone: the nodes are the projective map itself
    m = np.array([[1.0, 0.02, 3.0], [0.01, 1.0, -2.0], [1e-4, 2e-4, 1.0]])
    ks = F.warp_homography(m, (40, 50), 16).numpy()
    d = m[2, 0] * 32 + m[2, 1] * 16 + m[2, 2]
    assert ks[1, 2].tolist() == [int(np.floor((m[1, 0] * 32 + m[1, 1] * 16 + m[1, 2]) / d * 256 + 0.5)),
                                 int(np.floor((m[0, 0] * 32 + m[0, 1] * 16 + m[0, 2]) / d * 256 + 0.5))]
    with pytest.raises(ValueError, match='denominator is -?[0-9.e+-]+ at node'):
        F.warp_homography([[1, 0, 0], [0, 1, 0], [-0.05, 0, 1]], (40, 50), 16)
    with pytest.raises(ValueError, match='3 x 3'):
        F.warp_homography(np.eye(2), (40, 50), 16)
    with pytest.raises(ValueError, match='3 x 3'):
        F.warp_homography([[1, 0, 0], [0, 1, 0], [0, float('nan'), 1]], (40, 50), 16)
    with pytest.raises(ValueError, match='cell 12'):
        F.warp_mesh(lambda y, x: (y, x), (9, 10), 12)
    with pytest.raises(ValueError, match='cell 512'):
        F.warp_homography(np.eye(3), (9, 10), 512)
    with pytest.raises(ValueError, match=r'size \(0, 10\)'):
        F.warp_mesh(lambda y, x: (y, x), (0, 10), 4)
    with pytest.raises(ValueError, match='not numbers at 16 nodes'):
        F.warp_mesh(lambda y, x: (y * float('nan'), x), (9, 10), 4)
    with pytest.raises(ValueError, match=r'\(sy, sx\)'):
        F.warp_mesh(lambda y, x: y, (9, 10), 4)
    with pytest.raises(ValueError, match='do not broadcast'):
        F.warp_mesh(lambda y, x: (np.zeros((3, 3)), x), (9, 10), 4)
    with pytest.raises(ValueError, match='zoom'):
        F.warp_radial(96, 128, (96, 128), 16, 0.1, zoom=0.0)
    with pytest.raises(ValueError, match='centre'):
        F.warp_radial(96, 128, (96, 128), 16, 0.1, centre=5)


def test_warp_check_names_what_is_wrong():
    import reconfigisp_amd.functional as F
    H, W, size = 37, 53, (19, 45)
    mesh = torch.from_numpy(WR.make_mesh('smooth', (H, W), size, 2, 1))
    got = F.warp_check((mesh, 4, size, 'bicubic'), H, W)
    assert got[0] is mesh and got[1:] == (2, size, 'bicubic')
    assert F.warp_check([mesh, 4, [np.int64(19), 45], 'bilinear'], H, W, mesh.device)[2] == size
    for warp, what in (((mesh, 4, size), 'a warp is'), (5, 'a warp is'),
                       ((mesh, 12, size, 'bilinear'), 'cell 12'), ((mesh, 2, size, 'bilinear'), 'cell 2'),
                       ((mesh, 4.0, size, 'bilinear'), 'cell 4.0'), ((mesh, True, size, 'bilinear'), 'cell True'),
                       ((mesh, 4, (0, 45), 'bilinear'), r'size \(0, 45\)'), ((mesh, 4, (19,), 'bilinear'), r'size \(19,\)'),
                       ((mesh, 4, (19.0, 45), 'bilinear'), 'size'), ((mesh, 4, (19, 2 ** 23 + 1), 'bilinear'), 'size'),
                       ((mesh, 4, size, 'lanczos'), "kernel 'lanczos'"), ((mesh, 4, size, 1), 'kernel 1'),
                       ((mesh.long(), 4, size, 'bilinear'), 'int32'), ((mesh.numpy(), 4, size, 'bilinear'), 'int32'),
                       ((mesh[:-1], 4, size, 'bilinear'), r'\(6,13,2\)'), ((mesh, 8, size, 'bilinear'), r'\(4,7,2\)'),
                       ((mesh.transpose(0, 1).contiguous().transpose(0, 1), 4, size, 'bilinear'), 'contiguous'),
                       ((torch.zeros((2 ** 20 // 16 + 2, 2, 2), dtype=torch.int32), 16, (2 ** 20 + 1, 3), 'bilinear'), 'row tiles')):
        with pytest.raises(ValueError, match=what):
            F.warp_check(warp, H, W)
    with pytest.raises(ValueError, match='even'):
        F.warp_check((mesh, 4, size, 'bilinear'), H, W, nv12=True)
    with pytest.raises(ValueError, match='lives on'):
        F.warp_check((mesh, 4, size, 'bilinear'), H, W, torch.device('meta'))
    odd = torch.zeros(mesh.numel() + 1, dtype=torch.int32)[1:].view(mesh.shape)
    if odd.data_ptr() % 8:
        with pytest.raises(ValueError, match='8-byte'):
            F.warp_check((odd, 4, size, 'bilinear'), H, W)
    with pytest.raises(ValueError, match='H and W'):
        F.warp_check((mesh, 4, size, 'bilinear'), 0, W)


def test_host_refusals_come_before_the_device():
    """on CPU tensors: whatever is wrong is named before the device is asked for, and a right call is refused for being there"""
    import reconfigisp_amd.functional as F
    from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF
    H, W, size = 24, 40, (10, 18)
    mesh = torch.from_numpy(WR.make_mesh('smooth', (H, W), size, 2, 2))
    warp = (mesh, 4, size, 'bilinear')
    img = torch.zeros((2, H, W, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match='uint8'):
        F.bgr8_warp(img.float(), warp)
    with pytest.raises(ValueError, match='uint8'):
        F.bgr8_warp(img[..., :2], warp)
    with pytest.raises(ValueError, match="kernel 'nearest'"):
        F.bgr8_warp(img, (mesh, 4, size, 'nearest'))
    for stage in ('ldz', 2, True):
        with pytest.raises(ValueError, match='stage'):
            F.bgr8_warp(img, warp, stage=stage)
    with pytest.raises(RuntimeError, match='img'):
        F.bgr8_warp(img, warp)                                          # all is right but the device
    raw = torch.zeros((1, H, W), dtype=torch.uint16)
    for kw, what in ((dict(warp=(mesh, 12, size, 'bilinear')), 'cell 12'), (dict(warp=(mesh, 4, size, 'cubic')), "kernel 'cubic'"),
                     (dict(warp=(mesh, 4, (10, 21), 'bilinear')), r'\(4,7,2\)'),
                     (dict(warp=(mesh, 4, (10, 18), 'bilinear'), out_format='nv12', reverse_channels=True), 'reverse_channels'),
                     (dict(warp=(torch.zeros((4, 6, 2), dtype=torch.int32), 4, (9, 18), 'bilinear'), out_format='nv12'), 'even'),
                     (dict(warp=warp, out_size=(4, 4), resample='lanczos'), 'resample'),
                     (dict(warp=warp, out_window=(0, 0, 11, 18)), 'out_window'),       # the window lies in the WARPED image
                     (dict(warp=warp, out_size=(5, 8), out_format='nv12'), 'even'),
                     (dict(warp=warp, out=torch.zeros((1, 10, 17, 3), dtype=torch.uint8)), 'out must be')):
        with pytest.raises(ValueError, match=what):
            PF.serve_frame([], [], raw, 1023.0, 16, 8, **kw)
        with pytest.raises(ValueError, match=what):
            PF.serve_frame([], [], raw[0], 1023.0, 16, 8, **{**kw, 'out': kw['out'][0]} if 'out' in kw else kw)
    for call in (lambda: PF.serve([], [], raw, 1023.0, warp=warp), lambda: PF.serve_frame([], [], raw, 1023.0, 16, 8, warp=warp)):
        with pytest.raises((RuntimeError, ValueError)):
            call()


# ---------------------------------------------------------------- plumbing
def _serve_functions():
    from reconfigisp_amd.codes.models.isp_model import IspModel
    from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF
    from reconfigisp_amd.codes.models.modules.isp_universal import IspUniversal
    from reconfigisp_amd.codes.models.modules.origin_universal import OriginUniversal
    return [(PF.serve, 'serve'), (PF.serve_frame, 'serve_frame')] + [
        (getattr(cls, name), name) for cls in (IspUniversal, OriginUniversal, IspModel) for name in ('serve', 'serve_frame')]


def test_the_keyword_on_all_eight_functions():
    fns = _serve_functions()
    assert len(fns) == 8
    for fn, name in fns:
        pars = inspect.signature(fn).parameters
        names = list(pars)
        p = pars['warp']
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None, fn
        assert 'warp' in fn.__doc__, fn
        at = names.index('warp')
        assert names[at - 1] == 'statistics' and names[at + 1] == 'raw_width', fn
        assert names[names.index('resample') + 1] == 'raw_format', fn
        if name == 'serve':
            assert names[-5:] == ['raw_width', 'lens_shading', 'defect_correction', 'fast_median', 'fast_denoise_scene'], fn
        else:
            assert names[-3:] == ['raw_width', 'defect_correction', 'lens_shading'], fn


def test_the_entry_point_is_declared():
    import reconfigisp_amd.functional as F
    from reconfigisp_amd import lib as L
    header = open(os.path.join(ROOT, 'include', 'risp.h')).read()
    assert re.search(r'^int risp_bgr8_warp\(', header, flags=re.M)
    assert 'risp_bgr8_warp' in L.SIGNATURES and len(L.SIGNATURES['risp_bgr8_warp'][1]) == 14
    decl = header[header.index('\nint risp_bgr8_warp('):]
    assert decl[:decl.index(';')].count(',') == 13
    for name, value in (('RISP_WARP_TILE_W', F.WARP_TILE_W), ('RISP_WARP_TILE_H', F.WARP_TILE_H),
                        ('RISP_WARP_LDS_BYTES', F.WARP_LDS_BYTES)):
        assert re.search(r'^#define %s %d$' % (name, value), header, flags=re.M), name
    assert F.WARP_KERNELS == ('bilinear', 'bicubic') and F.WARP_LDS_BYTES == 65536


def test_warp_stage_is_a_pure_table_and_the_table_is_the_measured_verdict():
    from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF
    assert isinstance(PF._WARP_STAGED, frozenset) and PF._WARP_STAGED <= {'bilinear', 'bicubic'}
    for kernel in ('bilinear', 'bicubic'):
        assert PF.warp_stage(kernel) == ('lds' if kernel in PF._WARP_STAGED else 'gather')
        assert PF.warp_stage(kernel) == PF.warp_stage(kernel)
    for kernel in ('box', None, 0):
        with pytest.raises(ValueError, match='kernel'):
            PF.warp_stage(kernel)
    assert read_verdict('serve_warp.txt', '_WARP_STAGED') == PF._WARP_STAGED
