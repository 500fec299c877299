"""The mesh-warp launch (risp_bgr8_warp, functional.bgr8_warp) against the numpy restatement of its definition
(tests/warp_reference.py): both kernels, both forms of the launch (stage 0: every tile samples global memory; stage 1: a tile
stages its source box in LDS where it fits), byte for byte, on the smallest shapes at which the kernel can go wrong."""
import ctypes as C
import os
import sys
import threading

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import warp_reference as WR  # noqa: E402
from bgr8_placement import _at_odd_address, _guards_intact  # noqa: E402

pytestmark = pytest.mark.gpu

_WANT = {}


def _want(ci, kernel):
    """the reference's bytes for case ci, computed once and shared"""
    if (ci, kernel) not in _WANT:
        out = WR.want(ci, kernel)
        out.setflags(write=False)
        _WANT[ci, kernel] = out
    return _WANT[ci, kernel]


def _counted(fn):
    from reconfigisp_amd import lib as L
    L.CALLS = {}
    try:
        out = fn()
        return out, dict(L.CALLS)
    finally:
        L.CALLS = None


def _case_id(ci):
    return '%s->%s cell %d %s' % (WR.CASES[ci][0], WR.CASES[ci][1], 1 << WR.CASES[ci][2], WR.CASES[ci][3])


@pytest.mark.parametrize('stage', (0, 1))
@pytest.mark.parametrize('kernel', WR.KERNELS)
@pytest.mark.parametrize('ci', range(len(WR.CASES)), ids=_case_id)
def test_bgr8_warp_equals_the_reference(ci, kernel, stage):
    """the image sits at an odd address inside a larger allocation of other bytes, so does the output: a read outside the image
    would show as a wrong byte wherever it had any weight, a write outside the output in the guard bytes"""
    import reconfigisp_amd.functional as F
    img, mesh, k, size = WR.case_inputs(ci)
    n, h, w = img.shape[:3]
    dev, big = _at_odd_address(img, 13, 51, np.random.default_rng(ci))
    host = big.cpu().numpy()
    out, guard = _at_odd_address((n, size[0], size[1], 3), 7, 25, 0x5A)
    warp = (torch.from_numpy(mesh).cuda(), 1 << k, size, kernel)
    got, calls = _counted(lambda: F.bgr8_warp(dev, warp, out=out, stage=stage))
    assert got is out and calls == {'risp_bgr8_warp': 1}
    torch.cuda.synchronize()
    want = _want(ci, kernel)
    diff = got.cpu().numpy() != want
    assert not diff.any(), '%d bytes differ, the first at %s' % (diff.sum(), np.argwhere(diff)[0])
    assert _guards_intact(guard, out, 0x5A), 'the launch wrote outside its image'
    assert np.array_equal(big.cpu().numpy(), host), 'the launch wrote into its input'


@pytest.mark.parametrize('kernel', WR.KERNELS)
def test_identity_flips_and_transpose(kernel):
    import reconfigisp_amd.functional as F
    h, w = 37, 83
    img = torch.from_numpy(WR.make_image(2, h, w, seed=3)).cuda()
    for stage in ('gather', 'lds', None):
        for cell in (4, 16, 256):
            ident = (F.warp_homography(np.eye(3), (h, w), cell).cuda(), cell, (h, w), kernel)
            assert torch.equal(F.bgr8_warp(img, ident, stage=stage), img)
            both = (F.warp_homography([[-1, 0, w - 1], [0, -1, h - 1], [0, 0, 1]], (h, w), cell).cuda(), cell, (h, w), kernel)
            assert torch.equal(F.bgr8_warp(img, both, stage=stage), torch.flip(img, (1, 2)))
            lr = (F.warp_homography([[-1, 0, w - 1], [0, 1, 0], [0, 0, 1]], (h, w), cell).cuda(), cell, (h, w), kernel)
            assert torch.equal(F.bgr8_warp(img, lr, stage=stage), torch.flip(img, (2,)))
            turn = (F.warp_homography([[0, 1, 0], [1, 0, 0], [0, 0, 1]], (w, h), cell).cuda(), cell, (w, h), kernel)
            assert torch.equal(F.bgr8_warp(img, turn, stage=stage), img.transpose(1, 2))


def test_a_single_image_out_reuse_and_a_strided_input():
    import reconfigisp_amd.functional as F
    img, mesh, k, size = WR.case_inputs(1)
    dev = torch.from_numpy(img).cuda()
    warp = (torch.from_numpy(mesh).cuda(), 1 << k, size, 'bicubic')
    want = torch.from_numpy(_want(1, 'bicubic').copy()).cuda()
    one = F.bgr8_warp(dev[1], warp)
    assert tuple(one.shape) == size + (3,) and torch.equal(one, want[1])
    buf = torch.zeros_like(want)
    assert F.bgr8_warp(dev, warp, out=buf, stage='lds') is buf and torch.equal(buf, want)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    F.bgr8_warp(dev, warp, out=buf, stage='gather')
    assert torch.cuda.memory_allocated() == before, 'a call with out= allocated'
    assert torch.equal(buf, want)
    wide = torch.zeros((2, 100, 310, 3), dtype=torch.uint8, device='cuda')
    wide[:, :, :300] = dev
    assert torch.equal(F.bgr8_warp(wide[:, :, :300], warp), want)         # copied first
    for bad, what in ((buf[:1], 'out must be'), (buf[:, :, :100], 'out must be'), (buf.int(), 'out must be')):
        with pytest.raises(ValueError, match=what):
            F.bgr8_warp(dev, warp, out=bad)
    same = (F.warp_homography(np.eye(3), (100, 300), 16).cuda(), 16, (100, 300), 'bilinear')
    with pytest.raises(ValueError, match='shares memory'):
        F.bgr8_warp(dev, same, out=dev)
    with pytest.raises(ValueError, match='lives on'):
        F.bgr8_warp(dev, (torch.from_numpy(mesh), 1 << k, size, 'bicubic'))


def test_refusals_through_the_c_abi_leave_the_output_alone():
    import reconfigisp_amd.functional as F
    from reconfigisp_amd import lib as L
    lib = L.load()
    img, mesh, k, size = WR.case_inputs(0)
    n, h, w = img.shape[:3]
    dev, m = torch.from_numpy(img).cuda(), torch.from_numpy(mesh).cuda()
    count = n * size[0] * size[1] * 3
    out = torch.full((count + 16,), 0x5A, device='cuda', dtype=torch.uint8)
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(img_p=p(dev), out_p=p(out), mesh_p=p(m), k=k, MH=m.shape[0], MW=m.shape[1], kernel=0, stage=1, N=n, H=h, W=w,
             WH=size[0], WW=size[1]):
        return lib.risp_bgr8_warp(img_p, out_p, mesh_p, k, MH, MW, kernel, stage, N, H, W, WH, WW, stream)

    refused = {'null img': (dict(img_p=None), b'img (nil)'), 'null out': (dict(out_p=None), b'out (nil)'),
               'null mesh': (dict(mesh_p=None), b'mesh (nil)'), 'N 0': (dict(N=0), b'N=0'), 'N 65536': (dict(N=65536), b'N=65536'),
               'H 0': (dict(H=0), b'H=0'), 'W too large': (dict(W=(1 << 23) + 1), b'W=8388609'), 'WH 0': (dict(WH=0), b'WH=0'),
               'WW too large': (dict(WW=(1 << 23) + 1), b'WW=8388609'), 'cell_log2 1': (dict(k=1), b'cell_log2 1'),
               'cell_log2 9': (dict(k=9), b'cell_log2 9'), 'MH short': (dict(MH=m.shape[0] - 1), b'a 5 x 13 mesh'),
               'MW long': (dict(MW=m.shape[1] + 1), b'a 6 x 14 mesh'), 'kernel 2': (dict(kernel=2), b'kernel 2'),
               'kernel -1': (dict(kernel=-1), b'kernel -1'), 'stage 2': (dict(stage=2), b'stage 2'),
               'out on img': (dict(out_p=C.c_void_p(dev.data_ptr() + 64)), b'overlaps'),
               'row tiles': (dict(WH=65536 * 16, MH=((65536 * 16 - 1) >> k) + 2), b'row tiles'),
               'mesh not aligned': (dict(mesh_p=C.c_void_p(m.data_ptr() + 4)), b'8-byte aligned')}
    stream, failures = F._stream(), []

    def body():                         # risp_last_error is per thread: the messages provoked here stay out of the main thread's
        try:
            for what, (kw, named) in refused.items():
                assert call(**kw) != 0, '%s was accepted' % what
                err = lib.risp_last_error()
                assert b'risp_bgr8_warp' in err and named in err, (what, err)
        except BaseException as e:      # noqa: BLE001 - handed to the main thread
            failures.append(e)
    t = threading.Thread(target=body)
    t.start()
    t.join()
    if failures:
        raise failures[0]
    torch.cuda.synchronize()
    assert (out == 0x5A).all().item() and np.array_equal(dev.cpu().numpy(), img), 'a refused call wrote'
    for kernel, stage in ((0, 0), (1, 1)):
        out.fill_(0x5A)
        assert call(kernel=kernel, stage=stage) == 0
        torch.cuda.synchronize()
        assert (out[count:] == 0x5A).all().item()
        assert np.array_equal(out[:count].view(n, size[0], size[1], 3).cpu().numpy(), _want(0, WR.KERNELS[kernel]))
