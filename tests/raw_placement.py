"""Sensor frames at chosen addresses, for the GPU tests of the raw-domain entry points: each helper copies numpy frames into a
contiguous device view that starts a given distance into a larger allocation of all-ones bytes, so that the 8-byte, the
2-byte-only and the odd-byte forms of the loads are all reached and a sample read outside the frames shows as 0xFFFF / 0xFF."""
import torch

import raw_packed_reference as PR


def _place16(x, at):
    """the numpy uint16 frames as a contiguous device view ``at`` words into an allocation of 0xFF bytes"""
    big = torch.full((x.size + 8,), 0xFFFF, dtype=torch.uint16).cuda()
    dev = big[at:at + x.size].view(x.shape)
    dev.copy_(torch.from_numpy(x))
    return dev


def _place(data, offset):
    """the packed (N,H,stride) numpy frames as a contiguous device view ``offset`` bytes into an allocation of 0xFF bytes"""
    size = data.size
    big = torch.full((size + 16,), 0xFF, dtype=torch.uint8, device='cuda')
    view = big[offset:offset + size].view(data.shape)
    view.copy_(torch.from_numpy(data))
    assert view.is_contiguous() and view.data_ptr() % 2 == offset % 2
    return view


def _place_packed(x, bits, stride, offset):
    """the numpy uint16 frames packed as RAW10 / RAW12 with rows of ``stride`` bytes (pseudo-random bytes in the padding), placed
    as ``_place`` does"""
    return _place(PR.pack(x, bits, stride, None), offset)
