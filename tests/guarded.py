"""An output buffer that shows where a launch writes: NaN inside, a band of sentinel floats on either side."""
import numpy as np
import torch

NAN, GUARD, BAND = float('nan'), 12345.0, 64


class Guarded:
    """a device buffer between two bands of BAND sentinel floats (256 bytes: the view stays 16-byte aligned), NaN inside.  ``off``: floats
    by which the view is moved into the second band's side (1 = a view 4 bytes off 16, the bands still BAND floats each)"""

    def __init__(self, *shape, off=0):
        numel = int(np.prod(shape))
        self.raw = torch.full((numel + 2 * BAND + off,), GUARD, device='cuda')
        self.lo, self.hi = BAND + off, BAND + off + numel
        self.t = self.raw[self.lo: self.hi].view(*shape)
        self.t.fill_(NAN)
        assert self.t.data_ptr() % 16 == 4 * (off % 4)

    def bands_intact(self):
        return (self.raw[:self.lo] == GUARD).all().item() and (self.raw[self.hi:] == GUARD).all().item()

    def untouched(self):
        return self.bands_intact() and torch.isnan(self.t).all().item()


def off16(t, off=1):
    """a copy of ``t`` as a view ``off`` floats off a 16-byte boundary"""
    raw = torch.empty(t.numel() + 4, device=t.device, dtype=t.dtype)
    assert raw.data_ptr() % 16 == 0
    v = raw[off: off + t.numel()].view(t.shape)
    v.copy_(t)
    return v
