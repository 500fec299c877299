"""Packed 8-bit images at chosen addresses, for the GPU tests of the output-stage entry points (resize, sharpen, warp, NV12): an
image or an output is a contiguous device view that starts a given number of bytes into a larger allocation of known bytes, so that
the loads and stores of every alignment are reached, a byte read outside an image shows as a wrong result and a byte written
outside an output shows in the guard bytes.  tests/raw_placement.py does the same for sensor frames."""
import numpy as np
import torch


def _at_odd_address(x, offset=1, tail=64, fill=0xA5):
    """x (a device tensor or a numpy array of bytes) as a contiguous view of its shape that starts ``offset`` bytes into a larger
    buffer of ``fill`` bytes - a byte, or a numpy Generator for random ones - with ``tail`` bytes behind it -> (view, buffer).
    x given as a shape: an output to be written, which holds the fill too, so that a byte never written shows as well"""
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(x)
    shape, count = (x, int(np.prod(x))) if isinstance(x, tuple) else (x.shape, x.numel())
    size = count + offset + tail
    if isinstance(fill, np.random.Generator):
        buf = torch.from_numpy(fill.integers(0, 256, size=(size,), dtype=np.uint8)).cuda()
    else:
        buf = torch.full((size,), fill, dtype=torch.uint8, device='cuda')
    view = buf[offset:offset + count].view(shape)
    if not isinstance(x, tuple):
        view.copy_(x)
    assert view.is_contiguous() and view.data_ptr() % 4 == (buf.data_ptr() + offset) % 4
    return view, buf


def _guards_intact(buf, view, fill=0xA5):
    """whether every byte of ``buf`` in front of and behind ``view`` still holds ``fill``"""
    at = view.data_ptr() - buf.data_ptr()
    return bool((buf[:at] == fill).all().item() and (buf[at + view.numel():] == fill).all().item())
