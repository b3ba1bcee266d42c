"""A device array between two guard bands, for the tests that launch a kernel on raw pointers (test_gpu_mobility_direct.py,
test_gpu_queue_direct.py): GUARD bytes of a byte pattern before and after the array, inside one allocation, so that a store next to
the array lands in memory the test owns and can see.  The allocation of test_gpu_channel_large.py, stated once."""
import numpy as np
import torch

GUARD = 4096


class Guarded:
    """A device array of `shape` and `dtype` inside a larger allocation: GUARD bytes of a pattern before and after it."""

    def __init__(self, shape, dtype):
        self.nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        pad = -self.nbytes % 16                                           # (the band behind the array starts right at its end)
        total = 2 * GUARD + self.nbytes + pad
        self.pattern = ((torch.arange(total, dtype=torch.int64, device='cuda') * 7 + 3) % 251).to(torch.uint8)
        self.buf = self.pattern.clone()
        self.array = self.buf[GUARD:GUARD + self.nbytes].view(dtype).view(shape)
        assert self.array.data_ptr() % 16 == 0 and self.array.data_ptr() == self.buf.data_ptr() + GUARD

    def intact(self):
        lo, hi = slice(0, GUARD), slice(GUARD + self.nbytes, None)
        return bool(torch.equal(self.buf[lo], self.pattern[lo])) and bool(torch.equal(self.buf[hi], self.pattern[hi]))


def bits(a):
    """The bytes of a tensor or an array, as NumPy uint8."""
    if torch.is_tensor(a):
        a = a.detach().contiguous().cpu().numpy()
    return np.ascontiguousarray(a).view(np.uint8)
