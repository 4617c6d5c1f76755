"""Guarded, poisoned device destinations shared by tests/test_gpu_weight_prep.py and tests/test_gpu_containment.py.

A destination of `n` bytes sits inside one allocation filled with a poison byte: GUARD poisoned bytes in front of it, 16x its
size (never less than GUARD) behind it.  A callee that writes a little outside its buffer shows up as a failed assertion, not
as a corrupted neighbour.  Running the callee twice, on buffers poisoned with POISON[0] and POISON[1], tells where it wrote: a
byte equal in both runs was written, a byte that differs was not (a written byte can equal one poison, never both)."""
import numpy as np
import torch

GUARD = 4096                                     # poisoned bytes in front of every destination; behind it 16x its size more
POISON = (0xA5, 0x5A)
ALIGN = 256


class Guarded:
    """A destination of `n` bytes inside one allocation of GUARD + n + GUARD + 16 n bytes filled with `poison`.  `offset`: the
    destination starts that many bytes past a 256-byte boundary (0: on the boundary itself)."""

    def __init__(self, n, poison, offset=0):
        # (the zone behind is large enough to hold what a pack with a wrong kernel volume or layer lookup would write: a
        # faulty packer shows up as a failed assertion, not as a corrupted neighbour)
        assert 0 <= offset < ALIGN
        self.n, self.poison = int(n), poison
        self.t = torch.full((2 * ALIGN + GUARD + self.n + GUARD + 16 * self.n,), poison, dtype=torch.uint8, device="cuda")
        self.front = (-(self.t.data_ptr() + GUARD)) % ALIGN + GUARD + offset      # >= GUARD poisoned bytes in front
        assert (self.t.data_ptr() + self.front - offset) % ALIGN == 0

    @property
    def ptr(self):
        return self.t.data_ptr() + self.front

    def fill(self, data):
        """Set the destination's bytes (a caller-initialised buffer, or an input to be checked for writes)."""
        data = np.ascontiguousarray(data).view(np.uint8).ravel()
        assert data.size == self.n
        if self.n:
            self.t[self.front:self.front + self.n] = torch.from_numpy(data).cuda()

    def read(self):
        """(every guard byte still holds the poison, the destination's bytes) from one copy of the allocation."""
        h = self.t.cpu().numpy()
        intact = bool(np.all(h[:self.front] == self.poison) and np.all(h[self.front + self.n:] == self.poison))
        return intact, h[self.front:self.front + self.n].copy()

    def body(self):
        intact, b = self.read()
        assert intact, "write outside the destination"
        return b


def written(a, b):
    """Bytes of two runs on buffers poisoned with POISON[0] / POISON[1]: True where the callee wrote."""
    return a == b
