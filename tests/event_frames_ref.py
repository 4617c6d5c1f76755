"""Numpy restatement of the event-frame stage (csrc/event_frames.hip, v2ce-toolbox_amd/event_frames.py), written afresh
from the rules: sequential f32 sums in plane order; the positive values of the mode's channels as f32 bit patterns; a
three-level selection on them (bits 30..20, 19..10, 9..0); np.percentile restated on two order statistics; frames =
trunc(min(max(x, 0), upper) / upper * 255) in float64 (polarity kept, blue = 0) or float32 (grey).  Not a test module."""
import numpy as np


def sums(vox):
    """[L,2,10,H,W] f32 -> [L,3,H,W] f32: each sum starts at its first plane and adds the rest in order."""
    pl = vox.reshape(vox.shape[0], 20, *vox.shape[3:])
    out = np.empty((vox.shape[0], 3, *vox.shape[3:]), np.float32)
    for c, idx in enumerate((range(0, 10), range(10, 20), range(0, 20))):
        acc = pl[:, idx[0]]
        for j in idx[1:]:
            acc = acc + pl[:, j]
        out[:, c] = acc
    return out


def positive_bits(S, keep_polarity):
    """The values > 0 of the mode's channels (S0 and S1, or S2 once) as int64 bit patterns."""
    v = np.ascontiguousarray(S[:, :2] if keep_polarity else S[:, 2]).ravel()
    return v[v > 0].view(np.uint32).astype(np.int64)


def level0_hist(bits):
    return np.bincount(bits >> 20, minlength=2048).astype(np.int64)


def refine_hist(bits, level, prefix):
    key, low = (bits >> 20, (bits >> 10) & 1023) if level == 1 else (bits >> 10, bits & 1023)
    return np.bincount(low[key == prefix], minlength=1024).astype(np.int64)


def select(bits, rank):
    """The rank-th smallest (0-based) of ``bits`` as f32, through the three histograms only."""
    c = np.cumsum(level0_hist(bits))
    prefix = int(np.searchsorted(c, rank, side="right"))
    rank -= int(c[prefix - 1]) if prefix else 0
    for level in (1, 2):
        c = np.cumsum(refine_hist(bits, level, prefix))
        b = int(np.searchsorted(c, rank, side="right"))
        rank -= int(c[b - 1]) if b else 0
        prefix = (prefix << 10) | b
    return np.array([prefix], np.uint32).view(np.float32)[0]


def render(S, upper, keep_polarity):
    """S [L,3,H,W] f32, upper as the host has it (numpy scalar or python number) -> uint8 [L,H,W,3]."""
    if keep_polarity:
        x = np.stack([S[:, 0], S[:, 1], np.zeros_like(S[:, 0])], -1).astype(np.float64)
        dt = np.float64
    else:
        x = np.stack([S[:, 2]] * 3, -1)
        dt = np.float32
    u = dt(upper)
    return (np.minimum(np.maximum(x, dt(0)), u) / u * dt(255)).astype(np.uint8)


def frames(S, ceil, q, keep_polarity, percentile_from_order_stats):
    """(uint8 frames, upper) the way the device path gets them; raises IndexError when nothing is positive."""
    bits = positive_bits(S, keep_polarity)
    mult, dt = (1, np.float64) if keep_polarity else (3, np.float32)
    n = bits.size * mult
    if n == 0:
        raise IndexError("no positive value")
    upper = min(percentile_from_order_stats(n, q, lambda i: select(bits, i // mult), dt), ceil)
    return render(S, upper, keep_polarity), upper
