"""NumPy restatement of the arithmetic of v2ce_physatt_batch / v2ce_log_residual_batch (csrc/physatt.hip): what the
kernels do, operation by operation, in the order they do it.  It shares no code with the reference's
train/scripts/utils/physical_att.py (whose results are the fixtures under tests/golden/.physatt); the CPU test holds it
to those bytes, the GPU test holds the kernels to it at shapes the fixtures do not cover.

Every step is float32 with separately rounded operations, except the two blur passes, which accumulate in float64."""
import math

import numpy as np

EVENT_DTYPE = np.dtype([("timestamp", "<i8"), ("x", "<i2"), ("y", "<i2"), ("polarity", "i1")])
GOLDEN_NAMES = ("ragged_19x27_p8", "r21x40_p4", "r33x50_p16", "no_events", "equal_frames", "counts_3_and_4",
                "crowd_70000", "all_equal_ratio", "mask_tie", "full_260x346_p8")
LFR_GOLDEN = "lfr_values"
F = np.float32


def lin_log_lut(offset):
    """float32 [256]: the reference's lin_log (v2e_utils.py:5-43) of v + offset for the 256 values of a uint8 pixel."""
    x = np.arange(256, dtype=np.float64) + offset
    f = (1.0 / 20) * math.log(20)
    x = x + 1e-8
    y = np.where(x <= 20, x * f, np.log(x))
    return (np.round(y * 1e8) / 1e8).astype(np.float32)


def gauss_weights():
    """float64 [5]: exp(-0.5 k^2) / sum over k = -4 .. 4, for k = 0 .. 4 (scipy's sigma = 1, truncate = 4)."""
    k = np.arange(-4, 5)
    phi = np.exp(-0.5 * k ** 2)
    phi = phi / phi.sum()
    return phi[4:].copy()


def _row_sums(x):
    """float32 sums over the last axis (one block row each) in the order of NumPy's pairwise inner loop (n <= 16: no
    recursion), every add an elementwise float32 operation."""
    n = x.shape[-1]
    if n < 8:
        s = np.zeros(x.shape[:-1], np.float32)
        for j in range(n):
            s = s + x[..., j]
        return s
    r = [x[..., j] for j in range(8)]
    k = 8
    while k + 8 <= n:
        r = [r[j] + x[..., k + j] for j in range(8)]
        k += 8
    s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for j in range(k, n):
        s = s + x[..., j]
    return s


def patch_mean(img, ps):
    """float32 [Hp, Wp]: zero-padded block mean of a float32 image, row sums added in row order, then / ps^2."""
    H, W = img.shape
    Hp, Wp = -(-H // ps), -(-W // ps)
    pad = np.zeros((Hp * ps, Wp * ps), np.float32)
    pad[:H, :W] = img
    rows = _row_sums(pad.reshape(Hp, ps, Wp, ps).transpose(0, 2, 1, 3))       # [Hp, Wp, ps]
    s = np.zeros((Hp, Wp), np.float32)
    for r in range(ps):
        s = s + rows[..., r]
    return s / F(ps * ps)


def count_patches(x, y, H, W, ps):
    """float32 [Hp, Wp]: events per patch / ps^2 (exact integers below 2^24, one rounding in the division)."""
    Hp, Wp = -(-H // ps), -(-W // ps)
    cell = (np.asarray(y, np.int64) // ps) * Wp + np.asarray(x, np.int64) // ps
    cnt = np.bincount(cell, minlength=Hp * Wp).reshape(Hp, Wp)
    assert cnt.max(initial=0) < 1 << 24
    return cnt.astype(np.float32) / F(ps * ps)


def _reflect(i, n):
    m = i % (2 * n)
    return m if m < n else 2 * n - 1 - m


def blur_axis(a, axis, w):
    """One pass of scipy's correlate1d with symmetric weights, mode reflect: float64 accumulation from the centre tap,
    then the tap pairs from the outermost inwards; float32 store."""
    a = np.moveaxis(a, axis, 0)
    n = a.shape[0]
    out = np.empty_like(a)
    a64 = a.astype(np.float64)
    for i in range(n):
        t = a64[i] * w[0]
        for j in range(4, 0, -1):
            t = t + (a64[_reflect(i - j, n)] + a64[_reflect(i + j, n)]) * w[j]
        out[i] = t.astype(np.float32)
    return np.moveaxis(out, 0, axis)


def _delta(frames, lut):
    return np.abs(lut[frames[1]] - lut[frames[0]])


def attention(x, y, frames, ps, ceiling, advanced):
    """physical_attention_generation (advanced=False) / _advanced: float32 [Hp, Wp]."""
    H, W = frames.shape[1:]
    ev = count_patches(x, y, H, W, ps)
    ev[ev < F(0.05)] = 0
    d = patch_mean(_delta(frames, lin_log_lut(1e-6)), ps)
    r = ev / (d + F(1e-3))
    r = np.minimum(np.maximum(r, F(0)), F(2 * ceiling))
    r = blur_axis(blur_axis(r, 0, gauss_weights()), 1, gauss_weights())
    r = np.minimum(np.maximum(r, F(0)), F(ceiling))
    lo, hi = r.min(), r.max()
    if hi == lo:
        return np.zeros_like(r)
    return (r - lo) / (hi - lo) if advanced else r / F(ceiling)


def ratio_map(x, y, frames, ps, threshold):
    """The ratio_map of physical_mask_generation: float32 [Hp, Wp]."""
    H, W = frames.shape[1:]
    ev = count_patches(x, y, H, W, ps)
    d = patch_mean(_delta(frames, lin_log_lut(1e-6)) / F(threshold), ps)
    return ev / (d + F(1e-6)) - F(1)


def top_k_mask(r, K):
    return r >= np.sort(r.reshape(-1))[-K]


def log_residual(frames):
    """gen_log_frame_residual_batch: float32 [N-1, 1, H, W]."""
    lut = lin_log_lut(0.0)
    v = lut[frames]
    return (v[1:] - v[:-1])[:, None]
