"""What the tests of v2ce_convn_wgrad / v2ce_convn_dgrad (include/v2ce_hip_convngrad.h) share: a numpy restatement of the
header's formulas at any channel counts, the f64 torch truths (one matmul per tap: tests/grad_walk_ref.py's `_tap_sums` and
`_tap_transposed`, which do not fix the channel counts), the shapes, the seeded inputs and the header's bounds.

Activations are in the reference's layout [B, C, L, H, W], weights as nn.Conv3d stores them.  Nothing here is rounded."""
import numpy as np
import torch

from tests import grad_walk_ref as G
from tests.last_conv_ref import shifted, ulp32                      # noqa: F401  (ulp32: for the tests)

PAIRS = ((64, 64), (64, 32), (32, 64))                               # (cin, cout); the asymmetric ones catch a transposed group
GROUP = 32                                                          # channels of a channel group on either side
CAP = 256                                                           # workgroups of the default grids at most
PRIME_GRID = 97                                                     # max_workgroups of the walk's second run

# [B, L, H, W] -> max_workgroups as a multiple of the pair count (0: the default grid)
SMALL = {(1, 1, 1, 1): 0,
         (2, 3, 5, 7): 0,                                           # batch and frame boundaries, one-row last tile
         (1, 2, 3, 70): 0,                                          # ragged second column tile
         (1, 2, 4, 65): 0,                                          # one-column last tile
         (1, 3, 6, 64): 0,                                          # exact tiles
         (1, 3, 20, 70): 1}                                         # one share of 60 tiles: a flush of the f32 chain mid-walk
WALK = (2, 3, 43, 131)                                              # 396 tiles: uneven shares at 256, 128 and 64 shares


def to_c16_np(a, pitch=None, fill=np.nan):
    """[B, 16 G, L, H, W] -> channels-last-16 [B, L, G, H, pitch, 16] f32 (numpy), padding columns filled with `fill`."""
    f = np.asarray(a, np.float32)
    B, Cx, L, H, W = f.shape
    pitch = W if pitch is None else pitch
    out = np.full((B, L, Cx // 16, H, pitch, 16), fill, np.float32)
    out[:, :, :, :, :W, :] = f.reshape(B, Cx // 16, 16, L, H, W).transpose(0, 3, 1, 4, 5, 2)
    return out


def pairs_of(cin, cout):
    return (cin // GROUP) * (cout // GROUP)


def wgrad_shares(cin, cout, tiles, max_workgroups=0):
    """The header's share count of v2ce_convn_wgrad."""
    p = pairs_of(cin, cout)
    s = min(tiles, CAP // p)
    return min(s, max(max_workgroups // p, 1)) if max_workgroups > 0 else s


def dgrad_shares(cin, tiles, max_workgroups=0):
    """The header's share count of v2ce_convn_dgrad."""
    g = cin // GROUP
    s = min(tiles, CAP // g)
    return min(s, max(max_workgroups // g, 1)) if max_workgroups > 0 else s


def masked_np(y, upstream):
    u = np.asarray(upstream, np.float64)
    return u if y is None else np.where(np.asarray(y) > 0, u, 0.0)


def wgrad_np(x, y, upstream):
    """The header's formulas of v2ce_convn_wgrad, term by term -> d_weight [cout, cin, 3, 3, 3], d_shift [cout]."""
    x, m = np.asarray(x, np.float64), masked_np(y, upstream)
    dw = np.zeros((m.shape[1], x.shape[1], 3, 3, 3))
    for kt in range(3):
        for kh in range(3):
            for kw in range(3):
                dw[:, :, kt, kh, kw] = np.einsum("bolhw,bilhw->oi", m, shifted(x, kt, kh, kw))
    return {"d_weight": dw, "d_shift": m.sum(axis=(0, 2, 3, 4))}


def dgrad_np(weight, y, upstream):
    """The header's formulas of v2ce_convn_dgrad -> d_x [B, cin, L, H, W], d_res [B, cout, L, H, W]."""
    w, m = np.asarray(weight, np.float64), masked_np(y, upstream)
    dx = np.zeros((m.shape[0], w.shape[1]) + m.shape[2:])
    for kt in range(3):
        for kh in range(3):
            for kw in range(3):
                dx += np.einsum("oi,bolhw->bilhw", w[:, :, kt, kh, kw], shifted(m, 2 - kt, 2 - kh, 2 - kw))
    return {"d_x": dx, "d_res": m}


def wgrad_truth(x, y, upstream):
    """f64 torch on the inputs' device -> d_weight, d_shift, abs_weight, abs_shift."""
    return G.conv32_wgrad(x, y, upstream)            # (the name is historical: the sums take any channel counts)


def dgrad_truth(weight, y, upstream):
    """f64 torch on the inputs' device -> d_x, d_res, abs_x."""
    return G.conv32_dgrad(weight, y, upstream)


def inputs(shape, cin, cout, exact, seed):
    """Seeded f32 inputs on the CPU.  exact: integers 1 .. 3 and a normal y with signed zeros, else standard normals."""
    B, L, H, W = shape
    gen = torch.Generator().manual_seed(seed + 7 * cin + cout)
    draw = G.integers if exact else G.normals
    out = (B, cout, L, H, W)
    return {"x": draw(gen, (B, cin, L, H, W)), "upstream": draw(gen, out),
            "y": G.signed_zero_normals(gen, out) if exact else G.normals(gen, out), "weight": draw(gen, (cout, cin, 3, 3, 3))}


def wgrad_bound(truth, abs_terms, n_pos, chain):
    """The header's bound of d_weight."""
    return ulp32(truth) + chain * 2.0 ** -24 * np.asarray(abs_terms) + n_pos * 2.0 ** -52 * np.asarray(abs_terms)


def dgrad_bound(abs_terms, cout):
    """The header's bound of d_x: (27 cout + 1) 2^-24 S + 27 cout 2^-126."""
    return (27 * cout + 1) * 2.0 ** -24 * np.asarray(abs_terms, np.float64) + 27 * cout * 2.0 ** -126
