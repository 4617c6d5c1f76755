"""What the tests of v2ce_convupn_wgrad (include/v2ce_hip_convupngrad.h) share: a numpy restatement of the header's formulas
at any channel counts, the f64 torch truth on the inputs' device (x0 gathered at (h >> 1, w >> 1), concatenated with x1,
then tests/grad_walk_ref.py's per-tap sums, which do not fix the channel counts, also on absolute values for S), the
channel triples, the shapes, the seeded inputs, the header's share count and its bound.

Tensors are in the reference's layouts: x0 [B, c0, L, H0, W0], x1 [B, c1, L, H, W], g1 / gd [B, cout, L, H, W], weights as
nn.Conv3d stores them.  Nothing here is rounded."""
import numpy as np
import torch

from tests import grad_walk_ref as G
from tests.last_conv_ref import shifted, ulp32                      # noqa: F401  (ulp32: for the tests)

# (c0, c1, cout): dec2, and two triples asymmetric on both axes, so that a transposed or mis-strided group index cannot cancel
TRIPLES = ((128, 64, 64), (64, 64, 32), (128, 32, 64))
OLD = (64, 32, 32)                                                  # the triple of v2ce_hip_convupgrad.h's entry
GROUP = 32                                                          # channels of a channel group on either side
CAP = 256                                                           # workgroups of the default grid at most
PRIME_GRID = 97                                                     # max_workgroups of the walk's second run

# [B, L, H, W] -> max_workgroups as a multiple of the pair count (0: the default grid)
SMALL = {(1, 1, 1, 1): 0,
         (2, 3, 5, 7): 0,                                           # odd H and W: the last source row / column is seen once
         (1, 2, 3, 70): 0,                                          # pitch 96, ragged second column tile
         (1, 3, 6, 64): 0,                                          # exact tiles
         (1, 3, 20, 70): 1}                                         # one share of 60 tiles: a flush of the f32 chain mid-walk
WALK = (2, 3, 43, 131)                                              # 396 tiles: uneven shares at every triple's cap


def pairs_of(c0, c1, cout):
    return (cout // GROUP) * ((c0 + c1) // GROUP)


def shares(c0, c1, cout, tiles, max_workgroups=0):
    """The header's share count."""
    p = pairs_of(c0, c1, cout)
    s = min(tiles, CAP // p)
    return min(s, max(max_workgroups // p, 1)) if max_workgroups > 0 else s


def virtual_input_np(x0, x1):
    """X [B, c0 + c1, L, H, W]: X[ci] = x0[ci] at (h >> 1, w >> 1) for ci < c0, x1[ci - c0] behind them."""
    x0, x1 = np.asarray(x0), np.asarray(x1)
    H, W = x1.shape[3], x1.shape[4]
    assert x0.shape[3] == (H + 1) // 2 and x0.shape[4] == (W + 1) // 2
    return np.concatenate([x0[:, :, :, np.arange(H) >> 1][:, :, :, :, np.arange(W) >> 1], x1], axis=1)


def wgrad_np(x0, x1, g1, gd):
    """The header's formulas, term by term -> d_weight [cout, c0 + c1, 3, 3, 3], d_short [cout, c0 + c1], d_short_bias [cout]."""
    X = virtual_input_np(x0, x1).astype(np.float64)
    g, s = np.asarray(g1, np.float64), np.asarray(gd, np.float64)
    dw = np.zeros((g.shape[1], X.shape[1], 3, 3, 3))
    for kt in range(3):
        for kh in range(3):
            for kw in range(3):
                dw[:, :, kt, kh, kw] = np.einsum("bolhw,bilhw->oi", g, shifted(X, kt, kh, kw))
    return {"d_weight": dw, "d_short": np.einsum("bolhw,bilhw->oi", s, X), "d_short_bias": s.sum(axis=(0, 2, 3, 4))}


def virtual_input(x0, x1):
    """The same on torch tensors, on their device."""
    H, W = x1.shape[3], x1.shape[4]
    assert x0.shape[3] == (H + 1) // 2 and x0.shape[4] == (W + 1) // 2
    ih, iw = torch.arange(H, device=x0.device) >> 1, torch.arange(W, device=x0.device) >> 1
    return torch.cat([x0[:, :, :, ih][:, :, :, :, iw], x1], dim=1)


def wgrad_truth(x0, x1, g1, gd):
    """f64 torch on the inputs' device -> d_weight, abs_weight, d_short, abs_short, d_short_bias, abs_short_bias."""
    X = virtual_input(G.f64(x0), G.f64(x1))
    d, a = G._tap_sums(G.f64(g1), X)
    g2, X2 = G.rows(G.f64(gd)), G.rows(X)
    return {"d_weight": d, "abs_weight": a, "d_short": g2 @ X2.t(), "abs_short": g2.abs() @ X2.abs().t(),
            "d_short_bias": g2.sum(dim=1), "abs_short_bias": g2.abs().sum(dim=1)}


def inputs(shape, c0, c1, cout, exact, seed):
    """Seeded f32 inputs on the CPU.  exact: integers 1 .. 3, else standard normals."""
    B, L, H, W = shape
    gen = torch.Generator().manual_seed(seed + 7 * c0 + 3 * c1 + cout)
    draw = G.integers if exact else G.normals
    out = (B, cout, L, H, W)
    return {"x0": draw(gen, (B, c0, L, (H + 1) // 2, (W + 1) // 2)), "x1": draw(gen, (B, c1, L, H, W)), "g1": draw(gen, out),
            "gd": draw(gen, out)}


def bound(truth, abs_terms, n_pos, chain):
    """The header's bound of d_weight and d_short: one f32 rounding, an fmaf chain of at most `chain` positions, N f64
    additions."""
    return ulp32(truth) + chain * 2.0 ** -24 * np.asarray(abs_terms) + n_pos * 2.0 ** -52 * np.asarray(abs_terms)
