"""What the tests of v2ce_convupn_dgrad (include/v2ce_hip_convupndgrad.h) share: a numpy f64 restatement of the header's
formulas with (c0, c1, cout) as arguments, the channel triples, the seeded inputs, the bound and the layout helpers.

Tensors are in the reference's layouts: g1 / gd [B, cout, L, H, W], d_x1 [B, c1, L, H, W], d_x0 [B, c0, L, H0, W0], weight
[cout, c0 + c1, 3, 3, 3], short_weight [cout, c0 + c1].  Every product and sum is f64; nothing is rounded here.  No
goldens: the inputs come from seeded generators and the truths are computed in the tests (cached with lru_cache)."""
import functools
import itertools

import numpy as np

from tests.last_block_dgrad_ref import dgrad_bound, pooled           # noqa: F401  (shared with the tests)
from tests.last_block_ref import src_to_c16 as to_c16                # [B, C, L, H, W] -> [B, L, C / 16, H, pitch, 16], any C
from tests.last_conv_ref import shifted, ulp32                       # noqa: F401

C0S, C1S, COUTS = (64, 128), (32, 64), (32, 64)
TRIPLES = tuple(itertools.product(C0S, C1S, COUTS))                  # all eight
DEC2, OLD = (128, 64, 64), (64, 32, 32)
UNITS = 28                                                           # 27 taps and the shortcut
# the integer data of the bit-for-bit check: |g| <= G_TOP, |w| <= W_TOP
G_TOP, W_TOP = 8, 4


def terms(cout):
    """V2CE_UPNDGRAD_TERMS(cout)."""
    return UNITS * cout


def from_c16(c16, lw):
    """channels-last-16 [B, L, G, H, pitch, 16] -> [B, 16 G, L, H, lw]."""
    c = np.asarray(c16)
    B, L, G, H, _, _ = c.shape
    return np.ascontiguousarray(c[:, :, :, :, :lw, :].transpose(0, 2, 5, 1, 3, 4).reshape(B, G * 16, L, H, lw))


def dgrad(c0, c1, cout, weight, short_weight, g1, gd):
    """The header's formulas -> dict d_X [B, c0 + c1, L, H, W], d_x0 [B, c0, L, H0, W0], d_x1 [B, c1, L, H, W], abs_x0 /
    abs_x1 = the sums of the absolute values of their terms, n_x0 = the number of output positions of each source pixel
    [H0, W0], all f64.  g1 or gd None: its share is left out."""
    ref = g1 if g1 is not None else gd
    B, co, L, H, W = ref.shape
    cin = c0 + c1
    assert co == cout
    dX, aX = np.zeros((B, cin, L, H, W)), np.zeros((B, cin, L, H, W))
    if g1 is not None:
        w, g = np.asarray(weight, np.float64), np.asarray(g1, np.float64)
        assert w.shape == (cout, cin, 3, 3, 3)
        for kt in range(3):
            for kh in range(3):
                for kw in range(3):
                    gs = shifted(g, 2 - kt, 2 - kh, 2 - kw)         # g1[b, co, l - kt + 1, h - kh + 1, w - kw + 1]
                    dX += np.einsum("bolhw,oc->bclhw", gs, w[:, :, kt, kh, kw], optimize=True)
                    aX += np.einsum("bolhw,oc->bclhw", np.abs(gs), np.abs(w[:, :, kt, kh, kw]), optimize=True)
    if gd is not None:
        s, g = np.asarray(short_weight, np.float64).reshape(cout, cin), np.asarray(gd, np.float64)
        dX += np.einsum("bolhw,oc->bclhw", g, s)
        aX += np.einsum("bolhw,oc->bclhw", np.abs(g), np.abs(s))
    n = pooled(np.ones((1, 1, 1, H, W)))[0, 0, 0]
    return {"d_X": dX, "d_x0": pooled(dX[:, :c0]), "d_x1": dX[:, c0:], "abs_x0": pooled(aX[:, :c0]), "abs_x1": aX[:, c0:], "n_x0": n}


def bounds(cout, abs_x0, abs_x1):
    """The header's bound per element of d_x0 and d_x1 -> {"x0": ..., "x1": ...}."""
    H, W = abs_x1.shape[3], abs_x1.shape[4]
    n0 = terms(cout) * pooled(np.ones((1, 1, 1, H, W)))
    return {"x0": dgrad_bound(abs_x0, n0), "x1": dgrad_bound(abs_x1, terms(cout))}


@functools.lru_cache(maxsize=None)
def inputs(shape, c0, c1, cout, kind="normal", seed=0):
    """Seeded f32 inputs -> dict kw [cout, cin, 3, 3, 3], ks [cout, cin], g1, gd [B, cout, L, H, W] (read-only arrays).
    kind: 'normal' (standard normals, weights scaled by 1 / 8), 'int' (integers in [-G_TOP, G_TOP] and [-W_TOP, W_TOP]:
    every sum of the kernel is exact), 'zero'."""
    B, L, H, W = shape
    cin = c0 + c1
    rng = np.random.default_rng([seed, c0, c1, cout, B, L, H, W])
    out = (B, cout, L, H, W)
    if kind == "int":
        z = {"kw": rng.integers(-W_TOP, W_TOP + 1, (cout, cin, 3, 3, 3)), "ks": rng.integers(-W_TOP, W_TOP + 1, (cout, cin)),
             "g1": rng.integers(-G_TOP, G_TOP + 1, out), "gd": rng.integers(-G_TOP, G_TOP + 1, out)}
    else:
        z = {"kw": rng.standard_normal((cout, cin, 3, 3, 3)) / 8, "ks": rng.standard_normal((cout, cin)) / 8,
             "g1": rng.standard_normal(out), "gd": rng.standard_normal(out)}
        if kind == "zero":
            z["g1"], z["gd"] = np.zeros(out), np.zeros(out)
    z = {k: np.ascontiguousarray(v, np.float32) for k, v in z.items()}
    for v in z.values():
        v.setflags(write=False)
    return z


@functools.lru_cache(maxsize=None)
def truth(shape, c0, c1, cout, kind="normal", seed=0):
    """``dgrad`` of ``inputs`` (read-only arrays)."""
    z = inputs(shape, c0, c1, cout, kind, seed)
    t = dgrad(c0, c1, cout, z["kw"], z["ks"], z["g1"], z["gd"])
    for v in t.values():
        v.setflags(write=False)
    return t
