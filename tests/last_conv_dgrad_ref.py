"""numpy f64 restatement of the input gradient of the last decoder convolution and of the block's other two BatchNorms
(include/v2ce_hip_convdgrad.h, last_conv.py: conv32_dgrad, TailNorms) in the reference's layouts: y / upstream / d_x / d_res
/ c1 / cd / z1 / zd [B, 32, L, H, W], weight [32, 32, 3, 3, 3].  Every product and sum is f64; nothing is rounded here."""
import glob
import os

import numpy as np

from tests import last_conv_ref as R
from tests.last_conv_ref import from_c16, masked, pitch_of, shifted, to_c16, ulp32  # noqa: F401  (shared with the tests)

C, TAPS = 32, 27
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", ".lastconv_dgrad")
KINDS = ("dx", "block")


def load_parts(base):
    """The arrays of base.0.npz, base.1.npz, ...; an array split along axis 1 into NAME@0, NAME@1, ... is joined."""
    z, parts = {}, {}
    for p in sorted(glob.glob(base + ".*.npz")):
        for k, v in np.load(p).items():
            if "@" in k:
                n, i = k.split("@")
                parts.setdefault(n, {})[int(i)] = v
            else:
                z[k] = v
    for n, d in parts.items():
        z[n] = np.concatenate([d[i] for i in sorted(d)], axis=1)
    return z


def load_case(name):
    """Every array of a case: tests/golden/.lastconv/NAME*.npz (t, y, upstream, the layer's constants) and the files of
    tests/make_last_conv_dgrad_goldens.py, NAME.dx.*.npz and NAME.block.*.npz."""
    z = R.load_case(name)
    for kind in KINDS:
        z.update(load_parts(os.path.join(GOLD, f"{name}.{kind}")))
    return z


def dgrad(weight, y, upstream):
    """The header's formulas: m = upstream where y > 0 else 0 (y None: m = upstream) -> dict d_x, d_res [B, 32, L, H, W]
    and abs_x = the sums of the absolute values of d_x's terms, all f64."""
    w = np.asarray(weight, np.float64)
    m = np.asarray(upstream, np.float64) if y is None else masked(y, upstream)
    dx, ax = np.zeros(m.shape), np.zeros(m.shape)
    for kt in range(3):
        for kh in range(3):
            for kw in range(3):
                ms = shifted(m, 2 - kt, 2 - kh, 2 - kw)             # m[b, co, l - kt + 1, h - kh + 1, w - kw + 1]
                dx += np.einsum("bolhw,oc->bclhw", ms, w[:, :, kt, kh, kw])
                ax += np.einsum("bolhw,oc->bclhw", np.abs(ms), np.abs(w[:, :, kt, kh, kw]))
    return {"d_x": dx, "d_res": m, "abs_x": ax}


def dgrad_bound(abs_terms, terms):
    """The header's bound of d_x: any order of a `terms`-term f32 sum, and the terms flushed below the normal range."""
    return (terms + 1) * 2.0 ** -24 * np.asarray(abs_terms, np.float64) + terms * 2.0 ** -126


def bc(v):
    return np.asarray(v, np.float64)[None, :, None, None, None]


def normed(c, running_mean, running_var, eps):
    """(c - mean) rsqrt(var + eps): a BatchNorm3d in eval mode without its affine part."""
    return (np.asarray(c, np.float64) - bc(running_mean)) / np.sqrt(bc(running_var) + float(eps))


def tail_forward(z1, zd, w1, b1, wd, bd):
    """TailNorms.forward: -> (t = relu(w1 z1 + b1), res = wd zd + bd, the pre-activation of t)."""
    pre = bc(w1) * np.asarray(z1, np.float64) + bc(b1)
    return np.maximum(pre, 0.0), bc(wd) * np.asarray(zd, np.float64) + bc(bd), pre


def tail_grads(z1, zd, w1, b1, d_t, d_res, active=None):
    """The gradients of TailNorms' four parameters from those of its outputs -> dict d_bn1_weight, d_bn1_bias, d_bnd_weight,
    d_bnd_bias [32] and abs_* = the sums of the absolute values of their terms.  ``active``: the relu's mask t > 0 where
    the caller has it (default: w1 z1 + b1 > 0)."""
    z1, zd = np.asarray(z1, np.float64), np.asarray(zd, np.float64)
    active = bc(w1) * z1 + bc(b1) > 0 if active is None else active
    g1 = np.where(active, np.asarray(d_t, np.float64), 0.0)
    gd = np.asarray(d_res, np.float64)
    s = lambda a: a.sum(axis=(0, 2, 3, 4))
    return {"d_bn1_weight": s(g1 * z1), "d_bn1_bias": s(g1), "d_bnd_weight": s(gd * zd), "d_bnd_bias": s(gd),
            "abs_d_bn1_weight": s(np.abs(g1 * z1)), "abs_d_bn1_bias": s(np.abs(g1)), "abs_d_bnd_weight": s(np.abs(gd * zd)),
            "abs_d_bnd_bias": s(np.abs(gd))}


def tail_bounds(z1, zd, w1, b1, e_t, e_res, active=None):
    """First-order bounds of ``tail_grads``' outputs when d_t is off by at most e_t and d_res by e_res (per element): the
    sums are linear in them, so the bound is the same form on absolute values."""
    z1, zd = np.asarray(z1, np.float64), np.asarray(zd, np.float64)
    active = bc(w1) * z1 + bc(b1) > 0 if active is None else active
    e1 = np.where(active, e_t, 0.0)
    s = lambda a: a.sum(axis=(0, 2, 3, 4))
    return {"d_bn1_weight": s(e1 * np.abs(z1)), "d_bn1_bias": s(e1), "d_bnd_weight": s(e_res * np.abs(zd)), "d_bnd_bias": s(e_res)}
