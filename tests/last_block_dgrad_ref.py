"""numpy f64 restatement of the input gradients of the last decoder block's conv1 and shortcut back through the concat and
the 2x nearest upsample (include/v2ce_hip_convupdgrad.h, last_block.py: convup_dgrad) in the reference's layouts: g1 / gd /
d_x1 [B, 32, L, H, W], d_x0 [B, 64, L, H0, W0], weight [32, 96, 3, 3, 3], short_weight [32, 96].  Every product and sum is
f64; nothing is rounded here.  The layout helpers of tests/last_block_ref.py convert to and from the kernels' tensors."""
import os

import numpy as np

from tests import last_block_ref as R
from tests.last_conv_dgrad_ref import load_parts
from tests.last_conv_ref import shifted
from tests.last_block_ref import from_c16, pitch_of, src_to_c16, to_c16, ulp32  # noqa: F401  (shared with the tests)

C, C0, C1, CIN, TAPS = 32, 64, 32, 96, 27
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", ".lastblock_dgrad")
NEW_CASES = {"b1_l2_4x65": (1, 2, 4, 65)}         # the case tests/golden/.lastblock lacks: its inputs are in .lastblock_dgrad


def load_case(name):
    """Every array of a case: the committed inputs of tests/golden/.lastblock (x0, x1, g1, gd, the block's constants; a
    NEW_CASES name has its g1 and gd among this maker's files) and the files of tests/make_last_block_dgrad_goldens.py,
    NAME.k.*.npz (the kernel truths) and NAME.layer.*.npz (the reference block's input gradients)."""
    z = {} if name in NEW_CASES else R.load_case(name)
    z.update(load_parts(os.path.join(GOLD, "weights.k")))           # kw, ks: the kernel truths' weights, shared by the cases
    for kind in ("k", "layer"):
        z.update(load_parts(os.path.join(GOLD, f"{name}.{kind}")))
    return z


def pooled(d_up):
    """The backward of the nearest upsample at h >> 1, w >> 1: [B, C, L, H, W] -> [B, C, L, (H + 1) // 2, (W + 1) // 2], a
    source pixel collecting the output positions that exist."""
    B, Cx, L, H, W = d_up.shape
    out = np.zeros((B, Cx, L, (H + 1) // 2, (W + 1) // 2))
    for dh in range(2):
        for dw in range(2):
            part = d_up[:, :, :, dh::2, dw::2]
            out[:, :, :, :part.shape[3], :part.shape[4]] += part
    return out


def dgrad(weight, short_weight, g1, gd):
    """The header's formulas -> dict d_X [B, 96, L, H, W], d_x0 [B, 64, L, H0, W0], d_x1 [B, 32, L, H, W], abs_x0 / abs_x1 =
    the sums of the absolute values of their terms, n_x0 = the number of output positions of each source pixel [H0, W0], all
    f64.  g1 or gd None: its share is left out."""
    ref = g1 if g1 is not None else gd
    B, _, L, H, W = ref.shape
    dX, aX = np.zeros((B, CIN, L, H, W)), np.zeros((B, CIN, L, H, W))
    if g1 is not None:
        w, g = np.asarray(weight, np.float64), np.asarray(g1, np.float64)
        for kt in range(3):
            for kh in range(3):
                for kw in range(3):
                    gs = shifted(g, 2 - kt, 2 - kh, 2 - kw)         # g1[b, co, l - kt + 1, h - kh + 1, w - kw + 1]
                    dX += np.einsum("bolhw,oc->bclhw", gs, w[:, :, kt, kh, kw])
                    aX += np.einsum("bolhw,oc->bclhw", np.abs(gs), np.abs(w[:, :, kt, kh, kw]))
    if gd is not None:
        s, g = np.asarray(short_weight, np.float64).reshape(C, CIN), np.asarray(gd, np.float64)
        dX += np.einsum("bolhw,oc->bclhw", g, s)
        aX += np.einsum("bolhw,oc->bclhw", np.abs(g), np.abs(s))
    n = pooled(np.ones((1, 1, 1, H, W)))[0, 0, 0]
    return {"d_X": dX, "d_x0": pooled(dX[:, :C0]), "d_x1": dX[:, C0:], "abs_x0": pooled(aX[:, :C0]), "abs_x1": aX[:, C0:], "n_x0": n}


def dgrad_bound(abs_terms, n):
    """The header's bound: any order of an `n`-term f32 sum (n an integer or an array that broadcasts against abs_terms), and
    the terms flushed below the normal range."""
    n = np.asarray(n, np.float64)
    return (n + 1) * 2.0 ** -24 * np.asarray(abs_terms, np.float64) + n * 2.0 ** -126
