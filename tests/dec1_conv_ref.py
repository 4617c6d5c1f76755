"""The f64 restatement of ``UNet.decoders[1].conv2`` + ``bn2`` + shortcut add + relu as a trainable layer (dec1_conv.py:
``Dec1Conv``) and the loader of tests/golden/.dec1conv (tests/make_dec1_conv_goldens.py).  The restatement is that of
tests/dec2_conv_ref.py, which reads the channel count from the weight: t / res / h1 / upstream [B, 128, L, H, W], weight
[128, 128, 3, 3, 3]; every product and sum is f64."""
import os

from tests.dec2_conv_ref import (CASES, CONSTS, GRADS, TAPS, conv, effective, f64_t, forward, kappa_of, layer_grads,  # noqa: F401
                                 param_bounds, param_grads, power_iteration, ulp32)
from tests.last_conv_dgrad_ref import load_parts

C = 128
COLS = C * TAPS                                # 3456 columns of the weight as a matrix
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", ".dec1conv")
SHARED = "consts"                              # the constants' files: one set for both cases
DIR_CAP = 9_000_000                            # bytes of the whole directory at most


def load_case(name):
    """Every array of a case: the constants shared by the cases (tests/golden/.dec1conv/consts.N.npz) and NAME.N.npz, split
    arrays joined."""
    z = load_parts(os.path.join(GOLD, SHARED))
    assert z and set(z) == set(CONSTS), f"no constants under {GOLD}"
    case = load_parts(os.path.join(GOLD, name))
    assert case and not set(case) & set(z), f"no golden files for {name} under {GOLD}"
    z.update(case)
    return z
