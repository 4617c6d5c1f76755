"""numpy f64 restatement of ``UNet.decoders[2].conv2`` + ``bn2`` + shortcut add + relu as a trainable layer (dec2_conv.py:
``Dec2Conv``) in the reference's layouts: t / res / x0 / upstream [B, 64, L, H, W], weight [64, 64, 3, 3, 3].  The forms are
those of tests/last_conv_ref.py with the channel count read from the weight; every product and sum is f64.  Also the
loader of tests/golden/.dec2conv (tests/make_dec2_conv_goldens.py)."""
import os

import numpy as np
import torch

from tests import convn_ref as N
from tests.last_conv_dgrad_ref import load_parts
from tests.last_conv_ref import conv, param_bounds, param_grads, ulp32  # noqa: F401  (channel-generic; shared with the tests)

C, TAPS = 64, 27
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", ".dec2conv")
CASES = {"b2_l3_5x7": (2, 3, 5, 7),            # batch and frame boundaries, one-row last tile
         "b1_l2_3x70": (1, 2, 3, 70)}          # pitch 96: padding columns; a ragged second column tile
CONSTS = ("weight_bar", "u", "v", "bn_weight", "bn_bias", "running_mean", "running_var", "eps")
GRADS = ("d_weight_bar", "d_bn_weight", "d_bn_bias", "d_t", "d_res")


def load_case(name):
    """Every array of a case: tests/golden/.dec2conv/NAME.N.npz, split arrays joined."""
    z = load_parts(os.path.join(GOLD, name))
    assert z, f"no golden files for {name} under {GOLD}"
    return z


def f64_t(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))


def power_iteration(weight_bar, u, v):
    """SpectralNorm._update_u_v's one iteration in f64 -> (u', v')."""
    w = np.asarray(weight_bar, np.float64)
    w = w.reshape(w.shape[0], -1)
    v = w.T @ np.asarray(u, np.float64)
    v = v / (np.linalg.norm(v) + 1e-12)
    u = w @ v
    return u / (np.linalg.norm(u) + 1e-12), v


def effective(c, u1, v1):
    """c: the layer's constants, u1 / v1: AFTER the iteration -> (W, sigma, scale, shift) in f64."""
    wb = np.asarray(c["weight_bar"], np.float64)
    sigma = u1 @ (wb.reshape(wb.shape[0], -1) @ v1)
    scale = np.asarray(c["bn_weight"], np.float64) / np.sqrt(np.asarray(c["running_var"], np.float64) + float(c["eps"]))
    shift = np.asarray(c["bn_bias"], np.float64) - np.asarray(c["running_mean"], np.float64) * scale
    return wb / sigma, sigma, scale, shift


def forward(t, res, W, scale, shift):
    """relu(scale conv(t, W) + shift + res) in f64 -> (x0, pre-activation)."""
    pre = conv(t, W) * scale[None, :, None, None, None] + shift[None, :, None, None, None] + np.asarray(res, np.float64)
    return np.maximum(pre, 0.0), pre


def kappa_of(weight_bar, u1, v1, sigma):
    """sum |u| |W_bar| |v| / |sigma|: how an f32 evaluation of sigma magnifies its roundings."""
    wb = np.abs(np.asarray(weight_bar, np.float64))
    return float((np.abs(u1)[:, None] * wb.reshape(wb.shape[0], -1) * np.abs(v1)[None, :]).sum() / abs(sigma))


def layer_grads(c, t, res, upstream):
    """The five gradients of the layer from the header's formulas and the closed forms -> dict with the keys of GRADS, and
    x0, pre, u1, v1, sigma, scale, W, dM, d_shift, abs_dM, abs_x (the sums of |terms| of dM, and of d_t on the folded weight)."""
    u1, v1 = power_iteration(c["weight_bar"], c["u"], c["v"])
    W, sigma, scale, shift = effective(c, u1, v1)
    x0, pre = forward(t, res, W, scale, shift)
    tw = N.wgrad_truth(f64_t(t), f64_t(x0), f64_t(upstream))
    td = N.dgrad_truth(f64_t(scale[:, None, None, None, None] * W), f64_t(x0), f64_t(upstream))
    dM, d_shift = tw["d_weight"].numpy(), tw["d_shift"].numpy()
    g = param_grads(dM, d_shift, c["weight_bar"], u1, v1, sigma, scale, c["running_mean"], c["running_var"], c["eps"])
    return {"d_weight_bar": g["d_weight_bar"], "d_bn_weight": g["d_bn_weight"], "d_bn_bias": g["d_bn_bias"], "d_t": td["d_x"].numpy(),
            "d_res": td["d_res"].numpy(), "x0": x0, "pre": pre, "u1": u1, "v1": v1, "sigma": sigma, "scale": scale, "W": W, "dM": dM,
            "d_shift": d_shift, "abs_dM": tw["abs_weight"].numpy(), "abs_x": td["abs_x"].numpy()}
