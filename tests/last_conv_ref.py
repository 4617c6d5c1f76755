"""numpy f64 restatement of the last decoder convolution as a trainable layer (include/v2ce_hip_convgrad.h, last_conv.py)
in the reference's layouts: t / res / feat / upstream [B, 32, L, H, W], weight [32, 32, 3, 3, 3].  Every product and sum is
f64; nothing is rounded here.  The layout helpers of tests/pred_head_ref.py convert to and from the kernels' tensors."""
import os

import numpy as np

from tests.pred_head_ref import from_c16, masked, pitch_of, to_c16, ulp32  # noqa: F401  (shared with the tests)

C, TAPS = 32, 27
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", ".lastconv")


def load_case(name):
    """Every array of a case of tests/make_last_conv_goldens.py: NAME.npz and its companions merged."""
    z = {}
    for sfx in ("", ".plain", ".layer", ".truth"):
        p = os.path.join(GOLD, f"{name}{sfx}.npz")
        if os.path.exists(p):
            z.update(np.load(p))
    return z


def shifted(x, kt, kh, kw):
    """x[b, c, l + kt - 1, h + kh - 1, w + kw - 1] with zeros outside the tensor: the zero-padded input a tap sees."""
    x = np.asarray(x)
    B, Cx, L, H, W = x.shape
    p = np.zeros((B, Cx, L + 2, H + 2, W + 2), x.dtype)
    p[:, :, 1:L + 1, 1:H + 1, 1:W + 1] = x
    return p[:, :, kt:kt + L, kh:kh + H, kw:kw + W]


def conv(x, weight):
    """The stride-1, zero-padded 3x3x3 convolution in f64 -> [B, 32, L, H, W]."""
    x, w = np.asarray(x, np.float64), np.asarray(weight, np.float64)
    z = np.zeros((x.shape[0], w.shape[0]) + x.shape[2:], np.float64)
    for kt in range(3):
        for kh in range(3):
            for kw in range(3):
                z += np.einsum("bclhw,oc->bolhw", shifted(x, kt, kh, kw), w[:, :, kt, kh, kw])
    return z


def wgrad(x, y, upstream):
    """The header's formulas: m = upstream where y > 0 else 0 (y None: m = upstream) -> dict d_weight [32, 32, 3, 3, 3],
    d_shift [32], and abs_weight / abs_shift = the sums of the absolute values of their terms, all f64."""
    x = np.asarray(x, np.float64)
    m = np.asarray(upstream, np.float64) if y is None else masked(y, upstream)
    dw, aw = np.zeros((C, C, 3, 3, 3)), np.zeros((C, C, 3, 3, 3))
    for kt in range(3):
        for kh in range(3):
            for kw in range(3):
                xs = shifted(x, kt, kh, kw)
                dw[:, :, kt, kh, kw] = np.einsum("bolhw,bclhw->oc", m, xs)
                aw[:, :, kt, kh, kw] = np.einsum("bolhw,bclhw->oc", np.abs(m), np.abs(xs))
    return {"d_weight": dw, "d_shift": m.sum(axis=(0, 2, 3, 4)), "abs_weight": aw, "abs_shift": np.abs(m).sum(axis=(0, 2, 3, 4))}


def power_iteration(weight_bar, u, v, dtype=np.float64):
    """SpectralNorm._update_u_v's one iteration in `dtype` -> (u', v')."""
    w = np.asarray(weight_bar, dtype).reshape(C, -1)
    v = w.T @ np.asarray(u, dtype)
    v = v / (np.linalg.norm(v) + dtype(1e-12))
    u = w @ v
    u = u / (np.linalg.norm(u) + dtype(1e-12))
    return u.astype(dtype), v.astype(dtype)


def effective(weight_bar, u, v, bn_weight, bn_bias, running_mean, running_var, eps):
    """u, v: AFTER the iteration -> (W, sigma, scale, shift) in f64."""
    wb = np.asarray(weight_bar, np.float64)
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    sigma = u @ (wb.reshape(C, -1) @ v)
    scale = np.asarray(bn_weight, np.float64) / np.sqrt(np.asarray(running_var, np.float64) + float(eps))
    shift = np.asarray(bn_bias, np.float64) - np.asarray(running_mean, np.float64) * scale
    return wb / sigma, sigma, scale, shift


def forward(t, res, W, scale, shift):
    """relu(scale conv(t, W) + shift + res) in f64 -> (feat, pre-activation)."""
    pre = conv(t, W) * scale[None, :, None, None, None] + shift[None, :, None, None, None] + np.asarray(res, np.float64)
    return np.maximum(pre, 0.0), pre


def param_grads(dM, d_shift, weight_bar, u, v, sigma, scale, running_mean, running_var, eps):
    """The closed forms behind LastConv's backward, from the kernel's raw outputs (u, v after the iteration, constants):
        dW = scale[co] dM[co];  d_scale[co] = <W[co], dM[co]>;
        d_weight_bar = dW / sigma - (<dW, W_bar> / sigma^2) u v^T        (W = W_bar / sigma, sigma = u . W_bar v)
        d_bn_weight = (d_scale - running_mean d_shift) / sqrt(running_var + eps);  d_bn_bias = d_shift."""
    wb = np.asarray(weight_bar, np.float64)
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    dM = np.asarray(dM, np.float64)
    dW = scale[:, None, None, None, None] * dM
    d_scale = (wb / sigma * dM).sum(axis=(1, 2, 3, 4))
    d_wb = dW / sigma - ((dW * wb).sum() / sigma ** 2) * np.outer(u, v).reshape(wb.shape)
    rs = 1.0 / np.sqrt(np.asarray(running_var, np.float64) + float(eps))
    d_bn_w = (d_scale - np.asarray(running_mean, np.float64) * np.asarray(d_shift, np.float64)) * rs
    return {"d_weight_bar": d_wb, "d_bn_weight": d_bn_w, "d_bn_bias": np.asarray(d_shift, np.float64), "dW": dW, "d_scale": d_scale}


def param_bounds(e_dM, e_shift, weight_bar, u, v, sigma, scale, running_mean, running_var, eps):
    """First-order bounds of the errors of ``param_grads``' outputs when dM is off by at most e_dM (per element) and
    d_shift by e_shift: the closed forms are linear in dM and d_shift, so the bound is the same form on absolute values."""
    wb = np.abs(np.asarray(weight_bar, np.float64))
    a_scale = np.abs(scale)[:, None, None, None, None]
    e_dW = a_scale * e_dM
    e_wb = e_dW / abs(sigma) + ((e_dW * wb).sum() / sigma ** 2) * np.abs(np.outer(u, v)).reshape(wb.shape)
    e_scale = (wb / abs(sigma) * e_dM).sum(axis=(1, 2, 3, 4))
    rs = 1.0 / np.sqrt(np.asarray(running_var, np.float64) + float(eps))
    return {"d_weight_bar": e_wb, "d_bn_weight": (e_scale + np.abs(running_mean) * e_shift) * rs, "d_bn_bias": e_shift}


def wgrad_bound(truth, abs_terms, n_pos, chain):
    """The header's bound of d_weight: one f32 rounding, an fmaf chain of at most `chain` positions, N f64 additions."""
    return ulp32(truth) + chain * 2.0 ** -24 * abs_terms + n_pos * 2.0 ** -52 * abs_terms
