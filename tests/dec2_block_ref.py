"""numpy / torch f64 restatement of the whole third decoder block, ``ResidualBlock3D(192, 64, norm='BN', sn=True)`` in
``.eval()`` on X = cat(upsample(x0), x1), as the trainable layer ``Dec2Block`` (dec2_block.py) composes it, in the reference's
layouts: x0 [B, 128, L, H0, W0], x1 [B, 64, L, H, W], everything behind them [B, 64, L, H, W].  The forms are those of
tests/last_block_ref.py with the channel counts read from the tensors; the sums over the positions are the f64 truths of
tests/convupn_ref.py and tests/convn_ref.py.  Every product and sum is f64; nothing is rounded here.  Also the loader of
tests/golden/.dec2block (tests/make_dec2_block_goldens.py)."""
import os

import numpy as np
import torch

from tests import convn_ref as N
from tests import convupn_ref as U
from tests import dec2_conv_ref as D2
from tests.last_conv_dgrad_ref import bc, load_parts, tail_grads
from tests.last_conv_ref import conv, param_bounds, param_grads, ulp32  # noqa: F401  (channel-generic; shared with the tests)

C, C0, C1, CIN, TAPS = 64, 128, 64, 192, 27
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", ".dec2block")
MARGIN = 1e-4
CASES = {"b2_l3_5x7": (2, 3, 5, 7),            # batch and frame boundaries, odd H and W: the last source row / column seen once
         "b1_l2_3x70": (1, 2, 3, 70)}          # pitch 96: padding columns; a ragged second column tile
PARAMS = ("weight_bar1", "u1", "v1", "short_weight", "short_bias", "bn1_weight", "bn1_bias", "bn1_mean", "bn1_var", "bnd_weight",
          "bnd_bias", "bnd_mean", "bnd_var", "weight_bar2", "u2", "v2", "bn2_weight", "bn2_bias", "bn2_mean", "bn2_var", "eps")
# the gradients the reference block's autograd gives, in the goldens' names
BLOCK_GRADS = ("d_weight_bar1", "d_short_weight", "d_short_bias", "d_bn1_weight", "d_bn1_bias", "d_bnd_weight", "d_bnd_bias",
               "d_weight_bar2", "d_bn2_weight", "d_bn2_bias")
# the second case keeps conv1's weight_bar gradient for the X groups 3 and 4 only, the seam of the concat (input channels
# 96 .. 159: the last 32 of x0 and the first 32 of x1); the first case and the kernel tests cover the rest
SEAM = slice(96, 160)
SEAM_ONLY = {"b1_l2_3x70": ("d_weight_bar1",)}


def load_case(name):
    """Every array of a case: the constants shared by the cases (tests/golden/.dec2block/consts.N.npz) and NAME.N.npz, split
    arrays joined."""
    z = load_parts(os.path.join(GOLD, "consts"))
    z.update(load_parts(os.path.join(GOLD, name)))
    assert "x0" in z and "weight_bar1" in z, f"no golden files for {name} under {GOLD}"
    return z


def f64_t(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))


def conv1x1(x, weight):
    w = np.asarray(weight, np.float64)
    return np.einsum("bclhw,oc->bolhw", np.asarray(x, np.float64), w.reshape(w.shape[0], -1))


def second_half(p):
    """The constants of conv2 + bn2 under the names tests/dec2_conv_ref.py uses."""
    return {"weight_bar": p["weight_bar2"], "u": p["u2"], "v": p["v2"], "bn_weight": p["bn2_weight"], "bn_bias": p["bn2_bias"],
            "running_mean": p["bn2_mean"], "running_var": p["bn2_var"], "eps": p["eps"]}


def block_forward(x0, x1, p):
    """The block in f64 from the constants `p` (PARAMS; u / v BEFORE the call) -> dict: X; the iterated u1a, v1a, u2a, v2a;
    sigma1, W1 = weight_bar1 / sigma1, rs1, rsd; c1, cd (the raw convolutions, cd with its bias), z1, zd (normalised), pre1,
    t = relu(pre1), res; sigma2, W2, scale2, shift2; pre, out = relu(pre)."""
    eps = float(p["eps"])
    X = U.virtual_input_np(x0, x1).astype(np.float64)
    u1a, v1a = D2.power_iteration(p["weight_bar1"], p["u1"], p["v1"])
    wb1 = np.asarray(p["weight_bar1"], np.float64)
    sigma1 = u1a @ (wb1.reshape(C, -1) @ v1a)
    W1 = wb1 / sigma1
    rs1 = 1.0 / np.sqrt(np.asarray(p["bn1_var"], np.float64) + eps)
    rsd = 1.0 / np.sqrt(np.asarray(p["bnd_var"], np.float64) + eps)
    c1 = conv(X, W1)
    cd = conv1x1(X, p["short_weight"]) + bc(p["short_bias"])
    z1, zd = (c1 - bc(p["bn1_mean"])) * bc(rs1), (cd - bc(p["bnd_mean"])) * bc(rsd)
    pre1 = bc(p["bn1_weight"]) * z1 + bc(p["bn1_bias"])
    t, res = np.maximum(pre1, 0.0), bc(p["bnd_weight"]) * zd + bc(p["bnd_bias"])
    c2 = second_half(p)
    u2a, v2a = D2.power_iteration(c2["weight_bar"], c2["u"], c2["v"])
    W2, sigma2, scale2, shift2 = D2.effective(c2, u2a, v2a)
    out, pre = D2.forward(t, res, W2, scale2, shift2)
    return dict(X=X, u1a=u1a, v1a=v1a, u2a=u2a, v2a=v2a, sigma1=sigma1, W1=W1, rs1=rs1, rsd=rsd, c1=c1, cd=cd, z1=z1, zd=zd,
                pre1=pre1, t=t, res=res, sigma2=sigma2, W2=W2, scale2=scale2, shift2=shift2, pre=pre, out=out)


def conv_grads(dM1, dMd, d_sum, weight_bar1, u1a, v1a, sigma1, rs1, rsd):
    """The closed forms behind Dec2Convs' backward, from the kernel's raw outputs for (g1, gd) = the gradients of (z1, zd):
        dW1 = rs1[co] dM1[co];  d_weight_bar1 = dW1 / sigma - (<dW1, W_bar> / sigma^2) u v^T     (W = W_bar / sigma, sigma = u . W_bar v)
        d_short_weight = rsd[co] dMd[co];  d_short_bias = rsd[co] d_sum[co]."""
    wb = np.asarray(weight_bar1, np.float64)
    dW1 = np.asarray(rs1)[:, None, None, None, None] * np.asarray(dM1, np.float64)
    d_wb = dW1 / sigma1 - ((dW1 * wb).sum() / sigma1 ** 2) * np.outer(u1a, v1a).reshape(wb.shape)
    d_sw = np.asarray(rsd)[:, None] * np.asarray(dMd, np.float64)
    return {"d_weight_bar1": d_wb, "d_short_weight": d_sw.reshape(d_sw.shape + (1, 1, 1)),
            "d_short_bias": np.asarray(rsd) * np.asarray(d_sum, np.float64), "dW1": dW1}


def conv_bounds(e_dM1, e_dMd, e_sum, weight_bar1, u1a, v1a, sigma1, rs1, rsd):
    """First-order bounds of ``conv_grads``' outputs when dM1, dMd and d_sum are off by at most e_dM1, e_dMd (per element)
    and e_sum: the closed forms are linear in them, so the bound is the same form on absolute values."""
    wb = np.abs(np.asarray(weight_bar1, np.float64))
    e_dW = np.abs(rs1)[:, None, None, None, None] * e_dM1
    e_wb = e_dW / abs(sigma1) + ((e_dW * wb).sum() / sigma1 ** 2) * np.abs(np.outer(u1a, v1a)).reshape(wb.shape)
    e_sw = np.abs(rsd)[:, None] * e_dMd
    return {"d_weight_bar1": e_wb, "d_short_weight": e_sw.reshape(e_sw.shape + (1, 1, 1)), "d_short_bias": np.abs(rsd) * e_sum}


def up_sums(x0, x1, g1, gd):
    """The kernel's three sums and their sums of |terms| for arbitrary f64 (g1, gd) -> numpy dict (tests/convupn_ref.py)."""
    return {k: v.numpy() for k, v in U.wgrad_truth(f64_t(x0), f64_t(x1), f64_t(g1), f64_t(gd)).items()}


def block_grads(x0, x1, p, upstream, f=None):
    """The block's backward in closed forms, every sum f64 -> dict of BLOCK_GRADS and the intermediate gradients d_t, d_res,
    g1 = the gradient of z1, gd = the gradient of zd, and the raw sums dM1, dMd, d_sum, dM2, d_shift2 with abs_* of the
    weight-gradient kernels' outputs and abs_d_t of the input-gradient kernel's.  ``f``: block_forward's result where the
    caller has it."""
    f = block_forward(x0, x1, p) if f is None else f
    eps = float(p["eps"])
    y = f["out"]
    tw = N.wgrad_truth(f64_t(f["t"]), f64_t(y), f64_t(upstream))
    dM2, d_shift2 = tw["d_weight"].numpy(), tw["d_shift"].numpy()
    pg = param_grads(dM2, d_shift2, p["weight_bar2"], f["u2a"], f["v2a"], f["sigma2"], f["scale2"], p["bn2_mean"], p["bn2_var"], eps)
    td = N.dgrad_truth(f64_t(f["scale2"][:, None, None, None, None] * f["W2"]), f64_t(y), f64_t(upstream))
    d_t, d_res = td["d_x"].numpy(), td["d_res"].numpy()
    tg = tail_grads(f["z1"], f["zd"], p["bn1_weight"], p["bn1_bias"], d_t, d_res, active=f["pre1"] > 0)
    g1 = np.where(f["pre1"] > 0, d_t, 0.0) * bc(p["bn1_weight"])
    gd = d_res * bc(p["bnd_weight"])
    k = up_sums(x0, x1, g1, gd)
    cg = conv_grads(k["d_weight"], k["d_short"], k["d_short_bias"], p["weight_bar1"], f["u1a"], f["v1a"], f["sigma1"], f["rs1"], f["rsd"])
    out = {"d_weight_bar1": cg["d_weight_bar1"], "d_short_weight": cg["d_short_weight"], "d_short_bias": cg["d_short_bias"],
           "d_weight_bar2": pg["d_weight_bar"], "d_bn2_weight": pg["d_bn_weight"], "d_bn2_bias": pg["d_bn_bias"]}
    out.update({n: tg[n] for n in ("d_bn1_weight", "d_bn1_bias", "d_bnd_weight", "d_bnd_bias")})
    out.update(d_t=d_t, d_res=d_res, abs_d_t=td["abs_x"].numpy(), g1=g1, gd=gd, dW1=cg["dW1"], dM1=k["d_weight"], dMd=k["d_short"],
               d_sum=k["d_short_bias"], abs_dM1=k["abs_weight"], abs_dMd=k["abs_short"], abs_d_sum=k["abs_short_bias"],
               dM2=dM2, d_shift2=d_shift2, abs_dM2=tw["abs_weight"].numpy(), abs_d_shift2=tw["abs_shift"].numpy(), tail=tg)
    return out
