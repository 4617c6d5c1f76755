"""numpy f64 restatement of the weight gradients of the last decoder block's conv1 and shortcut
(include/v2ce_hip_convupgrad.h, last_block.py) in the reference's layouts: x0 [B, 64, L, H0, W0], x1 / g1 / gd
[B, 32, L, H, W], weight [32, 96, 3, 3, 3], short [32, 96].  Every product and sum is f64; nothing is rounded here.  The
layout helpers of tests/pred_head_ref.py convert to and from the kernels' tensors."""
import os

import numpy as np

from tests.last_conv_ref import shifted
from tests.pred_head_ref import from_c16, pitch_of, to_c16, ulp32  # noqa: F401  (shared with the tests)

C, C0, C1, CIN, TAPS = 32, 64, 32, 96, 27
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", ".lastblock")
SUFFIXES = (".x", ".g", ".s", ".w0", ".w1", ".w2")
LAYER_SUFFIXES = (".layer", ".lw0", ".lw1", ".lw2", ".l2")


def load_case(name):
    """Every array of a case of tests/make_last_block_goldens.py: its files merged, the per-group weight truths joined
    along ci into ref64_dW / abs_terms_dW / ref64_d_weight_bar1 [32, 96, 3, 3, 3]."""
    z = {}
    for sfx in SUFFIXES + LAYER_SUFFIXES:
        p = os.path.join(GOLD, f"{name}{sfx}.npz")
        if os.path.exists(p):
            z.update(np.load(p))
    for k in ("ref64_dW", "abs_terms_dW", "ref64_d_weight_bar1"):
        if f"{k}_g0" in z:
            z[k] = np.concatenate([z[f"{k}_g{g}"] for g in range(3)], axis=1)
    if "ref32_dev_dW_g0" in z:
        z["ref32_dev_dW"] = np.max([z[f"ref32_dev_dW_g{g}"] for g in range(3)])
    return z


def virtual_input(x0, x1):
    """X [B, 96, L, H, W]: X[ci] = x0[ci] at (h >> 1, w >> 1) for ci < 64, x1[ci - 64] behind them."""
    x0, x1 = np.asarray(x0), np.asarray(x1)
    H, W = x1.shape[3], x1.shape[4]
    assert x0.shape[3] == (H + 1) // 2 and x0.shape[4] == (W + 1) // 2 and x0.shape[1] == C0 and x1.shape[1] == C1
    up = x0[:, :, :, np.arange(H) >> 1][:, :, :, :, np.arange(W) >> 1]
    return np.concatenate([up, x1], axis=1)


def wgrad(x0, x1, g1, gd):
    """The header's formulas -> dict d_weight [32, 96, 3, 3, 3], d_short [32, 96], d_short_bias [32], and abs_weight /
    abs_short / abs_short_bias = the sums of the absolute values of their terms, all f64.  g1 or gd None: its outputs are
    left out."""
    X = virtual_input(x0, x1).astype(np.float64)
    out = {}
    if g1 is not None:
        g = np.asarray(g1, np.float64)
        dw, aw = np.zeros((C, CIN, 3, 3, 3)), np.zeros((C, CIN, 3, 3, 3))
        for kt in range(3):
            for kh in range(3):
                for kw in range(3):
                    xs = shifted(X, kt, kh, kw)
                    dw[:, :, kt, kh, kw] = np.einsum("bolhw,bclhw->oc", g, xs)
                    aw[:, :, kt, kh, kw] = np.einsum("bolhw,bclhw->oc", np.abs(g), np.abs(xs))
        out.update(d_weight=dw, abs_weight=aw)
    if gd is not None:
        g = np.asarray(gd, np.float64)
        out.update(d_short=np.einsum("bolhw,bclhw->oc", g, X), abs_short=np.einsum("bolhw,bclhw->oc", np.abs(g), np.abs(X)),
                   d_short_bias=g.sum(axis=(0, 2, 3, 4)), abs_short_bias=np.abs(g).sum(axis=(0, 2, 3, 4)))
    return out


def wgrad_bound(truth, abs_terms, n_pos, chain):
    """The header's bound of d_weight and d_short: one f32 rounding, an fmaf chain of at most `chain` positions, N f64
    additions."""
    return ulp32(truth) + chain * 2.0 ** -24 * abs_terms + n_pos * 2.0 ** -52 * abs_terms


# ---------------------------------------------------------------------------------------------------------------------
# the whole block: ResidualBlock3D(96, 32, norm='BN', sn=True) in .eval() on X = cat(upsample(x0), x1)

PARAMS = ("weight_bar1", "u1", "v1", "short_weight", "short_bias", "bn1_weight", "bn1_bias", "bn1_mean", "bn1_var", "bnd_weight",
          "bnd_bias", "bnd_mean", "bnd_var", "weight_bar2", "u2", "v2", "bn2_weight", "bn2_bias", "bn2_mean", "bn2_var", "eps")
# the gradients the reference block's autograd gives, in the goldens' names
BLOCK_GRADS = ("d_weight_bar1", "d_short_weight", "d_short_bias", "d_bn1_weight", "d_bn1_bias", "d_bnd_weight", "d_bnd_bias",
               "d_weight_bar2", "d_bn2_weight", "d_bn2_bias")


def bc(v):
    return np.asarray(v, np.float64)[None, :, None, None, None]


def conv1x1(x, weight):
    return np.einsum("bclhw,oc->bolhw", np.asarray(x, np.float64), np.asarray(weight, np.float64).reshape(C, -1))


def block_forward(x0, x1, p):
    """The block in f64 from the constants `p` (PARAMS; u / v BEFORE the call) -> dict: X; the iterated u1a, v1a, u2a, v2a;
    sigma1, W1 = weight_bar1 / sigma1, rs1, rsd; c1, cd (the raw convolutions, cd with its bias), z1, zd (normalised), pre1,
    t = relu(pre1), res; sigma2, W2, scale2, shift2; pre, feat = relu(pre)."""
    from tests import last_conv_ref as R2
    eps = float(p["eps"])
    X = virtual_input(x0, x1).astype(np.float64)
    u1a, v1a = R2.power_iteration(p["weight_bar1"], p["u1"], p["v1"])
    wb1 = np.asarray(p["weight_bar1"], np.float64)
    sigma1 = u1a @ (wb1.reshape(C, -1) @ v1a)
    W1 = wb1 / sigma1
    rs1 = 1.0 / np.sqrt(np.asarray(p["bn1_var"], np.float64) + eps)
    rsd = 1.0 / np.sqrt(np.asarray(p["bnd_var"], np.float64) + eps)
    c1 = R2.conv(X, W1)
    cd = conv1x1(X, p["short_weight"]) + bc(p["short_bias"])
    z1, zd = (c1 - bc(p["bn1_mean"])) * bc(rs1), (cd - bc(p["bnd_mean"])) * bc(rsd)
    pre1 = bc(p["bn1_weight"]) * z1 + bc(p["bn1_bias"])
    t, res = np.maximum(pre1, 0.0), bc(p["bnd_weight"]) * zd + bc(p["bnd_bias"])
    u2a, v2a = R2.power_iteration(p["weight_bar2"], p["u2"], p["v2"])
    W2, sigma2, scale2, shift2 = R2.effective(p["weight_bar2"], u2a, v2a, p["bn2_weight"], p["bn2_bias"], p["bn2_mean"],
                                              p["bn2_var"], eps)
    feat, pre = R2.forward(t, res, W2, scale2, shift2)
    return dict(X=X, u1a=u1a, v1a=v1a, u2a=u2a, v2a=v2a, sigma1=sigma1, W1=W1, rs1=rs1, rsd=rsd, c1=c1, cd=cd, z1=z1, zd=zd,
                pre1=pre1, t=t, res=res, sigma2=sigma2, W2=W2, scale2=scale2, shift2=shift2, pre=pre, feat=feat)


def conv_grads(dM1, dMd, d_sum, weight_bar1, u1a, v1a, sigma1, rs1, rsd):
    """The closed forms behind TailConvs' backward, from the kernel's raw outputs for (g1, gd) = the gradients of (z1, zd):
        dW1 = rs1[co] dM1[co];  d_weight_bar1 = dW1 / sigma - (<dW1, W_bar> / sigma^2) u v^T     (W = W_bar / sigma, sigma = u . W_bar v)
        d_short_weight = rsd[co] dMd[co];  d_short_bias = rsd[co] d_sum[co]."""
    wb = np.asarray(weight_bar1, np.float64)
    dW1 = np.asarray(rs1)[:, None, None, None, None] * np.asarray(dM1, np.float64)
    d_wb = dW1 / sigma1 - ((dW1 * wb).sum() / sigma1 ** 2) * np.outer(u1a, v1a).reshape(wb.shape)
    return {"d_weight_bar1": d_wb, "d_short_weight": (np.asarray(rsd)[:, None] * np.asarray(dMd, np.float64)).reshape(C, CIN, 1, 1, 1),
            "d_short_bias": np.asarray(rsd) * np.asarray(d_sum, np.float64), "dW1": dW1}


def conv_bounds(e_dM1, e_dMd, e_sum, weight_bar1, u1a, v1a, sigma1, rs1, rsd):
    """First-order bounds of ``conv_grads``' outputs when dM1, dMd and d_sum are off by at most e_dM1, e_dMd (per element)
    and e_sum: the closed forms are linear in them, so the bound is the same form on absolute values."""
    wb = np.abs(np.asarray(weight_bar1, np.float64))
    e_dW = np.abs(rs1)[:, None, None, None, None] * e_dM1
    e_wb = e_dW / abs(sigma1) + ((e_dW * wb).sum() / sigma1 ** 2) * np.abs(np.outer(u1a, v1a)).reshape(wb.shape)
    return {"d_weight_bar1": e_wb, "d_short_weight": (np.abs(rsd)[:, None] * e_dMd).reshape(C, CIN, 1, 1, 1),
            "d_short_bias": np.abs(rsd) * e_sum}


def block_grads(x0, x1, p, upstream, f=None):
    """The block's backward in closed forms, every sum f64 -> dict of BLOCK_GRADS and the intermediate gradients d_t, d_res,
    g1 = the gradient of z1, gd = the gradient of zd, and the raw sums dM1, dMd, d_sum, dM2, d_shift2 with abs_* of the four
    weight-gradient kernels' outputs.  ``f``: block_forward's result where the caller has it."""
    from tests import last_conv_dgrad_ref as D2
    from tests import last_conv_ref as R2
    f = block_forward(x0, x1, p) if f is None else f
    eps = float(p["eps"])
    y = f["feat"]
    g2 = R2.wgrad(f["t"], y, upstream)
    pg = R2.param_grads(g2["d_weight"], g2["d_shift"], p["weight_bar2"], f["u2a"], f["v2a"], f["sigma2"], f["scale2"], p["bn2_mean"],
                        p["bn2_var"], eps)
    dg = D2.dgrad(f["scale2"][:, None, None, None, None] * f["W2"], y, upstream)
    tg = D2.tail_grads(f["z1"], f["zd"], p["bn1_weight"], p["bn1_bias"], dg["d_x"], dg["d_res"])
    g1 = np.where(f["pre1"] > 0, dg["d_x"], 0.0) * bc(p["bn1_weight"])
    gd = dg["d_res"] * bc(p["bnd_weight"])
    k = wgrad(x0, x1, g1, gd)
    cg = conv_grads(k["d_weight"], k["d_short"], k["d_short_bias"], p["weight_bar1"], f["u1a"], f["v1a"], f["sigma1"], f["rs1"], f["rsd"])
    out = {"d_weight_bar1": cg["d_weight_bar1"], "d_short_weight": cg["d_short_weight"], "d_short_bias": cg["d_short_bias"],
           "d_weight_bar2": pg["d_weight_bar"], "d_bn2_weight": pg["d_bn_weight"], "d_bn2_bias": pg["d_bn_bias"]}
    out.update({n: tg[n] for n in ("d_bn1_weight", "d_bn1_bias", "d_bnd_weight", "d_bnd_bias")})
    out.update(d_t=dg["d_x"], d_res=dg["d_res"], abs_d_t=dg["abs_x"], g1=g1, gd=gd, dW1=cg["dW1"], dM1=k["d_weight"], dMd=k["d_short"],
               d_sum=k["d_short_bias"], abs_dM1=k["abs_weight"], abs_dMd=k["abs_short"], abs_d_sum=k["abs_short_bias"],
               dM2=g2["d_weight"], d_shift2=g2["d_shift"], abs_dM2=g2["abs_weight"], abs_d_shift2=g2["abs_shift"], tail=tg)
    return out


def src_to_c16(x0, pitch0=None, fill=np.nan):
    """[B, 64, L, H0, W0] -> channels-last-16 [B, L, 4, H0, pitch0, 16] f32, padding columns filled with `fill`."""
    f = np.asarray(x0, np.float32)
    B, Cx, L, H0, W0 = f.shape
    pitch0 = W0 if pitch0 is None else pitch0
    out = np.full((B, L, Cx // 16, H0, pitch0, 16), fill, np.float32)
    out[:, :, :, :, :W0, :] = f.reshape(B, Cx // 16, 16, L, H0, W0).transpose(0, 3, 1, 4, 5, 2)
    return out
