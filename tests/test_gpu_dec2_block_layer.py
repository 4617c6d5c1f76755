"""Dec2Block (dec2_block.py: Dec2Convs -> Dec2Norms -> Dec2Conv) on an exact-f32 model against the reference block's own
f64 autograd of ResidualBlock3D(192, 64, norm='BN', sn=True) on cat(upsample(x0), x1) (tests/golden/.dec2block,
tests/make_dec2_block_goldens.py).

Every bound is a first-order propagation of the kernels' contracts and of the f32 closed forms (tests/dec2_block_ref.py), as
tests/test_gpu_last_block_autograd.py and tests/test_gpu_dec2_conv_layer.py derive them; none is taken from what the code
gives.  With eps = 2^-24, |.| elementwise, conv(|a|, |b|) the same sums on absolute values, and kappa = sum |u_i W_ij v_j| /
|sigma| the condition of a spectral norm whose sigma, u, v are f32 products of rows + cols terms (4 (rows + cols) kappa eps
relative on sigma); conv1 has 64 rows and 5184 columns, conv2 64 and 1728:

forward (the masks are pinned by the goldens' MARGIN; values carry these errors into the sums that read them)
  c1     an fmaf chain of 5184 terms on W1 = W_bar1 / sigma1:  E_c1 = (5184 + 4 + 4 * 5248 kappa1) eps conv(|X|, |W1|)
  z1     E_z1 = rs1 E_c1 + 6 eps rs1 (conv(|X|, |W1|) + |mean1|);   zd: E_zd = (192 + 8) eps rsd (conv(|X|, |Wd|) + |bias_d| + |mean_d|)
  t      E_t = mask_t (|w1| E_z1 + 3 eps (|w1 z1| + |b1|));   res: E_res = |wd| E_zd + 3 eps (|wd zd| + |bd|)
  out    one f32 ulp + (1728 + 8 + 4 * 1792 kappa2) eps (conv(|t|, |W2|) |scale2| + |shift2| + |res|) + conv(E_t, |W2|) |scale2| + E_res
backward
  d_t    the header of the input-gradient kernel on the folded weight Wf = scale2 W2: E_dt = (27 * 64 + 1) eps S + 27 * 64 2^-126
         + (4 * 1792 kappa2 + 8) eps S with S = sum |Wf| |m| (the fold and W2's own derivation in f32);  d_res is a copy
  g1     = w1 mask_t d_t:  E_g1 = |w1| mask_t E_dt + eps |g1|;   gd = wd d_res:  E_gd = eps |gd|
  dM1, dMd, sum gd   the header of v2ce_convupn_wgrad on the device's (g1, gd), plus the same sums on (E_g1, E_gd) in the
         places of (|g1|, |gd|): the kernel's outputs are linear in them
  conv1, shortcut    the closed forms (dec2_block_ref.conv_grads) are linear in dM1, dMd and the sum: the bound is the same
         form on absolute values (conv_bounds); on top torch evaluates them in f32: (64 * 5184 + 5184 + 4 * 5248 kappa1 + 16)
         eps times the closed form on absolute values for weight_bar1, 4 eps for the shortcut's
  bn1, bnd   d_weight = sum g z, d_bias = sum g over the n positions of a channel: E_dt through |z|, E_z through |g|, and
         (n + 4) eps times the sum of |terms| for torch's f32 evaluation
  conv2, bn2   the header of the 64-channel weight-gradient kernel on the device's t, plus sum |m| E_t; then
         last_conv_ref.param_bounds and the f32 slack of tests/test_gpu_dec2_conv_layer.py
each plus one f32 ulp of the truth.  The worst element of each is printed as a fraction of its bound.  Both relu masks are
the reference's, and the padding columns of what the layers return are zeros."""
import functools

import numpy as np
import pytest
import torch

from tests import convn_ref as N
from tests import convupn_ref as U
from tests import dec2_block_ref as R
from tests import grad_walk_ref as G
from v2ce_toolbox_amd import hip
from v2ce_toolbox_amd.dec2_block import Dec2Block, Dec2Convs, Dec2Norms
from v2ce_toolbox_amd.dec2_conv import Dec2Conv
from v2ce_toolbox_amd.v2ce_3d import V2ce3d

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -24
C, COLS1, COLS2 = 64, 192 * 27, 64 * 27


@functools.lru_cache(maxsize=None)
def f32_model():
    from v2ce_toolbox_amd import synth
    m = V2ce3d(precision="f32")
    m.load_state_dict(synth.make_state_dict(0))
    return m.eval().to("cuda:0")


def c16_dev(a):
    """[B, 16 G, L, H, W] -> the device's channels-last-16 tensor at the activation pitch, NaN in the padding columns."""
    t = torch.from_numpy(N.to_c16_np(a, G.pitch_of(a.shape[-1]))).cuda()
    t.lw, t.c16 = a.shape[-1], True
    return t


def planar(t):
    return G.from_c16(t.detach(), t.lw).cpu().numpy()


def block_from_golden(z, model):
    convs, norms, conv = Dec2Convs(model).cuda(), Dec2Norms().cuda(), Dec2Conv(model).cuda()
    put = lambda dst, key: dst.copy_(torch.from_numpy(np.asarray(z[key])))
    with torch.no_grad():
        for mod, pairs in ((convs, (("weight_bar", "weight_bar1"), ("weight_u", "u1"), ("weight_v", "v1"), ("short_weight", "short_weight"),
                                    ("short_bias", "short_bias"), ("bn1_mean", "bn1_mean"), ("bn1_var", "bn1_var"),
                                    ("bnd_mean", "bnd_mean"), ("bnd_var", "bnd_var"))),
                           (norms, (("bn1_weight", "bn1_weight"), ("bn1_bias", "bn1_bias"), ("bnd_weight", "bnd_weight"),
                                    ("bnd_bias", "bnd_bias"))),
                           (conv, (("weight_bar", "weight_bar2"), ("weight_u", "u2"), ("weight_v", "v2"), ("bn_weight", "bn2_weight"),
                                   ("bn_bias", "bn2_bias"), ("running_mean", "bn2_mean"), ("running_var", "bn2_var")))):
            for name, key in pairs:
                put(getattr(mod, name), key)
        convs.eps.fill_(float(z["eps"]))
        conv.eps.fill_(float(z["eps"]))
    return Dec2Block(convs, norms, conv)


def kappa_of(weight_bar, u, v, sigma):
    wb = np.abs(np.asarray(weight_bar, np.float64).reshape(C, -1))
    return float((np.abs(u)[:, None] * wb * np.abs(v)[None, :]).sum() / abs(sigma))


def close(label, k, got, want, bound):
    a = got.detach().cpu().numpy().astype(np.float64) if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    err = np.abs(a - want)
    bound = bound + R.ulp32(want)
    print(f"{label}: {k}: max error {err.max():.3e}, {float((err / bound).max()):.4f} of its bound")
    assert a.shape == want.shape and not np.isnan(a).any() and np.all(err <= bound), (label, k, float(err.max()))


def chain_bounds(x0, x1, p, f, g, upstream):
    """The module docstring's bounds for the block's output and the ten gradients of dec2_block_ref.BLOCK_GRADS (without the
    final ulp), from the f64 forward `f` (block_forward) and backward `g` (block_grads) of the block."""
    s5 = lambda a: a.sum(axis=(0, 2, 3, 4))
    bc = R.bc
    n = x1.size // x1.shape[1]
    aX = np.abs(f["X"])
    k1 = kappa_of(p["weight_bar1"], f["u1a"], f["v1a"], f["sigma1"])
    k2 = kappa_of(p["weight_bar2"], f["u2a"], f["v2a"], f["sigma2"])
    sig1, sig2 = 4 * (COLS1 + C) * k1 * EPS32, 4 * (COLS2 + C) * k2 * EPS32
    # forward
    mag1 = R.conv(aX, np.abs(f["W1"]))
    e_z1 = bc(f["rs1"]) * ((COLS1 + 4) * EPS32 * mag1 + sig1 * mag1 + 6 * EPS32 * (mag1 + bc(np.abs(p["bn1_mean"]))))
    magd = R.conv1x1(aX, np.abs(p["short_weight"])) + bc(np.abs(p["short_bias"])) + bc(np.abs(p["bnd_mean"]))
    e_zd = (192 + 8) * EPS32 * bc(f["rsd"]) * magd
    mask_t = f["pre1"] > 0
    aw1, awd = bc(np.abs(p["bn1_weight"])), bc(np.abs(p["bnd_weight"]))
    e_t = np.where(mask_t, aw1 * e_z1 + 3 * EPS32 * (aw1 * np.abs(f["z1"]) + bc(np.abs(p["bn1_bias"]))), 0.0)
    e_res = awd * e_zd + 3 * EPS32 * (awd * np.abs(f["zd"]) + bc(np.abs(p["bnd_bias"])))
    as2 = bc(np.abs(f["scale2"]))
    mag2 = R.conv(np.abs(f["t"]), np.abs(f["W2"])) * as2 + bc(np.abs(f["shift2"])) + np.abs(f["res"])
    out = {"out": (COLS2 + 8) * EPS32 * mag2 + sig2 * mag2 + R.conv(e_t, np.abs(f["W2"])) * as2 + e_res}
    # backward: conv2's input gradient, the norms' multiplications, the new kernel, the closed forms
    S = g["abs_d_t"]
    e_dt = N.dgrad_bound(S, C) + (8 * EPS32 + sig2) * S
    e_g1 = np.where(mask_t, aw1 * e_dt, 0.0) + EPS32 * np.abs(g["g1"])
    e_gd = EPS32 * np.abs(g["gd"])
    carried = R.up_sums(x0, x1, e_g1, e_gd)                # the kernel's sums with the errors in the gradients' places
    e_dM1 = U.bound(g["dM1"], g["abs_dM1"], n, hip.UPWGRAD_CHAIN) + carried["abs_weight"]
    e_dMd = U.bound(g["dMd"], g["abs_dMd"], n, hip.UPWGRAD_CHAIN) + carried["abs_short"]
    e_sum = R.ulp32(g["d_sum"]) + carried["abs_short_bias"]
    cargs = (p["weight_bar1"], f["u1a"], f["v1a"], f["sigma1"], f["rs1"], f["rsd"])
    out.update(R.conv_bounds(e_dM1, e_dMd, e_sum, *cargs))
    size = R.conv_bounds(np.abs(g["dM1"]), np.abs(g["dMd"]), np.abs(g["d_sum"]), *cargs)
    out["d_weight_bar1"] = out["d_weight_bar1"] + ((C * COLS1 + COLS1 + 16) * EPS32 + sig1) * size["d_weight_bar1"]
    out["d_short_weight"] = out["d_short_weight"] + 4 * EPS32 * size["d_short_weight"]
    out["d_short_bias"] = out["d_short_bias"] + 4 * EPS32 * size["d_short_bias"]
    # the two BatchNorms' affine parts
    g_t = np.where(mask_t, g["d_t"], 0.0)
    e_gt = np.where(mask_t, e_dt, 0.0)
    az1, azd, ares = np.abs(f["z1"]), np.abs(f["zd"]), np.abs(g["d_res"])
    out["d_bn1_weight"] = s5(e_gt * az1) + s5(np.abs(g_t) * e_z1) + (n + 4) * EPS32 * s5(np.abs(g_t) * az1)
    out["d_bn1_bias"] = s5(e_gt) + (n + 4) * EPS32 * s5(np.abs(g_t))
    out["d_bnd_weight"] = s5(ares * e_zd) + (n + 4) * EPS32 * s5(ares * azd)
    out["d_bnd_bias"] = (n + 4) * EPS32 * s5(ares)
    # conv2 and bn2: the kernel on the device's t
    carried_t = N.wgrad_truth(R.f64_t(e_t), R.f64_t(f["out"]), R.f64_t(np.abs(upstream)))["abs_weight"].numpy()
    e_dM2 = N.wgrad_bound(g["dM2"], g["abs_dM2"], n, hip.WGRAD_CHAIN) + carried_t
    pargs = (p["weight_bar2"], f["u2a"], f["v2a"], f["sigma2"], f["scale2"], p["bn2_mean"], p["bn2_var"], float(p["eps"]))
    c2 = R.param_bounds(e_dM2, R.ulp32(g["d_shift2"]), *pargs)
    size2 = R.param_bounds(np.abs(g["dM2"]), np.abs(g["d_shift2"]), *pargs)
    rel2 = (C * COLS2 + COLS2 + 16) * EPS32 + sig2
    for mine, theirs in (("d_weight_bar2", "d_weight_bar"), ("d_bn2_weight", "d_bn_weight"), ("d_bn2_bias", "d_bn_bias")):
        out[mine] = c2[theirs] + rel2 * size2[theirs]
    return out, (k1, k2)


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_block_matches_the_reference_blocks_autograd(name):
    z = R.load_case(name)
    shape = R.CASES[name]
    W = shape[3]
    p = {k: z[k] for k in R.PARAMS}
    block = block_from_golden(z, f32_model())
    x0, x1 = c16_dev(z["x0"]), c16_dev(z["x1"])            # (their padding columns hold NaN: it must not reach a result)
    z1, zd = block.convs(x0, x1)
    assert z1.grad_fn is not None and zd.grad_fn is not None and z1.lw == zd.lw == W
    assert z1.shape == zd.shape == (shape[0], shape[1], 4, shape[2], G.pitch_of(W), 16)
    t, res = block.norms(z1, zd)
    out = block.conv(t, res)
    assert out.grad_fn is not None and out.lw == W and out.shape == z1.shape
    for a in (t, res, out):
        assert not torch.isnan(a).any() and not a[:, :, :, :, W:, :].any()         # padding columns are zeros

    f = R.block_forward(z["x0"], z["x1"], p)
    g = R.block_grads(z["x0"], z["x1"], p, z["upstream"], f)
    assert np.abs(f["u1a"] - z["ref64_u1_after"]).max() <= 1e-13 and np.abs(f["v2a"] - z["ref64_v2_after"]).max() <= 1e-13
    bounds, (k1, k2) = chain_bounds(z["x0"], z["x1"], p, f, g, z["upstream"])
    print(f"{name}: kappa1 {k1:.1f}, kappa2 {k2:.1f}")
    assert np.array_equal(planar(t) > 0, f["pre1"] > 0) and np.array_equal(planar(out) > 0, z["ref64_out"] > 0)   # the reference's masks
    close(name, "out", planar(out).astype(np.float64), z["ref64_out"], bounds["out"])

    out.backward(c16_dev(z["upstream"]))                              # (its padding columns hold NaN: they are not read)
    got = {"d_weight_bar1": block.convs.weight_bar.grad, "d_short_weight": block.convs.short_weight.grad,
           "d_short_bias": block.convs.short_bias.grad, "d_bn1_weight": block.norms.bn1_weight.grad, "d_bn1_bias": block.norms.bn1_bias.grad,
           "d_bnd_weight": block.norms.bnd_weight.grad, "d_bnd_bias": block.norms.bnd_bias.grad, "d_weight_bar2": block.conv.weight_bar.grad,
           "d_bn2_weight": block.conv.bn_weight.grad, "d_bn2_bias": block.conv.bn_bias.grad}
    assert set(got) == set(R.BLOCK_GRADS) and len(list(block.parameters())) == 10
    for k in R.BLOCK_GRADS:
        have, bound = got[k], bounds[k]
        if k in R.SEAM_ONLY.get(name, ()):                 # this case stores the seam of the concat only; the restatement has it all
            assert np.abs(g[k][:, R.SEAM] - z["ref64_" + k]).max() <= 1e-11 * np.abs(z["ref64_" + k]).max()
            close(name, k + " (seam, stored)", have[:, R.SEAM], z["ref64_" + k], bound[:, R.SEAM])
            close(name, k + " (restated)", have, g[k], bound)
        else:
            close(name, k, have, z["ref64_" + k], bound)
        assert float(have.abs().max()) > 0
