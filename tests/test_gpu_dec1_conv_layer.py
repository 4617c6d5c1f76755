"""Dec1Conv (dec1_conv.py) on an exact-f32 model against the reference's own f64 autograd of SpectralNorm(Conv3d(128, 128))
-> BatchNorm3d -> += residual -> relu (tests/golden/.dec1conv, tests/make_dec1_conv_goldens.py).

The bounds are those of tests/test_gpu_dec2_conv_layer.py with C = 128 and 3456 columns: propagated from the kernel
contracts (include/v2ce_hip_convcgrad.h) and the arithmetic, not taken from what the code gives.  With eps = 2^-24, kappa =
sum |u| |W_bar| |v| / |sigma| (how an f32 evaluation of sigma magnifies its roundings; u of 128, v of 3456 components: (3456 +
128) terms, evaluated twice and normalised: 4 * 3584 kappa eps relative on sigma):
  h1            one f32 ulp + (3456 + 8 + 4 * 3584 kappa) eps times conv(|t|, |W|) |scale| + |shift| + |res|: an fmaf chain of
                3456 terms, the epilogue, and W, scale, shift derived on the device in f32;
  d_weight_bar, d_bn_weight, d_bn_bias
                the header's bounds of dM (ulp32 + V2CE_WGRAD_CHAIN eps S + N 2^-52 S) and d_shift (one ulp) carried through
                the closed forms, which are linear in them (last_conv_ref.param_bounds), plus the f32 evaluation of those
                forms: (128 * 3456 + 3456 + 4 * 3584 kappa + 16) eps times the same forms on absolute values, plus one ulp;
  d_t           the header's bound on the folded weight Wf = scale[co] W[co]: (27 * 128 + 1) eps S + 27 * 128 * 2^-126 with S
                = sum |Wf| |m|, plus (2 + 4 * 3584 kappa) eps S for the weight the device folds in f32 (one rounding of the
                division by sigma, one of the product, and sigma's own error);
  d_res         a copy: the bytes of the masked upstream (the mask is the reference's: no unit of the goldens sits within
                1e-4 of the relu's kink).
The padding columns of both input gradients are zeros.  The worst element of each is printed as a fraction of its bound."""
import functools

import numpy as np
import pytest
import torch

from tests import convn_ref as N
from tests import dec1_conv_ref as R
from tests import grad_walk_ref as G
from v2ce_toolbox_amd import hip
from v2ce_toolbox_amd.dec1_conv import Dec1Conv
from v2ce_toolbox_amd.v2ce_3d import V2ce3d

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -24
C, COLS = R.C, R.COLS


@functools.lru_cache(maxsize=None)
def f32_model():
    from v2ce_toolbox_amd import synth
    m = V2ce3d(precision="f32")
    m.load_state_dict(synth.make_state_dict(0))
    return m.eval().to("cuda:0")


def c16_dev(a):
    """[B, 128, L, H, W] -> the device's channels-last-16 tensor at the activation pitch, NaN in the padding columns."""
    t = torch.from_numpy(N.to_c16_np(a, G.pitch_of(a.shape[-1]))).cuda()
    t.lw, t.c16 = a.shape[-1], True
    return t


def layer_from_golden(z, model):
    layer = Dec1Conv(model).cuda()
    with torch.no_grad():
        for name, key in (("weight_bar", "weight_bar"), ("weight_u", "u"), ("weight_v", "v"), ("bn_weight", "bn_weight"),
                          ("bn_bias", "bn_bias"), ("running_mean", "running_mean"), ("running_var", "running_var")):
            getattr(layer, name).copy_(torch.from_numpy(z[key]))
        layer.eps.fill_(float(z["eps"]))
    return layer


def report(label, k, err, bound):
    frac = float((err / bound).max())
    print(f"{label}: {k}: max error {float(err.max()):.3e}, {frac:.4f} of its bound")
    assert np.all(err <= bound), (label, k, float(err.max()), frac)


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_layer_matches_the_references_autograd(name):
    z = R.load_case(name)
    shape = R.CASES[name]
    assert z["t"].shape == (shape[0], C) + shape[1:] and z["ref64_d_weight_bar"].shape == (C, C, 3, 3, 3)
    c = {k: z[k] for k in R.CONSTS}
    layer = layer_from_golden(z, f32_model())
    t, res = c16_dev(z["t"]).requires_grad_(True), c16_dev(z["res"]).requires_grad_(True)
    t.lw = res.lw = shape[3]
    assert (C, COLS) == (128, 3456) and layer.C == C and layer.INDEX == 3
    x0 = layer(t, res)
    assert x0.grad_fn is not None and x0.lw == shape[3] and x0.shape == t.shape

    # the restatement on the golden's constants: sums of |terms|, u, v, sigma in f64
    g = R.layer_grads(c, z["t"], z["res"], z["upstream"])
    u1, v1, sigma, scale, W = g["u1"], g["v1"], g["sigma"], g["scale"], g["W"]
    assert np.abs(u1 - z["ref64_u_after"]).max() <= 1e-13 and np.abs(v1 - z["ref64_v_after"]).max() <= 1e-13
    kappa = R.kappa_of(c["weight_bar"], u1, v1, sigma)
    sig_rel = 4 * (COLS + C) * kappa * EPS32

    got = G.from_c16(x0.detach(), shape[3]).cpu().numpy().astype(np.float64)
    shift = np.asarray(c["bn_bias"], np.float64) - np.asarray(c["running_mean"], np.float64) * scale
    mag = R.conv(np.abs(z["t"]), np.abs(W)) * np.abs(scale)[None, :, None, None, None] + \
        np.abs(shift)[None, :, None, None, None] + np.abs(z["res"])
    report(name, "x0", np.abs(got - z["ref64_x0"]), R.ulp32(z["ref64_x0"]) + (COLS + 8) * EPS32 * mag + sig_rel * mag)
    assert np.array_equal(got > 0, z["ref64_x0"] > 0)                  # the relu mask is the reference's

    x0.backward(c16_dev(z["upstream"]))                               # (its padding columns hold NaN: they are not read)
    n_pos = z["t"].size // C
    e_dM = N.wgrad_bound(g["dM"], g["abs_dM"], n_pos, hip.WGRAD_CHAIN)
    e_shift = R.ulp32(g["d_shift"])
    stats = (c["weight_bar"], u1, v1, sigma, scale, c["running_mean"], c["running_var"], c["eps"])
    carried = R.param_bounds(e_dM, e_shift, *stats)
    size = R.param_bounds(np.abs(g["dM"]), np.abs(g["d_shift"]), *stats)
    rel = (C * COLS + COLS + 16) * EPS32 + sig_rel
    for k, p in (("d_weight_bar", layer.weight_bar), ("d_bn_weight", layer.bn_weight), ("d_bn_bias", layer.bn_bias)):
        a = p.grad.detach().cpu().numpy().astype(np.float64)
        want = z["ref64_" + k]
        assert a.shape == want.shape and np.abs(want).max() > 0
        report(name, k, np.abs(a - want), carried[k] + rel * size[k] + R.ulp32(want))

    W_lw = shape[3]
    for gr in (t.grad, res.grad):
        assert gr.shape == t.shape and not torch.isnan(gr).any() and not gr[:, :, :, :, W_lw:, :].any(), name
    d_t = G.from_c16(t.grad, W_lw).cpu().numpy().astype(np.float64)
    report(name, "d_t", np.abs(d_t - z["ref64_d_t"]), N.dgrad_bound(g["abs_x"], C) + (2 * EPS32 + sig_rel) * g["abs_x"])
    assert np.abs(z["ref64_d_t"]).max() > 0
    d_res = G.from_c16(res.grad, W_lw).cpu().numpy()
    assert d_res.astype(np.float32).tobytes() == z["ref64_d_res"].astype(np.float32).tobytes(), name
