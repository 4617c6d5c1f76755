"""Recipe of tests/golden/.dec1conv/*.npz: the REFERENCE's own f64 autograd of the second half of its second decoder block,
``SpectralNorm(Conv3d(128, 128, 3, padding=1, bias=False))`` -> ``BatchNorm3d(128)`` -> ``+= residual`` -> ``relu``, composed
as train/scripts/model/submodules.py:249-257 composes them, in ``.eval().double()`` with seeded constants, at the two small
shapes of tests/dec2_conv_ref.py: CASES.  The recipe is that of tests/make_dec2_conv_goldens.py with C = 128, and one set of
constants for both cases.

consts.N.npz hold the layer's constants (weight_bar on the grid of 64ths, u, v before the call, bn_weight, bn_bias,
running_mean, running_var, eps).  Per case NAME.N.npz hold the seeded inputs t (relu-like: exact zeros), res, upstream
[B, 128, L, H, W] f32 on coarse grids and, from the f64 run with t and res requiring grad: ref64_x0 (the layer's output),
ref64_d_weight_bar, ref64_d_bn_weight, ref64_d_bn_bias, ref64_d_t, ref64_d_res, ref64_u_after, ref64_v_after.  res is nudged
until no unit sits within MARGIN of the relu's kink, so that an f32 forward has the reference's mask.  The maker asserts
that the restatement (tests/dec1_conv_ref.layer_grads) gives the reference's five gradients.

A file is NAME.N.npz; an array larger than PIECE bytes is split along axis 1 into KEY@0, KEY@1, ... (the piece plan of
tests/make_dec2_conv_goldens.py; tests/last_conv_dgrad_ref.load_parts joins them); every file stays under SIZE_CAP and the
directory under dec1_conv_ref.DIR_CAP.  Runs where the reference tree is present; not collected by pytest.

    python tests/make_dec1_conv_goldens.py [out_dir]   (default tests/golden/.dec1conv; V2CE_REFERENCE_ROOT names the tree)
"""
import glob
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import dec1_conv_ref as R  # noqa: E402
from tests.make_dec2_conv_goldens import MARGIN, grid, reference_spectral_norm, save  # noqa: E402

C = R.C


def inputs(name):
    B, L, H, W = R.CASES[name]
    rng = np.random.default_rng(sorted(R.CASES).index(name) + 3777)
    t = np.maximum(grid(rng, (B, C, L, H, W), 0.125), 0).astype(np.float32)
    res = grid(rng, (B, C, L, H, W), 1.0 / 64, 0.5)
    upstream = grid(rng, (B, C, L, H, W), 0.125)
    upstream[upstream == 0] = np.float32(0.125)
    return t, res, upstream


def constants(seed):
    g = torch.Generator().manual_seed(seed)
    u, v = torch.randn(C, generator=g), torch.randn(C * 27, generator=g)
    c = {"weight_bar": torch.round(torch.randn((C, C, 3, 3, 3), generator=g) * 0.07 * 64) / 64, "u": u / u.norm(), "v": v / v.norm(),
         "bn_weight": 1.0 + 0.3 * torch.randn(C, generator=g), "bn_bias": 0.1 * torch.randn(C, generator=g),
         "running_mean": 0.1 * torch.randn(C, generator=g), "running_var": 0.5 + torch.rand(C, generator=g)}
    out = {k: a.numpy().astype(np.float32) for k, a in c.items()}
    out["eps"] = np.float32(torch.nn.BatchNorm3d(C).eps)
    return out


def run_reference(sn_cls, c, t, res, upstream):
    """A fresh pair of the reference's modules with the constants `c`, composed as submodules.py:249-257 -> numpy arrays."""
    conv2 = sn_cls(torch.nn.Conv3d(C, C, kernel_size=3, stride=1, padding=1, bias=False))
    bn2 = torch.nn.BatchNorm3d(C)
    relu = torch.nn.ReLU(inplace=True)
    with torch.no_grad():
        m = conv2.module
        m.weight_bar.copy_(torch.from_numpy(c["weight_bar"]))
        m.weight_u.copy_(torch.from_numpy(c["u"]))
        m.weight_v.copy_(torch.from_numpy(c["v"]))
        bn2.weight.copy_(torch.from_numpy(c["bn_weight"]))
        bn2.bias.copy_(torch.from_numpy(c["bn_bias"]))
        bn2.running_mean.copy_(torch.from_numpy(c["running_mean"]))
        bn2.running_var.copy_(torch.from_numpy(c["running_var"]))
    assert abs(bn2.eps - float(c["eps"])) < 1e-12          # (stored as the f32 the device holds)
    conv2, bn2 = conv2.eval().double(), bn2.eval().double()
    tt = torch.from_numpy(t).double().requires_grad_(True)
    rr = torch.from_numpy(res).double().requires_grad_(True)
    out = conv2(tt)
    out = bn2(out)
    out += rr
    out = relu(out)
    out.backward(torch.from_numpy(upstream).double())
    m = conv2.module
    return {"ref64_x0": out.detach().numpy(), "ref64_d_weight_bar": m.weight_bar.grad.numpy(), "ref64_d_bn_weight": bn2.weight.grad.numpy(),
            "ref64_d_bn_bias": bn2.bias.grad.numpy(), "ref64_d_t": tt.grad.numpy(), "ref64_d_res": rr.grad.numpy(),
            "ref64_u_after": m.weight_u.detach().numpy().copy(), "ref64_v_after": m.weight_v.detach().numpy().copy()}


def main(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    sn_cls = reference_spectral_norm()
    c = constants(71)
    save(out_dir, R.SHARED, c)
    for name in R.CASES:
        t, res, upstream = inputs(name)
        for _ in range(8):                               # no unit within MARGIN of the relu's kink
            near = np.abs(R.layer_grads(c, t, res, upstream)["pre"]) < MARGIN
            if not near.any():
                break
            res[near] += np.float32(1.0 / 32)
        g = R.layer_grads(c, t, res, upstream)
        assert not (np.abs(g["pre"]) < MARGIN).any() and 0.2 < (g["pre"] > 0).mean() < 0.8, name
        ref = run_reference(sn_cls, c, t, res, upstream)
        assert np.array_equal(ref["ref64_x0"] > 0, g["pre"] > 0)
        for k in R.GRADS:
            want = ref["ref64_" + k]
            assert want.shape == g[k].shape and np.abs(g[k] - want).max() <= 1e-11 * np.abs(want).max() > 0, (name, k)
        assert np.abs(g["u1"] - ref["ref64_u_after"]).max() <= 1e-13 and np.abs(g["v1"] - ref["ref64_v_after"]).max() <= 1e-13
        save(out_dir, name, dict(t=t, res=res, upstream=upstream, **ref))
    total = sum(os.path.getsize(p) for p in glob.glob(os.path.join(out_dir, "*.npz")))
    print("directory", total)
    assert total <= R.DIR_CAP, total


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", ".dec1conv"))
