"""Recipe of tests/golden/.dec2block/*.npz: the REFERENCE's own f64 autograd of its whole third decoder block,
``ResidualBlock3D(192, 64, stride=1, norm='BN', sn=True)`` (train/scripts/model/submodules.py) in ``.eval().double()`` on
``cat(F.interpolate(x0, size, mode='nearest'), x1)`` with seeded constants on coarse grids, at two small shapes
(tests/dec2_block_ref.py: CASES).

consts.N.npz hold the block's constants (dec2_block_ref.PARAMS: weights on the grid of 64ths, u / v before the call,
BatchNorm weights of both signs, non-trivial statistics), shared by the cases.  Per case NAME.N.npz hold the seeded inputs
x0 [B, 128, L, H0, W0], x1 [B, 64, L, H, W] and upstream [B, 64, L, H, W] f32 and, from the f64 run: ref64_out (the block's
output), the ten parameter gradients ref64_d_* (dec2_block_ref.BLOCK_GRADS) and ref64_u1_after / v1_after / u2_after /
v2_after.  The second case keeps conv1's weight_bar gradient for the input channels of dec2_block_ref.SEAM only (X groups 3
and 4, the seam of the concat): both cases whole would pass the directory's budget of 8 MB.  x1 is nudged until neither
relu has a unit within MARGIN of its kink, so that an f32 forward has the reference's masks.  The maker asserts that the
restatement (tests/dec2_block_ref.block_grads) reproduces the reference.

A file is NAME.N.npz; an array larger than PIECE bytes is split along axis 1 into KEY@0, KEY@1, ...
(tests/make_dec2_conv_goldens.py's piece plan; tests/last_conv_dgrad_ref.load_parts joins them); every file stays under
SIZE_CAP.  Runs where the reference tree is present; not collected by pytest.

    python tests/make_dec2_block_goldens.py [out_dir]   (default tests/golden/.dec2block; V2CE_REFERENCE_ROOT names the tree)
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import dec2_block_ref as R  # noqa: E402
from tests.make_dec2_conv_goldens import grid, save  # noqa: E402
from tests.make_last_conv_goldens import reference_block_class  # noqa: E402

MARGIN = R.MARGIN
C, C0, C1, CIN = R.C, R.C0, R.C1, R.CIN


def inputs(name):
    B, L, H, W = R.CASES[name]
    rng = np.random.default_rng(sorted(R.CASES).index(name) + 5151)
    x0 = np.maximum(grid(rng, (B, C0, L, (H + 1) // 2, (W + 1) // 2), 0.125), 0).astype(np.float32)      # relu-like: dec1's output
    x1 = grid(rng, (B, C1, L, H, W), 0.125)
    upstream = grid(rng, (B, C, L, H, W), 0.125)
    upstream[upstream == 0] = np.float32(0.125)
    return x0, x1, upstream


def block_params():
    """The constants of the block (dec2_block_ref.PARAMS) as f32: weights on the grid of 64ths, u / v normalised, BatchNorm
    weights of both signs and none near zero, non-trivial statistics."""
    g = torch.Generator().manual_seed(6161)
    rn = lambda *s: torch.randn(*s, generator=g)
    unit = lambda v: v / v.norm()
    p = {"weight_bar1": torch.round(rn(C, CIN, 3, 3, 3) * 0.05 * 64) / 64, "u1": unit(rn(C)), "v1": unit(rn(CIN * 27)),
         "short_weight": torch.round(rn(C, CIN, 1, 1, 1) * 0.08 * 64) / 64, "short_bias": 0.1 * rn(C),
         "weight_bar2": torch.round(rn(C, C, 3, 3, 3) * 0.07 * 64) / 64, "u2": unit(rn(C)), "v2": unit(rn(C * 27))}
    for bn in ("bn1", "bnd", "bn2"):
        sign = torch.where(torch.rand(C, generator=g) < 0.25, -1.0, 1.0)
        p[f"{bn}_weight"] = (0.5 + torch.rand(C, generator=g)) * sign
        p[f"{bn}_bias"] = 0.1 * rn(C)
        p[f"{bn}_mean"] = 0.1 * rn(C)
        p[f"{bn}_var"] = 0.5 + torch.rand(C, generator=g)
    p = {k: v.float().numpy() for k, v in p.items()}
    p["eps"] = np.float32(1e-5)
    return p


def concat(x0, x1):
    x0, x1 = torch.from_numpy(x0).double(), torch.from_numpy(x1).double()
    return torch.cat([torch.nn.functional.interpolate(x0, size=tuple(x1.shape[2:]), mode="nearest"), x1], dim=1)


def run_block(cls, p, x0, x1, upstream):
    """A fresh reference block with the constants `p`, run on the concat in f64 -> its output, gradients and u / v as numpy."""
    torch.manual_seed(0)
    blk = cls(CIN, C, stride=1, norm="BN", sn=True).eval()
    assert np.float32(blk.bn1.eps) == p["eps"]
    c1, c2, sc = blk.conv1.module, blk.conv2.module, blk.downsample[0]
    with torch.no_grad():
        for dst, key in ((c1.weight_bar, "weight_bar1"), (c1.weight_u, "u1"), (c1.weight_v, "v1"), (sc.weight, "short_weight"),
                         (sc.bias, "short_bias"), (c2.weight_bar, "weight_bar2"), (c2.weight_u, "u2"), (c2.weight_v, "v2")):
            dst.copy_(torch.from_numpy(p[key]))
        for bn, mod in (("bn1", blk.bn1), ("bnd", blk.downsample[1]), ("bn2", blk.bn2)):
            mod.weight.copy_(torch.from_numpy(p[f"{bn}_weight"]))
            mod.bias.copy_(torch.from_numpy(p[f"{bn}_bias"]))
            mod.running_mean.copy_(torch.from_numpy(p[f"{bn}_mean"]))
            mod.running_var.copy_(torch.from_numpy(p[f"{bn}_var"]))
    blk = blk.double()
    trained = {"d_weight_bar1": c1.weight_bar, "d_short_weight": sc.weight, "d_short_bias": sc.bias, "d_bn1_weight": blk.bn1.weight,
               "d_bn1_bias": blk.bn1.bias, "d_bnd_weight": blk.downsample[1].weight, "d_bnd_bias": blk.downsample[1].bias,
               "d_weight_bar2": c2.weight_bar, "d_bn2_weight": blk.bn2.weight, "d_bn2_bias": blk.bn2.bias}
    for q in trained.values():
        q.requires_grad_(True)
    out = blk(concat(x0, x1))
    out.backward(torch.from_numpy(upstream).double())
    r = {k: q.grad.numpy() for k, q in trained.items()}
    r.update(out=out.detach().numpy(), u1_after=c1.weight_u.detach().numpy().copy(), v1_after=c1.weight_v.detach().numpy().copy(),
             u2_after=c2.weight_u.detach().numpy().copy(), v2_after=c2.weight_v.detach().numpy().copy())
    return r


def settle(name, p, x0, x1):
    """Nudge x1 on its grid until no unit of either relu sits within 4 MARGIN of the kink -> block_forward's result."""
    rng = np.random.default_rng(sorted(R.CASES).index(name) + 7171)
    for _ in range(40):
        f = R.block_forward(x0, x1, p)
        close = (np.abs(f["pre1"]) < 4 * MARGIN) | (np.abs(f["pre"]) < 4 * MARGIN)
        if not close.any():
            return f
        for b, _, l, h, w in np.argwhere(close):
            x1[b, rng.integers(0, C1), l, h, w] += np.float32(0.125)
    raise AssertionError(name)


def main(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    cls = reference_block_class()
    p = block_params()
    save(out_dir, "consts", p)
    for name, (B, L, H, W) in R.CASES.items():
        x0, x1, upstream = inputs(name)
        # ATen's nearest map is dst >> 1 for these sizes: the interpolated tensor is the formula's virtual input
        assert np.array_equal(concat(x0, x1).numpy(), R.U.virtual_input_np(x0, x1).astype(np.float64)), name
        f = settle(name, p, x0, x1)
        for q in (f["pre1"], f["pre"]):
            assert not (np.abs(q) < MARGIN).any() and 0.2 < (q > 0).mean() < 0.8, (name, (q > 0).mean())
        ref = run_block(cls, p, x0, x1, upstream)
        assert np.array_equal(ref["out"] > 0, f["pre"] > 0)
        assert np.abs(f["out"] - ref["out"]).max() <= 1e-11 * np.abs(ref["out"]).max()
        g = R.block_grads(x0, x1, p, upstream, f)
        for k in R.BLOCK_GRADS:
            assert ref[k].shape == g[k].shape and np.abs(g[k] - ref[k]).max() <= 1e-11 * np.abs(ref[k]).max() > 0, (name, k)
        for k, key in (("u1a", "u1_after"), ("v1a", "v1_after"), ("u2a", "u2_after"), ("v2a", "v2_after")):
            assert np.abs(f[k] - ref[key]).max() <= 1e-13, (name, k)
        arrays = dict(x0=x0, x1=x1, upstream=upstream, ref64_out=ref["out"])
        for k in R.BLOCK_GRADS:
            arrays["ref64_" + k] = np.ascontiguousarray(ref[k][:, R.SEAM]) if k in R.SEAM_ONLY.get(name, ()) else ref[k]
        for k in ("u1_after", "v1_after", "u2_after", "v2_after"):
            arrays["ref64_" + k] = ref[k]
        save(out_dir, name, arrays)
    total = sum(os.path.getsize(os.path.join(out_dir, n)) for n in os.listdir(out_dir))
    print("directory", total)
    assert total <= 8 * 2 ** 20, total


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", ".dec2block"))
