"""Recipe of tests/golden/.lastblock/*.npz: inputs of the weight gradients of the last decoder block's conv1 and shortcut
(include/v2ce_hip_convupgrad.h) with torch's own f64 results, and the REFERENCE block's own autograd on the same inputs.

Kernel truths.  ``torch.nn.grad.conv3d_weight`` in f64 on ``cat(F.interpolate(x0, mode='nearest'), x1)`` -- the reference's
own way to the block's input (train/scripts/model/unet_2layer.py:360-361) -- with g1 for the 3x3x3 weight and with gd for
the 1x1x1 weight.  Six files per case, each at most SIZE_CAP bytes (the inputs sit on coarse grids so that the exact f64
sums compress):
  NAME.x.npz    x0 [B, 64, L, H0, W0], x1 [B, 32, L, H, W] f32: the source of the upsampled channels and the skip tensor
  NAME.g.npz    g1, gd [B, 32, L, H, W] f32: the gradients with respect to the two convolutions' raw outputs
  NAME.s.npz    ref64_dMd [32, 96], ref64_d_sum [32], abs_terms_dMd, abs_terms_d_sum: the f64
                results for gd and the f64 sums of |terms|; ref32_dev_dMd, ref32_dev_d_sum: max |f32 run - f64
                run| of the same torch expressions
  NAME.wG.npz   G = 0, 1, 2, the 32-channel groups of the input: ref64_dW_gG, abs_terms_dW_gG [32, 32, 3, 3, 3] and
                ref32_dev_dW_gG for the input channels 32 G .. 32 G + 31 of the 3x3x3 weight gradient
The large case (KERNEL_ONLY: more than V2CE_UPWGRAD_CHAIN positions) carries low mantissa bits in g1 and gd, so that the f32
chains of the kernel do round: the maker asserts that torch's own f32 run is off there.  The zero case has g1 = gd = 0:
every gradient is exactly 0.

Layer truths (not the KERNEL_ONLY case).  The reference's ``ResidualBlock3D(96, 32, stride=1, norm='BN', sn=True)``
(train/scripts/model/submodules.py:210-258, with spectral_norm.py), loaded by path as tests/make_last_conv_goldens.py
loads it, in ``.eval()`` with non-trivial statistics and affine parameters, run as a whole on that concat with ``upstream``
on its output (zero in the zero case), in ``.double()`` and in f32:
  NAME.layer.npz  the block's constants as f32 (tests/last_block_ref.PARAMS: weight_bar1, u1, v1 of conv1 before the call,
                  short_weight, short_bias, bn1_*, bnd_*, weight_bar2, u2, v2, bn2_*, eps); upstream [B, 32, L, H, W] f32;
                  mask_t, mask_y [B, 32, L, H, W] bool: where the block's two relus are active (t > 0 behind bn1, the
                  block's output > 0) in the ``.double()`` run; ref64_<g> for the gradients g of
                  last_block_ref.BLOCK_GRADS except the two weight_bar ones; ref64_/ref32_ u1_after, v1_after, u2_after,
                  v2_after; ref32_dev_<g> of all ten: max |f32 run - f64 run|
  NAME.lwG.npz    ref64_d_weight_bar1_gG [32, 32, 3, 3, 3]: the gradient of conv1's weight_bar, input channels 32 G ..
  NAME.l2.npz     ref64_d_weight_bar2 [32, 32, 3, 3, 3]: the gradient of conv2's weight_bar
x1 is nudged on its grid until no unit of either relu sits within 4 MARGIN of the kink (before the kernel truths are
taken: both kinds of truth share x0 and x1).  The maker asserts that both relu masks are unambiguous (a non-zero
pre-activation is at least MARGIN from 0), that the f32 and f64 runs agree on them, that the restatement
(tests/last_block_ref.py) gives the block's output and gradients, and that the reference's gradient of the normalised
conv1 weight equals rs1 dM1.  Runs where the reference tree is present; not collected by pytest.

    python tests/make_last_block_goldens.py [out_dir]   (default tests/golden/.lastblock; V2CE_REFERENCE_ROOT names the tree)
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import last_block_ref as R  # noqa: E402
from tests.make_last_conv_goldens import MARGIN, reference_block_class  # noqa: E402

SIZE_CAP = 300_000
# name -> (B, L, H, W)
CASES = {
    "b1_l1_1x1": (1, 1, 1, 1),                # H0 = W0 = 1; 26 of 27 taps are pure padding
    "b2_l3_5x7": (2, 3, 5, 7),                # odd H and W: the last source row and column feed one output row and column
    "b1_l2_3x70": (1, 2, 3, 70),              # pitch 96; the width crosses a 64-wide tile and leaves a ragged one; W0 = 35
    "b1_l3_6x64": (1, 3, 6, 64),              # even sizes, one full-width tile: halo column W is padding, source column 31 is not
    "zero": (1, 2, 4, 6),                     # g1 == gd == 0 and upstream == 0: every gradient is exactly 0
    "b1_l3_20x70": (1, 3, 20, 70),            # 4200 positions: one workgroup flushes its f32 chain
}
KERNEL_ONLY = ("b1_l3_20x70",)


def grid(rng, shape, step, scale=1.0):
    return (np.round(rng.standard_normal(shape) * scale / step) * step).astype(np.float32)


def inputs(name):
    """Seeded f32 inputs of a case on coarse grids -> (x0, x1, g1, gd)."""
    B, L, H, W = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 1777)
    step = 0.5 if name in KERNEL_ONLY else 0.125      # (the large case: halves, or its files would not fit the cap)
    x0 = grid(rng, (B, 64, L, (H + 1) // 2, (W + 1) // 2), step)
    x1 = grid(rng, (B, 32, L, H, W), step)
    g1, gd = grid(rng, (B, 32, L, H, W), step), grid(rng, (B, 32, L, H, W), step)
    if name in KERNEL_ONLY:
        # low mantissa bits at little entropy: the products are not exact in f32 any more, so the chains do round
        g1 = (g1 * (1 + rng.integers(0, 4, g1.shape) * 2.0 ** -18)).astype(np.float32)
        gd = (gd * (1 + rng.integers(0, 4, gd.shape) * 2.0 ** -18)).astype(np.float32)
    if name == "zero":
        g1, gd = np.zeros_like(g1), np.zeros_like(gd)
    return x0, x1, g1, gd


def concat(x0, x1, dtype):
    """The reference's way to the block's input: nearest upsample to the skip's size, then cat."""
    a, b = torch.from_numpy(x0).to(dtype), torch.from_numpy(x1).to(dtype)
    return torch.cat([F.interpolate(a, size=tuple(b.shape[2:]), mode="nearest"), b], dim=1)


def torch_wgrads(X, g1, gd, dtype):
    """torch's own weight gradients -> (dW [32, 96, 3, 3, 3], d_short [32, 96], d_short_bias [32])."""
    X, g1, gd = X.to(dtype), torch.from_numpy(g1).to(dtype), torch.from_numpy(gd).to(dtype)
    dw = torch.nn.grad.conv3d_weight(X, (32, 96, 3, 3, 3), g1, padding=1)
    ds = torch.nn.grad.conv3d_weight(X, (32, 96, 1, 1, 1), gd)
    return dw.numpy(), ds.reshape(32, 96).numpy(), gd.sum(dim=(0, 2, 3, 4)).numpy()


def kernel_arrays(x0, x1, g1, gd):
    """-> (arrays of NAME.s.npz, [arrays of NAME.wG.npz for G = 0, 1, 2])."""
    X = concat(x0, x1, torch.float64)
    w64, s64, b64 = torch_wgrads(X, g1, gd, torch.float64)
    w32, s32, b32 = torch_wgrads(X, g1, gd, torch.float32)
    aw, asr, ab = torch_wgrads(X.abs(), np.abs(g1), np.abs(gd), torch.float64)
    garr = {"ref64_dMd": s64, "ref64_d_sum": b64, "abs_terms_dMd": asr, "abs_terms_d_sum": ab,
            "ref32_dev_dMd": np.abs(s32.astype(np.float64) - s64).max(),
            "ref32_dev_d_sum": np.abs(b32.astype(np.float64) - b64).max()}
    warrs = []
    for g in range(3):
        sl = slice(32 * g, 32 * g + 32)
        warrs.append({f"ref64_dW_g{g}": np.ascontiguousarray(w64[:, sl]), f"abs_terms_dW_g{g}": np.ascontiguousarray(aw[:, sl]),
                      f"ref32_dev_dW_g{g}": np.abs(w32[:, sl].astype(np.float64) - w64[:, sl]).max()})
    return garr, warrs


def block_params(name):
    """The constants of the block (last_block_ref.PARAMS) as f32: weights on the grid of 64ths, u / v normalised, BatchNorm
    weights of both signs and none near zero, non-trivial statistics."""
    g = torch.Generator().manual_seed(sorted(CASES).index(name) + 2929)
    rn = lambda *s: torch.randn(*s, generator=g)
    unit = lambda v: v / v.norm()
    p = {"weight_bar1": torch.round(rn(32, 96, 3, 3, 3) * 0.06 * 64) / 64, "u1": unit(rn(32)), "v1": unit(rn(96 * 27)),
         "short_weight": torch.round(rn(32, 96, 1, 1, 1) * 0.1 * 64) / 64, "short_bias": 0.1 * rn(32),
         "weight_bar2": torch.round(rn(32, 32, 3, 3, 3) * 0.1 * 64) / 64, "u2": unit(rn(32)), "v2": unit(rn(32 * 27))}
    for bn in ("bn1", "bnd", "bn2"):
        sign = torch.where(torch.rand(32, generator=g) < 0.25, -1.0, 1.0)
        p[f"{bn}_weight"] = (0.5 + torch.rand(32, generator=g)) * sign
        p[f"{bn}_bias"] = 0.1 * rn(32)
        p[f"{bn}_mean"] = 0.1 * rn(32)
        p[f"{bn}_var"] = 0.5 + torch.rand(32, generator=g)
    p = {k: v.float().numpy() for k, v in p.items()}
    p["eps"] = np.float32(1e-5)
    return p


def run_block(cls, p, x0, x1, upstream, double):
    """A fresh reference block with the constants `p`, run on the concat -> its output, gradients and u / v as numpy."""
    dtype = torch.float64 if double else torch.float32
    torch.manual_seed(0)
    blk = cls(96, 32, stride=1, norm="BN", sn=True).eval()
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
    if double:
        blk = blk.double()
    trained = {"d_weight_bar1": c1.weight_bar, "d_short_weight": sc.weight, "d_short_bias": sc.bias, "d_bn1_weight": blk.bn1.weight,
               "d_bn1_bias": blk.bn1.bias, "d_bnd_weight": blk.downsample[1].weight, "d_bnd_bias": blk.downsample[1].bias,
               "d_weight_bar2": c2.weight_bar, "d_bn2_weight": blk.bn2.weight, "d_bn2_bias": blk.bn2.bias}
    for q in trained.values():
        q.requires_grad_(True)
    inner_forward = c1.forward

    def forward_keeping_the_weights_gradient(*args):     # (SpectralNorm calls module.forward itself: hooks do not fire)
        c1.weight.retain_grad()
        return inner_forward(*args)
    c1.forward = forward_keeping_the_weights_gradient
    kept = {}

    def keep_t(mod, args, out):                          # the block's one relu module runs twice: t is its first output
        kept.setdefault("t", out.detach().clone())
    blk.relu.register_forward_hook(keep_t)
    feat = blk(concat(x0, x1, dtype))
    feat.backward(torch.from_numpy(upstream).to(dtype))
    out = {k: q.grad.numpy() for k, q in trained.items()}
    out.update(feat=feat.detach().numpy(), t=kept["t"].numpy(), d_W1=c1.weight.grad.numpy(),
               u1_after=c1.weight_u.detach().numpy().copy(), v1_after=c1.weight_v.detach().numpy().copy(),
               u2_after=c2.weight_u.detach().numpy().copy(), v2_after=c2.weight_v.detach().numpy().copy())
    return out


def settle(name, p, x0, x1):
    """Nudge x1 on its grid until no unit of either relu sits within 4 MARGIN of the kink -> block_forward's result."""
    rng = np.random.default_rng(sorted(CASES).index(name) + 3939)
    for _ in range(40):
        f = R.block_forward(x0, x1, p)
        close = (np.abs(f["pre1"]) < 4 * MARGIN) | (np.abs(f["pre"]) < 4 * MARGIN)
        if not close.any():
            return f
        for b, _, l, h, w in np.argwhere(close):
            x1[b, rng.integers(0, 32), l, h, w] += np.float32(0.125)
    raise AssertionError(name)


def layer_arrays(cls, name, p, x0, x1, f):
    """-> (arrays of NAME.layer.npz, [NAME.lwG.npz for G = 0, 1, 2], NAME.l2.npz)."""
    B, L, H, W = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 4949)
    upstream = grid(rng, (B, 32, L, H, W), 0.125)
    upstream[upstream == 0] = np.float32(0.125)
    if name == "zero":
        upstream = np.zeros_like(upstream)
    r64, r32 = run_block(cls, p, x0, x1, upstream, True), run_block(cls, p, x0, x1, upstream, False)
    assert r64["feat"].dtype == np.float64 and r32["feat"].dtype == np.float32
    # the restatement is the block: output, masks, gradients
    assert np.abs(f["feat"] - r64["feat"]).max() <= 1e-12 * max(1.0, np.abs(f["feat"]).max()), name
    assert np.abs(f["t"] - r64["t"]).max() <= 1e-12 * max(1.0, np.abs(f["t"]).max()), name
    for mask, a, b in ((f["pre1"] > 0, r32["t"], r64["t"]), (f["pre"] > 0, r32["feat"], r64["feat"])):
        assert np.array_equal(a > 0, mask) and np.array_equal(b > 0, mask), name
        assert 0.2 < mask.mean() < 0.8, (name, mask.mean())
    for q in (f["pre1"], f["pre"]):
        assert np.abs(q[q != 0]).min() >= MARGIN, name
    y = r64["feat"].astype(np.float32)
    assert np.array_equal(y > 0, f["pre"] > 0)
    g = R.block_grads(x0, x1, p, upstream, f)
    for k in R.BLOCK_GRADS:
        assert np.abs(g[k] - r64[k]).max() <= 1e-11 * max(np.abs(r64[k]).max(), 1e-300), (name, k)
    # the reference's gradient with respect to the normalised conv1 weight is rs1 dM1
    want_dW = f["rs1"][:, None, None, None, None] * g["dM1"]
    assert np.abs(r64["d_W1"] - want_dW).max() <= 1e-12 * max(1.0, np.abs(want_dW).max()), name
    if name == "zero":
        assert not any(r64[k].any() for k in R.BLOCK_GRADS)
    else:
        assert all(np.abs(r64[k]).max() > 0 for k in R.BLOCK_GRADS), name
    larr = dict(p, upstream=upstream, mask_t=f["pre1"] > 0, mask_y=y > 0)
    for k in R.BLOCK_GRADS:
        if k not in ("d_weight_bar1", "d_weight_bar2"):
            larr[f"ref64_{k}"] = r64[k]
        larr[f"ref32_dev_{k}"] = np.abs(r32[k].astype(np.float64) - r64[k]).max()
    for k in ("u1_after", "v1_after", "u2_after", "v2_after"):
        larr[f"ref64_{k}"], larr[f"ref32_{k}"] = r64[k], r32[k]
    lw = [{f"ref64_d_weight_bar1_g{G}": np.ascontiguousarray(r64["d_weight_bar1"][:, 32 * G:32 * G + 32])} for G in range(3)]
    return larr, lw, {"ref64_d_weight_bar2": r64["d_weight_bar2"]}


def save(path, arrays):
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    print(path, size)
    assert size <= SIZE_CAP, (path, size)


def main(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    cls = reference_block_class()
    for name, (B, L, H, W) in CASES.items():
        x0, x1, g1, gd = inputs(name)
        # ATen's nearest map is dst >> 1 for these sizes: the interpolated tensor is the formula's virtual input
        up = concat(x0, x1, torch.float32)[:, :64].numpy()
        assert np.array_equal(up, x0[:, :, :, np.arange(H) >> 1][:, :, :, :, np.arange(W) >> 1]), name
        if name not in KERNEL_ONLY:
            p = block_params(name)
            f = settle(name, p, x0, x1)
            larr, lw, l2 = layer_arrays(cls, name, p, x0, x1, f)
            save(os.path.join(out_dir, f"{name}.layer.npz"), larr)
            for G, w in enumerate(lw):
                save(os.path.join(out_dir, f"{name}.lw{G}.npz"), w)
            save(os.path.join(out_dir, f"{name}.l2.npz"), l2)
        garr, warrs = kernel_arrays(x0, x1, g1, gd)
        if name in KERNEL_ONLY:
            assert B * L * H * W > 4096 and max(float(w[f"ref32_dev_dW_g{g}"]) for g, w in enumerate(warrs)) > 0, name
            assert float(garr["ref32_dev_dMd"]) > 0, name
        if name == "zero":
            assert not garr["ref64_dMd"].any() and not any(w[f"ref64_dW_g{g}"].any() for g, w in enumerate(warrs))
        save(os.path.join(out_dir, f"{name}.x.npz"), {"x0": x0, "x1": x1})
        save(os.path.join(out_dir, f"{name}.g.npz"), {"g1": g1, "gd": gd})
        save(os.path.join(out_dir, f"{name}.s.npz"), garr)
        for g, w in enumerate(warrs):
            save(os.path.join(out_dir, f"{name}.w{g}.npz"), w)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", ".lastblock"))
