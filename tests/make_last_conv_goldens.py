"""Recipe of tests/golden/.lastconv/*.npz: inputs of the last decoder convolution with the REFERENCE block's own results.

The reference's ``ResidualBlock3D(96, 32, stride=1, norm='BN', sn=True)`` (train/scripts/model/submodules.py:210-258, with
spectral_norm.py) is loaded by path, as tests/make_pred_head_goldens.py loads its layer; it is put in ``.eval()`` with
non-trivial running statistics and affine parameters.  The block runs as a whole; a pre-hook on ``conv2`` and a hook on
``downsample`` put the stored f32 ``t`` and ``res`` in the places of relu(bn1(conv1 x)) and of the shortcut branch, so what
is recorded is the reference's own conv2 (one spectral-norm iteration included) -> bn2 -> add -> relu and its autograd.

Three files per case, each at most SIZE_CAP bytes (the inputs sit on coarse grids so that the exact f64 sums compress):
  NAME.npz        the kernel's view: t, res, y, upstream [B, 32, L, H, W] f32 (y = the f32-rounded ref64_feat);
                  ref64_feat: the block's output in ``.double()``, ref32_dev_feat: max |f32 run - f64 run| of it;
                  ref64_dM [32, 32, 3, 3, 3], ref64_d_shift [32]: the gradient with respect to conv2's output of
                  torch's own f64 conv3d, through the relu mask; abs_terms_dM, abs_terms_d_shift: the f64 sums of |terms|;
                  ref32_dev_dM, ref32_dev_d_shift: max |f32 run - f64 run| of the same torch expressions
  NAME.plain.npz  ref64_dM_plain, ... : the same six results without the mask (y == NULL)
  NAME.layer.npz  weight_bar, u, v (before the call), bn_weight, bn_bias, running_mean, running_var, eps as f32;
                  ref64_d_weight_bar, ref64_d_bn_weight, ref64_d_bn_bias, ref64_u_after, ref64_v_after: the block in
                  ``.double()``; ref32_u_after, ref32_v_after and ref32_dev_<d_weight_bar, d_bn_weight, d_bn_bias>: the
                  block in f32 and max |f32 run - f64 run|
The kernel-only case (KERNEL_ONLY: 4200 positions, more than V2CE_WGRAD_CHAIN) has its inputs (t, y, upstream; y a
synthetic relu-like tensor) in NAME.npz and its results in NAME.truth.npz; upstream carries low mantissa bits there, so
that the f32 chains of the kernel do round.  The maker asserts that the f32 and f64 runs agree on which units are active, that a non-zero
pre-activation is at least MARGIN from 0, and that the reference's gradient with respect to the normalised weight equals
scale * ref64_dM.  Runs where the reference tree is present; not collected by pytest.

    python tests/make_last_conv_goldens.py [out_dir]   (default tests/golden/.lastconv; V2CE_REFERENCE_ROOT names the tree)
"""
import importlib
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("V2CE_REFERENCE_ROOT", "/root/reference")
SIZE_CAP = 300_000
MARGIN = 1e-4
# name -> (B, L, H, W)
CASES = {
    "b1_l1_1x1": (1, 1, 1, 1),                # 26 of 27 taps are pure padding
    "b2_l3_5x7": (2, 3, 5, 7),                # batch and time boundaries
    "b1_l2_3x70": (1, 2, 3, 70),              # pitch 96; the width crosses a 64-wide tile and leaves a ragged one
    "b1_l3_5x33": (1, 3, 5, 33),              # odd H against a two-row tile
    "inactive": (1, 2, 5, 9),                 # feat == 0 everywhere: every gradient is exactly 0
    "b1_l3_20x70": (1, 3, 20, 70),            # 4200 positions: one workgroup flushes its f32 chain
}
KERNEL_ONLY = ("b1_l3_20x70",)


def reference_block_class():
    pkg = types.ModuleType("ref_model")
    pkg.__path__ = [os.path.join(REF, "train", "scripts", "model")]
    sys.modules["ref_model"] = pkg
    return importlib.import_module("ref_model.submodules").ResidualBlock3D


def grid(rng, shape, step, scale=1.0):
    return (np.round(rng.standard_normal(shape) * scale / step) * step).astype(np.float32)


def inputs(name):
    """Seeded f32 inputs of a case on coarse grids: t relu-like (exact zeros), upstream in eighths."""
    B, L, H, W = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 777)
    step = 0.5 if name in KERNEL_ONLY else 0.125      # (the large case: halves, or its file would not fit the cap)
    t = np.maximum(grid(rng, (B, 32, L, H, W), step), 0).astype(np.float32)
    res = grid(rng, (B, 32, L, H, W), 1.0 / 64, 0.5)
    upstream = grid(rng, (B, 32, L, H, W), step)
    upstream[upstream == 0] = np.float32(step)
    if name in KERNEL_ONLY:
        # low mantissa bits at little entropy: the products are not exact in f32 any more, so the chains do round
        upstream = (upstream * (1 + rng.integers(0, 4, upstream.shape) * 2.0 ** -18)).astype(np.float32)
    if name == "inactive":
        res = -np.abs(res) - np.float32(1000.0)
    return t, res, upstream


def make_block(cls, seed):
    torch.manual_seed(seed)
    blk = cls(96, 32, stride=1, norm="BN", sn=True).eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        m = blk.conv2.module
        m.weight_bar.copy_(torch.round(torch.randn(m.weight_bar.shape, generator=g) * 0.1 * 64) / 64)
        u, v = torch.randn(32, generator=g), torch.randn(864, generator=g)
        m.weight_u.copy_(u / u.norm())
        m.weight_v.copy_(v / v.norm())
        blk.bn2.weight.copy_(1.0 + 0.3 * torch.randn(32, generator=g))
        blk.bn2.bias.copy_(0.1 * torch.randn(32, generator=g))
        blk.bn2.running_mean.copy_(0.1 * torch.randn(32, generator=g))
        blk.bn2.running_var.copy_(0.5 + torch.rand(32, generator=g))
    return blk


def run_block(blk, t, res, upstream, double):
    """The reference block (a fresh one per run: the call advances its u / v) with t and res substituted -> its outputs
    and gradients as numpy arrays."""
    cast = (lambda a: torch.from_numpy(a).double()) if double else (lambda a: torch.from_numpy(a).clone())
    if double:
        blk = blk.double()
    blk.conv2.module.weight_bar.requires_grad_(True)
    blk.bn2.weight.requires_grad_(True)
    blk.bn2.bias.requires_grad_(True)
    tt, rr = cast(t), cast(res)
    blk.conv2.register_forward_pre_hook(lambda mod, args: (tt,))
    blk.downsample.register_forward_hook(lambda mod, args, out: rr.clone())
    inner, inner_forward = blk.conv2.module, blk.conv2.module.forward

    def forward_keeping_the_weights_gradient(*args):     # (SpectralNorm calls module.forward itself: hooks do not fire)
        inner.weight.retain_grad()
        return inner_forward(*args)
    inner.forward = forward_keeping_the_weights_gradient
    x = torch.zeros((t.shape[0], 96) + t.shape[2:], dtype=tt.dtype)
    feat = blk(x)
    feat.backward(cast(upstream))
    m = blk.conv2.module
    return {"feat": feat.detach().numpy(), "d_weight_bar": m.weight_bar.grad.numpy(), "d_bn_weight": blk.bn2.weight.grad.numpy(),
            "d_bn_bias": blk.bn2.bias.grad.numpy(), "u_after": m.weight_u.detach().numpy().copy(),
            "v_after": m.weight_v.detach().numpy().copy(), "d_W": m.weight.grad.numpy()}


def torch_wgrad(t, m, dtype):
    """torch's own conv3d weight gradient and the channel sums -> (dM [32, 32, 3, 3, 3], d_shift [32])."""
    w = torch.zeros((32, 32, 3, 3, 3), dtype=dtype, requires_grad=True)
    z = F.conv3d(torch.from_numpy(t).to(dtype), w, padding=1)
    z.backward(torch.from_numpy(m).to(dtype))
    return w.grad.numpy(), torch.from_numpy(m).to(dtype).sum(dim=(0, 2, 3, 4)).numpy()


def kernel_arrays(t, y, upstream):
    """y None: no mask (the *_plain truth)."""
    out = {"t": t, "y": y, "upstream": upstream} if y is not None else {}
    for sfx in (("",) if y is not None else ("_plain",)):
        m = np.where(y > 0, upstream, np.float32(0)) if y is not None else upstream
        d64, s64 = torch_wgrad(t, m, torch.float64)
        d32, s32 = torch_wgrad(t, m, torch.float32)
        a64, as64 = torch_wgrad(np.abs(t), np.abs(m), torch.float64)
        out.update({f"ref64_dM{sfx}": d64, f"ref64_d_shift{sfx}": s64, f"abs_terms_dM{sfx}": a64,
                    f"abs_terms_d_shift{sfx}": as64,
                    f"ref32_dev_dM{sfx}": np.abs(d32.astype(np.float64) - d64).max(),
                    f"ref32_dev_d_shift{sfx}": np.abs(s32.astype(np.float64) - s64).max()})
    return out


def save(path, arrays):
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    print(path, size)
    assert size <= SIZE_CAP, (path, size)


def main(out_dir):
    sys.path.insert(0, ROOT)
    from tests import last_conv_ref as R
    os.makedirs(out_dir, exist_ok=True)
    cls = reference_block_class()
    for name in CASES:
        t, res, upstream = inputs(name)
        if name in KERNEL_ONLY:
            rng = np.random.default_rng(99)
            y = np.maximum(grid(rng, t.shape, 0.5), 0).astype(np.float32)
            karr = kernel_arrays(t, y, upstream)
            save(os.path.join(out_dir, f"{name}.npz"), {k: karr.pop(k) for k in ("t", "y", "upstream")})
            save(os.path.join(out_dir, f"{name}.truth.npz"), karr)
            continue
        blk = make_block(cls, sorted(CASES).index(name) + 31)          # (read only: the runs below build their own)
        m, bn = blk.conv2.module, blk.bn2
        before = {"weight_bar": m.weight_bar.detach().numpy().copy(), "u": m.weight_u.detach().numpy().copy(),
                  "v": m.weight_v.detach().numpy().copy(), "bn_weight": bn.weight.detach().numpy().copy(),
                  "bn_bias": bn.bias.detach().numpy().copy(), "running_mean": bn.running_mean.numpy().copy(),
                  "running_var": bn.running_var.numpy().copy(), "eps": np.float32(bn.eps)}
        # the restatement's pre-activation: nudge res until no unit sits within MARGIN of the relu's kink
        u1, v1 = R.power_iteration(before["weight_bar"], before["u"], before["v"])
        W, sigma, scale, shift = R.effective(before["weight_bar"], u1, v1, before["bn_weight"], before["bn_bias"],
                                             before["running_mean"], before["running_var"], before["eps"])
        for _ in range(8):
            _, pre = R.forward(t, res, W, scale, shift)
            close = (np.abs(pre) < 4 * MARGIN)
            if not close.any():
                break
            res[close] += np.float32(1.0 / 64)
        seed = sorted(CASES).index(name) + 31
        r64, r32 = run_block(make_block(cls, seed), t, res, upstream, True), run_block(make_block(cls, seed), t, res, upstream, False)
        assert r64["feat"].dtype == np.float64 and r32["feat"].dtype == np.float32
        feat_own, pre = R.forward(t, res, W, scale, shift)
        assert np.abs(feat_own - r64["feat"]).max() <= 1e-12 * max(1.0, np.abs(feat_own).max()), name
        assert np.array_equal(r32["feat"] > 0, pre > 0) and np.array_equal(r64["feat"] > 0, pre > 0), name
        nz = pre[pre != 0]
        assert np.abs(nz).min() >= MARGIN, (name, np.abs(nz).min())
        y = r64["feat"].astype(np.float32)
        assert np.array_equal(y > 0, pre > 0)
        karr = kernel_arrays(t, y, upstream)
        # the reference's gradient with respect to the normalised weight is scale * dM
        want_dW = scale[:, None, None, None, None] * karr["ref64_dM"]
        assert np.abs(r64["d_W"] - want_dW).max() <= 1e-12 * max(1.0, np.abs(want_dW).max()), name
        if name == "inactive":
            assert not r64["feat"].any() and not r64["d_weight_bar"].any() and not karr["ref64_dM"].any()
        else:
            assert (r64["feat"] > 0).mean() > 0.2, name
        karr["res"], karr["ref64_feat"] = res, r64["feat"]
        karr["ref32_dev_feat"] = np.abs(r32["feat"].astype(np.float64) - r64["feat"]).max()
        save(os.path.join(out_dir, f"{name}.npz"), karr)
        save(os.path.join(out_dir, f"{name}.plain.npz"), kernel_arrays(t, None, upstream))
        larr = dict(before)
        for k in ("d_weight_bar", "d_bn_weight", "d_bn_bias"):
            larr[f"ref64_{k}"] = r64[k]
            larr[f"ref32_dev_{k}"] = np.abs(r32[k].astype(np.float64) - r64[k]).max()
        for k in ("u_after", "v_after"):
            larr[f"ref64_{k}"], larr[f"ref32_{k}"] = r64[k], r32[k]
        save(os.path.join(out_dir, f"{name}.layer.npz"), larr)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", ".lastconv"))
