"""Recipe of tests/golden/.lastconv_dgrad/*.npz: truths of the input gradient of the last decoder convolution and of the
last decoder block's other two BatchNorms, for the cases of tests/make_last_conv_goldens.py by name.

  NAME.dx.K.npz     the kernel's view, on the t / y / upstream of tests/golden/.lastconv/NAME.npz: weight [32, 32, 3, 3, 3] f32
                    as the kernel gets it (a coarse grid; in the KERNEL_ONLY case it also carries low mantissa bits, so that
                    f32 sums of the terms do round); ref64_dx [B, 32, L, H, W]: torch's own f64 conv3d input gradient
                    through the relu mask; abs_terms_dx: the f64 sums of |terms|; ref32_dev_dx: max |f32 run - f64 run| of
                    the same torch expression; and the same three with the suffix _plain, without the mask (y == NULL;
                    not in the KERNEL_ONLY case)
  NAME.block.K.npz  (not the KERNEL_ONLY case) the REFERENCE's ``ResidualBlock3D(96, 32, norm='BN', sn=True)``, loaded by
                    path as the other maker does, in ``.eval()``, as a whole: hooks on ``conv1`` and ``downsample[0]`` put
                    the stored f32 c1 and cd in the places of the two convolutions' outputs.  conv2 and bn2 are those of
                    tests/golden/.lastconv/NAME.layer.npz (the maker asserts it), upstream that of NAME.npz.  bn1_weight,
                    bn1_bias, bn1_mean, bn1_var, bnd_weight, bnd_bias, bnd_mean, bnd_var as f32; y_block: the block's
                    output in ``.double()``, rounded to f32; ref64_d_t, ref64_d_res: the gradients of relu(bn1(c1)) and of
                    the downsample branch's output; ref64_d_bn1_weight, ref64_d_bn1_bias, ref64_d_bnd_weight,
                    ref64_d_bnd_bias; ref32_dev_* of the six: max |f32 run - f64 run|
A file holds at most SIZE_CAP bytes: the arrays of a kind are spread over NAME.KIND.0.npz, NAME.KIND.1.npz, ..., and an array
too large for one file is cut along its channel axis into NAME@0, NAME@1, ... (tests/last_conv_dgrad_ref.load_parts joins
them).  The maker asserts that the f32 and f64 runs agree on both relu masks, that a non-zero pre-activation of either relu
is at least MARGIN from 0, and that the restatement (tests/last_conv_dgrad_ref.py) gives the block's gradients.  Runs where
the reference tree is present; not collected by pytest.

    python tests/make_last_conv_dgrad_goldens.py [out_dir]   (default tests/golden/.lastconv_dgrad)
"""
import io
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import last_conv_dgrad_ref as D  # noqa: E402
from tests import last_conv_ref as R  # noqa: E402
from tests.make_last_conv_goldens import CASES, KERNEL_ONLY, MARGIN, SIZE_CAP, grid, make_block, reference_block_class  # noqa: E402

BLOCK_GRADS = ("d_t", "d_res", "d_bn1_weight", "d_bn1_bias", "d_bnd_weight", "d_bnd_bias")


def packed_size(arrays):
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    return buf.getbuffer().nbytes


def save_parts(base, arrays):
    """Spread `arrays` over base.0.npz, base.1.npz, ... of at most SIZE_CAP bytes each."""
    room = SIZE_CAP - 4096
    pieces = []
    for k, v in arrays.items():
        v = np.asarray(v)
        n = 1
        while v.ndim == 5 and n < v.shape[1] and max(packed_size({k: c}) for c in np.array_split(v, n, axis=1)) > room // 2:
            n *= 2
        pieces += [(k, v)] if n == 1 else [(f"{k}@{i}", c) for i, c in enumerate(np.array_split(v, n, axis=1))]
    files, cur = [], {}
    for k, v in pieces:
        if cur and packed_size({**cur, k: v}) > room:
            files.append(cur)
            cur = {}
        cur[k] = v
    files.append(cur)
    for i, f in enumerate(files):
        path = f"{base}.{i}.npz"
        np.savez_compressed(path, **f)
        size = os.path.getsize(path)
        print(path, size)
        assert size <= SIZE_CAP, (path, size)


def kernel_weight(name):
    rng = np.random.default_rng(sorted(CASES).index(name) + 4242)
    w = grid(rng, (32, 32, 3, 3, 3), 1.0 / 64, 0.1)
    if name in KERNEL_ONLY:
        w = (w * (1 + rng.integers(0, 4, w.shape) * 2.0 ** -18)).astype(np.float32)
    return w


def torch_dgrad(weight, m, dtype):
    """torch's own conv3d input gradient -> d_x [B, 32, L, H, W]."""
    x = torch.zeros(m.shape, dtype=dtype, requires_grad=True)
    z = F.conv3d(x, torch.from_numpy(weight).to(dtype), padding=1)
    z.backward(torch.from_numpy(m).to(dtype))
    return x.grad.numpy()


def kernel_arrays(weight, y, upstream, variants=("", "_plain")):
    out = {"weight": weight}
    for sfx in variants:
        m = upstream if sfx else np.where(y > 0, upstream, np.float32(0))
        d64, d32 = torch_dgrad(weight, m, torch.float64), torch_dgrad(weight, m, torch.float32)
        out.update({f"ref64_dx{sfx}": d64, f"abs_terms_dx{sfx}": torch_dgrad(np.abs(weight), np.abs(m), torch.float64),
                    f"ref32_dev_dx{sfx}": np.abs(d32.astype(np.float64) - d64).max()})
    return out


def norm_params(name):
    """Non-trivial statistics and affine parameters (weights of both signs, none near zero) of bn1 and downsample[1]."""
    g = torch.Generator().manual_seed(sorted(CASES).index(name) + 5151)
    p = {}
    for bn in ("bn1", "bnd"):
        sign = torch.where(torch.rand(32, generator=g) < 0.25, -1.0, 1.0)
        p[f"{bn}_weight"] = ((0.5 + torch.rand(32, generator=g)) * sign).numpy()
        p[f"{bn}_bias"] = (0.1 * torch.randn(32, generator=g)).numpy()
        p[f"{bn}_mean"] = (0.1 * torch.randn(32, generator=g)).numpy()
        p[f"{bn}_var"] = (0.5 + torch.rand(32, generator=g)).numpy()
    return p


def run_block(blk, p, c1, cd, upstream, double):
    """The reference block (a fresh one per run) with c1 and cd substituted -> its output and gradients as numpy arrays."""
    cast = (lambda a: torch.from_numpy(np.asarray(a)).double()) if double else (lambda a: torch.from_numpy(np.asarray(a)).clone())
    with torch.no_grad():
        for bn, mod in (("bn1", blk.bn1), ("bnd", blk.downsample[1])):
            mod.weight.copy_(torch.from_numpy(p[f"{bn}_weight"]))
            mod.bias.copy_(torch.from_numpy(p[f"{bn}_bias"]))
            mod.running_mean.copy_(torch.from_numpy(p[f"{bn}_mean"]))
            mod.running_var.copy_(torch.from_numpy(p[f"{bn}_var"]))
    if double:
        blk = blk.double()
    for q in (blk.bn1.weight, blk.bn1.bias, blk.downsample[1].weight, blk.downsample[1].bias):
        q.requires_grad_(True)
    cc1, ccd = cast(c1), cast(cd)
    blk.conv1.register_forward_hook(lambda mod, args, out: cc1.clone())
    blk.downsample[0].register_forward_hook(lambda mod, args, out: ccd.clone())
    kept = {}

    def keep_t(mod, args, out):                              # the block's one relu module runs twice: t is its first output
        if "t" not in kept:
            out.retain_grad()
            kept["t"] = out

    def keep_res(mod, args, out):
        out.retain_grad()
        kept["res"] = out
    blk.relu.register_forward_hook(keep_t)
    blk.downsample.register_forward_hook(keep_res)
    x = torch.zeros((c1.shape[0], 96) + c1.shape[2:], dtype=cc1.dtype)
    feat = blk(x)
    feat.backward(cast(upstream))
    bn1, bnd = blk.bn1, blk.downsample[1]
    return {"feat": feat.detach().numpy(), "t": kept["t"].detach().numpy(), "res": kept["res"].detach().numpy(),
            "d_t": kept["t"].grad.numpy(), "d_res": kept["res"].grad.numpy(), "d_bn1_weight": bn1.weight.grad.numpy(),
            "d_bn1_bias": bn1.bias.grad.numpy(), "d_bnd_weight": bnd.weight.grad.numpy(), "d_bnd_bias": bnd.bias.grad.numpy()}


def block_arrays(cls, name):
    z = R.load_case(name)
    B, L, H, W = CASES[name]
    seed = sorted(CASES).index(name) + 31
    blk = make_block(cls, seed)
    m, bn2 = blk.conv2.module, blk.bn2
    for got, key in ((m.weight_bar, "weight_bar"), (m.weight_u, "u"), (m.weight_v, "v"), (bn2.weight, "bn_weight"),
                     (bn2.bias, "bn_bias"), (bn2.running_mean, "running_mean"), (bn2.running_var, "running_var")):
        assert np.array_equal(got.detach().numpy(), z[key]), (name, key)        # the layer of .lastconv/NAME.layer.npz
    p = norm_params(name)
    rng = np.random.default_rng(sorted(CASES).index(name) + 6161)
    c1, cd = grid(rng, (B, 32, L, H, W), 0.125), grid(rng, (B, 32, L, H, W), 1.0 / 64, 0.5)
    eps = float(blk.bn1.eps)
    if name == "inactive":                                   # res about -1000: the block's output is 0 everywhere
        rs = 1.0 / np.sqrt(p["bnd_var"].astype(np.float64) + eps)
        target = D.bc(p["bnd_mean"]) + (-1000.0 - np.abs(cd) - D.bc(p["bnd_bias"])) / D.bc(p["bnd_weight"] * rs)
        cd = (np.round(target * 64) / 64).astype(np.float32)
    u1, v1 = R.power_iteration(z["weight_bar"], z["u"], z["v"])
    W2, sigma, scale, shift = R.effective(z["weight_bar"], u1, v1, z["bn_weight"], z["bn_bias"], z["running_mean"],
                                          z["running_var"], z["eps"])
    for _ in range(8):                                       # nudge until no unit sits within MARGIN of either relu's kink
        z1, zd = D.normed(c1, p["bn1_mean"], p["bn1_var"], eps), D.normed(cd, p["bnd_mean"], p["bnd_var"], eps)
        t, res, pre1 = D.tail_forward(z1, zd, p["bn1_weight"], p["bn1_bias"], p["bnd_weight"], p["bnd_bias"])
        close1 = np.abs(pre1) < 4 * MARGIN
        c1[close1] += np.float32(0.125)
        if close1.any():
            continue
        _, pre = R.forward(t, res, W2, scale, shift)
        close = np.abs(pre) < 4 * MARGIN
        if not close.any():
            break
        cd[close] += np.float32(1.0 / 64)
    else:
        raise AssertionError(name)
    r64 = run_block(make_block(cls, seed), p, c1, cd, z["upstream"], True)
    r32 = run_block(make_block(cls, seed), p, c1, cd, z["upstream"], False)
    assert r64["feat"].dtype == np.float64 and r32["feat"].dtype == np.float32
    assert np.abs(t - r64["t"]).max() <= 1e-12 * max(1.0, np.abs(t).max()) and np.abs(res - r64["res"]).max() <= 1e-12 * np.abs(res).max()
    feat_own, pre = R.forward(t, res, W2, scale, shift)
    assert np.abs(feat_own - r64["feat"]).max() <= 1e-12 * max(1.0, np.abs(feat_own).max()), name
    for mask, a, b in ((pre1 > 0, r32["t"], r64["t"]), (pre > 0, r32["feat"], r64["feat"])):
        assert np.array_equal(a > 0, mask) and np.array_equal(b > 0, mask), name
    for q in (pre1, pre):
        assert np.abs(q[q != 0]).min() >= MARGIN, name
    y = r64["feat"].astype(np.float32)
    assert np.array_equal(y > 0, pre > 0)
    # the restatement gives the block's own gradients
    g = D.dgrad(scale[:, None, None, None, None] * W2, y, z["upstream"])
    tg = D.tail_grads(z1, zd, p["bn1_weight"], p["bn1_bias"], g["d_x"], g["d_res"])
    for k, got in (("d_t", g["d_x"]), ("d_res", g["d_res"])) + tuple((k, tg[k]) for k in BLOCK_GRADS[2:]):
        assert np.abs(got - r64[k]).max() <= 1e-11 * max(np.abs(r64[k]).max(), 1e-300), (name, k)
    if name == "inactive":
        assert not r64["feat"].any() and not any(r64[k].any() for k in BLOCK_GRADS)
    else:
        assert (r64["feat"] > 0).mean() > 0.2 and 0.2 < (r64["t"] > 0).mean() < 0.8, name
        assert all(np.abs(r64[k]).max() > 0 for k in BLOCK_GRADS), name
    out = {"c1": c1, "cd": cd, "y_block": y, **p}
    for k in BLOCK_GRADS:
        out[f"ref64_{k}"] = r64[k]
        out[f"ref32_dev_{k}"] = np.abs(r32[k].astype(np.float64) - r64[k]).max()
    return out


def main(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    cls = reference_block_class()
    for name in CASES:
        z = R.load_case(name)
        karr = kernel_arrays(kernel_weight(name), z["y"], z["upstream"], ("",) if name in KERNEL_ONLY else ("", "_plain"))
        if name in KERNEL_ONLY:
            assert float(karr["ref32_dev_dx"]) > 0
        save_parts(os.path.join(out_dir, f"{name}.dx"), karr)
        if name not in KERNEL_ONLY:
            save_parts(os.path.join(out_dir, f"{name}.block"), block_arrays(cls, name))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", ".lastconv_dgrad"))
