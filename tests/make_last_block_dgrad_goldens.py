"""Recipe of tests/golden/.lastblock_dgrad/*.npz: torch's own f64 input gradients of the last decoder block's conv1 and
shortcut back through the concat and the 2x nearest upsample (include/v2ce_hip_convupdgrad.h), and the REFERENCE block's own
autograd with respect to its two sources.

The inputs are the committed ones of tests/golden/.lastblock (tests/last_block_ref.load_case: x0, x1, g1, gd and the block's
constants); they are not regenerated.  One case is new, NEW_CASES of tests/last_block_dgrad_ref.py: (B, L, H, W) =
(1, 2, 4, 65), whose last tile is one column wide and whose source column 32 has a single output column; its g1 and gd are
seeded here on the same grid of eighths and stored with its truths.

Kernel truths (every case).  ``torch.nn.grad.conv3d_input`` in f64 for both convolutions on the weights of weights.k.*.npz
(kw [32, 96, 3, 3, 3] and ks [32, 96], seeded on the grid of 64ths, shared by the cases), summed to d_X [B, 96, L, H, W];
d_x1 = its last 32 channels; d_x0 = autograd through ``F.interpolate(mode='nearest')`` -- the reference's own way to the
block's input (train/scripts/model/unet_2layer.py:360-361) -- on its first 64.
  NAME.k.N.npz    ref64_d_x0 [B, 64, L, H0, W0], ref64_d_x1 [B, 32, L, H, W]; abs_terms_d_x0, abs_terms_d_x1: the same sums
                  on absolute values; ref32_dev_d_x0, ref32_dev_d_x1: max |f32 run - f64 run| of the same torch expressions;
                  (new case) g1, gd
Layer truths (not KERNEL_ONLY, not the new case).  The reference's ``ResidualBlock3D(96, 32, stride=1, norm='BN', sn=True)``
in ``.eval()`` and ``.double()`` with the committed constants, x0 and x1 requiring grad, ``upstream`` on its output:
  NAME.layer.N.npz  ref64_d_x0, ref64_d_x1 under the names ref64_layer_d_x0 / ref64_layer_d_x1; ref32_dev_layer_d_x0 / _d_x1
                    of the f32 run
The maker asserts that the block's two relu masks on those inputs equal the committed mask_t and mask_y, that ATen's nearest
map is dst >> 1 for the sizes used, and that the restatement (tests/last_block_dgrad_ref.py) gives the kernel truths.
A file is NAME.KIND.N.npz; an array larger than PIECE bytes is split along axis 1 into KEY@0, KEY@1, ... (``plan`` is a
function of the shapes alone, so the file list is known without running the maker); every file stays under SIZE_CAP.
Runs where the reference tree is present; not collected by pytest.

    python tests/make_last_block_dgrad_goldens.py [out_dir]   (default tests/golden/.lastblock_dgrad; V2CE_REFERENCE_ROOT
                                                               names the tree)
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import last_block_dgrad_ref as D  # noqa: E402
from tests import last_block_ref as R  # noqa: E402
from tests import make_last_block_goldens as M  # noqa: E402

SIZE_CAP = 300_000
PIECE = 280_000                                 # raw bytes of one piece of an array, and of one file's arrays together
CASES = dict(M.CASES, **D.NEW_CASES)
KERNEL_ONLY = M.KERNEL_ONLY + tuple(D.NEW_CASES)
NEAREST_CHECKED = (1, 3, 4, 5, 6, 7, 20, 64, 65, 70)
K_KEYS = ("ref64_d_x0", "ref64_d_x1", "abs_terms_d_x0", "abs_terms_d_x1", "ref32_dev_d_x0", "ref32_dev_d_x1")
LAYER_KEYS = ("ref64_layer_d_x0", "ref64_layer_d_x1", "ref32_dev_layer_d_x0", "ref32_dev_layer_d_x1")


def shapes(name, kind):
    """{key: (shape, itemsize)} of the arrays of NAME.KIND.*.npz."""
    if name == "weights":
        return {"kw": ((32, 96, 3, 3, 3), 4), "ks": ((32, 96), 4)}
    B, L, H, W = CASES[name]
    x0, x1 = (B, 64, L, (H + 1) // 2, (W + 1) // 2), (B, 32, L, H, W)
    pre = "ref64_d_" if kind == "k" else "ref64_layer_d_"
    s = {f"{pre}x0": (x0, 8), f"{pre}x1": (x1, 8), pre.replace("ref64", "ref32_dev") + "x0": ((), 8),
         pre.replace("ref64", "ref32_dev") + "x1": ((), 8)}
    if kind == "k":
        s.update(abs_terms_d_x0=(x0, 8), abs_terms_d_x1=(x1, 8))
        if name in D.NEW_CASES:
            s.update(g1=(x1, 4), gd=(x1, 4))
    return s


def plan(name, kind):
    """-> [[(key in the file, source key, piece index or None, pieces)]]: the arrays of each file NAME.KIND.N.npz."""
    files, cur, used = [], [], 0
    for key, (shape, item) in sorted(shapes(name, kind).items()):
        nbytes = int(np.prod(shape, dtype=np.int64)) * item
        n = min(-(-nbytes // PIECE), shape[1]) if len(shape) > 1 else 1
        for i in range(n):
            part = -(-nbytes // n)
            if cur and used + part > PIECE:
                files.append(cur)
                cur, used = [], 0
            cur.append((f"{key}@{i}" if n > 1 else key, key, i if n > 1 else None, n))
            used += part
    return files + ([cur] if cur else [])


def file_names():
    names = [f"weights.k.{i}.npz" for i in range(len(plan("weights", "k")))]
    for name in CASES:
        for kind in ("k",) + (() if name in KERNEL_ONLY else ("layer",)):
            names += [f"{name}.{kind}.{i}.npz" for i in range(len(plan(name, kind)))]
    return names


def save(out_dir, name, kind, arrays):
    want = shapes(name, kind)
    assert set(arrays) == set(want), (sorted(arrays), sorted(want))
    for i, entries in enumerate(plan(name, kind)):
        out = {}
        for fkey, key, piece, n in entries:
            a = np.asarray(arrays[key])
            assert a.shape == want[key][0] and a.dtype.itemsize == want[key][1], (name, key, a.shape, a.dtype)
            out[fkey] = a if piece is None else np.ascontiguousarray(np.array_split(a, n, axis=1)[piece])
        path = os.path.join(out_dir, f"{name}.{kind}.{i}.npz")
        np.savez_compressed(path, **out)
        size = os.path.getsize(path)
        print(path, size)
        assert size <= SIZE_CAP, (path, size)


def kernel_weights():
    rng = np.random.default_rng(6161)
    return M.grid(rng, (32, 96, 3, 3, 3), 1 / 64, 0.06), M.grid(rng, (32, 96), 1 / 64, 0.1)


def new_inputs(name):
    B, L, H, W = CASES[name]
    rng = np.random.default_rng(sorted(D.NEW_CASES).index(name) + 5757)
    return M.grid(rng, (B, 32, L, H, W), 0.125), M.grid(rng, (B, 32, L, H, W), 0.125)


def torch_dgrads(kw, ks, g1, gd, dtype):
    """torch's own input gradients -> (d_x0 [B, 64, L, H0, W0], d_x1 [B, 32, L, H, W]) as numpy."""
    B, _, L, H, W = g1.shape
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    dX = torch.nn.grad.conv3d_input((B, 96, L, H, W), t(kw), t(g1), padding=1) + \
        torch.nn.grad.conv3d_input((B, 96, L, H, W), t(ks).view(32, 96, 1, 1, 1), t(gd))
    src = torch.zeros(B, 64, L, (H + 1) // 2, (W + 1) // 2, dtype=dtype, requires_grad=True)
    F.interpolate(src, size=(L, H, W), mode="nearest").backward(dX[:, :64].contiguous())
    return src.grad.numpy(), dX[:, 64:].contiguous().numpy()


def kernel_arrays(kw, ks, g1, gd):
    x0_64, x1_64 = torch_dgrads(kw, ks, g1, gd, torch.float64)
    x0_32, x1_32 = torch_dgrads(kw, ks, g1, gd, torch.float32)
    a0, a1 = torch_dgrads(np.abs(kw), np.abs(ks), np.abs(g1), np.abs(gd), torch.float64)
    assert x0_64.dtype == np.float64 and x0_32.dtype == np.float32
    r = D.dgrad(kw, ks, g1, gd)
    for got, want in ((r["d_x0"], x0_64), (r["d_x1"], x1_64), (r["abs_x0"], a0), (r["abs_x1"], a1)):
        assert np.abs(got - want).max() <= 1e-12 * max(np.abs(want).max(), 1e-300)
    return {"ref64_d_x0": x0_64, "ref64_d_x1": x1_64, "abs_terms_d_x0": a0, "abs_terms_d_x1": a1,
            "ref32_dev_d_x0": np.abs(x0_32.astype(np.float64) - x0_64).max(),
            "ref32_dev_d_x1": np.abs(x1_32.astype(np.float64) - x1_64).max()}


def run_block(cls, z, double):
    """A fresh reference block with the committed constants, run on cat(upsample(x0), x1) with x0 and x1 requiring grad ->
    (d_x0, d_x1, mask_t, mask_y) as numpy."""
    dtype = torch.float64 if double else torch.float32
    torch.manual_seed(0)
    blk = cls(96, 32, stride=1, norm="BN", sn=True).eval()
    c1, c2, sc = blk.conv1.module, blk.conv2.module, blk.downsample[0]
    with torch.no_grad():
        for dst, key in ((c1.weight_bar, "weight_bar1"), (c1.weight_u, "u1"), (c1.weight_v, "v1"), (sc.weight, "short_weight"),
                         (sc.bias, "short_bias"), (c2.weight_bar, "weight_bar2"), (c2.weight_u, "u2"), (c2.weight_v, "v2")):
            dst.copy_(torch.from_numpy(z[key]))
        for bn, mod in (("bn1", blk.bn1), ("bnd", blk.downsample[1]), ("bn2", blk.bn2)):
            mod.weight.copy_(torch.from_numpy(z[f"{bn}_weight"]))
            mod.bias.copy_(torch.from_numpy(z[f"{bn}_bias"]))
            mod.running_mean.copy_(torch.from_numpy(z[f"{bn}_mean"]))
            mod.running_var.copy_(torch.from_numpy(z[f"{bn}_var"]))
    if double:
        blk = blk.double()
    kept = {}

    def keep_t(mod, args, out):                          # the block's one relu module runs twice: t is its first output
        kept.setdefault("t", out.detach().clone())
    blk.relu.register_forward_hook(keep_t)
    a = torch.from_numpy(z["x0"]).to(dtype).requires_grad_(True)
    b = torch.from_numpy(z["x1"]).to(dtype).requires_grad_(True)
    feat = blk(torch.cat([F.interpolate(a, size=tuple(b.shape[2:]), mode="nearest"), b], dim=1))
    feat.backward(torch.from_numpy(z["upstream"]).to(dtype))
    return a.grad.numpy(), b.grad.numpy(), (kept["t"] > 0).numpy(), (feat.detach() > 0).numpy()


def layer_arrays(cls, name, z):
    x0_64, x1_64, mask_t, mask_y = run_block(cls, z, True)
    assert np.array_equal(mask_t, z["mask_t"]) and np.array_equal(mask_y, z["mask_y"]), name
    x0_32, x1_32, mt32, my32 = run_block(cls, z, False)
    assert np.array_equal(mt32, z["mask_t"]) and np.array_equal(my32, z["mask_y"]), name
    # the restatement: the kernel's formulas on the block's own (g1, gd) and on rs1 W1, rsd W_short
    p = {k: z[k] for k in R.PARAMS}
    f = R.block_forward(z["x0"], z["x1"], p)
    g = R.block_grads(z["x0"], z["x1"], p, z["upstream"], f)
    r = D.dgrad(f["rs1"][:, None, None, None, None] * f["W1"], f["rsd"][:, None] * np.asarray(z["short_weight"], np.float64).reshape(32, 96),
                g["g1"], g["gd"])
    for got, want in ((r["d_x0"], x0_64), (r["d_x1"], x1_64)):
        assert np.abs(got - want).max() <= 1e-11 * max(np.abs(want).max(), 1e-300), name
    if name == "zero":
        assert not x0_64.any() and not x1_64.any()
    else:
        assert np.abs(x0_64).max() > 0 and np.abs(x1_64).max() > 0
    return {"ref64_layer_d_x0": x0_64, "ref64_layer_d_x1": x1_64,
            "ref32_dev_layer_d_x0": np.abs(x0_32.astype(np.float64) - x0_64).max(),
            "ref32_dev_layer_d_x1": np.abs(x1_32.astype(np.float64) - x1_64).max()}


def main(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    for n in NEAREST_CHECKED:                           # ATen's nearest map is dst >> 1 for every size used here
        src = torch.arange((n + 1) // 2, dtype=torch.float32).view(1, 1, 1, 1, -1)
        assert F.interpolate(src, size=(1, 1, n), mode="nearest").flatten().tolist() == [i >> 1 for i in range(n)], n
    assert all(v in NEAREST_CHECKED for c in CASES.values() for v in c[2:])
    cls = M.reference_block_class()
    kw, ks = kernel_weights()
    save(out_dir, "weights", "k", {"kw": kw, "ks": ks})
    for name in CASES:
        if name in D.NEW_CASES:
            g1, gd = new_inputs(name)
            extra = {"g1": g1, "gd": gd}
        else:
            z = R.load_case(name)
            g1, gd, extra = z["g1"], z["gd"], {}
        k = kernel_arrays(kw, ks, g1, gd)
        if name == "zero":
            assert not k["ref64_d_x0"].any() and not k["ref64_d_x1"].any()
        save(out_dir, name, "k", dict(k, **extra))
        if name not in KERNEL_ONLY:
            save(out_dir, name, "layer", layer_arrays(cls, name, z))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", ".lastblock_dgrad"))
