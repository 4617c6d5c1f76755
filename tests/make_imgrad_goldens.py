"""Recipe of tests/golden/.imgrad/*.npz: uint8 frame packets with the REFERENCE's own blurred image gradient and
three-channel image units, and the reference's error against the float64 truth of tests/image_grad_ref.py.

The functions of the reference's train/scripts/utils/image_derivative.py are pulled out with ast (the module imports cv2,
torchvision and scipy at the top) and run in torch float32 on the CPU.  torchvision is not needed: gaussian_blur is
supplied as its documented equivalent for a float tensor -- the 1-D kernel linspace / exp / normalise in float32, the 2-D
kernel torch.mm(ky[:, None], kx[None, :]), reflect padding by kernel_size // 2, a depthwise conv2d -- and Normalize as
(x - mean[:, None, None]) / std[:, None, None].  The units follow train/scripts/data/event_pack_dataset.py:66-73 packet by
packet.

Each fixture holds arrays only: frames uint8 [S, L+1, H, W], kernel_size, sigma, weights f32 [kernel_size] (the 1-D
kernel), blur f32 [S, L, H, W] (the reference's un-normalised channel), units f32 [S, L, 3, H, W] (the reference's image
units), and err_ref_blur / err_ref_units, the reference's largest absolute error against the truth on the blur and on
channel 2 of the units.  Runs where the reference tree is present; not collected by pytest.

    python tests/make_imgrad_goldens.py [out_dir]   (default tests/golden/.imgrad; V2CE_REFERENCE_ROOT names the tree)
"""
import ast
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_grad_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("V2CE_REFERENCE_ROOT", "/root/reference")
MAX_FIXTURE_BYTES = 248581                      # the largest fixture under tests/golden/.voxmetrics


def gaussian_kernel1d(kernel_size, sigma):
    half = (kernel_size - 1) * 0.5
    x = torch.linspace(-half, half, steps=kernel_size)
    pdf = torch.exp(-0.5 * (x / sigma).pow(2))
    return pdf / pdf.sum()


def gaussian_blur(img, kernel_size, sigma):
    assert img.is_floating_point() and img.dim() == 4
    k1 = gaussian_kernel1d(int(kernel_size), float(sigma)).to(img.dtype)
    k2 = torch.mm(k1[:, None], k1[None, :])
    c, r = img.shape[1], int(kernel_size) // 2
    padded = F.pad(img, [r, r, r, r], mode="reflect")
    return F.conv2d(padded, k2.expand(c, 1, *k2.shape), groups=c)


def reference_functions():
    path = os.path.join(REF, "train", "scripts", "utils", "image_derivative.py")
    ns = {"np": np, "torch": torch, "F": F, "gaussian_blur": gaussian_blur}
    tree = ast.parse(open(path).read(), path)
    want = ("get_batch_double_blurred_image_gradient", "batch_img_gradient", "batch_img_residual")
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in want]
    assert len(fns) == len(want)
    exec(compile(ast.Module(body=fns, type_ignores=[]), path, "exec"), ns)
    return ns


def frame_normalize(x):
    mean = torch.as_tensor([R.MEAN, R.MEAN], dtype=x.dtype)[:, None, None]
    std = torch.as_tensor([R.STD, R.STD], dtype=x.dtype)[:, None, None]
    return (x - mean) / std


def reference_packet(ns, images, kernel_size, sigma):
    """event_pack_dataset.py:66-73 for one packet uint8 [L+1, H, W] -> (blur [L, H, W], units [L, 3, H, W])."""
    image_units = np.stack([images[:-1], images[1:]], axis=1)
    image_units = torch.from_numpy(image_units).float() / 255
    blur = ns["get_batch_double_blurred_image_gradient"](image_units[:, 0:1], image_units[:, 1:2], sigma=sigma,
                                                         kernel_size=kernel_size)
    norm = blur / blur.max()
    units = torch.cat([frame_normalize(image_units), norm], dim=1)
    return blur[:, 0].numpy(), units.numpy()


def smooth(rng, n, H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    out = []
    for i in range(n):
        a, b, c = rng.uniform(2, 9), rng.uniform(2, 9), rng.uniform(0, 60)
        out.append(np.clip(a * yy + b * xx + c + 3 * i, 0, 255))
    return np.stack(out).round().astype(np.uint8)


def cases():
    rng = np.random.default_rng(1911)
    rand = lambda n, H, W: rng.integers(0, 256, (n, H, W), dtype=np.uint8)
    out = {}                                    # name -> (frames [S, L+1, H, W], kernel_size, sigma)
    out["min_6x6"] = (rand(3, 6, 6)[None], 11, 3)                          # H = W = radius + 1
    out["ragged_7x70"] = (rand(2, 7, 70)[None], 11, 3)
    out["tile_edges"] = (rand(3, R.TILE_H + 1, R.TILE_W + 1)[None], 11, 3)
    out["r37x50"] = (rand(5, 37, 50)[None], 11, 3)
    out["ramp_12x13"] = (smooth(rng, 3, 12, 13)[None], 11, 3)
    hot = np.zeros((3, 9, 9), np.uint8)
    hot[0, 0, 0] = hot[1, 4, 8] = hot[2, 4, 4] = 255                       # a corner, an edge, the centre
    out["one_hot_9x9"] = (hot[None], 11, 3)
    out["k5_s1p5_21x40"] = (rand(3, 21, 40)[None], 5, 1.5)
    faint = rng.integers(0, 4, (3, 10, 11)).astype(np.uint8)             # dark, so the zero-padded border stays faint too
    out["two_packets"] = (np.stack([rand(3, 10, 11), faint]), 11, 3)
    out["flat_8x8"] = (np.zeros((1, 3, 8, 8), np.uint8), 11, 3)
    return out


def main(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    ns = reference_functions()
    assert tuple(cases()) == R.GOLDEN_NAMES
    for name, (frames, ksize, sigma) in cases().items():
        weights = gaussian_kernel1d(ksize, float(sigma)).numpy()
        assert weights.dtype == np.float32
        per_packet = [reference_packet(ns, fr, ksize, sigma) for fr in frames]
        blur = np.stack([b for b, _ in per_packet])
        units = np.stack([u for _, u in per_packet])
        assert blur.dtype == units.dtype == np.float32
        truth = R.blurred_gradient(frames, weights)
        truth_c2, _ = R.units_channel2(frames, weights)
        err_blur = float(np.abs(blur - truth).max())
        with np.errstate(invalid="ignore"):
            d = np.abs(units[:, :, 2] - truth_c2)
        assert np.array_equal(np.isnan(units[:, :, 2]), np.isnan(truth_c2))
        err_units = float(np.nanmax(d)) if not np.isnan(d).all() else 0.0
        assert np.array_equal(units[:, :, :2], R.normalised_frames(frames))
        path = os.path.join(out_dir, f"{name}.npz")
        np.savez_compressed(path, frames=frames, kernel_size=np.int64(ksize), sigma=np.float64(sigma), weights=weights,
                            blur=blur, units=units, err_ref_blur=np.float64(err_blur), err_ref_units=np.float64(err_units))
        size = os.path.getsize(path)
        assert size <= MAX_FIXTURE_BYTES, (path, size)
        print(path, size, frames.shape, f"blur max {blur.max():.4f} err_ref_blur {err_blur:.3e} err_ref_units {err_units:.3e}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", ".imgrad"))
