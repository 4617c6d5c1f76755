"""Recipe of tests/golden/.physatt/*.npz: frame pairs and events with the REFERENCE's own physical-attention maps, masks
and log-frame residuals.

The functions of the reference's train/scripts/utils/physical_att.py and lin_log of train/scripts/utils/v2e_utils.py are
pulled out with ast (the modules import skimage and torch at the top) and run with scipy's gaussian_filter.
scikit-image is not needed: block_reduce is supplied as its documented NumPy equivalent -- zero-pad to a multiple of the
block, reshape (H/b, b, W/b, b), transpose (0, 2, 1, 3), func(axis=(2, 3)) -- which has the strides of skimage's
view_as_blocks, so np.mean walks the same memory in the same order.

Each fixture holds arrays only: frames uint8 [2,H,W], events (the LDATI record dtype), pool, ceiling, K, threshold, and
the reference's plain [Hp,Wp] f32 (its default ceiling 10), advanced [Hp,Wp] f32 (the fixture's ceiling), ratio [Hp,Wp]
f32 and mask [Hp,Wp] bool.  lfr_values.npz holds frames uint8 [5,H,W], lfr [4,1,H,W] f32, lfr_pair [1,H,W] f32 and the two
lin_log tables lut_att (of v + 1e-6) and lut_plain (of v).  Runs where the reference tree is present; not collected by
pytest.

    python tests/make_physatt_goldens.py [out_dir]   (default tests/golden/.physatt; V2CE_REFERENCE_ROOT names the tree)
"""
import ast
import math
import os
import sys

import numpy as np
from scipy.ndimage import gaussian_filter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("V2CE_REFERENCE_ROOT", "/root/reference")
EVENT_DTYPE = np.dtype([("timestamp", "<i8"), ("x", "<i2"), ("y", "<i2"), ("polarity", "i1")])
MAX_FIXTURE_BYTES = 248581                      # the largest fixture under tests/golden/.voxmetrics


def block_reduce(image, block_size, func=np.sum, cval=0):
    bh, bw = block_size
    H, W = image.shape
    image = np.pad(image, ((0, -H % bh), (0, -W % bw)), mode="constant", constant_values=cval)
    blocks = image.reshape(image.shape[0] // bh, bh, image.shape[1] // bw, bw).transpose(0, 2, 1, 3)
    return func(blocks, axis=(2, 3))


def reference_functions():
    utils = os.path.join(REF, "train", "scripts", "utils")
    ns = {"np": np, "math": math, "gaussian_filter": gaussian_filter, "block_reduce": block_reduce}
    try:
        import torch
        ns["torch"] = torch
    except ImportError:
        pass
    for fname, want in (("v2e_utils.py", ("lin_log",)), ("physical_att.py", None)):
        path = os.path.join(utils, fname)
        tree = ast.parse(open(path).read(), path)
        fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and (want is None or n.name in want)]
        assert fns
        exec(compile(ast.Module(body=fns, type_ignores=[]), path, "exec"), ns)
    return ns


def frames_of(rng, H, W):
    """Two frames that cover the linear part of lin_log (< 20), the knee and the log part, and differ moderately."""
    a = rng.integers(0, 256, (H, W))
    dark = rng.random((H, W)) < 0.3
    a[dark] = rng.integers(0, 24, int(dark.sum()))
    b = np.clip(a + rng.integers(-9, 10, (H, W)), 0, 255)
    return np.stack([a, b]).astype(np.uint8)


def events_of(rng, n, H, W):
    e = np.zeros(n, EVENT_DTYPE)
    e["timestamp"] = np.sort(rng.integers(0, 33333, n))
    e["x"], e["y"], e["polarity"] = rng.integers(0, W, n), rng.integers(0, H, n), rng.choice([-1, 1], n)
    return e


def at(cells):
    """Events at given (y, x, count) cells."""
    ys = np.concatenate([np.full(c, y) for y, x, c in cells]) if cells else np.zeros(0)
    xs = np.concatenate([np.full(c, x) for y, x, c in cells]) if cells else np.zeros(0)
    e = np.zeros(len(ys), EVENT_DTYPE)
    e["timestamp"], e["x"], e["y"], e["polarity"] = np.arange(len(ys)), xs, ys, 1
    return e


def cases():
    rng = np.random.default_rng(77)
    out = {}                                    # name -> (frames, events, pool, advanced ceiling, K, threshold)
    # a 3 x 4 map: both sides below the blur radius (the reflection repeats), both sides ragged
    out["ragged_19x27_p8"] = (frames_of(rng, 19, 27), events_of(rng, 150, 19, 27), 8, 5, 3, 0.6)
    out["r21x40_p4"] = (frames_of(rng, 21, 40), events_of(rng, 150, 21, 40), 4, 5, 7, 0.6)
    out["r33x50_p16"] = (frames_of(rng, 33, 50), events_of(rng, 900, 33, 50), 16, 25, 2, 0.3)
    out["no_events"] = (frames_of(rng, 19, 27), events_of(rng, 0, 19, 27), 8, 5, 2, 0.6)
    f = frames_of(rng, 21, 40)
    out["equal_frames"] = (np.stack([f[0], f[0]]), events_of(rng, 25, 21, 40), 4, 5, 4, 0.6)
    # pool 8: 3 / 64 = 0.046875 is cut to zero, 4 / 64 = 0.0625 stays
    out["counts_3_and_4"] = (frames_of(rng, 24, 32), at([(1, 2, 3), (9, 17, 4), (20, 30, 2), (17, 3, 1), (16, 4, 3)]),
                             8, 5, 2, 0.6)
    crowd = np.concatenate([events_of(rng, 300, 19, 27), at([(10, 13, 70001)])])
    out["crowd_70000"] = (frames_of(rng, 19, 27), crowd, 8, 25, 1, 0.6)
    # every patch far above 2 * ceiling: the blurred map is flat, max == min, the answer all zeros
    f = frames_of(rng, 16, 24)
    out["all_equal_ratio"] = (np.stack([f[0], f[0]]), events_of(rng, 6000, 16, 24), 8, 5, 3, 0.6)
    # equal frames, three patches of 5 events: the 2nd largest ratio is shared by three cells
    f = frames_of(rng, 24, 32)
    out["mask_tie"] = (np.stack([f[1], f[1]]), at([(0, 0, 5), (9, 9, 5), (23, 31, 5), (12, 20, 3), (3, 27, 1)]), 8, 5, 2, 0.6)
    # the recording's size, the call of tools/gen_phy_att.py (pool 8, advanced, ceiling 25); smooth frames and sparse
    # events keep the compressed fixture small
    yy, xx = np.mgrid[0:260, 0:346]
    a = ((yy // 20 + xx // 30) * 9 % 256).astype(np.uint8)
    b = a.copy()
    b[60:200, 100:250] = np.clip(b[60:200, 100:250].astype(int) + 6, 0, 255)
    ev = events_of(rng, 3000, 140, 150)
    ev["x"] += 100
    ev["y"] += 60
    out["full_260x346_p8"] = (np.stack([a, b]), ev, 8, 25, 40, 0.6)
    return out


def main(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    ns = reference_functions()
    for name, (frames, ev, pool, ceiling, K, threshold) in cases().items():
        rows = np.stack([ev["timestamp"], ev["x"], ev["y"], ev["polarity"]], axis=1).astype(np.float64)
        before = frames.copy()
        plain = ns["physical_attention_generation"](rows, frames, pool_size=pool)
        adv = ns["physical_attention_generation_advanced"](rows, frames, pool_size=pool, ceiling=ceiling)
        mask, ratio = ns["physical_mask_generation"](rows, frames, K, threshold=threshold, pool_size=pool)
        assert plain.dtype == adv.dtype == ratio.dtype == np.float32 and mask.dtype == bool
        assert np.array_equal(frames, before)
        path = os.path.join(out_dir, f"{name}.npz")
        np.savez_compressed(path, frames=frames, events=ev, pool=np.int64(pool), ceiling=np.int64(ceiling), K=np.int64(K),
                            threshold=np.float64(threshold), plain=plain, advanced=adv, ratio=ratio, mask=mask)
        size = os.path.getsize(path)
        assert size <= MAX_FIXTURE_BYTES, (path, size)
        print(path, size, plain.shape, f"plain max {plain.max():.4f} adv nonzero {int((adv != 0).sum())} mask true {int(mask.sum())}")
    rng = np.random.default_rng(5)
    fr = rng.choice(np.array([0, 19, 20, 21, 255], np.uint8), (5, 6, 7))
    lfr = ns["gen_log_frame_residual_batch"](fr)
    pair = ns["gen_log_frame_residual"](fr[:2])
    lut_plain = ns["lin_log"](np.arange(256, dtype=np.float64))
    lut_att = ns["lin_log"](np.arange(256, dtype=np.uint8) + 1e-6)
    assert lfr.dtype == lut_plain.dtype == lut_att.dtype == np.float32 and lfr.shape == (4, 1, 6, 7)
    path = os.path.join(out_dir, "lfr_values.npz")
    np.savez_compressed(path, frames=fr, lfr=lfr, lfr_pair=pair, lut_plain=lut_plain, lut_att=lut_att)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", ".physatt"))
