"""Recipe of tests/golden/.efvideo/*.npz: voxel grids with the frames the REFERENCE's write_event_frame_video
(v2ce.py:241-280) hands to cv2.VideoWriter, for cases tests/golden/event_frames_g9.npz lacks.

The reference's v2ce.py is imported through oracle.make_goldens.import_reference_v2ce (third-party imports stubbed) and
cv2.VideoWriter is replaced by a recorder, as gen_event_frames does there; cvtColor RGB2BGR = channel reversal.  Each
file holds ``vox`` [L,2,10,H,W] f32 and per run ``args_<name>`` = [keep_polarity, ceil, percentile] with ``bgr_<name>``
uint8 [L,H,W,3].  Runs where the reference tree is present; not collected by pytest.

    python tests/make_efvideo_goldens.py [out_dir]      (default tests/golden/.efvideo)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sparse_gamma(rng, shape, density):
    return (rng.gamma(0.3, 1.2, shape) * (rng.random(shape) < density)).astype(np.float32)


def first_plane_only(values, L, H, W):
    """Voxels whose S0 equals ``values`` (L*H*W of them) exactly: everything in plane 0 of polarity 0."""
    vox = np.zeros((L, 2, 10, H, W), np.float32)
    vox[:, 0, 0] = np.asarray(values, np.float32).reshape(L, H, W)
    return vox


def cases():
    rng = np.random.default_rng(21)
    out = {}
    # odd size 11x13: grey with a binding ceil, q = 100, a small q
    out["odd_11x13"] = (sparse_gamma(rng, (5, 2, 10, 11, 13), 0.4),
                        [("gray_ceil", False, 1, 98), ("rgb_q100", True, 1000, 100), ("gray_q100", False, 1000, 100),
                         ("rgb_q3", True, 10, 3), ("gray_q1", False, 10, 1)])
    # wider than 346 with few rows
    out["wide_3x400"] = (sparse_gamma(rng, (3, 2, 10, 3, 400), 0.3), [("rgb", True, 10, 98), ("gray", False, 10, 98)])
    # the two ranks of the median in different first-level bins (0.9 | 1.1: another exponent)
    out["two_bins"] = (first_plane_only([0.5, 0.9, 1.1, 3.0, 0.0, 0.0], 1, 2, 3),
                       [("rgb_q50", True, 10, 50), ("gray_q50", False, 10, 50), ("rgb_q40", True, 10, 40)])
    # many equal sums: halves, ties across the ranks
    v = np.round(sparse_gamma(rng, (4, 2, 10, 7, 9), 0.15) * 2) / 2
    out["ties"] = (v.astype(np.float32), [("rgb_q50", True, 10, 50), ("gray_q90", False, 10, 90), ("rgb_q98", True, 2, 98)])
    # denormal sums beside very large ones
    v = sparse_gamma(rng, (2, 2, 10, 6, 10), 0.5)
    v[:, :, :, :3] *= np.float32(1e-40)
    v[:, :, :, 5] *= np.float32(1e30)
    out["denormal_large"] = (v, [("rgb_q30", True, 10, 30), ("gray_q30", False, 10, 30), ("rgb_q98", True, 10, 98),
                                 ("gray_q98", False, 10, 98), ("rgb_q100", True, 2 ** 62, 100)])
    # exactly one positive value
    vals = np.zeros(2 * 4 * 5, np.float32)
    vals[17] = 0.37
    out["one_positive"] = (first_plane_only(vals, 2, 4, 5), [("rgb", True, 10, 98), ("gray", False, 10, 98), ("gray_q0", False, 10, 0)])
    return out


def main(out_dir):
    from oracle.make_goldens import import_reference_v2ce
    ref = import_reference_v2ce()
    cv2 = sys.modules["cv2"]
    got = []

    class Recorder:
        def __init__(self, path, fourcc, fps, size):
            got.append({"size": size, "frames": []})

        def write(self, frame):
            got[-1]["frames"].append(frame.copy())

        def release(self):
            pass
    cv2.VideoWriter = Recorder
    cv2.VideoWriter_fourcc = lambda *a: 0
    cv2.COLOR_RGB2BGR = 4
    cv2.cvtColor = lambda img, code: img[..., ::-1]
    os.makedirs(out_dir, exist_ok=True)
    for name, (vox, runs) in cases().items():
        out = {"vox": vox}
        for run, keep, ceil, pct in runs:
            ref.write_event_frame_video(vox, "unused.mp4", 30, ceil, pct, keep)
            out[f"bgr_{run}"] = np.stack(got[-1]["frames"])
            out[f"args_{run}"] = np.array([int(keep), ceil, pct], np.int64)
            assert got[-1]["size"] == (vox.shape[4], vox.shape[3])
        path = os.path.join(out_dir, f"efvideo_{name}.npz")
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", ".efvideo"))
