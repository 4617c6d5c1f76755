"""Recipe of tests/golden/.ldati_edges/ldati_edges_<case>.npz: LDATI on voxel values at the branch points of the relocation
recurrence ``ceil(y - debt - 1e-6)`` -- the REFERENCE's own events for them, with the uniforms it drew.

The grids of every other LDATI fixture are drawn from continuous distributions, in which these values almost never occur.
Here each class below replaces about 1/12 of the voxels of a ``relu(0.8 randn)`` base (classes()):

    integer     exact integers 0..4 (counted by classes(): 1..4)
    near        integer + s 1e-6, s in {-2, -1, -0.5, 0.5, 1, 2}, integer in 1..4 (rounded to f32)
    tiny        U(0, 2e-6)
    negzero     -0.0
    below       nextafter(integer + 1, 0), integer in 0..3: the largest f32 below an integer
    subnormal   1e-40
    negative    -U(0, 1.5), in the signed cases only
    large       a handful of voxels at 32, 33 and 40, exact and + 1e-6: counts and neighbour differences beyond the 31-entry
                slope table of csrc/ldati.hip

The top level of tests/golden/ is exactly the output set of oracle/make_goldens.py (test_oracle_goldens_recipe compares the
two file for file), so these fixtures of a further recipe sit in a directory of their own that it skips.

The files hold the arrays of the ldati_g3_opt_* fixtures.  Two differences, both to keep a file below 250 KB although one
voxel of 40 makes the reference draw 41 uniforms for EVERY voxel: the draws the reference never reads (index >= the
voxel's relocated count, LDATI.py:171-203 masks them) are stored as 0, and ``uniforms`` stops at the largest count.  As in
oracle/make_goldens.py a torch seed is searched for which the reference gives the same bytes with this torch build's MKL
sqrt (not correctly rounded) and with an IEEE sqrt.  Runs where the reference tree is present; not collected by pytest.

    python tests/make_ldati_edge_goldens.py [out_dir]      (default tests/golden/.ldati_edges; V2CE_REFERENCE_ROOT names the tree)
"""
import logging
import os
import sys
import warnings

import numpy as np
import torch

warnings.filterwarnings("ignore")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("V2CE_REFERENCE_ROOT", "/root/reference")
EVENT_DTYPE = np.dtype([("timestamp", "<i8"), ("x", "<i2"), ("y", "<i2"), ("polarity", "i1")])
NEAR_STEPS = (-2.0, -1.0, -0.5, 0.5, 1.0, 2.0)
LARGE = (32.0, 33.0, 40.0)
MIN_PER_CLASS, MIN_LARGE = 100, 4


def edge_voxels(rng, shape, signed, scale=1.0, uniform_base=0.0):
    """[B,2,10,H,W] f32: a relu(0.8 randn) base, each class drawn for about 1/12 of the voxels, twelve large voxels.
    ``scale`` < 1 thins the grid out: it multiplies the base and is the probability that a voxel of a class that emits
    events (an integer >= 1, its near neighbours, the float below it) keeps its value instead of becoming 0.
    ``uniform_base`` = k > 0 thickens it: the base is k U[0,1) instead."""
    n = int(np.prod(shape))
    if uniform_base > 0:
        v = (uniform_base * rng.random(n)).astype(np.float32)
    else:
        v = (np.maximum(0.8 * rng.standard_normal(n), 0.0) * scale).astype(np.float32)
    cls = rng.integers(0, 12, n)
    keep = rng.random(n) < scale
    ints = rng.integers(0, 5, n).astype(np.float64)
    pos_ints = rng.integers(1, 5, n).astype(np.float64)
    steps = rng.choice(NEAR_STEPS, n)
    tiny = rng.random(n) * 2e-6
    below = np.nextafter((rng.integers(0, 4, n) + 1).astype(np.float32), np.float32(0))
    neg = -1.5 * rng.random(n)
    v = np.where(cls == 0, np.where(keep, ints, 0.0), v)
    v = np.where(cls == 1, np.where(keep, pos_ints + steps * 1e-6, steps * 0.0), v)
    v = np.where(cls == 2, tiny, v)
    v = np.where(cls == 3, -0.0, v)
    v = np.where(cls == 4, np.where(keep, below, 0.0), v)
    v = np.where(cls == 5, 1e-40, v)
    if signed:
        v = np.where(cls == 6, neg, v)
    v = v.astype(np.float32)
    where = rng.choice(n, 2 * 2 * len(LARGE), replace=False)
    v[where] = np.repeat(np.array([[x, x + 1e-6] for x in LARGE], np.float64).reshape(-1), 2).astype(np.float32)
    return v.reshape(shape)


def classes(vox, signed):
    """How often each class occurs in a grid (tests/test_ldati_edges_cpu.py re-checks the committed files with it)."""
    v = np.asarray(vox, np.float32).reshape(-1)
    r = np.rint(v)
    d = np.abs(v.astype(np.float64) - r)
    out = {
        "integer": int(((v == r) & (v >= 1) & (v <= 4)).sum()),            # (0 is everywhere: the base is a relu)
        "near": int(((d > 0) & (d <= 2.5e-6) & (r >= 1) & (r <= 4)).sum()),
        "tiny": int(((v > 1e-30) & (v < 2e-6)).sum()),
        "negzero": int(((v == 0) & np.signbit(v)).sum()),
        "below": int(((v == np.nextafter(r.astype(np.float32), np.float32(0))) & (r >= 1) & (r <= 4)).sum()),
        "subnormal": int(((v > 0) & (v < np.finfo(np.float32).tiny)).sum()),
        "large": int((v >= 32).sum()),
    }
    if signed:
        out["negative"] = int((v < 0).sum())
    return out


def assert_classes(vox, signed, name=""):
    got = classes(vox, signed)
    for k, n in got.items():
        assert n >= (MIN_LARGE if k == "large" else MIN_PER_CLASS), (name, k, got)
    if not signed:
        assert not (np.asarray(vox) < 0).any(), name


def cases():
    shape = (2, 2, 10, 12, 14)
    out = {}

    def case(name, seed, signed, fps=30, t0=0.0, **opts):
        out[name] = (edge_voxels(np.random.default_rng(seed), shape, signed), fps, t0, signed, opts)

    case("slope", 501, False)
    case("slope_signed", 502, True)
    case("bidir", 503, False, bidirectional=True)
    case("bidir_signed", 504, True, bidirectional=True)
    case("none", 505, False, additional_events_strategy="none")
    case("weighted_signed", 506, True, pooling_type="weighted")
    case("fps60_t0", 507, True, fps=60, t0=0.5)
    # the reference's own self-test input (LDATI.py:343): the tensor reaches the call as int16
    out["int16"] = (np.random.default_rng(508).integers(0, 10, (2, 2, 10, 9, 11)).astype(np.int16), 30, 0.0, None, {})
    return out


class RandCapture:
    """Wraps torch.rand to record the uniforms the reference draws (LDATI.py:171)."""

    def __enter__(self):
        self.orig, self.last = torch.rand, None

        def wrap(*a, **k):
            self.last = self.orig(*a, **k)
            return self.last.clone()
        torch.rand = wrap
        return self

    def __exit__(self, *exc):
        torch.rand = self.orig


class IeeeSqrt:
    """Routes torch.sqrt through numpy (IEEE correctly rounded) instead of MKL VML."""

    def __enter__(self):
        self.orig = torch.sqrt
        torch.sqrt = lambda x: torch.from_numpy(np.sqrt(x.numpy()))
        return self

    def __exit__(self, *exc):
        torch.sqrt = self.orig


def run_reference(REF_LDATI, vox, fps, t0, seed, ieee, opts):
    with RandCapture() as cap:
        torch.manual_seed(seed)
        call = lambda: REF_LDATI.sample_voxel_statistical(torch.from_numpy(vox.copy()), t0=t0, fps=fps, **opts)
        if ieee:
            with IeeeSqrt():
                res = call()
        else:
            res = call()
    return [np.asarray(r) for r in res], cap.last.numpy()


def main(out_dir):
    sys.path.insert(0, REF)
    import scripts.LDATI as REF_LDATI
    logging.getLogger(REF_LDATI.__name__).setLevel(logging.WARNING)
    torch.set_num_threads(4)
    os.makedirs(out_dir, exist_ok=True)
    for name, (vox, fps, t0, signed, opts) in cases().items():
        if signed is None:
            assert vox.dtype == np.int16 and vox.min() == 0 and vox.max() == 9
        else:
            assert vox.dtype == np.float32 and np.isfinite(vox).all()
            assert_classes(vox, signed, name)
        for seed in range(300, 360):
            res, u = run_reference(REF_LDATI, vox, fps, t0, seed, False, opts)
            res_ieee, u2 = run_reference(REF_LDATI, vox, fps, t0, seed, True, opts)
            assert np.array_equal(u, u2)
            if all(a.shape == b.shape and a.tobytes() == b.tobytes() for a, b in zip(res, res_ieee)):
                break
        else:
            raise AssertionError(f"{name}: MKL-VML sqrt and IEEE sqrt disagree for every seed tried")
        B, _, _, H, W = vox.shape
        u = u.reshape(B, 2, 9, H, W, -1)
        # the relocated counts, from the reference: draws at or beyond them are never read (LDATI.py:203)
        n, _ = REF_LDATI.y_relocate(torch.from_numpy(vox.copy()).reshape(B * 2, 10, H, W).float(),
                                    bidirectional=bool(opts.get("bidirectional", False)))
        n = n.numpy().reshape(B, 2, 9, H, W)
        assert u.shape[-1] == int(n.max())
        u = np.where(np.arange(u.shape[-1]) < n[..., None], u, np.float32(0)).astype(np.float32)
        lens = np.array([len(r) for r in res], np.int64)
        ev = np.concatenate(res)
        assert ev.dtype.itemsize == 13 and lens.min() > 0
        path = os.path.join(out_dir, f"ldati_edges_{name}.npz")
        np.savez_compressed(path, vox=vox, uniforms=u, fps=np.float64(fps), t0=np.float64(t0), lens=lens,
                            events=np.frombuffer(ev.tobytes(), np.uint8),
                            strategy=np.array(opts.get("additional_events_strategy", "slope")),
                            bidirectional=np.array(bool(opts.get("bidirectional", False))),
                            pooling_type=np.array(opts.get("pooling_type", "none")),
                            pooling_kernel_size=np.array(int(opts.get("pooling_kernel_size", 3))))
        assert os.path.getsize(path) <= 250 * 1024, (path, os.path.getsize(path))
        print(f"{name}: torch seed {seed} fps={fps} t0={t0} max_n={u.shape[-1]} events={lens} bytes={os.path.getsize(path)}"
              + ("" if signed is None else f" classes={classes(vox, signed)}"))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", ".ldati_edges"))
