"""Recipe of tests/golden/.evgrids/*.npz: event lists with the REFERENCE's own signed, split and statistics grids.

events_to_voxel_grid, structured_events_to_voxel_grid and structured_events_to_voxel_stat are pulled out of the
reference's train/scripts/utils/events_utils.py with ast (the module imports h5py, pandas, numba ...) and run on copies
of the inputs (they write into their argument).  Each fixture holds arrays only: events (the LDATI record dtype), bins,
H, W, the reference's signed [bins,H,W] f32, split [2,bins,H,W] f32 and stat_count / stat_mean / stat_std [2,bins,H,W]
f64, or stat_raises = 1 where the reference's stat encoder raises IndexError on these events (then without stat
arrays).  Runs where the reference tree is present; not collected by pytest.

    python tests/make_event_grids_goldens.py [out_dir]   (default tests/golden/.evgrids; V2CE_REFERENCE_ROOT names the tree)
"""
import ast
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("V2CE_REFERENCE_ROOT", "/root/reference")
EVENT_DTYPE = np.dtype([("timestamp", "<i8"), ("x", "<i2"), ("y", "<i2"), ("polarity", "i1")])
H, W = 11, 13                                   # ragged frame: no multiple of anything
MAX_FIXTURE_BYTES = 248581                      # the largest fixture under tests/golden/.voxmetrics


def reference_encoders():
    path = os.path.join(REF, "train", "scripts", "utils", "events_utils.py")
    tree = ast.parse(open(path).read(), path)
    want = ("events_to_voxel_grid", "structured_events_to_voxel_grid", "structured_events_to_voxel_stat")
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in want]
    assert len(fns) == 3
    ns = {"np": np}
    exec(compile(ast.Module(body=fns, type_ignores=[]), path, "exec"), ns)
    return tuple(ns[n] for n in want)


def events(rng, n, pol, t0=0, t1=33333):
    e = np.zeros(n, EVENT_DTYPE)
    e["timestamp"] = np.sort(rng.integers(t0, t1, n))
    e["x"], e["y"], e["polarity"] = rng.integers(0, W, n), rng.integers(0, H, n), rng.choice(pol, n)
    return e


def crowd(rng, base, n, y, x, pol, t0=0, t1=33333):
    """base plus n events in the cell (y, x), merged in time order."""
    c = events(rng, n, pol, t0, t1)
    c["x"], c["y"] = x, y
    e = np.concatenate([base, c])
    return e[np.argsort(e["timestamp"], kind="stable")]


def of(ts, pol=1, y=4, x=6):
    e = np.zeros(len(ts), EVENT_DTYPE)
    e["timestamp"], e["x"], e["y"], e["polarity"] = ts, x, y, pol
    return e


def cases():
    rng = np.random.default_rng(41)
    out = {}
    # a cell of 40 events (beyond the 32 that a walking lane sorts itself) and one of 5 000 (beyond one 4 096 LDS tile)
    out["cell40_b5"] = (crowd(rng, events(rng, 600, [-1, 1]), 40, 3, 7, [-1, 1]), 5)
    out["cell5000_b16"] = (crowd(rng, events(rng, 500, [0, 1]), 5000, 10, 12, [0, 1]), 16)
    # the rounding trap: 300 fractional contributions of mixed sign in one cell, span 33331 (prime-ish, no exact weights)
    trap = crowd(rng, events(rng, 200, [-1, 1], 0, 33331), 300, 5, 5, [-1, 1], 13000, 20000)
    trap["timestamp"][0], trap["timestamp"][-1] = 0, 33331
    out["trap_b5"] = (trap, 5)
    out["random_b1"] = (events(rng, 300, [-1, 0, 1]), 1)
    out["random_b16"] = (events(rng, 900, [-1, 1]), 16)
    out["one_event_b5"] = (events(rng, 1, [1]), 5)
    same = events(rng, 9, [-1, 1])
    same["timestamp"] = 12345
    out["same_stamp_b5"] = (same, 5)
    last = events(rng, 200, [-1, 1])
    last["timestamp"][0], last["timestamp"][-7:] = 0, 33332              # seven events exactly on the last stamp
    out["on_last_stamp_b5"] = (last, 5)
    out["pol_0_m1_mixed_b5"] = (events(rng, 400, [-1, 0, 1, 0, -1]), 5)
    # stat
    span = events(rng, 500, [-1, 0, 1], 100, 33000)
    span["timestamp"][0], span["timestamp"][-1] = 100, 33107            # span 33007 = 10 * 3300 + 7
    out["span_not_multiple_b10"] = (span, 10)
    out["stat_777_b10"] = (of([7, 7, 7]), 10)                            # delta_t = 0
    out["six_residues_b10"] = (of([0, 1, 2, 3, 5, 8, 99]), 10)           # count 6, mean 3.1666..., std 2.9268... in bin 0
    big = of(np.concatenate([[0], np.sort(rng.integers(990000, 1000001, 5000)), [2000001]]))
    out["big_residues_b2"] = (big, 2)                                    # sum tr^2 about 5e15 < 2^53
    out["top_edge_b10"] = (of([0, 50, 100]), 10)                         # tb == bins: the stat encoder raises
    # equal residues: sumsq - sum^2 / n rounds below zero for some (r, n): a NaN std
    neg = None
    for r in range(20000001, 20001000):                                   # n r^2 < 2^53 < (n r)^2: the square rounds
        for n in range(3, 23):
            S, SS = np.float64(n * r), np.float64(n * r * r)
            if (SS - (S * S) / np.float64(n)) / np.float64(n - 1) < 0:
                neg = (r, n)
                break
        if neg:
            break
    assert neg, "no negative-variance example found"
    r, n = neg
    nv = of([0] + [r] * n + [2 * r + 3])                                 # delta_t = r + 2: residue r, n times, in bin 0
    nv["x"][0] = 0                                                       # the first event (residue 0) in a cell of its own
    out["negative_var_b2"] = (nv, 2)
    return out


def main(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    signed, split, stat = reference_encoders()
    for name, (ev, bins) in cases().items():
        rows = np.stack([ev["timestamp"], ev["x"], ev["y"], ev["polarity"]], axis=1).astype(np.float64)
        res = {"signed": signed(rows, bins, W, H), "split": split(ev.copy(), bins, W, H)}
        assert res["signed"].dtype == np.float32 and res["split"].dtype == np.float32
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            try:
                c, m, s = stat(ev.copy(), bins, W, H)
                res.update(stat_count=c, stat_mean=m, stat_std=s)
            except IndexError:
                res["stat_raises"] = np.int64(1)
        path = os.path.join(out_dir, f"{name}.npz")
        np.savez_compressed(path, events=ev, bins=np.int64(bins), H=np.int64(H), W=np.int64(W), **res)
        size = os.path.getsize(path)
        assert size <= MAX_FIXTURE_BYTES, (path, size)
        print(path, size, "stat raises" if "stat_raises" in res else
              f"nan std cells: {int(np.isnan(res['stat_std']).sum())}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", ".evgrids"))
