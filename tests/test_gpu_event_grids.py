"""GPU: the signed / split / statistics event grids (v2ce_event_grids_batch through v2ce_toolbox_amd.event_grids)
against the reference's own results (tests/golden/.evgrids) and the NumPy restatement (tests/event_grids_ref.py),
compared as raw bytes: float32 grids by tobytes(), the float64 statistics as int64 views so that NaNs compare too."""
import os

import numpy as np
import pytest
import torch

import event_grids_ref as R
from v2ce_toolbox_amd import hip, synth

pytestmark = pytest.mark.gpu
H, W = 11, 13


def load(gold_dir, name):
    z = np.load(os.path.join(gold_dir, ".evgrids", f"{name}.npz"))
    assert (int(z["H"]), int(z["W"])) == (H, W)
    return z, z["events"], int(z["bins"])


def same_bytes(got, want, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    view = np.int64 if want.dtype == np.float64 else np.int32
    bad = np.flatnonzero(got.view(view).reshape(-1) != want.view(view).reshape(-1))
    assert bad.size == 0, (f"{what}: {bad.size} cells differ, first at {np.unravel_index(bad[0], want.shape)}: "
                           f"{got.reshape(-1)[bad[0]]!r} != {want.reshape(-1)[bad[0]]!r}")


def rows_of(ev):
    return np.stack([ev["timestamp"], ev["x"], ev["y"], ev["polarity"]], axis=1).astype(np.float64)


def device_columns(ev):
    return tuple(torch.from_numpy(np.array(ev[f])).cuda() for f in ("timestamp", "x", "y", "polarity"))


def events_of(ts, x=6, y=4, pol=1):
    e = np.zeros(len(ts), R.EVENT_DTYPE)
    e["timestamp"], e["x"], e["y"], e["polarity"] = ts, x, y, pol
    return e


@pytest.mark.parametrize("name", R.GOLDEN_NAMES)
def test_drop_ins_give_the_reference_bytes(gold_dir, name):
    from v2ce_toolbox_amd import event_grids as EG
    z, ev, bins = load(gold_dir, name)
    before, rows = ev.copy(), rows_of(ev)
    rows_before = rows.copy()
    same_bytes(EG.events_to_voxel_grid(ev, bins, W, H), z["signed"], "signed")
    same_bytes(EG.events_to_voxel_grid(rows, bins, W, H), z["signed"], "signed from [N, 4] rows")
    same_bytes(EG.events_to_voxel_grid(device_columns(ev), bins, W, H), z["signed"], "signed from device columns")
    same_bytes(EG.structured_events_to_voxel_grid(ev, bins, W, H), z["split"], "split")
    if "stat_raises" in z.files:
        with pytest.raises(IndexError):
            EG.structured_events_to_voxel_stat(ev, bins, W, H)
    else:
        got = EG.structured_events_to_voxel_stat(ev, bins, W, H)
        for g, k in zip(got, R.STAT_KEYS):
            same_bytes(g, z[k], k)
    assert ev.tobytes() == before.tobytes() and rows.tobytes() == rows_before.tobytes()     # inputs are never written


@pytest.mark.parametrize("bins", [1, 2, 5, 10, 16])
def test_batch_gives_the_reference_bytes(gold_dir, bins):
    """All fixtures of one bin count as the lists of ONE call, every kind from one bucketing."""
    from v2ce_toolbox_amd import event_grids as EG
    names = [n for n in R.GOLDEN_NAMES if n.endswith(f"_b{bins}")]
    assert names
    zs = [load(gold_dir, n)[0] for n in names]
    ev = np.concatenate([z["events"] for z in zs])
    grids, st = EG.event_grids_batch(ev, [len(z["events"]) for z in zs], bins, H, W)
    assert st.dtype == np.int32 and st.shape == (len(names),)
    for i, (n, z) in enumerate(zip(names, zs)):
        same_bytes(grids["signed"][i], z["signed"], f"{n} signed")
        same_bytes(grids["split"][i], z["split"], f"{n} split")
        if "stat_raises" in z.files:
            assert st[i] == hip.EVENT_GRIDS_STAT_TOP_EDGE, n
            for k in R.STAT_KEYS:
                assert not grids[k][i].any(), (n, k)
        else:
            assert st[i] == 0, n
            for k in R.STAT_KEYS:
                same_bytes(grids[k][i], z[k], f"{n} {k}")


@pytest.fixture(scope="module")
def random_events():
    rng = np.random.default_rng(7)
    n = 20000
    ev = np.zeros(n, R.EVENT_DTYPE)
    t = np.sort(rng.integers(1000, 34331, n))
    t[0], t[-1] = 1000, 34331                       # span 33331: no multiple of 5 or 16
    ev["timestamp"] = t
    ev["x"], ev["y"], ev["polarity"] = rng.integers(0, W, n), rng.integers(0, H, n), rng.choice([-1, 0, 1], n)
    ev.setflags(write=False)
    return ev


@pytest.mark.parametrize("bins", [1, 5, 16])
def test_random_events_against_the_restatement(random_events, bins):
    """20 000 sorted events on 143 pixels: about 140 per cell list, every bucket on the workgroup sort path."""
    from v2ce_toolbox_amd import event_grids as EG
    ev = random_events
    grids, st = EG.event_grids_batch(ev, [len(ev)], bins, H, W)
    same_bytes(grids["signed"][0], R.events_to_voxel_grid(ev, bins, W, H), "signed")
    same_bytes(grids["split"][0], R.structured_events_to_voxel_grid(ev, bins, W, H), "split")
    if bins == 1:                                    # every span is a multiple of 1: the last event falls into bin 1
        assert st[0] == hip.EVENT_GRIDS_STAT_TOP_EDGE
        with pytest.raises(IndexError):
            R.structured_events_to_voxel_stat(ev, bins, W, H)
    else:
        assert st[0] == 0
        for k, want in zip(R.STAT_KEYS, R.structured_events_to_voxel_stat(ev, bins, W, H)):
            same_bytes(grids[k][0], want, k)


def test_batch_with_empty_single_and_unsorted_lists(gold_dir):
    from v2ce_toolbox_amd import event_grids as EG
    a = load(gold_dir, "cell40_b5")[1]
    b = load(gold_dir, "pol_0_m1_mixed_b5")[1]
    single = load(gold_dir, "one_event_b5")[1]
    unsorted = a[:50].copy()
    unsorted["timestamp"][10] = unsorted["timestamp"][-1] + 1           # beyond the last row's stamp
    lists = [a, a[:0], single, unsorted, b]
    ev = np.concatenate(lists)
    grids, st = EG.event_grids_batch(device_columns(ev), [len(e) for e in lists], 5, H, W)
    assert st.tolist() == [0, hip.EVENT_GRIDS_EMPTY, 0, hip.EVENT_GRIDS_BAD_TIME, 0]
    for i in (1, 3):
        for k, g in grids.items():
            assert not g[i].any(), (i, k)
    for i in (0, 2, 4):
        same_bytes(grids["signed"][i], EG.events_to_voxel_grid(lists[i], 5, W, H).cpu().numpy(), f"list {i} signed")
        same_bytes(grids["split"][i], EG.structured_events_to_voxel_grid(lists[i], 5, W, H).cpu().numpy(), f"list {i} split")
        for k, want in zip(R.STAT_KEYS, EG.structured_events_to_voxel_stat(lists[i], 5, W, H)):
            same_bytes(grids[k][i], want.cpu().numpy(), f"list {i} {k}")
    for fn in (EG.events_to_voxel_grid, EG.structured_events_to_voxel_grid, EG.structured_events_to_voxel_stat):
        with pytest.raises(IndexError):
            fn(a[:0], 5, W, H)
        with pytest.raises(ValueError):
            fn(unsorted, 5, W, H)
        outside = a[:20].copy()
        outside["x"][3] = W
        with pytest.raises(ValueError):
            fn(outside, 5, W, H)
        outside["x"][3], outside["y"][7] = 0, -1
        with pytest.raises(ValueError):
            fn(outside, 5, W, H)
    with pytest.raises(EG.hip.V2ceHipError):
        EG.events_to_voxel_grid(tuple(t.cpu() for t in device_columns(a)), 5, W, H)


def test_stat_top_edge_raises_while_the_signed_grid_is_returned():
    from v2ce_toolbox_amd import event_grids as EG
    ev = events_of([0, 50, 100])
    with pytest.raises(IndexError):
        EG.structured_events_to_voxel_stat(ev, 10, W, H)
    with pytest.raises(IndexError):
        R.structured_events_to_voxel_stat(ev, 10, W, H)
    same_bytes(EG.events_to_voxel_grid(ev, 10, W, H), R.events_to_voxel_grid(ev, 10, W, H), "signed")
    grids, st = EG.event_grids_batch(ev, [3], 10, H, W)
    assert st.tolist() == [hip.EVENT_GRIDS_STAT_TOP_EDGE]
    same_bytes(grids["signed"][0], R.events_to_voxel_grid(ev, 10, W, H), "signed in the batch")


def test_sum_of_squares_beyond_2_53_is_refused():
    """200 events of residue 10^7 in one cell: sum tr^2 = 2 * 10^16 > 2^53; one fewer zero is answered."""
    from v2ce_toolbox_amd import event_grids as EG
    r = 10 ** 7
    ev = events_of([0] + [r] * 200 + [2 * r + 5])                      # 2 bins: delta_t = r + 3, residue r in bin 0
    ev["x"][0] = 0
    with pytest.raises(ValueError, match="2\\^53"):
        EG.structured_events_to_voxel_stat(ev, 2, W, H)
    with pytest.raises(ValueError):
        R.structured_events_to_voxel_stat(ev, 2, W, H)
    ok = events_of([0, 10, 25, 31])
    grids, st = EG.event_grids_batch(np.concatenate([ev, ok]), [len(ev), len(ok)], 2, H, W)
    assert st.tolist() == [hip.EVENT_GRIDS_STAT_OVERFLOW, 0]
    for k, want in zip(R.STAT_KEYS, R.structured_events_to_voxel_stat(ok, 2, W, H)):
        assert not grids[k][0].any(), k
        same_bytes(grids[k][1], want, k)
    same_bytes(grids["split"][0], R.structured_events_to_voxel_grid(ev, 2, W, H), "split of the refused list")
    small = events_of([0] + [r // 10] * 200 + [2 * (r // 10) + 5])
    small["x"][0] = 0
    for g, want in zip(EG.structured_events_to_voxel_stat(small, 2, W, H), R.structured_events_to_voxel_stat(small, 2, W, H)):
        same_bytes(g, want, "residue 10^6")


def test_two_runs_give_identical_bytes(gold_dir):
    from v2ce_toolbox_amd import event_grids as EG
    ev = load(gold_dir, "cell5000_b16")[1]
    cols = device_columns(np.concatenate([ev, ev[:700]]))
    first, st1 = EG.event_grids_batch(cols, [len(ev), 700], 16, H, W)
    first = {k: v.cpu().numpy().copy() for k, v in first.items()}
    again, st2 = EG.event_grids_batch(cols, [len(ev), 700], 16, H, W)
    assert st1.tolist() == st2.tolist() == [0, 0]
    for k, v in again.items():
        same_bytes(v, first[k], k)


def test_ldati_round_trip():
    """LDATI events stay on the device: per pixel the split grid's two planes, summed over bins, hold (#positive -
    #negative) events, and the stat counts add up to the event count."""
    from v2ce_toolbox_amd import event_grids as EG
    from v2ce_toolbox_amd.LDATI import ldati_device
    h, w, bins = 24, 32, 10
    vox = torch.from_numpy(synth.synthetic_voxels(2, h, w, seed=3, regime="stress")).cuda()
    ev = ldati_device(vox, fps=30, seed=5)
    counts = np.asarray(ev.frame_counts, np.int64)
    assert counts.min() > 100
    grids, st = EG.event_grids_batch(ev, None, bins, h, w, kinds=("signed", "split"))
    assert st.tolist() == [0, 0]
    pix = ev.y.long() * w + ev.x.long()
    sign = torch.where(ev.p == 1, 1.0, -1.0).double()
    lo = 0
    for i, n in enumerate(counts):
        want = torch.zeros(h * w, dtype=torch.float64, device=pix.device).index_add_(0, pix[lo:lo + n], sign[lo:lo + n])
        got = grids["split"][i].double().sum(dim=(0, 1)).reshape(-1)
        assert float((got - want).abs().max()) < 1e-3
        assert float((grids["signed"][i].double().sum(0).reshape(-1) - want).abs().max()) < 1e-3
        cols = tuple(c[lo:lo + n].contiguous() for c in (ev.ts, ev.x, ev.y, ev.p))
        span = int(ev.ts[lo + n - 1] - ev.ts[lo])
        sb = next(b for b in (10, 9, 7, 11) if span % b)              # the reference raises when bins divides the span
        count, mean, std = EG.structured_events_to_voxel_stat(cols, sb, w, h)
        assert float(count.sum()) == n
        assert float(count[1].sum()) == int((ev.p[lo:lo + n] == 1).sum())
        lo += int(n)


def test_command_line_writes_what_the_api_returns(tmp_path):
    from v2ce_toolbox_amd import event_grids as EG
    rng = np.random.default_rng(3)
    n = 3000
    ev = np.zeros(n, R.EVENT_DTYPE)
    ev["timestamp"] = np.sort(rng.integers(0, 99000, n))
    ev["x"], ev["y"], ev["polarity"] = rng.integers(0, W, n), rng.integers(0, H, n), rng.integers(0, 2, n)
    T = np.array([0, 33331, 66667, 99001], np.int64)
    np.save(tmp_path / "events.npy", ev)
    np.save(tmp_path / "T.npy", T)
    out = tmp_path / "grids"
    EG.main(["--events", str(tmp_path / "events.npy"), "--frame_timestamps", str(tmp_path / "T.npy"), "--kind", "signed",
             "split", "stat", "--bins", "7", "--width", str(W), "--height", str(H), "-o", str(out), "-l", "error"])
    counts = np.histogram(ev["timestamp"], T)[0]
    grids, st = EG.event_grids_batch(ev, counts, 7, H, W)
    assert sorted(os.listdir(out)) == sorted([f"{k}.npy" for k in grids] + ["status.npy"])
    assert np.load(out / "status.npy").tolist() == st.tolist()
    for k, g in grids.items():
        same_bytes(np.load(out / f"{k}.npy"), g.cpu().numpy(), k)
    assert np.load(out / "signed.npy").shape == (3, 7, H, W) and np.load(out / "signed.npy").any()


def test_command_line_fps_and_single_list(tmp_path):
    """--fps builds the frame times T_i = int(i * 1 / fps * 1e6) up to the first one beyond the last event; with neither
    --fps nor --frame_timestamps the file is one list."""
    from v2ce_toolbox_amd import event_grids as EG
    from v2ce_toolbox_amd import glue
    rng = np.random.default_rng(4)
    n = 2500
    ev = np.zeros(n, R.EVENT_DTYPE)
    ev["timestamp"] = np.sort(rng.integers(0, 120000, n))
    ev["timestamp"][-1] = 119999
    ev["x"], ev["y"], ev["polarity"] = rng.integers(0, W, n), rng.integers(0, H, n), rng.choice([-1, 1], n)
    np.savez(tmp_path / "events.npz", event_stream=ev)
    common = ["--events", str(tmp_path / "events.npz"), "--kind", "signed", "split", "--bins", "5", "--width", str(W),
              "--height", str(H), "-l", "error"]
    EG.main(common + ["--fps", "30", "-o", str(tmp_path / "fps")])
    T = np.array([glue.frame_offset_us(i, 30.0) for i in range(5)], np.int64)       # 0, 33333, 66666, 100000, 133333
    assert T[-2] <= 119999 < T[-1]
    counts = np.histogram(ev["timestamp"], T)[0]
    assert counts.sum() == n and (counts > 0).all()
    grids, st = EG.event_grids_batch(ev, counts, 5, H, W, kinds=("signed", "split"))
    assert sorted(os.listdir(tmp_path / "fps")) == ["signed.npy", "split.npy", "status.npy"]
    assert np.load(tmp_path / "fps" / "status.npy").tolist() == st.tolist() == [0, 0, 0, 0]
    for k, g in grids.items():
        same_bytes(np.load(tmp_path / "fps" / f"{k}.npy"), g.cpu().numpy(), k)
    EG.main(common + ["-o", str(tmp_path / "one")])
    same_bytes(np.load(tmp_path / "one" / "signed.npy"), EG.events_to_voxel_grid(ev, 5, W, H).cpu().numpy()[None], "one list")
    same_bytes(np.load(tmp_path / "one" / "split.npy"), R.structured_events_to_voxel_grid(ev, 5, W, H)[None], "one list split")
    assert np.load(tmp_path / "one" / "status.npy").tolist() == [0]
