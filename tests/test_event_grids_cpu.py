"""CPU: the NumPy restatement of the signed / split / statistics encoders (tests/event_grids_ref.py) against the
reference's own results (tests/golden/.evgrids, recipe tests/make_event_grids_goldens.py) byte for byte, the proof that
the rounding-trap fixture separates the two ways of adding a float64 weight to a float32 cell, and the host-side
validation of v2ce_toolbox_amd.event_grids, which needs no GPU."""
import os

import numpy as np
import pytest
import torch

import event_grids_ref as R
from v2ce_toolbox_amd import event_grids as EG
from v2ce_toolbox_amd import hip


def load(gold_dir, name):
    z = np.load(os.path.join(gold_dir, ".evgrids", f"{name}.npz"))
    return z, z["events"], int(z["bins"]), int(z["H"]), int(z["W"])


@pytest.mark.parametrize("name", R.GOLDEN_NAMES)
def test_restatement_matches_reference_bytes(gold_dir, name):
    z, ev, bins, H, W = load(gold_dir, name)
    before = ev.copy()
    assert R.events_to_voxel_grid(ev, bins, W, H).tobytes() == z["signed"].tobytes()
    assert R.structured_events_to_voxel_grid(ev, bins, W, H).tobytes() == z["split"].tobytes()
    if "stat_raises" in z.files:
        with pytest.raises(IndexError):
            R.structured_events_to_voxel_stat(ev, bins, W, H)
    else:
        got = R.structured_events_to_voxel_stat(ev, bins, W, H)
        for g, k in zip(got, R.STAT_KEYS):
            assert g.dtype == np.float64 and np.array_equal(g.view(np.int64), z[k].view(np.int64)), k
    assert ev.tobytes() == before.tobytes()


def test_fixtures_hold_arrays_only_and_stay_small(gold_dir):
    limit = max(os.path.getsize(os.path.join(gold_dir, ".voxmetrics", f)) for f in os.listdir(os.path.join(gold_dir, ".voxmetrics")))
    files = sorted(os.listdir(os.path.join(gold_dir, ".evgrids")))
    assert files == sorted(f"{n}.npz" for n in R.GOLDEN_NAMES)
    for f in files:
        path = os.path.join(gold_dir, ".evgrids", f)
        assert os.path.getsize(path) <= limit, f
        z = np.load(path, allow_pickle=False)
        assert all(z[k].dtype != object for k in z.files)


def test_rounding_trap_tells_f64_add_from_f32_add(gold_dir):
    """np.add.at(float32 grid, idx, float64 weights) is acc = f32(f64(acc) + v); adding f32(v) in f32 gives other bytes
    on the fixture whose cell (5, 5) takes 300 fractional weights of mixed sign."""
    z, ev, bins, H, W = load(gold_dir, "trap_b5")
    assert int(((ev["x"] == 5) & (ev["y"] == 5)).sum()) >= 200
    assert {-1, 1} <= set(ev["polarity"][(ev["x"] == 5) & (ev["y"] == 5)].tolist())
    wrong = R.events_to_voxel_grid(ev, bins, W, H, add=R.f32_add)
    assert wrong.tobytes() != z["signed"].tobytes()
    assert (wrong[:, 5, 5] != z["signed"][:, 5, 5]).any()
    wrong = R.structured_events_to_voxel_grid(ev, bins, W, H, add=R.f32_add)
    assert wrong.tobytes() != z["split"].tobytes()
    assert np.allclose(wrong, z["split"], rtol=0, atol=1e-4)          # the same sums up to f32 rounding


def test_known_statistics(gold_dir):
    z, ev, bins, H, W = load(gold_dir, "six_residues_b10")
    assert z["stat_count"][1, 0, 4, 6] == 6 and z["stat_mean"][1, 0, 4, 6] == 3.1666666666666665
    assert z["stat_std"][1, 0, 4, 6] == 2.9268868558020253
    z = load(gold_dir, "negative_var_b2")[0]
    assert int(np.isnan(z["stat_std"]).sum()) == 1
    z = load(gold_dir, "stat_777_b10")[0]
    assert z["stat_count"][1, 0, 4, 6] == 3 and z["stat_count"].sum() == 3 and not z["stat_std"].any()


def ev_of(ts):
    e = np.zeros(len(ts), R.EVENT_DTYPE)
    e["timestamp"], e["x"], e["y"], e["polarity"] = ts, 1, 2, 1
    return e


def test_host_side_validation():
    e = ev_of([0, 5, 9])
    for bins in (0, 17):
        with pytest.raises(ValueError):
            EG.event_grids_batch(e, [3], bins, 4, 4)
    with pytest.raises(ValueError):
        EG.events_to_voxel_grid(e, 0, 4, 4)
    with pytest.raises(ValueError):
        EG.events_to_voxel_grid(e, 5, 0, 4)
    with pytest.raises(ValueError):
        EG.event_grids_batch(e, [3], 5, 4, 4, kinds=("signed", "mean"))
    with pytest.raises(ValueError):
        EG.event_grids_batch(e, [3], 5, 4, 4, kinds=())
    with pytest.raises(ValueError):
        EG.event_grids_batch(e, [4, -1], 5, 4, 4)
    with pytest.raises(ValueError):
        EG.event_grids_batch(e, [], 5, 4, 4)
    rows = np.array([[0, 1, 2, 1], [7, 1, 2, -1]], np.float64)
    for bad in (np.array([[0.5, 1, 2, 1]]), np.array([[0, 1.25, 2, 1]]), np.array([[0, 1, 2, 2]]), np.array([[0, 1, 2, 0.5]]),
                np.array([[np.nan, 1, 2, 1]]), rows[:, :3], rows.astype(np.float32)):
        with pytest.raises(ValueError):
            EG.events_to_voxel_grid(bad, 5, 4, 4)
    for fn in (EG.structured_events_to_voxel_grid, EG.structured_events_to_voxel_stat):
        with pytest.raises(TypeError):
            fn(rows, 5, 4, 4)
    with pytest.raises(TypeError):
        EG.events_to_voxel_grid(np.zeros(3, [("t", "<i8"), ("x", "<i2")]), 5, 4, 4)
    assert rows.tolist() == [[0, 1, 2, 1], [7, 1, 2, -1]]


def test_status_words_become_the_documented_exceptions():
    EG.raise_for_status(np.zeros(3, np.int32))
    for bit, exc in ((hip.EVENT_GRIDS_EMPTY, IndexError), (hip.EVENT_GRIDS_BAD_XY, ValueError),
                     (hip.EVENT_GRIDS_BAD_TIME, ValueError), (hip.EVENT_GRIDS_STAT_TOP_EDGE, IndexError),
                     (hip.EVENT_GRIDS_STAT_OVERFLOW, ValueError)):
        with pytest.raises(exc):
            EG.raise_for_status(np.array([0, bit], np.int32))


def test_no_cpu_path():
    cols = (torch.zeros(3, dtype=torch.int64), torch.zeros(3, dtype=torch.int16), torch.zeros(3, dtype=torch.int16),
            torch.ones(3, dtype=torch.int8))
    for fn in (EG.events_to_voxel_grid, EG.structured_events_to_voxel_grid, EG.structured_events_to_voxel_stat):
        with pytest.raises(hip.V2ceHipError):
            fn(cols, 5, 4, 4)
        with pytest.raises(hip.V2ceHipError):
            fn(torch.zeros(3, 4, dtype=torch.float64), 5, 4, 4)
    with pytest.raises(hip.V2ceHipError):
        EG.event_grids_batch(cols, [3], 5, 4, 4)
    with pytest.raises(hip.V2ceHipError):
        EG.event_grids_batch(ev_of([0, 1]), [2], 5, 4, 4, device="cpu")
    if not torch.cuda.is_available():                     # host arrays need a device to go to
        with pytest.raises(hip.V2ceHipError):
            EG.events_to_voxel_grid(ev_of([0, 1]), 5, 4, 4)
        with pytest.raises(hip.V2ceHipError):
            EG.event_grids_batch(ev_of([0, 1]), [2], 5, 4, 4)


def test_entry_refuses_bad_arguments_without_gpu():
    L = hip.lib()
    assert L.v2ce_event_grids_workspace_bytes(2, 10, 11, 13, 1000, 7) > 2 * 4 * 1000
    assert L.v2ce_event_grids_workspace_bytes(2, 1, 11, 13, 0, 1) > 0
    for args in ((2, 0, 11, 13, 10, 7), (2, 17, 11, 13, 10, 7), (0, 10, 11, 13, 10, 7), (2, 10, 11, 13, 10, 0),
                 (2, 10, 11, 13, 10, 8), (2, 10, 11, 13, -1, 7)):
        assert L.v2ce_event_grids_workspace_bytes(*args) == 0, args
    assert L.v2ce_event_grids_batch(None, None, None, None, None, 0, 1, 5, 4, 4, 7, None, None, None, None, None, None,
                                    None, 0, None) == -1
    assert b"null" in L.v2ce_last_error()
