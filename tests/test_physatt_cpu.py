"""CPU: the NumPy restatement of the physical-attention kernels (tests/physatt_ref.py) gives the reference's own bytes
(tests/golden/.physatt, recipe tests/make_physatt_goldens.py); the host's lin_log tables; the argument refusals of
v2ce_toolbox_amd.physical_att and of the C entries that need no GPU."""
import os

import numpy as np
import pytest
import torch

import physatt_ref as R
from v2ce_toolbox_amd import hip


def load(gold_dir, name):
    return np.load(os.path.join(gold_dir, ".physatt", f"{name}.npz"))


def same_bytes(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    assert got.tobytes() == want.tobytes(), (what, np.flatnonzero(got.reshape(-1) != want.reshape(-1))[:5])


@pytest.mark.parametrize("name", R.GOLDEN_NAMES)
def test_restatement_gives_the_reference_bytes(gold_dir, name):
    z = load(gold_dir, name)
    ev, fr, ps = z["events"], z["frames"], int(z["pool"])
    assert fr.dtype == np.uint8 and ev.dtype == R.EVENT_DTYPE
    same_bytes(R.attention(ev["x"], ev["y"], fr, ps, 10, False), z["plain"], "plain")
    same_bytes(R.attention(ev["x"], ev["y"], fr, ps, int(z["ceiling"]), True), z["advanced"], "advanced")
    ratio = R.ratio_map(ev["x"], ev["y"], fr, ps, float(z["threshold"]))
    same_bytes(ratio, z["ratio"], "ratio")
    same_bytes(R.top_k_mask(ratio, int(z["K"])), z["mask"], "mask")


def test_fixtures_cover_what_they_are_for(gold_dir):
    assert load(gold_dir, "ragged_19x27_p8")["plain"].shape == (3, 4)                 # both sides below the blur radius
    assert not load(gold_dir, "no_events")["advanced"].any() and load(gold_dir, "no_events")["mask"].all()
    flat = load(gold_dir, "all_equal_ratio")
    assert len(flat["events"]) > 0 and not flat["plain"].any() and not flat["advanced"].any()       # max == min
    tie = load(gold_dir, "mask_tie")
    assert int(tie["mask"].sum()) > int(tie["K"])
    cut = load(gold_dir, "counts_3_and_4")
    cnt = np.zeros((3, 4), np.int64)
    np.add.at(cnt, (cut["events"]["y"] // 8, cut["events"]["x"] // 8), 1)
    assert {3, 4} <= set(cnt.reshape(-1).tolist())
    crowd = load(gold_dir, "crowd_70000")["events"]
    assert np.unique(crowd["y"].astype(np.int64) * 1000 + crowd["x"], return_counts=True)[1].max() > 70000
    assert load(gold_dir, "full_260x346_p8")["advanced"].shape == (33, 44)


def test_log_residual_and_tables(gold_dir):
    from v2ce_toolbox_amd import physical_att as PA
    z = load(gold_dir, R.LFR_GOLDEN)
    assert set(np.unique(z["frames"]).tolist()) == {0, 19, 20, 21, 255}
    same_bytes(R.log_residual(z["frames"]), z["lfr"], "lfr")
    same_bytes(R.log_residual(z["frames"][:2])[0], z["lfr_pair"], "lfr of one pair")
    for offset, key in ((0.0, "lut_plain"), (1e-6, "lut_att")):
        same_bytes(PA.lin_log_lut(offset), z[key], key)
        same_bytes(R.lin_log_lut(offset), z[key], key)
    same_bytes(PA.gauss_weights(), R.gauss_weights(), "gauss weights")
    w = PA.gauss_weights()
    assert w.dtype == np.float64 and abs(w[0] + 2 * w[1:].sum() - 1) < 1e-15


def test_argument_refusals_without_gpu():
    from v2ce_toolbox_amd import physical_att as PA
    fr = np.zeros((2, 19, 27), np.uint8)
    ev = np.zeros(3, R.EVENT_DTYPE)
    with pytest.raises(ValueError, match="integers in \\[0, 255\\]"):
        PA.physical_attention_generation(ev, fr + 0.5)
    with pytest.raises(ValueError, match="integers in \\[0, 255\\]"):
        PA.gen_log_frame_residual(fr.astype(np.int32) + 256)
    with pytest.raises(ValueError, match="integers in \\[0, 255\\]"):
        PA.gen_log_frame_residual_batch(fr.astype(np.int16) - 1)
    with pytest.raises(ValueError, match="K must lie"):
        PA.physical_mask_generation(ev, fr, 0)
    with pytest.raises(ValueError, match="K must lie"):
        PA.physical_mask_generation(ev, fr, 13)                    # the map is 3 x 4
    for pool in (1, 17):
        with pytest.raises(ValueError, match="pool_size"):
            PA.physical_attention_generation_advanced(ev, fr, pool_size=pool)
    with pytest.raises(ValueError, match="counts add up"):
        PA.physical_attention_batch(fr, ev, [2])
    with pytest.raises(ValueError, match="counts for"):
        PA.physical_attention_batch(fr, ev, [2, 1])
    with pytest.raises(ValueError, match="unknown mode"):
        PA.physical_attention_batch(fr, ev, [3], mode="median")
    with pytest.raises(ValueError, match="clip"):
        PA.physical_attention_batch(fr[0], ev, [3])
    with pytest.raises(ValueError, match="one pair"):
        PA.physical_attention_generation(ev, np.zeros((3, 19, 27), np.uint8))


def test_no_cpu_path():
    from v2ce_toolbox_amd import physical_att as PA
    fr = np.zeros((2, 19, 27), np.uint8)
    ev = np.zeros(3, R.EVENT_DTYPE)
    with pytest.raises(hip.V2ceHipError, match="no CPU path"):
        PA.physical_attention_generation(ev, torch.from_numpy(fr))
    with pytest.raises(hip.V2ceHipError, match="no CPU path"):
        PA.gen_log_frame_residual_batch(torch.from_numpy(fr))
    with pytest.raises(hip.V2ceHipError, match="no CPU path"):
        PA.physical_attention_generation(ev, fr, device="cpu")


def test_c_entries_refuse_without_touching_the_device():
    L = hip.lib()
    assert L.v2ce_physatt_workspace_bytes(64, 260, 346, 8, 1300000) >= 64 * 33 * 44 * 8 + 64 * 4
    for pool in (4, 5, 8, 12, 16):
        assert L.v2ce_physatt_workspace_bytes(1, 260, 346, pool, 0) > 0, pool
    for pool in (1, 2, 17):                                        # pool 2 at this size: 130 x 173 cells, beyond the LDS
        assert L.v2ce_physatt_workspace_bytes(1, 260, 346, pool, 0) == 0, pool
    assert L.v2ce_physatt_workspace_bytes(1, 64, 64, 2, 0) > 0
    assert L.v2ce_physatt_workspace_bytes(0, 64, 64, 8, 0) == 0
    assert L.v2ce_physatt_workspace_bytes(1, 64, 64, 8, -1) == 0
    args = lambda pool, mode, stride=1: (None, stride, 1, 260, 346, None, None, None, 0, pool, mode, 5.0, 0.6, 0, None, None,
                                         None, None, None, None, 0, None)
    assert L.v2ce_physatt_batch(*args(17, hip.PHYSATT_PLAIN)) == -2
    assert b"pool_size" in L.v2ce_last_error()
    assert L.v2ce_physatt_batch(*args(2, hip.PHYSATT_PLAIN)) == -2
    assert L.v2ce_physatt_batch(*args(8, 3)) == -1
    assert L.v2ce_physatt_batch(*args(8, hip.PHYSATT_PLAIN, stride=3)) == -1
    assert L.v2ce_physatt_batch(*args(8, hip.PHYSATT_PLAIN)) == -1 and b"null" in L.v2ce_last_error()
    assert L.v2ce_log_residual_batch(None, 1, 4, 4, None, None, None) == -1
    assert L.v2ce_log_residual_batch(None, 2, 4, 4, None, None, None) == -1 and b"null" in L.v2ce_last_error()
