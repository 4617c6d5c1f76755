"""GPU: physical-attention maps, ratio maps / masks and log-frame residuals (v2ce_physatt_batch, v2ce_log_residual_batch
through v2ce_toolbox_amd.physical_att) against the reference's own results (tests/golden/.physatt) and the NumPy
restatement (tests/physatt_ref.py), compared as raw bytes."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import physatt_ref as R
from v2ce_toolbox_amd import hip

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(8, 8), (9, 17), (19, 27), (64, 61), (260, 346)]
POOLS = [4, 8, 16]
PAIRS = [1, 3, 16]


def load(gold_dir, name):
    return np.load(os.path.join(gold_dir, ".physatt", f"{name}.npz"))


def same_bytes(got, want, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    bad = np.flatnonzero(np.frombuffer(got.tobytes(), np.uint8) != np.frombuffer(want.tobytes(), np.uint8))
    assert bad.size == 0, (f"{what}: {bad.size} bytes differ, first in cell "
                           f"{np.unravel_index(bad[0] // want.itemsize, want.shape)}: "
                           f"{got.reshape(-1)[bad[0] // want.itemsize]!r} != {want.reshape(-1)[bad[0] // want.itemsize]!r}")


def rows_of(ev):
    return np.stack([ev["timestamp"], ev["x"], ev["y"], ev["polarity"]], axis=1).astype(np.float64)


def device_columns(ev):
    return tuple(torch.from_numpy(np.array(ev[f])).cuda() for f in ("timestamp", "x", "y", "polarity"))


def scene(seed, P, H, W, per_pair):
    """A clip [P+1, H, W] with dark (linear lin_log) and bright regions, and P event lists of varied length; the list
    of pair 1 (if any) is empty."""
    rng = np.random.default_rng(seed)
    clip = rng.integers(0, 256, (P + 1, H, W))
    dark = rng.random((P + 1, H, W)) < 0.3
    clip[dark] = rng.integers(0, 24, int(dark.sum()))
    clip[1:] = np.clip(clip[:-1] + rng.integers(-9, 10, (P, H, W)), 0, 255)
    counts = rng.integers(per_pair // 2, per_pair * 2, P)
    if P > 1:
        counts[1] = 0
    n = int(counts.sum())
    ev = np.zeros(n, R.EVENT_DTYPE)
    ev["timestamp"] = np.sort(rng.integers(0, 33333 * P, n))
    ev["x"], ev["y"], ev["polarity"] = rng.integers(0, W, n), rng.integers(0, H, n), rng.choice([-1, 1], n)
    return clip.astype(np.uint8), ev, counts.astype(np.int64)


@pytest.mark.parametrize("name", R.GOLDEN_NAMES)
def test_drop_ins_give_the_reference_bytes(gold_dir, name):
    from v2ce_toolbox_amd import physical_att as PA
    z = load(gold_dir, name)
    ev, fr, ps, c, K, thr = z["events"], z["frames"], int(z["pool"]), int(z["ceiling"]), int(z["K"]), float(z["threshold"])
    ev_before, fr_before = ev.copy(), fr.copy()
    same_bytes(PA.physical_attention_generation(ev, fr, pool_size=ps), z["plain"], "plain")
    same_bytes(PA.physical_attention_generation_advanced(ev, fr, pool_size=ps, ceiling=c), z["advanced"], "advanced")
    mask, ratio = PA.physical_mask_generation(ev, fr, K, threshold=thr, pool_size=ps)
    same_bytes(ratio, z["ratio"], "ratio")
    assert mask.dtype == torch.bool
    same_bytes(mask, z["mask"], "mask")
    batch = PA.physical_attention_batch_generation([ev, ev[:0], ev], np.stack([fr, fr, fr]), ps, advanced=True, ceiling=c)
    same_bytes(batch[0], z["advanced"], "advanced, first of a batch")
    same_bytes(batch[2], z["advanced"], "advanced, last of a batch")
    plain = PA.physical_attention_batch_generation([ev], fr[None], ps, advanced=False, ceiling=c)    # ceiling is ignored
    same_bytes(plain[0], z["plain"], "plain through the batch drop-in")
    assert ev.tobytes() == ev_before.tobytes() and fr.tobytes() == fr_before.tobytes()              # inputs are never written


def test_log_frame_residual_gives_the_reference_bytes(gold_dir):
    from v2ce_toolbox_amd import physical_att as PA
    z = load(gold_dir, R.LFR_GOLDEN)
    fr = z["frames"]                                                  # 6 x 7: the scalar kernel
    same_bytes(PA.gen_log_frame_residual_batch(fr), z["lfr"], "lfr")
    same_bytes(PA.gen_log_frame_residual(fr[:2]), z["lfr_pair"], "lfr of one pair")
    same_bytes(PA.gen_log_frame_residual_batch(fr.astype(np.float64)), z["lfr"], "lfr from integral float frames")
    same_bytes(PA.gen_log_frame_residual_batch(torch.from_numpy(fr).cuda().float()), z["lfr"], "lfr from a device tensor")
    rng = np.random.default_rng(2)
    for shape in ((3, 8, 12), (4, 9, 17), (2, 260, 346)):             # H * W a multiple of four (vector kernel) or not
        big = rng.integers(0, 256, shape).astype(np.uint8)
        same_bytes(PA.gen_log_frame_residual_batch(big), R.log_residual(big), f"lfr {shape}")
    odd = torch.from_numpy(rng.integers(0, 256, (3, 8, 12)).astype(np.uint8)).cuda()
    view = odd.reshape(-1)[1:1 + 2 * 96].reshape(2, 8, 12)            # a base that is not 4-byte aligned
    same_bytes(PA.gen_log_frame_residual_batch(view), R.log_residual(view.cpu().numpy()), "lfr from an unaligned base")


@pytest.mark.parametrize("pool", POOLS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_random_shapes_against_the_restatement(size, pool):
    """Every mode of one call over P pairs against the restatement pair by pair; P walks through 1, 3, 16 with the case."""
    from v2ce_toolbox_amd import physical_att as PA
    H, W = size
    P = PAIRS[(SIZES.index(size) + POOLS.index(pool)) % 3]
    Hp, Wp = -(-H // pool), -(-W // pool)
    clip, ev, counts = scene(100 * H + pool, P, H, W, per_pair=4 + int(0.3 * pool * pool * Hp * Wp))
    K = max(1, (Hp * Wp) // 3)
    cols = device_columns(ev)
    plain, st0 = PA.physical_attention_batch(clip, cols, counts, pool, "plain", ceiling=10)
    adv, st1 = PA.physical_attention_batch(clip, cols, counts, pool, "advanced", ceiling=5)
    ratio, mask, st2 = PA.physical_attention_batch(clip, cols, counts, pool, "ratio", threshold=0.6, K=K)
    assert st0.tolist() == st1.tolist() == st2.tolist() == [0] * P
    assert plain.shape == adv.shape == ratio.shape == mask.shape == (P, Hp, Wp)
    lo = 0
    for i in range(P):
        e, fr = ev[lo:lo + counts[i]], clip[i:i + 2]
        same_bytes(plain[i], R.attention(e["x"], e["y"], fr, pool, 10, False), f"plain, pair {i}")
        same_bytes(adv[i], R.attention(e["x"], e["y"], fr, pool, 5, True), f"advanced, pair {i}")
        want = R.ratio_map(e["x"], e["y"], fr, pool, 0.6)
        same_bytes(ratio[i], want, f"ratio, pair {i}")
        same_bytes(mask[i], R.top_k_mask(want, K), f"mask, pair {i}")
        lo += int(counts[i])
    if Hp * Wp >= 6:                          # a map of one or two cells may be flat (max == min: zeros), a larger one not
        assert float(adv.max()) == 1.0 and float(plain.max()) > 0


def test_pool_sizes_with_a_remainder_in_the_row_sum():
    """Pools 2 and 5: the serial row sum; 12: eight accumulators plus a remainder of four."""
    from v2ce_toolbox_amd import physical_att as PA
    clip, ev, counts = scene(9, 2, 31, 45, per_pair=120)
    for pool in (2, 5, 12):
        adv, st = PA.physical_attention_batch(clip, ev, counts, pool, "advanced", ceiling=5)
        assert st.tolist() == [0, 0]
        same_bytes(adv[0], R.attention(ev["x"][:counts[0]], ev["y"][:counts[0]], clip[:2], pool, 5, True), f"pool {pool}")
        same_bytes(adv[1], np.zeros_like(adv[1].cpu().numpy()), f"pool {pool}, the pair without events")


@pytest.fixture(scope="module")
def packet():
    """A 17-frame 19 x 27 packet, its maps from ONE call, kept unchanged."""
    from v2ce_toolbox_amd import physical_att as PA
    clip, ev, counts = scene(5, 16, 19, 27, per_pair=40)
    maps = PA.packet_physical_att(clip, ev, counts).cpu().numpy()
    maps.setflags(write=False)
    return clip, ev, counts, maps


def test_packet_equals_its_single_calls(packet):
    from v2ce_toolbox_amd import physical_att as PA
    clip, ev, counts, maps = packet
    assert maps.shape == (16, 3, 4) and maps.dtype == np.float32
    lo = 0
    for i in range(16):
        single = PA.physical_attention_generation_advanced(ev[lo:lo + counts[i]], clip[i:i + 2], 8, ceiling=25)
        same_bytes(single, maps[i], f"pair {i}")
        lo += int(counts[i])
    assert maps.any()


def test_both_frame_layouts_and_a_repeated_call(packet):
    from v2ce_toolbox_amd import physical_att as PA
    clip, ev, counts, maps = packet
    pairs = np.stack([clip[:-1], clip[1:]], axis=1)                   # [P, 2, H, W]
    for frames in (pairs, torch.from_numpy(pairs).cuda(), torch.from_numpy(clip).cuda(), clip.astype(np.float32)):
        got, st = PA.physical_attention_batch(frames, ev, counts, 8, "advanced", ceiling=25)
        assert not st.any()
        same_bytes(got, maps, "layout")
    same_bytes(PA.packet_physical_att(clip, ev, counts), maps, "second run")


def test_event_containers(packet):
    from v2ce_toolbox_amd import physical_att as PA
    from v2ce_toolbox_amd.LDATI import DeviceEvents
    clip, ev, counts, maps = packet
    cols = device_columns(ev)
    same_bytes(PA.packet_physical_att(clip, cols, counts), maps, "column tuple")
    same_bytes(PA.packet_physical_att(clip, rows_of(ev), counts), maps, "[N, 4] rows")
    seg = np.zeros((16, 9), np.int64)                                 # the events of a pair as one LDATI segment
    seg[:, 0] = counts
    same_bytes(PA.packet_physical_att(clip, DeviceEvents(None, seg, 0, soa=cols), None), maps, "DeviceEvents")
    with pytest.raises(ValueError):
        PA.packet_physical_att(clip, rows_of(ev) + 0.25, counts)
    with pytest.raises(hip.V2ceHipError):
        PA.packet_physical_att(clip, tuple(t.cpu() for t in cols), counts)


def test_a_bad_coordinate_zeroes_its_own_pair_only(packet):
    from v2ce_toolbox_amd import physical_att as PA
    clip, ev, counts, maps = packet
    off = np.concatenate([[0], np.cumsum(counts)])
    for field, value in (("x", 27), ("y", 19), ("x", -1), ("y", -3)):
        bad = ev.copy()
        bad[field][off[4] + 2] = value                                # inside pair 4
        got, st = PA.physical_attention_batch(clip, bad, counts, 8, "advanced", ceiling=25)
        assert st.tolist() == [0] * 4 + [hip.PHYSATT_BAD_XY] + [0] * 11, (field, value)
        assert not got[4].any()
        keep = [i for i in range(16) if i != 4]
        same_bytes(got[keep], maps[keep], f"neighbours of the pair with {field} = {value}")
        ratio, mask, st = PA.physical_attention_batch(clip, bad, counts, 8, "ratio", K=2)
        assert st[4] == hip.PHYSATT_BAD_XY and not ratio[4].any() and not mask[4].any() and int(mask[3].sum()) >= 2
        with pytest.raises(ValueError, match="outside the frame"):
            PA.packet_physical_att(clip, bad, counts)
        with pytest.raises(ValueError, match="outside the frame"):
            PA.physical_attention_generation(bad[off[4]:off[5]], clip[4:6])


def test_descending_offsets_are_reported_per_pair():
    """The C entry takes the offsets from the device and never synchronises: a table that does not ascend is answered
    by status words and zero maps, without a read or write out of bounds."""
    from v2ce_toolbox_amd import physical_att as PA
    clip, ev, counts = scene(11, 3, 19, 27, per_pair=40)
    fr = torch.from_numpy(clip).cuda()
    _, x, y, _ = device_columns(ev)
    n = len(ev)
    L = hip.lib()
    nb = L.v2ce_physatt_workspace_bytes(3, 19, 27, 8, n)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    c0 = int(counts[0])
    off = torch.tensor([0, c0, c0 - 5, n], dtype=torch.int64, device="cuda")                          # pair 1 descends
    maps = torch.full((3, 3, 4), 7.0, device="cuda")
    status = torch.full((3,), -1, dtype=torch.int32, device="cuda")
    gw = PA.gauss_weights()
    import ctypes
    hip.check(L.v2ce_physatt_batch(fr.data_ptr(), 1, 3, 19, 27, x.data_ptr(), y.data_ptr(), off.data_ptr(), n, 8,
                                   hip.PHYSATT_ADVANCED, 5.0, 0.6, 0, PA._lut(1e-6, fr.device).data_ptr(),
                                   gw.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), maps.data_ptr(), None,
                                   status.data_ptr(), ws.data_ptr(), nb, hip.stream_ptr(fr.device)), "v2ce_physatt_batch")
    assert status.cpu().tolist() == [0, hip.PHYSATT_BAD_OFFSETS, 0]
    assert not maps[1].any()
    with pytest.raises(ValueError, match="do not ascend"):
        PA.raise_for_status(status.cpu().numpy())


def test_command_line_writes_what_the_api_returns(tmp_path):
    from v2ce_toolbox_amd import physical_att as PA
    clip, ev, _ = scene(21, 4, 19, 27, per_pair=60)
    T = np.array([0, 33333, 66666, 100000, 133333], np.int64)         # --fps 30 on a 5-frame clip
    ev["timestamp"] = np.sort(np.random.default_rng(1).integers(0, 133333, len(ev)))
    np.save(tmp_path / "clip.npy", clip)
    np.savez(tmp_path / "events.npz", event_stream=ev)
    out = tmp_path / "prep"
    run = subprocess.run([sys.executable, os.path.join(ROOT, "v2ce_prep.py"), "--frames", str(tmp_path / "clip.npy"),
                          "--events", str(tmp_path / "events.npz"), "--fps", "30", "--pool", "8", "--ceiling", "25",
                          "--mode", "advanced", "--chunk", "3", "-o", str(out), "-l", "error"],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    counts = np.histogram(ev["timestamp"], T)[0]
    assert counts.sum() == len(ev)
    assert sorted(os.listdir(out)) == ["lfr.npy", "physical_att.npy", "status.npy"]
    same_bytes(np.load(out / "physical_att.npy"), PA.packet_physical_att(clip, ev, counts).cpu().numpy(), "physical_att")
    same_bytes(np.load(out / "lfr.npy"), PA.gen_log_frame_residual_batch(clip).cpu().numpy(), "lfr")
    assert np.load(out / "status.npy").tolist() == [0, 0, 0, 0]
    bad = ev.copy()
    bad["x"][5] = 27
    np.savez(tmp_path / "bad.npz", event_stream=bad)
    run = subprocess.run([sys.executable, os.path.join(ROOT, "v2ce_prep.py"), "--frames", str(tmp_path / "clip.npy"),
                          "--events", str(tmp_path / "bad.npz"), "--fps", "30", "-o", str(tmp_path / "bad"), "-l", "error"],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode != 0 and "outside the frame" in run.stderr
