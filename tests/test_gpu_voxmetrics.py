"""GPU: the stage-1 score (csrc/voxmetrics.hip through v2ce_voxmetrics; stage1_metrics.py) against the numpy
restatement (tests/voxmetrics_ref.py: counts equal, f64 sums to 1e-12) and the reference's results
(tests/golden/.voxmetrics/); invariance to batching and repetition; refusals.  The batched voxeliser against the serial
put_ of the reference, bit for bit; its status bits; polarity -1.  The driver at full size and the command line."""
import csv
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import voxmetrics_ref as R
from tests.test_voxmetrics_cpu import METRIC_GOLDENS, VOX_GOLDENS, check_values_against_reference, restated_values
from v2ce_toolbox_amd import hip, synth
from v2ce_toolbox_amd import stage1_metrics as S
from v2ce_toolbox_amd.LDATI import EVENT_DTYPE, ldati_device
from v2ce_toolbox_amd.voxelize import gen_discretized_event_volume, gen_discretized_event_volume_batch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check_stats(got, want):
    for k in ("n", "tp", "fp", "fn", "pool_n"):
        assert np.array_equal(got[k] if isinstance(got, dict) else getattr(got, k), want[k]), k
    for k in ("abs_diff_sum", "ratio_sum", "pool_sq_sum"):
        g = got[k] if isinstance(got, dict) else getattr(got, k)
        w = want[k]
        nan = np.isnan(w)
        assert np.array_equal(np.isnan(g), nan), k
        assert np.all(np.abs(g[~nan] - w[~nan]) <= 1e-12 * np.abs(w[~nan])), (k, g, w)


def voxels(rng, shape, density=0.3, scale=0.05):
    v = rng.exponential(scale, shape).astype(np.float32) * (rng.random(shape) < density)
    return v.astype(np.float32)


@pytest.mark.parametrize("B,L,H,W,ks", [(1, 1, 5, 7, (1, 2, 3, 4)), (1, 2, 9, 13, (2, 4)), (3, 3, 11, 10, (1, 2, 3, 4)),
                                        (1, 16, 17, 23, (2, 3, 4)), (3, 2, 4, 4, (4,)), (2, 3, 260, 346, (2, 4))])
def test_statistics_match_the_restatement(B, L, H, W, ks):
    rng = np.random.default_rng(B * 1000 + L * 100 + H)
    p, g = voxels(rng, (B, L, 20, H, W)), voxels(rng, (B, L, 20, H, W))
    p.reshape(-1)[::13] = np.float32(0.01)          # exactly at the threshold: not above it
    g.reshape(-1)[::29] = np.float32(0.01)
    st = S.voxel_metrics_batch(dev(p), dev(g), pool_sizes=ks)
    check_stats(st, R.stats(p, g, pool_sizes=ks))
    assert st.pool_sizes == ks


def test_odd_width_and_misaligned_rows():
    rng = np.random.default_rng(5)
    p, g = voxels(rng, (2, 3, 20, 7, 9)), voxels(rng, (2, 3, 20, 7, 9))
    check_stats(S.voxel_metrics_batch(dev(p), dev(g), pool_sizes=(2, 3, 4)), R.stats(p, g, pool_sizes=(2, 3, 4)))
    big = torch.zeros(1 + p.size, device="cuda")
    pv = big[1:].view(p.shape)                        # contiguous, but 4-B aligned only
    pv.copy_(dev(p))
    check_stats(S.voxel_metrics_batch(pv, dev(g), pool_sizes=(2, 4)), R.stats(p, g, pool_sizes=(2, 4)))


def test_zero_gt_and_nan():
    rng = np.random.default_rng(6)
    p = voxels(rng, (1, 2, 20, 8, 12))
    g = np.zeros_like(p)
    st = S.voxel_metrics_batch(dev(p), dev(g))
    check_stats(st, R.stats(p, g))
    assert all(float(st.binary_match_f1(op)[0]) == 0.0 for op in S.OPS)
    q = p.copy()
    q[0, 1, 3, 2, 5] = np.nan
    st = S.voxel_metrics_batch(dev(q), dev(g))
    want = R.stats(q, g)
    check_stats(st, want)
    assert np.isnan(st.abs_diff_sum[0]) and np.isnan(st.ratio_sum[0]) and np.isnan(st.pool_sq_sum[0]).all()


@pytest.mark.parametrize("path", METRIC_GOLDENS, ids=lambda p: os.path.basename(p)[8:-4])
def test_drop_ins_against_reference(path):
    z = np.load(path)
    p, g = dev(z["pred"]), dev(z["gt"])
    ks = tuple(int(n[12:]) for n in z.files if n.startswith("ref_PoolMSE_"))
    _, bl = restated_values(z["pred"], z["gt"], ks)
    got = {}
    for op in S.OPS:
        v = S.BinaryMatch(op_type=op)(p, g)
        assert v.dtype == torch.float64 and v.dim() == 0 and v.is_cuda
        got[f"BinaryMatch_{op}"] = float(v)
        v = S.BinaryMatchF1(op_type=op)(p, g)
        assert v.dtype == torch.float32 and v.dim() == 0
        got[f"BinaryMatchF1_{op}"] = float(v)
    for k in ks:
        v = S.PoolMSE(kernel_size=k)(p, g)
        assert v.dtype == torch.float32
        got[f"PoolMSE_{k}"] = float(v)
    got["MeanRatio"] = float(S.MeanRatio()(p, g))
    got["L1"] = float(S.L1()(p, g))
    check_values_against_reference(got, z, bl)
    pb, gb = (p > 0.01).float(), (g > 0.01).float()
    assert abs(float(S.f1score(pb, gb)) - float(z["ref_BinaryMatchF1_raw"])) <= 1e-6


def test_batch_equals_single_calls_and_repeats():
    rng = np.random.default_rng(8)
    p, g = voxels(rng, (3, 5, 20, 13, 18)), voxels(rng, (3, 5, 20, 13, 18))
    ks = (2, 3, 4)
    a = S.voxel_metrics_batch(dev(p), dev(g), pool_sizes=ks).raw
    b = S.voxel_metrics_batch(dev(p), dev(g), pool_sizes=ks).raw
    assert a.tobytes() == b.tobytes()
    for i in range(3):
        one = S.voxel_metrics_batch(dev(p[i:i + 1]), dev(g[i:i + 1]), pool_sizes=ks).raw
        assert one.tobytes() == a[i:i + 1].tobytes(), i


def test_refusals():
    x = torch.zeros(1, 2, 20, 8, 8, device="cuda")
    with pytest.raises(ValueError):
        S.voxel_metrics_batch(torch.zeros(1, 2, 18, 8, 8, device="cuda"), torch.zeros(1, 2, 18, 8, 8, device="cuda"))
    with pytest.raises(ValueError):
        S.voxel_metrics_batch(x, x, pool_sizes=(9,))
    with pytest.raises(ValueError):
        S.voxel_metrics_batch(x, x, pool_sizes=(0,))
    nc = torch.zeros(1, 2, 20, 8, 16, device="cuda")[..., ::2]
    with pytest.raises(ValueError):
        S.voxel_metrics_batch(nc, nc)
    with pytest.raises(hip.V2ceHipError):
        S.voxel_metrics_batch(x.cpu(), x.cpu())
    with pytest.raises(ValueError):
        S.voxel_metrics_batch(x, torch.zeros(1, 3, 20, 8, 8, device="cuda"))


# ---------------------------------------------------------------------------------------------------------------------
# the batched voxeliser

@pytest.mark.parametrize("path", VOX_GOLDENS, ids=lambda p: os.path.basename(p)[9:-4])
def test_batch_voxeliser_bit_identical_to_serial_put(path):
    z = np.load(path)
    ev, counts, bins, H, W = z["events"], z["counts"], int(z["bins"]), int(z["H"]), int(z["W"])
    vol, st = gen_discretized_event_volume_batch(ev, counts, bins, H, W)
    got = vol.cpu().numpy()
    assert got.tobytes() == z["volume"].tobytes(), np.argwhere(got != z["volume"])[:5]
    assert ((st & hip.VOXELIZE_SINGLE_TIMESTAMP) != 0).tolist() == [int(c) == 1 for c in counts]
    off = np.concatenate([[0], np.cumsum(counts)])
    for i in range(len(counts)):       # a loop of single-pair calls of itself
        v1, _ = gen_discretized_event_volume_batch(ev[off[i]:off[i + 1]], counts[i:i + 1], bins, H, W)
        assert v1.cpu().numpy()[0].tobytes() == got[i].tobytes(), i


def test_batch_voxeliser_long_buckets_ranges_and_status():
    rng = np.random.default_rng(21)
    H, W, bins = 6, 5, 10
    lists = []
    e = np.zeros(9000, EVENT_DTYPE)             # one hot pixel: a bucket far beyond one LDS tile
    e["timestamp"] = rng.integers(0, 10 ** 6, 9000)
    e["x"], e["y"], e["polarity"] = 2, 3, rng.choice([-1, 1], 9000)
    lists.append(e)
    lists.append(np.zeros(0, EVENT_DTYPE))      # empty
    s = np.zeros(5, EVENT_DTYPE); s["timestamp"] = 77; s["x"] = 1
    lists.append(s)                              # single timestamp
    r = np.zeros(3000, EVENT_DTYPE)
    r["timestamp"] = rng.integers(0, 5000, 3000)
    r["x"], r["y"], r["polarity"] = rng.integers(0, W, 3000), rng.integers(0, H, 3000), rng.choice([0, 1], 3000)
    lists.append(r)
    ev = np.concatenate(lists)
    counts = [len(x) for x in lists]
    vol, st = gen_discretized_event_volume_batch(ev, counts, bins, H, W)
    assert st.tolist() == [0, hip.VOXELIZE_EMPTY, hip.VOXELIZE_SINGLE_TIMESTAMP, 0]
    got = vol.cpu().numpy()
    for i in (0, 3):
        want = R.voxelize_serial(lists[i]["timestamp"], lists[i]["x"], lists[i]["y"], lists[i]["polarity"], bins, H, W)
        assert got[i].tobytes() == want.tobytes(), i
    assert not got[1].any() and not got[2].any()
    rng_ = np.array([[-100, 2 * 10 ** 6], [0, 1], [0, 100], [1000, 4000]], np.int64)
    vol, st = gen_discretized_event_volume_batch(ev, counts, bins, H, W, t_range=rng_)
    got = vol.cpu().numpy()
    for i in (0, 2, 3):
        want = R.voxelize_serial(lists[i]["timestamp"], lists[i]["x"], lists[i]["y"], lists[i]["polarity"], bins, H, W,
                                 t_range=rng_[i])
        assert got[i].tobytes() == want.tobytes(), i
    bad = ev.copy(); bad["x"][-1] = W
    with pytest.raises(AssertionError):
        gen_discretized_event_volume_batch(bad, counts, bins, H, W)
    with pytest.raises(ValueError):
        gen_discretized_event_volume_batch(ev, counts, bins, H, W, t_range=[[5, 1]] * 4)


def test_minus_one_polarity_lands_in_the_negative_half():
    e = np.zeros(4, EVENT_DTYPE)
    e["timestamp"] = [0, 10, 20, 30]
    e["x"], e["y"], e["polarity"] = [0, 1, 2, 3], 0, [-1, -1, 1, 0]
    vol = gen_discretized_event_volume(e, (20, 2, 4)).cpu().numpy()          # the single-list drop-in
    assert vol[:10, 0, 0].sum() == 0 and vol[10:, 0, 0].sum() == 1.0
    assert vol[:10, 0, 1].sum() == 0 and vol[10:, 0, 1].sum() == 1.0
    assert vol[:10, 0, 2].sum() == 1.0 and vol[10:, 0, 3].sum() == 1.0
    vb, _ = gen_discretized_event_volume_batch(e, [4], 10, 2, 4)
    assert vb[0].cpu().numpy().tobytes() == R.voxelize_serial(e["timestamp"], e["x"], e["y"], e["polarity"], 10, 2, 4).tobytes()
    assert float(vb[0, 10:, 0, 0].sum()) == 1.0


# ---------------------------------------------------------------------------------------------------------------------
# the driver and the command line

def test_driver_full_size_matches_the_restatement():
    H, W, P = 260, 346, 33
    vox = torch.from_numpy(synth.synthetic_voxels(P, H, W, seed=4, regime="stress")).cuda().reshape(P, 2, 10, H, W)
    gvox = torch.from_numpy(synth.synthetic_voxels(P, H, W, seed=9, regime="sparse")).cuda().reshape(P, 2, 10, H, W)
    ev = ldati_device(gvox, fps=30, seed=3)
    ts, x, y, p = (t.cpu().numpy() for t in ev._unpacked())
    gt = np.zeros(ts.size, EVENT_DTYPE)
    gt["timestamp"], gt["x"], gt["y"], gt["polarity"] = ts, x, y, p
    counts = np.asarray(ev.frame_counts).reshape(-1)[:P].astype(np.int64)
    summary, rec = S.run_stage1_metric(vox, gt, counts, None, seq_len=16)
    assert rec["windows"] == [[0, 16], [16, 32], [32, 33]]
    gv, _ = gen_discretized_event_volume_batch(gt, counts, 10, H, W)
    gvn, pvn = gv.cpu().numpy(), vox.reshape(P, 20, H, W).cpu().numpy()
    names = list(summary)
    per = []
    for a, b in rec["windows"]:
        s = R.stats(pvn[a:b][None], gvn[a:b][None], pool_sizes=(2, 4))
        v = R.values(s)
        v["PoolMSE_2"], v["PoolMSE_4"] = v.pop("PoolMSE_q0"), v.pop("PoolMSE_q1")
        per.append(v)
    for i, v in enumerate(per):
        for k in names:
            w = rec["values"][i][k]
            assert abs(w - v[k]) <= 1e-6 * abs(v[k]) + (0 if k.startswith("BinaryMatch_") else 1e-7), (i, k, w, v[k])
    for k in names:
        assert abs(summary[k] - np.mean([v[k] for v in per])) <= 1e-6 * abs(summary[k]) + 1e-7


def _cli(args, cwd):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "v2ce_eval.py")] + args, capture_output=True, text=True,
                       cwd=cwd, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r


def test_cli_stage1_and_pred_events(tmp_path):
    from v2ce_toolbox_amd import glue
    from v2ce_toolbox_amd.v2ce_3d import V2ce3d
    H, W, N = 64, 80, 17
    frames = synth.synthetic_frames(N, H, W)
    np.save(tmp_path / "frames.npy", frames)
    model = V2ce3d(precision="f32")
    model.load_state_dict(synth.make_state_dict(0))
    model = model.eval().cuda()
    vox = glue.video_to_voxels(model, frames, seq_len=16, width=W, height=H, batch_size=1, device="cuda")
    T = np.array([glue.frame_offset_us(i, 30) for i in range(N)], dtype=np.int64)
    ev = ldati_device(vox, fps=30, seed=1)
    ts, x, y, p = (t.cpu().numpy() for t in ev._unpacked())
    seg = np.asarray(ev.frame_counts).reshape(-1)[:N - 1]
    gt = np.zeros(ts.size, EVENT_DTYPE)
    gt["timestamp"] = ts + np.repeat(T[:-1], seg)
    gt["x"], gt["y"], gt["polarity"] = x, y, np.where(p == 0, -1, p)
    np.savez(tmp_path / "gt.npz", event_stream=gt)
    np.save(tmp_path / "T.npy", T)
    base = ["--npy_frames", str(tmp_path / "frames.npy"), "--synthetic_weights", "0", "--precision", "f32",
            "--height", str(H), "--width", str(W), "--gt_events", str(tmp_path / "gt.npz"),
            "--frame_timestamps", str(tmp_path / "T.npy"), "--evaluate_on", "ours"]
    _cli(base + ["-o", str(tmp_path / "plain")], tmp_path)
    assert sorted(os.listdir(tmp_path / "plain")) == ["abbr_result.csv", "full_record.json"]
    r = _cli(base + ["--stage1", "-o", str(tmp_path / "s1")], tmp_path)
    assert sorted(os.listdir(tmp_path / "s1")) == ["abbr_result.csv", "full_record.json", "stage1_record.json",
                                                   "stage1_result.csv"]
    for f in ("abbr_result.csv", "full_record.json"):
        assert (tmp_path / "plain" / f).read_bytes() == (tmp_path / "s1" / f).read_bytes()
    rows = list(csv.reader(open(tmp_path / "s1" / "stage1_result.csv")))
    assert rows[0] == ["metric", "mean"] and [r_[0] for r_ in rows[1:]] == list(S.METRIC_NAMES)
    rec = json.load(open(tmp_path / "s1" / "stage1_record.json"))
    assert rec["windows"] == [[0, N - 1]]
    # the GT is the LDATI output of the model's own voxels: every pair has events, so the ratio is finite
    assert np.isfinite(rec["summary"]["MeanRatio"]) and "BinaryMatchF1_sum_cp" in r.stdout
    r = _cli(["--stage1", "--pred_events", str(tmp_path / "gt.npz"), "--gt_events", str(tmp_path / "gt.npz"),
              "--frame_timestamps", str(tmp_path / "T.npy"), "--height", str(H), "--width", str(W),
              "-o", str(tmp_path / "pe")], tmp_path)
    assert sorted(os.listdir(tmp_path / "pe")) == ["stage1_record.json", "stage1_result.csv"]
    rec = json.load(open(tmp_path / "pe" / "stage1_record.json"))
    assert rec["summary"]["BinaryMatch_raw"] == 1.0 and rec["summary"]["L1"] == 0.0     # the stream against itself
