"""GPU: the stage-2 score (csrc/tsdiff.hip through v2ce_tsdiff; stage2_metrics.py) against the reference's results
(tests/golden/.tsdiff/tsdiff_g11_*.npz) and against the numpy restatement (tests/tsdiff_ref.py): per-event d bit-equal, S and
K exact; invariance to batching, event order, input container and repetition; refusals; the driver and the CLI."""
import csv
import glob
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

from tests.tsdiff_ref import tsdiff_ref
from v2ce_toolbox_amd import glue, hip, synth
from v2ce_toolbox_amd import stage2_metrics as SM
from v2ce_toolbox_amd.LDATI import EVENT_DTYPE, DeviceEvents, ldati_device
from v2ce_toolbox_amd.sample_methods import sampler_device

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDENS = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", ".tsdiff", "tsdiff_g11_*.npz")))


def ev(ts, x, y, p):
    e = np.zeros(len(ts), EVENT_DTYPE)
    e["timestamp"], e["x"], e["y"], e["polarity"] = ts, x, y, p
    return e


def fields(e):
    return e["timestamp"], e["x"], e["y"], e["polarity"]


def ref_pairs(gt, gc, pred, pc, fps, r, H, W):
    """Restatement per pair: concatenated d, per-pair S, K."""
    go, po = np.concatenate([[0], np.cumsum(gc)]), np.concatenate([[0], np.cumsum(pc)])
    fps = np.broadcast_to(np.asarray(fps, np.float64), (len(gc),))
    ds, S, K = [], [], []
    for i in range(len(gc)):
        d, s, k, _ = tsdiff_ref(*fields(gt[go[i]:go[i + 1]]), *fields(pred[po[i]:po[i + 1]]), fps[i], r, H, W)
        ds.append(d); S.append(s); K.append(k)
    return np.concatenate(ds), np.array(S, np.int64), np.array(K, np.int64)


def check_against_ref(gt, gc, pred, pc, fps, r, H, W):
    res = SM.ts_diff_metric_batch(gt, gc, pred, pc, fps, r, height=H, width=W, per_event=True)
    d, S, K = ref_pairs(gt, gc, pred, pc, fps, r, H, W)
    got = res.per_event_d.cpu().numpy()
    assert got.tobytes() == d.tobytes(), np.flatnonzero(got != d)[:10]
    assert np.array_equal(res.S, S) and np.array_equal(res.overflow, K)
    assert np.array_equal(res.n_gt, np.asarray(gc)) and np.array_equal(res.n_pred, np.asarray(pc))
    return res


@pytest.mark.parametrize("path", GOLDENS, ids=lambda p: os.path.basename(p)[11:-4])
def test_goldens_drop_in_and_batch(path):
    z = np.load(path)
    gt, pred, want, r, fps = z["gt"], z["pred"], z["result"], int(z["search_range"]), float(z["fps"])
    gt_before = gt.copy()
    got = SM.ts_diff_metric(gt, pred, search_range=r, fps=fps)
    assert np.array_equal(gt, gt_before)                         # the caller's polarity is not overwritten
    n = len(gt)
    assert got.dtype == np.float64 and got.shape == (2,)
    assert got[1] == want[1] and abs(got[0] - want[0]) <= n * 2.0 ** -52 * abs(want[0]), (got, want)
    res = check_against_ref(gt, [n], pred, [len(pred)], fps, r, 260, 346)
    assert res.avg[0] == got[0]


def random_case(rng, pairs, H, W, n_gt, n_pred, t_lo, t_hi, pred_pol=(0, 1), gt_pol=(-1, 1)):
    gc = rng.integers(n_gt // 2, n_gt + 1, pairs)
    pc = rng.integers(0, n_pred + 1, pairs)
    gt = ev(rng.integers(t_lo, t_hi, gc.sum()), rng.integers(0, W, gc.sum()), rng.integers(0, H, gc.sum()),
            rng.choice(gt_pol, gc.sum()))
    pred = ev(rng.integers(t_lo, t_hi, pc.sum()), rng.integers(0, W, pc.sum()), rng.integers(0, H, pc.sum()),
              rng.choice(pred_pol, pc.sum()))
    fps = rng.uniform(8, 120, pairs)
    return gt, gc, pred, pc, fps


SHAPES = [(260, 346), (64, 80), (5, 7), (1, 1)]


# r = "max": beyond the sensor (every cell of the polarity); at full size that is test_full_window_at_full_size, the
# restatement's (2r+1)^2 loop being too slow there
RANDOM_CASES = [(H, W, r, dens) for H, W in SHAPES for r in (0, 1, 2, 5, "max") for dens in ("sparse", "dense")
                if not (r == "max" and H * W > 64 * 80)]


@pytest.mark.parametrize("H,W,r,density", RANDOM_CASES)
def test_random_against_restatement(H, W, r, density):
    if r == "max":
        r = max(H, W) + 3
    rng = np.random.default_rng(zlib.crc32(repr((H, W, r, density)).encode()))
    n_pred = 30 * H * W if density == "dense" else max(4, H * W // 8)
    n_pred = min(n_pred, 200000)
    gt, gc, pred, pc, fps = random_case(rng, 3, H, W, 3000, n_pred, -2000, 40000)
    check_against_ref(gt, gc, pred, pc, fps, r, H, W)


def test_chunks_of_pairs():
    """More pairs than one 46 MB cell table holds at 346x260 (64): two chunks."""
    rng = np.random.default_rng(23)
    gt, gc, pred, pc, fps = random_case(rng, 70, 260, 346, 300, 3000, 0, 33333)
    check_against_ref(gt, gc, pred, pc, fps, 1, 260, 346)


def test_full_window_at_full_size():
    rng = np.random.default_rng(5)
    gt, gc, pred, pc, fps = random_case(rng, 2, 260, 346, 40, 3000, 0, 33333)
    res = SM.ts_diff_metric_batch(gt, gc, pred, pc, fps, 400, per_event=True)
    # every cell of the polarity is searched: the nearest predicted time of that polarity over the whole sensor
    go, po = np.concatenate([[0], np.cumsum(gc)]), np.concatenate([[0], np.cumsum(pc)])
    d = res.per_event_d.cpu().numpy()
    for i in range(2):
        g, p = gt[go[i]:go[i + 1]], pred[po[i]:po[i + 1]]
        for j, e in enumerate(g):
            t = p["timestamp"][(p["polarity"] != 0) == (e["polarity"] == 1)]
            best = min(1000000, int(np.abs(t - e["timestamp"]).min())) if t.size else 1000000
            cap = 1e6 / fps[i] / 10 * 3
            assert d[go[i] + j] == (cap if best > cap else float(best))


def test_ties_negative_and_large_timestamps_and_polarity_minus_one():
    rng = np.random.default_rng(7)
    for t_lo, t_hi in [(-50, 50), (-40000, -1000), (10 ** 12 - 30000, 10 ** 12 + 30000)]:
        gt, gc, pred, pc, fps = random_case(rng, 4, 64, 80, 2000, 20000, t_lo, t_hi, pred_pol=(-1, 0, 1, 5),
                                            gt_pol=(-1, 0, 1))
        check_against_ref(gt, gc, pred, pc, fps, 1, 64, 80)


def test_empty_prediction_and_empty_gt():
    rng = np.random.default_rng(3)
    gt, _, _, _, _ = random_case(rng, 1, 260, 346, 500, 0, 0, 33333)
    n = len(gt)
    got = SM.ts_diff_metric(gt, ev([], [], [], []), search_range=2, fps=30)
    assert got[0] == 1e6 / 30 / 10 * 3 and got[1] == n
    pred = ev([5, 6], [1, 2], [1, 2], [1, 0])
    res = SM.ts_diff_metric_batch(np.concatenate([gt, gt[:0]]), [n, 0], pred, [0, 2], [30.0, 25.0])
    assert res.overflow[0] == n and res.avg[0] == 1e6 / 30 / 10 * 3
    assert np.isnan(res.avg[1]) and res.n_gt[1] == 0 and res.overflow[1] == 0
    with pytest.raises(ZeroDivisionError):
        SM.ts_diff_metric(gt[:0], pred)


def test_stress_one_dense_cell():
    rng = np.random.default_rng(11)
    npred, ngt = (1 << 20) + 12345, 100000
    pred = ev(rng.integers(-(1 << 30), 1 << 30, npred), np.full(npred, 100), np.full(npred, 50), np.ones(npred))
    gt = ev(rng.integers(-(1 << 30), 1 << 30, ngt), np.full(ngt, 100), np.full(ngt, 50), np.ones(ngt))
    # a second pair with cells just above and below the sort thresholds
    sizes = [16, 17, 2048, 2049, 5000]
    p2 = np.concatenate([ev(rng.integers(0, 30000, s), np.full(s, k), np.full(s, 3), np.zeros(s)) for k, s in enumerate(sizes)])
    g2 = ev(rng.integers(0, 30000, 4000), rng.integers(0, len(sizes), 4000), np.full(4000, 3), np.zeros(4000))
    fps = [1e-3, 30.0]            # cap far above 1e6 for the first pair: every d is a real distance
    check_against_ref(np.concatenate([gt, g2]), [ngt, len(g2)], np.concatenate([pred, p2]), [npred, len(p2)], fps, 0, 260, 346)


def test_invariance():
    rng = np.random.default_rng(13)
    gt, gc, pred, pc, fps = random_case(rng, 6, 260, 346, 20000, 60000, 0, 33333)
    a = SM.ts_diff_metric_batch(gt, gc, pred, pc, fps, 2, per_event=True)
    b = SM.ts_diff_metric_batch(gt, gc, pred, pc, fps, 2, per_event=True)
    assert a.per_event_d.cpu().numpy().tobytes() == b.per_event_d.cpu().numpy().tobytes()
    assert a.avg.tobytes() == b.avg.tobytes() and np.array_equal(a.S, b.S)
    go, po = np.concatenate([[0], np.cumsum(gc)]), np.concatenate([[0], np.cumsum(pc)])
    d = a.per_event_d.cpu().numpy()
    for i in range(6):                                    # batch == per-pair calls
        one = SM.ts_diff_metric_batch(gt[go[i]:go[i + 1]], [gc[i]], pred[po[i]:po[i + 1]], [pc[i]], fps[i], 2, per_event=True)
        assert one.avg.tobytes() == a.avg[i:i + 1].tobytes() and one.S[0] == a.S[i] and one.overflow[0] == a.overflow[i]
        assert one.per_event_d.cpu().numpy().tobytes() == d[go[i]:go[i + 1]].tobytes()
    gperm = np.concatenate([go[i] + rng.permutation(gc[i]) for i in range(6)])   # shuffle inside each pair
    pperm = np.concatenate([po[i] + rng.permutation(pc[i]) for i in range(6)])
    s = SM.ts_diff_metric_batch(gt[gperm], gc, pred[pperm], pc, fps, 2, per_event=True)
    assert np.array_equal(s.S, a.S) and np.array_equal(s.overflow, a.overflow) and s.avg.tobytes() == a.avg.tobytes()
    assert s.per_event_d.cpu().numpy().tobytes() == d[gperm].tobytes()
    soa = tuple(torch.from_numpy(np.array(c)).cuda() for c in fields(pred))
    dev = DeviceEvents(None, np.asarray(pc).reshape(-1, 1), 0, soa=soa)
    packed = dev.packed()
    for form, counts in [(soa, pc), (dev, None), (packed, pc), (DeviceEvents(packed, np.asarray(pc).reshape(-1, 1), 0), None)]:
        f = SM.ts_diff_metric_batch(gt, gc, form, counts, fps, 2, per_event=True)
        assert f.per_event_d.cpu().numpy().tobytes() == d.tobytes() and f.avg.tobytes() == a.avg.tobytes()


def _raw_call(gt, pred, goff, poff, fps, r=1, H=260, W=346):
    """v2ce_tsdiff straight through the C ABI with sentinel outputs; returns (rc, status, stats, d)."""
    L = hip.lib()
    g = [torch.from_numpy(np.array(c)).cuda() for c in fields(gt)]
    p = [torch.from_numpy(np.array(c)).cuda() for c in fields(pred)]
    go, po = torch.tensor(goff, dtype=torch.int64).cuda(), torch.tensor(poff, dtype=torch.int64).cuda()
    f = torch.tensor(fps, dtype=torch.float64).cuda()
    pairs = len(fps)
    stats = torch.full((pairs * 3,), -7, dtype=torch.int64).cuda()
    d = torch.full((len(gt),), -3.5, dtype=torch.float64).cuda()
    status = torch.zeros(1, dtype=torch.int32).cuda()
    nb = L.v2ce_tsdiff_workspace_bytes(pairs, H, W, len(pred))
    ws = torch.empty(nb, dtype=torch.uint8).cuda()
    rc = L.v2ce_tsdiff(*(t.data_ptr() for t in g), go.data_ptr(), len(gt), *(t.data_ptr() for t in p), po.data_ptr(),
                       len(pred), f.data_ptr(), pairs, H, W, r, d.data_ptr(), stats.data_ptr(), status.data_ptr(),
                       ws.data_ptr(), nb, hip.stream_ptr())
    torch.cuda.synchronize()
    return rc, int(status.item()), stats.cpu().numpy(), d.cpu().numpy()


def test_refusals_leave_outputs_untouched():
    rng = np.random.default_rng(17)
    gt, gc, pred, pc, fps = random_case(rng, 2, 260, 346, 300, 1000, 0, 33333)
    goff, poff = [0, int(gc[0]), int(gc.sum())], [0, int(pc[0]), int(pc.sum())]
    rc, st, stats, d = _raw_call(gt, pred, goff, poff, list(fps))
    assert rc == 0 and st == 0 and stats[2] == gc[0] and (d != -3.5).all()

    def refused(bit, gt=gt, pred=pred, goff=goff, poff=poff, fps=list(fps)):
        rc, st, stats, d = _raw_call(gt, pred, goff, poff, fps)
        assert rc == 0 and st & bit, (st, bit)
        assert (stats == -7).all() and (d == -3.5).all()

    for field, val, bit in [("x", 346, 4), ("x", -1, 4), ("y", 260, 4), ("polarity", 2, 8), ("polarity", -2, 8)]:
        bad = gt.copy(); bad[field][5] = val
        refused(bit, gt=bad)
    for field, val in [("x", 400), ("y", -3)]:
        bad = pred.copy(); bad[field][7] = val
        refused(16, pred=bad)
    for f in (0.0, -30.0, float("nan"), float("inf")):
        refused(2, fps=[30.0, f])
    refused(1, goff=[0, goff[2], goff[1]])
    refused(1, poff=[0, poff[1], poff[2] + 1])
    refused(1, goff=[-1, goff[1], goff[2]])
    rc, _, stats, _ = _raw_call(gt, pred, goff, poff, list(fps), r=-1)
    assert rc == -1 and (stats == -7).all()
    # and through the Python API
    bad = gt.copy(); bad["polarity"][0] = 3
    with pytest.raises(hip.V2ceHipError):
        SM.ts_diff_metric_batch(bad, gc, pred, pc, fps)
    bad = gt.copy(); bad["y"][0] = 260
    with pytest.raises(hip.V2ceHipError):
        SM.ts_diff_metric_batch(bad, gc, pred, pc, fps)
    for kw in [dict(search_range=-1), dict(fps=0.0), dict(fps=float("nan"))]:
        args = dict(search_range=0, fps=fps); args.update(kw)
        with pytest.raises(ValueError):
            SM.ts_diff_metric_batch(gt, gc, pred, pc, args["fps"], args["search_range"])
    with pytest.raises(ValueError):
        SM.ts_diff_metric_batch(gt, [gc[0] + 5, gc[1] - 5 - gc[1]], pred, pc, fps)


def _clip(frames=33, H=64, W=96):
    sd = synth.make_state_dict(0)
    from v2ce_toolbox_amd.v2ce_3d import V2ce3d
    model = V2ce3d()
    model.load_state_dict(sd)
    model = model.eval().cuda()
    fr = synth.synthetic_frames(frames, H, W)
    return glue.video_to_voxels(model, fr, width=W, height=H, device="cuda")


def _gt_of(vox, T, seed=777):
    """A second LDATI draw stands in for the recording: pair i's events at absolute times T[i] + t."""
    out, counts = [], []
    for i in range(vox.shape[0]):
        fps = 30 / (T[i + 1] - T[i]) * 33333
        e = ldati_device(vox[i:i + 1], fps=fps, seed=seed, frame_base=i)
        a = np.ascontiguousarray(e.packed().cpu().numpy()).view(EVENT_DTYPE).copy()
        a["timestamp"] += T[i]
        out.append(a); counts.append(len(a))
    return np.concatenate(out), np.array(counts, np.int64)


def test_run_metric_equals_direct_calls():
    vox = _clip()
    P = vox.shape[0]
    rng = np.random.default_rng(19)
    T = np.concatenate([[1000], 1000 + np.cumsum(33333 + rng.integers(-3000, 3000, P))]).astype(np.int64)
    gt, gc = _gt_of(vox, T)
    methods = ("ours", "random", "even", "slope")
    summary, records = SM.run_metric(vox, gt, gc, T, methods, search_range=1, seed=5, chunk=7)
    go = np.concatenate([[0], np.cumsum(gc)])
    for m in methods:
        avg, ovf, ratio = [], [], []
        for i in range(P):
            fps = 30 / (T[i + 1] - T[i]) * 33333
            if m == "ours":
                e = ldati_device(vox[i:i + 1], t0=0, fps=fps, seed=5, frame_base=i)
            else:
                mode = {"random": hip.SAMPLER_RANDOM, "even": hip.SAMPLER_EVEN, "slope": hip.SAMPLER_PURE_SLOPE}[m]
                e = sampler_device(vox[i:i + 1], mode, 0, fps, seed=5, frame_base=i)
            g = gt[go[i]:go[i + 1]].copy()
            g["timestamp"] -= T[i]
            r = SM.ts_diff_metric_batch(g, [len(g)], e, None, fps, 1)
            avg.append(r.avg[0]); ovf.append(r.overflow[0]); ratio.append(e.num_events / len(g))
            pr = np.ascontiguousarray(e.packed().cpu().numpy()).view(EVENT_DTYPE)
            _, S, K, ravg = tsdiff_ref(*fields(g), *fields(pr), fps, 1, 64, 96)
            assert S == r.S[0] and K == r.overflow[0]
            assert abs(ravg - r.avg[0]) <= len(g) * 2.0 ** -52 * abs(ravg)
        assert np.array(records[m]["avg"]).tobytes() == np.array(avg).tobytes()
        assert records[m]["overflow"] == [int(v) for v in ovf]
        want = np.stack([np.array(avg), np.array(ovf, np.float64), np.array(ratio)], axis=1).mean(axis=0)
        assert summary[m].tobytes() == want.tobytes(), (m, summary[m], want)


def test_cli_matches_api(tmp_path):
    H, W, n = 64, 96, 33
    vox = _clip(n, H, W)
    T = np.array([glue.frame_offset_us(i, 30) for i in range(n)], dtype=np.int64)
    gt, _ = _gt_of(vox, T, seed=99)
    extra = ev([-5, T[-1] + 10], [0, 0], [0, 0], [1, 1])          # outside the clip: dropped
    np.savez(tmp_path / "gt.npz", event_stream=np.concatenate([gt, extra]))
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "v2ce_eval.py"), "--synthetic", str(n), "--synthetic_weights", "0",
                        "--height", str(H), "--width", str(W), "--gt_events", str(tmp_path / "gt.npz"), "--fps", "30",
                        "--search_range", "1", "-o", str(out)], capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "2 outside" in r.stderr
    kept, counts, dropped = SM.split_by_frames(np.concatenate([gt, extra]), T)
    assert dropped == 2
    summary, records = SM.run_metric(vox, kept, counts, T, ("ours", "random", "slope"), search_range=1, seed=42)
    rec = json.load(open(out / "full_record.json"))
    for m in ("ours", "random", "slope"):
        assert rec["pairs"][m]["avg"] == records[m]["avg"] and rec["pairs"][m]["overflow"] == records[m]["overflow"]
        assert rec["summary"][m] == [float(v) for v in summary[m]]
    rows = list(csv.reader(open(out / "abbr_result.csv")))
    assert rows[0] == ["", "Avg Error", "#Overflow", "Pred GT Event # Ratio"]
    for row, m in zip(rows[1:], ("ours", "random", "slope")):
        v = summary[m]
        assert row == [m, repr(round(float(v[0]), 3)), str(int(round(float(v[1]), 3))), repr(round(float(v[2]), 3))]
