"""GPU: the stage-1 loss terms (csrc/voxlosses.hip through v2ce_voxlosses / v2ce_volume_losses; losses.py) against the
numpy f64 restatement (tests/voxlosses_ref.py: counts equal, f64 sums to 1e-12) and the reference's own results
(tests/golden/.voxlosses/, two-sided bound of tests/test_voxlosses_cpu.py); the [N, D, H, W] entry against the 5-D
entry, bit for bit; invariance to batching and repetition; NaN; match_low; refusals; the driver and the command line."""
import csv
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import voxlosses_ref as R
from tests.test_voxlosses_cpu import ALL_LOSS, GOLDENS, check_two_sided, golden_inputs, name_of, specs
from v2ce_toolbox_amd import hip, synth
from v2ce_toolbox_amd import losses as VL
from v2ce_toolbox_amd import stage1_metrics as S
from v2ce_toolbox_amd.LDATI import EVENT_DTYPE
from v2ce_toolbox_amd.voxelize import gen_discretized_event_volume_batch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = ("n", "pyr_n", "temporal_n", "ef_n", "comp_n", "match_n", "match_low")
SUMS = ("sq_sum", "abs_diff_sum", "pred_abs_sum", "pred_sq_sum", "pyr_sq_sum", "temporal_sq_sum", "ef_sq_sum",
        "comp_sq_sum")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def voxels(rng, shape, density=0.3, scale=0.5):
    return (rng.exponential(scale, shape) * (rng.random(shape) < density)).astype(np.float32)


def check_stats(got, want, pred):
    """got: VoxLosses with one row per b; want: the restated record of each b.  Counts equal; f64 sums to 1e-12
    relative; the match sum to 1e-12 |want| + 1e-13 columns (1 + max |pred|): device exp / log are within a few ulps of
    libm, not equal to it, and logsumexp - pred[t] cancels."""
    assert len(got) == len(want)
    for b, w in enumerate(want):
        for k in COUNTS:
            assert np.array_equal(getattr(got, k)[b], w[k]), (b, k, getattr(got, k)[b], w[k])
        for k in SUMS:
            g, x = np.atleast_1d(getattr(got, k)[b]), np.atleast_1d(np.asarray(w[k], np.float64))
            nan = np.isnan(x)
            assert np.array_equal(np.isnan(g), nan), (b, k, g, x)
            assert np.all(np.abs(g[~nan] - x[~nan]) <= 1e-12 * np.abs(x[~nan])), (b, k, g, x)
        g, x = got.match_sum[b], w["match_sum"]
        if np.isnan(x):
            assert np.isnan(g), (b, g)
        else:
            bound = 1e-12 * abs(x) + 1e-13 * w["match_n"] * (1 + float(np.nanmax(np.abs(pred[b]))))
            assert abs(g - x) <= bound, (b, g, x, bound)


@pytest.mark.parametrize("B,L,H,W,terms", [
    (1, 1, 8, 8, VL.ALL), (1, 1, 9, 15, VL.ALL), (2, 3, 11, 13, VL.ALL), (1, 4, 16, 24, VL.ALL), (3, 2, 8, 70, VL.ALL),
    (1, 5, 17, 23, VL.ALL), (2, 3, 7, 9, ("temporal", "ef", "compensation", "match")), (1, 16, 260, 346, VL.ALL)])
def test_statistics_match_the_restatement(B, L, H, W, terms):
    rng = np.random.default_rng(B * 1000 + L * 100 + H)
    p, g = voxels(rng, (B, L, 20, H, W)), voxels(rng, (B, L, 20, H, W))
    p.reshape(-1)[::13] = np.float32(0.01)          # exactly at the threshold: not above it
    g.reshape(-1)[::29] = np.float32(0.01)
    st = VL.voxel_losses_batch(dev(p), dev(g), terms=terms)
    check_stats(st, R.batch_stats(p, g, terms), p)
    assert (st.raw["term_mask"] == VL.term_mask(terms)).all()


def test_misaligned_base():
    rng = np.random.default_rng(5)
    p, g = voxels(rng, (2, 3, 20, 9, 11)), voxels(rng, (2, 3, 20, 9, 11))
    big = torch.zeros(1 + p.size, device="cuda")
    pv = big[1:].view(p.shape)                        # contiguous, but 4-B aligned only
    pv.copy_(dev(p))
    check_stats(VL.voxel_losses_batch(pv, dev(g)), R.batch_stats(p, g), p)


def to_volumes(t):
    B, L, C, H, W = t.shape
    return t.reshape(B, L, 2, 10, H, W).permute(0, 2, 1, 3, 4, 5).reshape(B * 2, L * 10, H, W).contiguous()


@pytest.mark.parametrize("path", GOLDENS, ids=name_of)
def test_drop_ins_and_calculate_loss_against_reference(path):
    z, pn, gn, p2n = golden_inputs(path)
    p, g = dev(pn), dev(gn)
    stages = [p, dev(p2n)] if p2n is not None else None
    for suffix, kw, pick, staged in specs(z):
        total, d = VL.calculate_loss(stages if staged else p, g, **kw)
        assert total.dtype == torch.float32 and total.dim() == 0 and total.is_cuda
        assert list(d) == [k for k in ("ef_loss", "pyramid_loss", "pt_loss", "match", "compensation", "norml1", "norml2")
                           if k in d]
        assert all(v.dtype == torch.float32 and v.dim() == 0 and not v.is_cuda for v in d.values())
        check_two_sided(float(total) if pick == "loss" else float(d[pick]), z, suffix, "calculate_loss")
    pv, gv = to_volumes(p), to_volumes(g)
    for base in (False, True):
        v = VL.Pyramid3dLoss(add_base_loss=base)(pv, gv)
        assert v.dtype == torch.float32 and v.dim() == 0 and v.is_cuda
        check_two_sided(float(v), z, f"pyramid_base{int(base)}", "Pyramid3dLoss")
    check_two_sided(float(VL.PyramidTemporalLoss()(pv, gv)), z, "pt_loss", "PyramidTemporalLoss")
    check_two_sided(float(VL.CompensationLoss()(p, g)), z, "compensation", "CompensationLoss")
    check_two_sided(float(VL.MatchLoss()(p, g)), z, "match", "MatchLoss")
    # the [N, D, H, W] entry on the rearranged copy: the record of b is the sum of its two volumes, bit for bit
    s5 = VL.voxel_losses_batch(p, g)
    sv = VL.volume_losses_batch(pv, gv)
    assert len(sv) == 2 * len(s5)
    for k in ("n", "sq_sum", "abs_diff_sum", "pred_abs_sum", "pred_sq_sum", "pyr_n", "pyr_sq_sum", "temporal_n",
              "temporal_sq_sum"):
        a = getattr(sv, k)
        assert (a[0::2] + a[1::2]).tobytes() == getattr(s5, k).tobytes(), k
    assert not sv.ef_n.any() and not sv.comp_n.any() and not sv.match_n.any()


def test_batch_equals_single_calls_and_repeats():
    rng = np.random.default_rng(8)
    p, g = voxels(rng, (3, 5, 20, 13, 18)), voxels(rng, (3, 5, 20, 13, 18))
    a = VL.voxel_losses_batch(dev(p), dev(g)).raw
    b = VL.voxel_losses_batch(dev(p), dev(g)).raw
    assert a.tobytes() == b.tobytes()
    for i in range(3):
        one = VL.voxel_losses_batch(dev(p[i:i + 1]), dev(g[i:i + 1])).raw
        assert one.tobytes() == a[i:i + 1].tobytes(), i
    pv, gv = to_volumes(dev(p)), to_volumes(dev(g))
    a = VL.volume_losses_batch(pv, gv).raw
    assert a.tobytes() == VL.volume_losses_batch(pv, gv).raw.tobytes()
    for i in (0, 5):
        assert VL.volume_losses_batch(pv[i:i + 1], gv[i:i + 1]).raw.tobytes() == a[i:i + 1].tobytes(), i


def test_volume_entry_at_any_depth():
    rng = np.random.default_rng(9)
    for D in (8, 9, 11, 13, 25):                      # D % 3 = 2, 0, 2, 1, 1; the last chunk of ten planes is partial
        p, g = voxels(rng, (2, D, 9, 10)), voxels(rng, (2, D, 9, 10))
        st = VL.volume_losses_batch(dev(p), dev(g))
        for n in range(2):
            w = R.volume_stats(p[n], g[n])
            for k in ("n", "pyr_n", "temporal_n"):
                assert np.array_equal(getattr(st, k)[n], w[k]), (D, k)
            for k in ("sq_sum", "abs_diff_sum", "pred_abs_sum", "pred_sq_sum", "pyr_sq_sum", "temporal_sq_sum"):
                a, x = np.atleast_1d(getattr(st, k)[n]), np.atleast_1d(w[k])
                assert np.all(np.abs(a - x) <= 1e-12 * np.abs(x)), (D, k, a, x)
    p, g = voxels(rng, (1, 5, 3, 3)), voxels(rng, (1, 5, 3, 3))
    st = VL.volume_losses_batch(dev(p), dev(g), terms=("temporal",))
    w = R.volume_stats(p[0], g[0], pyramid=False)
    assert np.all(np.abs(st.temporal_sq_sum[0] - w["temporal_sq_sum"]) <= 1e-12 * w["temporal_sq_sum"])


def test_nan_propagates_into_every_sum_it_touches():
    rng = np.random.default_rng(6)
    p, g = voxels(rng, (2, 2, 20, 8, 12)), voxels(rng, (2, 2, 20, 8, 12))
    p[0, 1, 3, 2, 11] = np.nan                        # column 11 of 12 lies outside the floored k = 8 window
    st = VL.voxel_losses_batch(dev(p), dev(g))
    want = R.batch_stats(p, g)
    check_stats(st, want, p)
    for k in ("sq_sum", "abs_diff_sum", "pred_abs_sum", "pred_sq_sum", "comp_sq_sum", "match_sum"):
        assert np.isnan(getattr(st, k)[0]) and np.isfinite(getattr(st, k)[1]), k
    assert np.isnan(st.pyr_sq_sum[0, :2]).all() and np.isfinite(st.pyr_sq_sum[0, 2])
    assert np.isnan(st.temporal_sq_sum[0]).all() and np.isnan(st.ef_sq_sum[0]).all()
    assert np.isfinite(st.pyr_sq_sum[1]).all() and np.isfinite(st.ef_sq_sum[1]).all()


def test_match_low_counts_a_column_with_spread_100():
    rng = np.random.default_rng(7)
    p, g = voxels(rng, (1, 3, 20, 8, 9)), voxels(rng, (1, 3, 20, 8, 9))
    assert int(VL.voxel_losses_batch(dev(p), dev(g), terms=("match",)).match_low[0]) == 0
    p[0, :, 13, 2, 4] = (0.0, 100.0, 1.0)
    g[0, :, 13, 2, 4] = (2.0, 0.0, 1.0)               # the argmax of gt is frame 0, where pred is 100 below its maximum
    st = VL.voxel_losses_batch(dev(p), dev(g), terms=("match",))
    assert int(st.match_low[0]) == 1
    check_stats(st, R.batch_stats(p, g, ("match",)), p)


def test_refusals():
    x = torch.zeros(1, 2, 20, 8, 8, device="cuda")
    with pytest.raises(ValueError):
        VL.voxel_losses_batch(torch.zeros(1, 2, 18, 8, 8, device="cuda"), torch.zeros(1, 2, 18, 8, 8, device="cuda"))
    small = torch.zeros(1, 2, 20, 7, 9, device="cuda")
    with pytest.raises(ValueError, match="smaller than kernel size"):
        VL.voxel_losses_batch(small, small)
    with pytest.raises(ValueError, match="smaller than kernel size"):
        VL.calculate_loss(small, small)
    with pytest.raises(ValueError, match="smaller than kernel size"):
        VL.Pyramid3dLoss()(torch.zeros(1, 1, 5, 7, device="cuda"), torch.zeros(1, 1, 5, 7, device="cuda"))
    with pytest.raises(ValueError, match="too small"):
        VL.PyramidTemporalLoss()(torch.zeros(2, 4, 8, 8, device="cuda"), torch.zeros(2, 4, 8, 8, device="cuda"))
    with pytest.raises(ValueError):
        VL.volume_losses_batch(x[0], x[0], terms=("ef",))
    nc = torch.zeros(1, 2, 20, 8, 16, device="cuda")[..., ::2]
    with pytest.raises(ValueError, match="contiguous"):
        VL.voxel_losses_batch(nc, nc)
    with pytest.raises(hip.V2ceHipError, match="no CPU path"):
        VL.voxel_losses_batch(x.cpu(), x.cpu())
    with pytest.raises(ValueError):
        VL.voxel_losses_batch(x, torch.zeros(1, 3, 20, 8, 8, device="cuda"))
    with pytest.raises(ValueError, match="discriminator"):
        VL.calculate_loss(x, x, loss=("pyramid", "gan"))
    total, d = VL.calculate_loss(x, x, loss=("ef", "physical"))     # skipped, as without attention maps
    assert list(d) == ["ef_loss"] and float(total) == 0.0
    with pytest.raises(ValueError, match="not requested"):
        VL.voxel_losses_batch(x, x, terms=("ef",)).pyramid()


# ---------------------------------------------------------------------------------------------------------------------
# the driver and the command line

def random_events(rng, T, H, W, per_pair):
    """A host event stream grouped by pair: per_pair events in each [T_i, T_{i+1})."""
    lists = []
    for i in range(len(T) - 1):
        e = np.zeros(per_pair, EVENT_DTYPE)
        e["timestamp"] = np.sort(rng.integers(T[i], T[i + 1], per_pair))
        e["x"], e["y"], e["polarity"] = rng.integers(0, W, per_pair), rng.integers(0, H, per_pair), rng.choice([-1, 1], per_pair)
        lists.append(e)
    return np.concatenate(lists), np.full(len(T) - 1, per_pair, np.int64)


def test_driver_reports_the_losses_of_each_window():
    H, W, P = 64, 80, 33
    rng = np.random.default_rng(11)
    T = np.arange(P + 1, dtype=np.int64) * 33333
    gt, counts = random_events(rng, T, H, W, 3000)
    vox = torch.from_numpy(synth.synthetic_voxels(P, H, W, seed=4, regime="sparse")).cuda().reshape(P, 2, 10, H, W)
    opts = dict(ef_type="only_c", add_base_loss=True, alpha_pyramid=10.0)
    base_summary, base_rec = S.run_stage1_metric(vox, gt, counts, None, seq_len=16)
    summary, rec = S.run_stage1_metric(vox, gt, counts, None, seq_len=16, losses=ALL_LOSS, loss_options=opts)
    assert summary == base_summary and rec["values"] == base_rec["values"]
    assert "losses" not in base_rec and "summary_losses" not in base_rec
    assert rec["windows"] == [[0, 16], [16, 32], [32, 33]] and len(rec["losses"]) == 3
    gv, _ = gen_discretized_event_volume_batch(gt, counts, 10, H, W)
    gvn, pvn = gv.cpu().numpy(), vox.reshape(P, 20, H, W).cpu().numpy()
    close = lambda a, b: abs(a - b) <= 1e-6 * abs(b) + 1e-12
    per = []
    for i, (a, b) in enumerate(rec["windows"]):
        total, d = R.loss_values([R.seq_stats(pvn[a:b], gvn[a:b])], loss=ALL_LOSS, ef_type="only_c", add_base_loss=True,
                                 alpha_pyramid=10.0)
        got = rec["losses"][i]
        assert list(got["loss_dict"]) == list(d)                     # the 1-pair window reports every term too
        for k, v in d.items():
            assert close(got["loss_dict"][k], v), (i, k, got["loss_dict"][k], v)
        assert close(got["loss"], total), (i, got["loss"], total)
        per.append({**d, "loss": total})
    for k in per[0]:
        assert close(rec["summary_losses"][k], np.mean([v[k] for v in per])), k


def test_driver_records_null_for_a_term_the_window_is_too_small_for():
    H, W, P = 6, 9, 3
    rng = np.random.default_rng(12)
    T = np.arange(P + 1, dtype=np.int64) * 1000
    gt, counts = random_events(rng, T, H, W, 50)
    vox = dev(voxels(rng, (P, 2, 10, H, W)))
    _, rec = S.run_stage1_metric(vox, gt, counts, None, seq_len=2, pool_sizes=(2,), losses=("pyramid", "ef", "pt"))
    assert len(rec["losses"]) == 2
    for r in rec["losses"]:
        assert r["loss"] is None and r["loss_dict"]["pyramid_loss"] is None
        assert r["loss_dict"]["ef_loss"] > 0 and r["loss_dict"]["pt_loss"] > 0
    assert rec["summary_losses"]["pyramid_loss"] is None and rec["summary_losses"]["ef_loss"] > 0


def _cli(args, cwd):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "v2ce_eval.py")] + args, capture_output=True, text=True,
                       cwd=cwd, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r


def test_cli_stage1_losses(tmp_path):
    H, W, P = 16, 24, 8                               # two windows of four pairs: a 1-pair window has match = log 1 = 0
    rng = np.random.default_rng(13)
    T = np.arange(P + 1, dtype=np.int64) * 33333
    ev, _ = random_events(rng, T, H, W, 400)
    np.savez(tmp_path / "ev.npz", event_stream=ev)
    np.save(tmp_path / "T.npy", T)
    base = ["--stage1", "--pred_events", str(tmp_path / "ev.npz"), "--gt_events", str(tmp_path / "ev.npz"),
            "--frame_timestamps", str(tmp_path / "T.npy"), "--height", str(H), "--width", str(W), "--seq_len", "4"]
    _cli(base + ["-o", str(tmp_path / "plain")], tmp_path)
    assert sorted(os.listdir(tmp_path / "plain")) == ["stage1_record.json", "stage1_result.csv"]
    r = _cli(base + ["--stage1_losses"] + list(ALL_LOSS) + ["--ef_type", "cl", "-o", str(tmp_path / "with")], tmp_path)
    assert sorted(os.listdir(tmp_path / "with")) == ["stage1_loss_result.csv", "stage1_record.json", "stage1_result.csv"]
    assert (tmp_path / "plain" / "stage1_result.csv").read_bytes() == (tmp_path / "with" / "stage1_result.csv").read_bytes()
    plain = json.load(open(tmp_path / "plain" / "stage1_record.json"))
    rec = json.load(open(tmp_path / "with" / "stage1_record.json"))
    assert "losses" not in plain and "summary_losses" not in plain
    losses_, mean = rec.pop("losses"), rec.pop("summary_losses")
    assert rec == plain and list(rec) == list(plain)
    assert len(losses_) == 2 and "stage1_loss_result.csv" in r.stdout
    # the stream against itself: every term is zero except the norms of pred and the match term (log of a sum >= 1)
    for w in losses_:
        d = w["loss_dict"]
        assert list(d) == ["ef_loss", "pyramid_loss", "pt_loss", "match", "compensation", "norml1", "norml2"]
        assert d["ef_loss"] == 0.0 and d["pyramid_loss"] == 0.0 and d["pt_loss"] == 0.0 and d["compensation"] == 0.0
        assert d["match"] > 0 and d["norml1"] > 0 and d["norml2"] > 0
    rows = list(csv.reader(open(tmp_path / "with" / "stage1_loss_result.csv")))
    assert rows[0] == ["term", "mean"] and [r_[0] for r_ in rows[1:]] == list(mean) == list(losses_[0]["loss_dict"]) + ["loss"]
    assert float(rows[1][1]) == 0.0 and float(rows[-1][1]) == mean["loss"] > 0
    # the defaults of the reference's training run without 'gan'
    _cli(base + ["--stage1_losses", "-o", str(tmp_path / "dflt")], tmp_path)
    d = json.load(open(tmp_path / "dflt" / "stage1_record.json"))["losses"][0]["loss_dict"]
    assert list(d) == ["ef_loss", "pyramid_loss", "compensation"]
