"""Vectorised numpy restatement of the stage-2 score ts_diff_metric (stage2_metrics.py:22-88), written afresh: per GT
event d = min(1e6, min |t_pred - t_gt|) over the predicted events of its polarity in the clamped (2r+1)^2 window, capped
at cap = 1e6 / fps / 10 * 3.  Returns per-event d (f64), S (int64 sum of the uncapped d), K (capped count) and
avg = (S + K * cap) / N.  Not a test module (no test_ prefix)."""
import numpy as np


def tsdiff_ref(gt_ts, gt_x, gt_y, gt_p, pr_ts, pr_x, pr_y, pr_p, fps, r, H=260, W=346):
    gt_ts, pr_ts = np.asarray(gt_ts, np.int64), np.asarray(pr_ts, np.int64)
    gx, gy = np.asarray(gt_x, np.int64), np.asarray(gt_y, np.int64)
    px, py = np.asarray(pr_x, np.int64), np.asarray(pr_y, np.int64)
    gp = (np.asarray(gt_p) == 1).astype(np.int64)               # -1 and 0 -> 0
    pp = (np.asarray(pr_p) != 0).astype(np.int64)               # any non-zero -> 1
    assert ((gx >= 0) & (gx < W) & (gy >= 0) & (gy < H)).all() and ((px >= 0) & (px < W) & (py >= 0) & (py < H)).all()
    n = gt_ts.size
    best = np.full(n, 1000000, dtype=np.int64)
    if pr_ts.size:
        cell = (pp * H + py) * W + px
        order = np.lexsort((pr_ts, cell))
        sc, st = cell[order], pr_ts[order]
        uniq = np.unique(np.concatenate([st, gt_ts]))
        R = np.int64(uniq.size + 1)
        key = sc * R + np.searchsorted(uniq, st)
        tq = np.searchsorted(uniq, gt_ts)
        ra, rb = min(int(r), W - 1), min(int(r), H - 1)
        for db in range(-rb, rb + 1):
            b = gy + db
            for da in range(-ra, ra + 1):
                a = gx + da
                ok = (a >= 0) & (a < W) & (b >= 0) & (b < H)
                if not ok.any():
                    continue
                qc = (gp * H + b) * W + a
                lo = np.searchsorted(sc, qc, "left")
                hi = np.searchsorted(sc, qc, "right")
                idx = np.searchsorted(key, qc * R + tq, "left")
                for cand in (idx, idx - 1):
                    m = ok & (cand >= lo) & (cand < hi)
                    c = np.clip(cand, 0, st.size - 1)
                    diff = np.abs(st[c] - gt_ts)
                    best = np.where(m, np.minimum(best, diff), best)
    cap = 1e6 / fps / 10 * 3
    capped = best.astype(np.float64) > cap
    d = np.where(capped, cap, best.astype(np.float64))
    S = int(best[~capped].sum())
    K = int(capped.sum())
    avg = (float(S) + float(K) * cap) / n if n else float("nan")
    return d, S, K, avg
