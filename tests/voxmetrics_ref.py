"""Numpy restatement of the stage-1 statistics (csrc/voxmetrics.hip, train/scripts/model/metrics.py), written afresh
from the rules: binarise v > f32 threshold; sum_c = the 10 bins of a polarity added in order, sum_cp = the 20 channels
in order, both f32 from zero; |p - g| and r = (p + 0.01f) / (g + 0.01f), r < 1 ? 1 / r : r in f32; AvgPool3d(k, k) over
((l c), h, w) per (b, polarity), each axis floored to a multiple of k, a pooled value the f32 sum of its k^3 values in
(d, h, w) order / f32(k^3).  Sums in f64.  ``borderline`` flags op elements within 8 ulps of the threshold, where
torch's own summation order may decide the other way.  Also the serial-put_ voxeliser.  Not a test module."""
import numpy as np

F = np.float32


def _ops(v):
    """[B, L, 20, H, W] -> (raw, sum_c [B, L, 2, H, W], sum_cp [B, L, H, W]) with sequential f32 sums."""
    B, L, C, H, W = v.shape
    sc = np.zeros((B, L, 2, H, W), F)
    for p in range(2):
        for c in range(10):
            sc[:, :, p] = sc[:, :, p] + v[:, :, p * 10 + c]
    scp = np.zeros((B, L, H, W), F)
    for ch in range(C):
        scp = scp + v[:, :, ch]
    return v, sc, scp


def _pool(v, k):
    """[B, L, 20, H, W] -> pooled [B, 2, Dk, Hk, Wk] f32."""
    B, L, C, H, W = v.shape
    x = v.reshape(B, L, 2, 10, H, W).transpose(0, 2, 1, 3, 4, 5).reshape(B, 2, 10 * L, H, W)
    Dk, Hk, Wk = 10 * L // k, H // k, W // k
    x = x[:, :, :Dk * k, :Hk * k, :Wk * k].reshape(B, 2, Dk, k, Hk, k, Wk, k)
    s = np.zeros((B, 2, Dk, Hk, Wk), F)
    for dd in range(k):
        for hh in range(k):
            for ww in range(k):
                s = s + x[:, :, :, dd, :, hh, :, ww]
    return s / F(k * k * k)


def stats(pred, gt, threshold=0.01, pool_sizes=(2, 4)):
    """Per b: dict of n, tp, fp, fn [B, 3], abs_diff_sum, ratio_sum [B], pool_sq_sum, pool_n [B, K], borderline [B, 3]."""
    pred, gt = np.asarray(pred, F), np.asarray(gt, F)
    B = pred.shape[0]
    thr = F(threshold)
    out = {k: np.zeros((B, 3), np.int64) for k in ("n", "tp", "fp", "fn", "borderline")}
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for o, (a, b) in enumerate(zip(_ops(pred), _ops(gt))):
            pa, ga = a > thr, b > thr
            ax = tuple(range(1, a.ndim))
            out["n"][:, o] = int(np.prod(a.shape[1:]))
            out["tp"][:, o] = (pa & ga).sum(axis=ax)
            out["fp"][:, o] = (pa & ~ga).sum(axis=ax)
            out["fn"][:, o] = (~pa & ga).sum(axis=ax)
            ulp = np.spacing(thr) * 8
            near = (np.abs(a - thr) <= ulp) | (np.abs(b - thr) <= ulp)
            out["borderline"][:, o] = near.sum(axis=ax) if o else 0
        d = np.abs(pred - gt).astype(np.float64)
        out["abs_diff_sum"] = d.reshape(B, -1).sum(axis=1)
        r = (pred + F(0.01)) / (gt + F(0.01))
        r = np.where(r < F(1), F(1) / r, r)
        out["ratio_sum"] = r.astype(np.float64).reshape(B, -1).sum(axis=1)
        sq, pn = [], []
        for k in pool_sizes:
            df = _pool(pred, k) - _pool(gt, k)
            sq.append((df * df).astype(np.float64).reshape(B, -1).sum(axis=1))
            pn.append(np.full(B, df[0].size, np.int64))
        out["pool_sq_sum"] = np.stack(sq, 1) if sq else np.zeros((B, 0))
        out["pool_n"] = np.stack(pn, 1) if pn else np.zeros((B, 0), np.int64)
    return out


def f1(tp, fp, fn):
    tp, fp, fn, eps = F(tp), F(fp), F(fn), F(1e-8)
    p = tp / (tp + fp + eps)
    r = tp / (tp + fn + eps)
    return F(F(2) * (p * r)) / (p + r + eps)


def values(s):
    """The values of the whole batch (what the reference returns for [B, ...])."""
    t = {k: np.asarray(v).sum(axis=0) for k, v in s.items()}
    out = {}
    for o, op in enumerate(("raw", "sum_c", "sum_cp")):
        out[f"BinaryMatch_{op}"] = (t["n"][o] - t["fp"][o] - t["fn"][o]) / float(t["n"][o])
        out[f"BinaryMatchF1_{op}"] = float(f1(t["tp"][o], t["fp"][o], t["fn"][o]))
    out["L1"] = float(F(t["abs_diff_sum"] / t["n"][0]))
    out["MeanRatio"] = float(F(t["ratio_sum"] / t["n"][0]))
    for q in range(np.asarray(s["pool_n"]).shape[1]):
        out[f"PoolMSE_q{q}"] = float(F(t["pool_sq_sum"][q] / t["pool_n"][q]))
    return out


def voxelize_serial(ts, x, y, p, bins, H, W, t_range=None):
    """The reference's gen_discretized_event_volume with a serial put_: floor contributions in event order, then ceil
    contributions, f32 from zero; polarity <= 0 to the negative half."""
    ts = np.asarray(ts, np.int64)
    vol = np.zeros(2 * bins * H * W, F)
    if ts.size == 0:
        return vol.reshape(2 * bins, H, W)
    t_min, t_max = (int(ts.min()), int(ts.max())) if t_range is None else (int(t_range[0]), int(t_range[1]))
    if t_max == t_min:
        return vol.reshape(2 * bins, H, W)
    scale = F(F(1) / F(t_max - t_min)) * F(bins - 1)
    t = np.clip((ts - t_min).astype(F) * scale, F(0), F(bins - 1)).astype(F)
    fl = np.floor(t + F(1e-8)).astype(F)
    ce = np.ceil(t - F(1e-8)).astype(F)
    d_fl = (np.floor(t) + F(1)) - t
    d_ce = t - fl
    half = (np.asarray(p) <= 0).astype(np.int64) * bins
    pix = np.asarray(y, np.int64) * W + np.asarray(x, np.int64)
    for b, d in ((fl, d_fl), (ce, d_ce)):
        idx = (b.astype(np.int64) + half) * H * W + pix
        for i, v in zip(idx.tolist(), d.tolist()):     # serial: float32 adds one by one
            vol[i] = F(vol[i] + F(v))
    return vol.reshape(2 * bins, H, W)
