"""The stage-1 score of the reference's study -- voxel grids against a recording's voxels, mirroring
``train/scripts/model/metrics.py`` (and the baseline scripts ``train/scripts/tools/esim_metric.py`` /
``v2e_metric.py``):

* drop-ins ``BinaryMatch(op_type)``, ``BinaryMatchF1(threshold, op_type)``, ``f1score``, ``PoolMSE(kernel_size)``,
  ``MeanRatio()`` and ``L1()`` (the value of ``nn.L1Loss()``): the reference's constructor arguments and
  ``forward(pred, y)`` on ``[b, l, 20, h, w]`` f32 device tensors, 0-d device tensors in the reference's dtypes back
* ``voxel_metrics_batch(pred, gt)``   per-sequence sufficient statistics and values of all of them in one device pass
  (``csrc/voxmetrics.hip`` through ``v2ce_voxmetrics``) and one host synchronisation
* ``run_stage1_metric(voxels, gt_events, ...)``   the per-recording driver: GT voxelised per pair
  (``voxelize.gen_discretized_event_volume_batch``), windows of ``seq_len`` pairs scored as one sequence each; with
  ``losses=...`` also the voxel loss terms of ``losses.calculate_loss`` per window

Values from the statistics: BinaryMatch = (N - FP - FN) / N in f64; BinaryMatchF1 evaluates the reference's f32
formula (metrics.py:65-90) on the exact counts cast to f32; PoolMSE, MeanRatio and L1 are the f64 sum / count rounded
to f32.  The sums of 10 or 20 channels are taken in order; torch's own order differs by a few ulps, so a threshold
decision can differ from the reference only for a sum within a few ulps of the threshold.  There is no CPU path.
"""
from __future__ import annotations

import ctypes
import logging
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import hip

logger = logging.getLogger("V2CE")

OPS = ("raw", "sum_c", "sum_cp")
CHANNELS = 20
STATS_DTYPE = np.dtype([("struct_size", "<i8"), ("n", "<i8", 3), ("tp", "<i8", 3), ("fp", "<i8", 3), ("fn", "<i8", 3),
                        ("abs_diff_sum", "<f8"), ("ratio_sum", "<f8"), ("n_pools", "<i8"),
                        ("pool_size", "<i8", hip.VOXMETRICS_MAX_POOLS), ("pool_n", "<i8", hip.VOXMETRICS_MAX_POOLS),
                        ("pool_sq_sum", "<f8", hip.VOXMETRICS_MAX_POOLS)])
assert STATS_DTYPE.itemsize == ctypes.sizeof(hip.VoxMetricsStats)
# the metrics of v2e_metric.py:84-93, then L1 and MeanRatio
METRIC_NAMES = ("BinaryMatchF1_sum_c", "BinaryMatchF1_sum_cp", "BinaryMatchF1_raw", "BinaryMatch_sum_c",
                "BinaryMatch_sum_cp", "BinaryMatch_raw", "PoolMSE_2", "PoolMSE_4", "L1", "MeanRatio")


def f1_from_counts(tp, fp, fn) -> np.float32:
    """metrics.py:65-90 in f32 on counts: precision = TP / (TP + FP + 1e-8), recall likewise, 2 p r / (p + r + 1e-8)."""
    tp, fp, fn = np.float32(tp), np.float32(fp), np.float32(fn)
    eps = np.float32(1e-8)
    precision = tp / (tp + fp + eps)
    recall = tp / (tp + fn + eps)
    return np.float32(np.float32(2) * (precision * recall)) / (precision + recall + eps)


@dataclass
class VoxMetrics:
    """Per-sequence statistics of ``voxel_metrics_batch`` (host numpy arrays, one row per b) and what they add up to.

    ``n, tp, fp, fn``: int64 [B, 3] (ops raw, sum_c, sum_cp); ``abs_diff_sum, ratio_sum``: f64 [B];
    ``pool_sq_sum``: f64 [B, K] and ``pool_n``: int64 [B, K] for ``pool_sizes`` [K]."""
    n: np.ndarray
    tp: np.ndarray
    fp: np.ndarray
    fn: np.ndarray
    abs_diff_sum: np.ndarray
    ratio_sum: np.ndarray
    pool_sizes: tuple
    pool_sq_sum: np.ndarray
    pool_n: np.ndarray
    raw: np.ndarray = field(repr=False, default=None)     # the records as returned (STATS_DTYPE [B])

    def select(self, rows) -> "VoxMetrics":
        """The statistics of some sequences (an index or slice of b)."""
        r = np.atleast_1d(np.arange(self.n.shape[0])[rows])
        return VoxMetrics(self.n[r], self.tp[r], self.fp[r], self.fn[r], self.abs_diff_sum[r], self.ratio_sum[r],
                          self.pool_sizes, self.pool_sq_sum[r], self.pool_n[r], None if self.raw is None else self.raw[r])

    def _op(self, op_type):
        if op_type not in OPS:
            raise ValueError(f"op_type must be one of {OPS}, got {op_type!r}")
        return OPS.index(op_type)

    def binary_match(self, op_type="raw") -> np.ndarray:
        """Per sequence, f64 (N - FP - FN) / N."""
        o = self._op(op_type)
        return (self.n[:, o] - self.fp[:, o] - self.fn[:, o]) / self.n[:, o].astype(np.float64)

    def binary_match_f1(self, op_type="sum_cp") -> np.ndarray:
        o = self._op(op_type)
        return np.array([f1_from_counts(*v) for v in zip(self.tp[:, o], self.fp[:, o], self.fn[:, o])], np.float32)

    def pool_mse(self, k) -> np.ndarray:
        q = self.pool_sizes.index(int(k))
        return (self.pool_sq_sum[:, q] / self.pool_n[:, q]).astype(np.float32)

    def mean_ratio(self) -> np.ndarray:
        return (self.ratio_sum / self.n[:, 0]).astype(np.float32)

    def l1(self) -> np.ndarray:
        return (self.abs_diff_sum / self.n[:, 0]).astype(np.float32)

    def total(self) -> "VoxMetrics":
        """All sequences as one batch: what the reference returns for the whole [B, ...] input."""
        s = lambda a: a.sum(axis=0, keepdims=True)
        return VoxMetrics(s(self.n), s(self.tp), s(self.fp), s(self.fn), s(self.abs_diff_sum), s(self.ratio_sum),
                          self.pool_sizes, s(self.pool_sq_sum), s(self.pool_n))

    def values(self) -> Dict[str, np.ndarray]:
        """Per sequence, every metric of METRIC_NAMES whose pool size was computed."""
        out = {}
        for op in ("sum_c", "sum_cp", "raw"):
            out[f"BinaryMatchF1_{op}"] = self.binary_match_f1(op)
        for op in ("sum_c", "sum_cp", "raw"):
            out[f"BinaryMatch_{op}"] = self.binary_match(op)
        for k in (2, 4):
            if k in self.pool_sizes:
                out[f"PoolMSE_{k}"] = self.pool_mse(k)
        out["L1"] = self.l1()
        out["MeanRatio"] = self.mean_ratio()
        return out


def _check_voxels(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch tensor")
    if not t.is_cuda:
        raise hip.V2ceHipError(f"{name} must live on a HIP device (got {t.device}); there is no CPU path")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32 (got {t.dtype})")
    if t.dim() != 5 or t.shape[2] != CHANNELS:
        raise ValueError(f"{name} must be [b, l, 20, h, w] (channels (p c): 2 polarities x 10 bins), got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def voxel_metrics_batch(pred: torch.Tensor, gt: torch.Tensor, *, threshold: float = 0.01,
                        pool_sizes: Sequence[int] = (2, 4)) -> VoxMetrics:
    """Sufficient statistics of the stage-1 metrics per sequence b of ``pred``, ``gt`` [B, L, 20, H, W] (f32,
    contiguous, on one device), in one pass and one host synchronisation.  ``pool_sizes``: up to 8 sizes, each in
    [1, min(10 L, H, W)]; 2 and 4 ride along with the fused pass, every other size costs one extra launch."""
    _check_voxels(pred, "pred")
    _check_voxels(gt, "gt")
    if pred.shape != gt.shape:
        raise ValueError(f"pred {tuple(pred.shape)} and gt {tuple(gt.shape)} differ in shape")
    if pred.device != gt.device:
        raise ValueError("pred and gt live on different devices")
    B, Lq, C, H, W = (int(v) for v in pred.shape)
    ks = tuple(int(k) for k in pool_sizes)
    if len(ks) > hip.VOXMETRICS_MAX_POOLS:
        raise ValueError(f"at most {hip.VOXMETRICS_MAX_POOLS} pool sizes")
    kmax = min(10 * Lq, H, W)
    for k in ks:
        if not 1 <= k <= kmax:
            raise ValueError(f"pool size {k} outside [1, {kmax}] (torch refuses a window larger than its input)")
    L = hip.lib()
    karr = (ctypes.c_int * max(1, len(ks)))(*ks)
    ws_bytes = L.v2ce_voxmetrics_workspace_bytes(B, Lq, C, H, W, karr, len(ks))
    if ws_bytes == 0:
        raise hip.V2ceHipError(f"v2ce_voxmetrics: unsupported shape {tuple(pred.shape)} with pool sizes {ks}")
    dev = pred.device
    with torch.cuda.device(dev):
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        out = torch.empty(B * STATS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        hip.check(L.v2ce_voxmetrics(pred.data_ptr(), gt.data_ptr(), B, Lq, C, H, W, float(threshold), karr, len(ks),
                                    out.data_ptr(), ctypes.sizeof(hip.VoxMetricsStats), ws.data_ptr(), ws_bytes,
                                    hip.stream_ptr(dev)), "v2ce_voxmetrics")
        rec = out.cpu().numpy().view(STATS_DTYPE)                         # the one synchronisation
    if (rec["struct_size"] != STATS_DTYPE.itemsize).any():
        raise hip.V2ceHipError("v2ce_voxmetrics wrote records of another layout")
    nk = len(ks)
    return VoxMetrics(rec["n"].copy(), rec["tp"].copy(), rec["fp"].copy(), rec["fn"].copy(), rec["abs_diff_sum"].copy(),
                      rec["ratio_sum"].copy(), ks, rec["pool_sq_sum"][:, :nk].copy(), rec["pool_n"][:, :nk].copy(), rec)


def _scalar(v, dtype, device):
    return torch.tensor(v, dtype=dtype, device=device)


class BinaryMatch(torch.nn.Module):
    """metrics.py BinaryMatch: f64 fraction of equal binarised (v > 0.01) values after the op."""

    def __init__(self, op_type="raw", **kwargs):
        super().__init__()
        assert op_type in OPS
        self.op_type = op_type

    def forward(self, pred, y):
        s = voxel_metrics_batch(pred, y, pool_sizes=()).total()
        return _scalar(float(s.binary_match(self.op_type)[0]), torch.float64, pred.device)


class BinaryMatchF1(torch.nn.Module):
    """metrics.py BinaryMatchF1: f32 F1 of the binarised (v > threshold) values after the op."""

    def __init__(self, threshold=0.01, op_type="sum_cp", **kwargs):
        super().__init__()
        assert op_type in OPS
        self.threshold = threshold
        self.op_type = op_type

    def forward(self, pred, y):
        s = voxel_metrics_batch(pred, y, threshold=self.threshold, pool_sizes=()).total()
        return _scalar(float(s.binary_match_f1(self.op_type)[0]), torch.float32, pred.device)


def f1score(pred, y):
    """metrics.py:65-90 on two binary (0 / 1) device tensors of any shape: TP, FP, FN counted exactly (f64 device
    sums), then the f32 formula."""
    for t, name in ((pred, "pred"), (y, "y")):
        if not t.is_cuda:
            raise hip.V2ceHipError(f"{name} must live on a HIP device (got {t.device}); there is no CPU path")
    p, g = pred.double(), y.double()
    tp, fp, fn = (float(v) for v in torch.stack([(p * g).sum(), (p * (1 - g)).sum(), ((1 - p) * g).sum()]).tolist())
    return _scalar(float(f1_from_counts(tp, fp, fn)), torch.float32, pred.device)


class PoolMSE(torch.nn.Module):
    """metrics.py:117-128: MSE of AvgPool3d(k, stride k) over ((l c), h, w) per (b, polarity); f32."""

    def __init__(self, kernel_size=2):
        super().__init__()
        self.kernel_size = int(kernel_size)

    def forward(self, pred, target):
        s = voxel_metrics_batch(pred, target, pool_sizes=(self.kernel_size,)).total()
        return _scalar(float(s.pool_mse(self.kernel_size)[0]), torch.float32, pred.device)


class MeanRatio(torch.nn.Module):
    """metrics.py MeanRatio: mean of max(r, 1 / r), r = (pred + 0.01) / (y + 0.01); f32."""

    def forward(self, pred, y):
        s = voxel_metrics_batch(pred, y, pool_sizes=()).total()
        return _scalar(float(s.mean_ratio()[0]), torch.float32, pred.device)


class L1(torch.nn.Module):
    """The value of nn.L1Loss() (train/main.py's 'L1'): mean |pred - y|; f32."""

    def forward(self, pred, y):
        s = voxel_metrics_batch(pred, y, pool_sizes=()).total()
        return _scalar(float(s.l1()[0]), torch.float32, pred.device)


# ---------------------------------------------------------------------------------------------------------------------
# the driver (esim_metric.py / v2e_metric.py per recording)

def run_stage1_metric(voxels: torch.Tensor, gt_events, gt_counts, frame_timestamps=None, *, seq_len: int = 16,
                      chunk: int = 64, threshold: float = 0.01, pool_sizes: Sequence[int] = (2, 4),
                      pred_events=None, pred_counts=None, height: Optional[int] = None, width: Optional[int] = None,
                      device=None, losses: Optional[Sequence[str]] = None, loss_options: Optional[dict] = None):
    """Score the voxels of P frame pairs against the recording.  ``voxels``: [P, 2, 10, H, W] f32 device tensor (the
    model's output), or None with ``pred_events`` (host structured array grouped by pair), ``pred_counts`` [P],
    ``height`` and ``width``: an event stream voxelised per pair like the GT.
    ``gt_events``: host structured array grouped by pair with ``gt_counts`` [P].  The GT of each pair is voxelised
    over its own time range (``gen_discretized_event_volume`` of its events), ``chunk`` pairs at a time.  Windows of
    ``seq_len`` consecutive pairs are scored as one [1, L, 20, H, W] sequence each (the last may be shorter).
    ``frame_timestamps`` is not needed for the score (each pair uses its events' own range) and only recorded.

    Returns ``(summary, records)``: summary[name] = unweighted mean over windows; records = per-window values, the
    pairs of each window, and the pairs whose GT (or predicted events) were empty or had a single timestamp (they
    score with a zero volume; the reference would raise).

    ``losses``: a tuple of loss names of ``losses.calculate_loss`` (``loss_options``: its keyword options).  Each
    window's ``loss`` and ``loss_dict`` then go into ``records["losses"]`` and their unweighted means over windows
    into ``records["summary_losses"]``.  A window too small for a requested term (the pyramid needs H, W >= 8) records
    None for it and for ``loss``."""
    from .voxelize import gen_discretized_event_volume_batch
    if losses is not None:
        from . import losses as VL
        losses = VL.check_loss_names(losses)
        loss_options = dict(loss_options or {})
    loss_records: List[dict] = []
    counts = np.asarray(gt_counts, dtype=np.int64).reshape(-1)
    P = counts.size
    if voxels is not None:
        if voxels.dim() != 5 or voxels.shape[1] != 2 or voxels.shape[2] != 10:
            raise ValueError(f"expected voxels [P,2,10,H,W], got {tuple(voxels.shape)}")
        if int(voxels.shape[0]) != P:
            raise ValueError(f"{int(voxels.shape[0])} voxel pairs for {P} GT counts")
        H, W = int(voxels.shape[3]), int(voxels.shape[4])
        device = voxels.device
    else:
        if pred_events is None or pred_counts is None:
            raise ValueError("give voxels, or pred_events with pred_counts")
        if height is None or width is None:
            raise ValueError("pred_events need height and width")
        H, W = int(height), int(width)
        device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        pred_counts = np.asarray(pred_counts, dtype=np.int64).reshape(-1)
        if pred_counts.size != P:
            raise ValueError(f"{pred_counts.size} predicted counts for {P} GT counts")
    if seq_len < 1:
        raise ValueError("seq_len must be >= 1")
    step = max(1, int(chunk) // seq_len) * seq_len                 # chunks hold whole windows
    goff = np.concatenate([[0], np.cumsum(counts)])
    poff = np.concatenate([[0], np.cumsum(pred_counts)]) if voxels is None else None
    per_window: List[Dict[str, float]] = []
    windows, degenerate = [], {"gt_empty": [], "gt_single_timestamp": [], "pred_empty": [], "pred_single_timestamp": []}
    for c0 in range(0, P, step):
        c1 = min(P, c0 + step)
        gvol, gst = gen_discretized_event_volume_batch(gt_events[goff[c0]:goff[c1]], counts[c0:c1], 10, H, W,
                                                      device=device)
        for i in np.flatnonzero(gst & hip.VOXELIZE_EMPTY):
            degenerate["gt_empty"].append(int(c0 + i))
        for i in np.flatnonzero(gst & hip.VOXELIZE_SINGLE_TIMESTAMP):
            degenerate["gt_single_timestamp"].append(int(c0 + i))
        if voxels is not None:
            pvol = voxels[c0:c1].reshape(c1 - c0, 20, H, W).contiguous()
        else:
            pvol, pst = gen_discretized_event_volume_batch(pred_events[poff[c0]:poff[c1]], pred_counts[c0:c1], 10, H, W,
                                                          device=device)
            for i in np.flatnonzero(pst & hip.VOXELIZE_EMPTY):
                degenerate["pred_empty"].append(int(c0 + i))
            for i in np.flatnonzero(pst & hip.VOXELIZE_SINGLE_TIMESTAMP):
                degenerate["pred_single_timestamp"].append(int(c0 + i))
        n = c1 - c0
        full = n // seq_len
        parts = []
        if full:
            parts.append((0, full, seq_len))
        if n - full * seq_len:
            parts.append((full * seq_len, 1, n - full * seq_len))
        for s0, nb, L in parts:
            sl = slice(s0, s0 + nb * L)
            st = voxel_metrics_batch(pvol[sl].reshape(nb, L, 20, H, W), gvol[sl].reshape(nb, L, 20, H, W),
                                     threshold=threshold, pool_sizes=pool_sizes)
            vals = st.values()
            for b in range(nb):
                per_window.append({k: float(v[b]) for k, v in vals.items()})
                windows.append([c0 + s0 + b * L, c0 + s0 + (b + 1) * L])
            if losses is not None:
                small = tuple(n for n in losses if n == "pyramid" and min(10 * L, H, W) < VL.PYRAMID_MIN)
                fit = tuple(n for n in losses if n not in small)
                ls = VL.voxel_losses_batch(pvol[sl].reshape(nb, L, 20, H, W), gvol[sl].reshape(nb, L, 20, H, W),
                                           terms=VL.terms_for(fit))
                for b in range(nb):
                    total, d = VL.loss_values([ls.select(b)], fit, **loss_options)
                    d = {k: float(v) for k, v in d.items()}
                    if small:
                        d["pyramid_loss"] = None
                    loss_records.append({"loss": None if small else float(total), "loss_dict": d})
        del gvol, pvol
    names = list(per_window[0].keys()) if per_window else []
    summary = {k: float(np.mean([w[k] for w in per_window])) for k in names}
    records = {"windows": windows, "values": per_window, "degenerate_pairs": degenerate, "seq_len": int(seq_len),
               "pairs": int(P)}
    if frame_timestamps is not None:
        records["frame_timestamps"] = [int(t) for t in np.asarray(frame_timestamps).reshape(-1)]
    if losses is not None:
        mean = lambda vs: float(np.mean([v for v in vs if v is not None])) if any(v is not None for v in vs) else None
        keys = list(loss_records[0]["loss_dict"]) if loss_records else []
        records["losses"] = loss_records
        records["summary_losses"] = {**{k: mean([r["loss_dict"][k] for r in loss_records]) for k in keys},
                                     "loss": mean([r["loss"] for r in loss_records])}
    return summary, records


def write_stage1_results(out_folder: str, summary: Dict[str, float], records) -> None:
    """stage1_result.csv (metric, mean over windows) and stage1_record.json (per-window values at full precision); with
    loss terms in the records also stage1_loss_result.csv (term, mean over windows)."""
    import csv
    import json
    import os
    import os.path as op
    os.makedirs(out_folder, exist_ok=True)
    with open(op.join(out_folder, "stage1_result.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["metric", "mean"])
        for k, v in summary.items():
            w.writerow([k, repr(float(v))])
    with open(op.join(out_folder, "stage1_record.json"), "w") as f:
        json.dump({"summary": summary, **records}, f, indent=1)
    if "summary_losses" in records:
        with open(op.join(out_folder, "stage1_loss_result.csv"), "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["term", "mean"])
            for k, v in records["summary_losses"].items():
                w.writerow([k, "" if v is None else repr(float(v))])
