"""The score of the reference's stage-2 study -- host side mirroring
``/root/reference/train/scripts/stage2/stage2_metrics.py``:

* ``ts_diff_metric(event_gt, event_pred, search_range, fps)``   stage2_metrics.py:22-88, same signature and return
  value (``np.array([avg error, overflow])``)
* ``ts_diff_metric_batch(...)``  the same for many frame pairs in one call, on the device (``csrc/tsdiff.hip``
  through ``v2ce_tsdiff``); no CPU path exists
* ``run_metric(voxels, gt_events, ...)``   the per-file driver run_metric_for_data (:91-201)
* ``main()``   the command line (``v2ce_eval.py``)

The score of one pair: every ground-truth (GT) event takes d = min(1e6, min |t_pred - t_gt|) over the predicted
events of its polarity in the (2r+1)^2 cells around it, capped at cap = 1e6 / fps / 10 * 3 (an "overflow").  The
kernel returns the exact int64 sum S of the uncapped d and the capped count K; the average is

    avg = ((double)S + (double)K * cap) / N_gt

The reference adds the d one by one (int64 until the first capped event, float64 after), so its last bits may differ
from this sum by the rounding of those adds (at most N_gt * 2^-52 relative).  Deliberate differences
(INTEGRATION.md): H and W are parameters (260 x 346 by default); out-of-range x or y and GT polarity outside
{-1, 0, 1} are refused; the caller's GT polarity is never overwritten; a pair without GT events scores NaN in the
batched API (the drop-in raises ZeroDivisionError like the reference).
"""
from __future__ import annotations

import argparse
import csv
import json
import logging
import os
import os.path as op
from dataclasses import dataclass
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import hip
from .LDATI import EVENT_DTYPE, DeviceEvents, ldati_device

logger = logging.getLogger("V2CE")

HEIGHT, WIDTH = 260, 346                  # stage2_metrics.py:44-47
METHODS = ("ours", "random", "even", "slope")
_STATUS_MESSAGES = {1: "pair offsets are not monotone or leave the event arrays", 2: "fps is not finite and positive",
                    4: "a GT event lies outside the sensor", 8: "a GT polarity is outside {-1, 0, 1}",
                    16: "a predicted event lies outside the sensor", 32: "internal cell list overflow"}


def overflow_cap(fps) -> float:
    """stage2_metrics.py:80: ``1e6/fps/10*3``, f64 left to right."""
    return 1e6 / fps / 10 * 3


@dataclass
class TsDiffResult:
    """Per-pair scores of ``ts_diff_metric_batch``: ``avg`` f64 (NaN for a pair without GT events), ``overflow``,
    ``n_gt``, ``n_pred``, ``S`` (exact int64 sum of the uncapped d), ``cap`` f64; ``per_event_d``: f64 [n_gt]
    device tensor in the order of the GT input, or None."""
    avg: np.ndarray
    overflow: np.ndarray
    n_gt: np.ndarray
    n_pred: np.ndarray
    S: np.ndarray
    cap: np.ndarray
    per_event_d: Optional[torch.Tensor] = None


def _soa(events, device, name):
    """Events as (ts int64, x int16, y int16, p int8) device tensors.  Accepted: a host structured array with the
    fields of EVENT_DTYPE, ``DeviceEvents``, a (ts, x, y, p) tuple of device tensors, or packed 13-byte records
    (uint8 device tensor).  Tensors on the CPU are refused: there is no CPU path."""
    if isinstance(events, DeviceEvents):
        return tuple(events._unpacked())
    if isinstance(events, np.ndarray):
        if events.dtype.names is None or not {"timestamp", "x", "y", "polarity"} <= set(events.dtype.names):
            raise ValueError(f"{name}: a structured array needs the fields timestamp, x, y, polarity")
        cols = [np.array(events[f], dtype=dt) for f, dt in             # fresh, packed copies of the fields
                (("timestamp", np.int64), ("x", np.int16), ("y", np.int16), ("polarity", np.int8))]
        return tuple(torch.from_numpy(c).to(device) for c in cols)
    if isinstance(events, (tuple, list)) and len(events) == 4:
        out = []
        for t, dt in zip(events, (torch.int64, torch.int16, torch.int16, torch.int8)):
            t = torch.as_tensor(t)
            if not t.is_cuda:
                raise hip.V2ceHipError(f"{name} must live on a HIP device (got {t.device}); there is no CPU path")
            out.append(t.to(dt).contiguous())
        return tuple(out)
    if isinstance(events, torch.Tensor) and events.dtype == torch.uint8:
        if not events.is_cuda:
            raise hip.V2ceHipError(f"{name} must live on a HIP device (got {events.device}); there is no CPU path")
        if events.numel() % EVENT_DTYPE.itemsize:
            raise ValueError(f"{name}: packed records are {EVENT_DTYPE.itemsize} bytes each")
        n = events.numel() // EVENT_DTYPE.itemsize
        return tuple(DeviceEvents(events.contiguous(), np.array([[n]]), 0)._unpacked())
    raise TypeError(f"{name}: unsupported event container {type(events).__name__}")


def _offsets(counts, n, pairs, name):
    c = np.asarray(counts, dtype=np.int64).reshape(-1)
    if c.size != pairs:
        raise ValueError(f"{name}: {c.size} counts for {pairs} pairs")
    if (c < 0).any():
        raise ValueError(f"{name}: negative count (pair offsets would not be monotone)")
    off = np.zeros(pairs + 1, dtype=np.int64)
    np.cumsum(c, out=off[1:])
    if off[-1] != n:
        raise ValueError(f"{name}: counts add up to {off[-1]}, the events are {n}")
    return off


def ts_diff_metric_batch(gt, gt_counts, pred, pred_counts, fps, search_range: int = 0, *, height: int = HEIGHT,
                         width: int = WIDTH, per_event: bool = False, device=None) -> TsDiffResult:
    """ts_diff_metric of many frame pairs in one device call.  Pair i owns the next ``gt_counts[i]`` GT events and
    ``pred_counts[i]`` predicted events (``None``: the segment counts of a ``DeviceEvents``); ``fps`` is a scalar or
    one value per pair.  One host synchronisation (the per-pair sums)."""
    if int(search_range) < 0:
        raise ValueError(f"search_range must be >= 0, got {search_range}")
    dev = torch.device(device) if device is not None else None
    for e in (gt, pred):
        if dev is None and isinstance(e, DeviceEvents):
            dev = e.device
        elif dev is None and isinstance(e, torch.Tensor):
            dev = e.device
        elif dev is None and isinstance(e, (tuple, list)) and len(e) == 4 and isinstance(e[0], torch.Tensor):
            dev = e[0].device
    if dev is None:
        dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cuda")
    if pred_counts is None and isinstance(pred, DeviceEvents):
        pred_counts = pred.frame_counts
    if gt_counts is None and isinstance(gt, DeviceEvents):
        gt_counts = gt.frame_counts
    g = _soa(gt, dev, "gt")
    p = _soa(pred, dev, "pred")
    dev = g[0].device
    n_gt, n_pred = int(g[0].numel()), int(p[0].numel())
    pairs = int(np.asarray(gt_counts).size)
    if pairs == 0:
        raise ValueError("no pairs")
    goff, poff = _offsets(gt_counts, n_gt, pairs, "gt_counts"), _offsets(pred_counts, n_pred, pairs, "pred_counts")
    fps_h = np.broadcast_to(np.asarray(fps, dtype=np.float64), (pairs,)).copy()
    if not (np.isfinite(fps_h).all() and (fps_h > 0).all()):
        raise ValueError("fps must be finite and positive")
    if n_gt >= 2 ** 31 or n_pred >= 2 ** 31:
        raise hip.V2ceHipError(f"{n_gt} GT / {n_pred} predicted events in one call: split the pairs")
    L = hip.lib()
    with torch.cuda.device(dev):
        st = hip.stream_ptr(dev)
        ws_bytes = L.v2ce_tsdiff_workspace_bytes(pairs, int(height), int(width), n_pred)
        if ws_bytes == 0:
            raise hip.V2ceHipError(f"v2ce_tsdiff: unsupported shape pairs={pairs}, H={height}, W={width}")
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        offs = torch.from_numpy(np.concatenate([goff, poff])).to(dev)
        fps_d = torch.from_numpy(fps_h).to(dev)
        out = torch.zeros(3 * pairs + 1, dtype=torch.int64, device=dev)       # pair_stats | status
        d = torch.empty(n_gt if per_event else 0, dtype=torch.float64, device=dev)
        hip.check(L.v2ce_tsdiff(*(t.data_ptr() for t in g), offs.data_ptr(), n_gt, *(t.data_ptr() for t in p),
                                offs[pairs + 1:].data_ptr(), n_pred, fps_d.data_ptr(), pairs, int(height), int(width),
                                int(search_range), d.data_ptr() if per_event and n_gt else None, out.data_ptr(),
                                out[3 * pairs:].data_ptr(), ws.data_ptr(), ws_bytes, st), "v2ce_tsdiff")
        host = out.cpu().numpy()                                              # the one synchronisation
    status = int(host[3 * pairs:].view(np.int32)[0])
    if status:
        why = "; ".join(m for b, m in _STATUS_MESSAGES.items() if status & b)
        raise hip.V2ceHipError(f"v2ce_tsdiff refused its input (status {status}): {why}")
    stats = host[:3 * pairs].reshape(pairs, 3)
    S, K, N = stats[:, 0].copy(), stats[:, 1].copy(), stats[:, 2].copy()
    cap = overflow_cap(fps_h)
    with np.errstate(invalid="ignore", divide="ignore"):
        avg = (S.astype(np.float64) + K.astype(np.float64) * cap) / N.astype(np.float64)
    return TsDiffResult(avg=avg, overflow=K, n_gt=N, n_pred=np.diff(poff), S=S, cap=cap,
                        per_event_d=d if per_event else None)


def ts_diff_metric(event_gt, event_pred, search_range=0, fps=30, *, height: int = HEIGHT, width: int = WIDTH):
    """Drop-in for stage2_metrics.py:22: ``np.array([avg error, overflow])`` (float64) of one frame pair.
    The caller's ``event_gt`` is not modified (the reference sets its polarity -1 to 0 in place)."""
    n_gt = len(event_gt) if not isinstance(event_gt, (tuple, list)) else int(torch.as_tensor(event_gt[0]).numel())
    if n_gt == 0:
        raise ZeroDivisionError("division by zero (no GT events; stage2_metrics.py:87 divides by their count)")
    n_pred = len(event_pred) if not isinstance(event_pred, (tuple, list)) else int(torch.as_tensor(event_pred[0]).numel())
    if isinstance(event_pred, torch.Tensor) and event_pred.dtype == torch.uint8:
        n_pred = event_pred.numel() // EVENT_DTYPE.itemsize
    if isinstance(event_pred, DeviceEvents):
        n_pred = event_pred.num_events
    if isinstance(event_gt, DeviceEvents):
        n_gt = event_gt.num_events
    r = ts_diff_metric_batch(event_gt, [n_gt], event_pred, [n_pred], fps, search_range, height=height, width=width)
    return np.array([r.avg[0], float(r.overflow[0])])


# ---------------------------------------------------------------------------------------------------------------------
# the driver (run_metric_for_data, stage2_metrics.py:91-201)

def pair_fps(frame_timestamps) -> np.ndarray:
    """stage2_metrics.py:128,131: ``30 / (T[i+1] - T[i]) * 33333`` (f64)."""
    T = np.asarray(frame_timestamps, dtype=np.int64)
    return 30 / np.diff(T).astype(np.float64) * 33333


def sample_pair(vox1: torch.Tensor, method: str, fps: float, pair: int, *, seed: int,
                additional_events_strategy: str = "slope", bidirectional: bool = False,
                pooling_type: str = "none") -> DeviceEvents:
    """The predicted events of one pair ([1,2,10,H,W] voxels, t0 = 0) by one of the study's samplers; the Philox
    draws are keyed by ``seed`` and ``frame_base = pair``, so they do not depend on how pairs are batched."""
    from .sample_methods import sampler_device
    if method == "ours":        # stage2_metrics.py:137: LDATI, -a / -b, pooling 'none'
        return ldati_device(vox1, t0=0, fps=fps, seed=seed, frame_base=pair, strategy=additional_events_strategy,
                            bidirectional=bidirectional)
    if method == "random":      # :151
        return sampler_device(vox1, hip.SAMPLER_RANDOM, 0, fps, seed=seed, frame_base=pair)
    if method == "even":        # :164
        return sampler_device(vox1, hip.SAMPLER_EVEN, 0, fps, seed=seed, frame_base=pair)
    if method == "slope":       # :177, -p
        return sampler_device(vox1, hip.SAMPLER_PURE_SLOPE, 0, fps, seed=seed, frame_base=pair, pooling_type=pooling_type)
    raise ValueError(f"unknown method {method!r} (one of {METHODS})")


def run_metric(voxels: torch.Tensor, gt_events: np.ndarray, gt_counts, frame_timestamps,
               evaluate_on: Sequence[str] = ("ours", "random", "slope"), *, search_range: int = 0,
               additional_events_strategy: str = "slope", bidirectional: bool = False, pooling_type: str = "none",
               seed: int = 42, chunk: int = 64):
    """run_metric_for_data without its file handling: ``voxels`` [P,2,10,H,W] (device), ``gt_events`` the GT events
    (host structured array, absolute timestamps in us) grouped by pair with ``gt_counts`` [P], ``frame_timestamps``
    [P+1] int64 us.  Pair i is scored with fps_i = 30 / (T[i+1] - T[i]) * 33333 and GT timestamps relative to T[i].
    Returns ``(summary, records)``: summary[m] = mean over pairs of [avg error, overflow, len(pred) / len(gt)];
    records[m] = per-pair dict of lists."""
    if voxels.dim() != 5 or voxels.shape[1] != 2 or voxels.shape[2] != 10:
        raise ValueError(f"expected voxels [P,2,10,H,W], got {tuple(voxels.shape)}")
    P, H, W = int(voxels.shape[0]), int(voxels.shape[3]), int(voxels.shape[4])
    T = np.asarray(frame_timestamps, dtype=np.int64)
    if T.size != P + 1:
        raise ValueError(f"{P} pairs need {P + 1} frame timestamps, got {T.size}")
    counts = np.asarray(gt_counts, dtype=np.int64)
    fps = pair_fps(T)
    gt = np.array(gt_events, copy=True)
    gt["timestamp"] = gt["timestamp"] - np.repeat(T[:-1], counts)           # :129
    summary, records = {}, {}
    for m in evaluate_on:
        if m not in METHODS:
            raise ValueError(f"unknown method {m!r} (one of {METHODS})")
        avg, ovf, ngt, npred = [], [], [], []
        for c0 in range(0, P, chunk):
            c1 = min(P, c0 + chunk)
            evs = [sample_pair(voxels[i:i + 1], m, float(fps[i]), i, seed=seed,
                               additional_events_strategy=additional_events_strategy, bidirectional=bidirectional,
                               pooling_type=pooling_type) for i in range(c0, c1)]
            for e in evs:
                e.check()
            soa = tuple(torch.cat([e._unpacked()[k] for e in evs]) for k in range(4))
            lo, hi = int(counts[:c0].sum()), int(counts[:c1].sum())
            r = ts_diff_metric_batch(gt[lo:hi], counts[c0:c1], soa, [e.num_events for e in evs], fps[c0:c1],
                                     search_range, height=H, width=W, device=voxels.device)
            avg.append(r.avg); ovf.append(r.overflow); ngt.append(r.n_gt); npred.append(r.n_pred)
        avg, ovf, ngt, npred = (np.concatenate(a) for a in (avg, ovf, ngt, npred))
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = npred / ngt
        summary[m] = np.stack([avg, ovf.astype(np.float64), ratio], axis=1).mean(axis=0)
        records[m] = {"avg": avg.tolist(), "overflow": ovf.tolist(), "n_gt": ngt.tolist(), "n_pred": npred.tolist(),
                      "fps": fps.tolist()}
    return summary, records


# ---------------------------------------------------------------------------------------------------------------------
# command line (v2ce_eval.py)

def build_parser():
    p = argparse.ArgumentParser(description="Score generated events against a DVS recording (stage2_metrics.py)")
    # frame source and model: the flags of v2ce.py
    p.add_argument("-f", "--image_folder", type=str, help="The folder containing the images to infer")
    p.add_argument("--npy_frames", type=str, help="uint8 [N,H,W] grayscale frames in a .npy file")
    p.add_argument("--synthetic", type=int, default=0, help="generate N synthetic frames instead of reading")
    p.add_argument("--synthetic_weights", type=int, default=None, help="seed of synthetic weights")
    p.add_argument("-m", "--model_path", type=str, default="./weights/v2ce_3d.pt")
    p.add_argument("-b", "--batch_size", type=int, default=1, help="Batch size for inference")
    p.add_argument("--precision", type=str, default="f16x2", choices=["f16x2", "f32"])
    p.add_argument("--seq_len", type=int, default=16)
    p.add_argument("--width", type=int, default=WIDTH)
    p.add_argument("--height", type=int, default=HEIGHT)
    p.add_argument("--max_frame_num", type=int, default=1800)
    p.add_argument("--device", type=str, default="cuda")
    # the recording
    p.add_argument("--gt_events", type=str, required=True,
                   help="GT events: .npz with key event_stream, or a structured .npy (timestamp, x, y, polarity)")
    p.add_argument("--frame_timestamps", type=str, help="int64 us frame times [N] (.npy)")
    p.add_argument("--fps", type=float, default=30, help="without --frame_timestamps: T_i = int(i * 1 / fps * 1e6)")
    # the flags of stage2_metrics.py:209-222 that apply ('-b' is v2ce.py's batch size here)
    p.add_argument("--search_range", type=int, default=0, help="search range for each GT event")
    p.add_argument("--evaluate_on", default=["ours", "random", "slope"], nargs="*", choices=list(METHODS))
    p.add_argument("-a", "--additional_events_strategy", default="slope", choices=["random", "slope", "none"])
    p.add_argument("-p", "--pooling_type", default="none", choices=["none", "weighted", "avg"])
    p.add_argument("--bidirectional", action="store_true", help="bidirectional y_relocate in LDATI")
    p.add_argument("--seed", type=int, default=42, help="Philox seed of the samplers")
    # the stage-1 score (stage1_metrics.py): opt-in
    p.add_argument("--stage1", action="store_true",
                   help="also score voxel grids (BinaryMatch[F1], PoolMSE, L1, MeanRatio) against the GT voxelised per "
                        "pair: writes stage1_result.csv and stage1_record.json")
    p.add_argument("--pred_events", type=str, default=None,
                   help="with --stage1: score this event stream (.npz event_stream or structured .npy), voxelised per "
                        "pair like the GT, instead of the model's voxels; needs --frame_timestamps, skips stage 2")
    # the stage-1 loss terms (losses.py): opt-in; the defaults of the reference's train/main.py without 'gan'
    p.add_argument("--stage1_losses", default=None, nargs="*", metavar="NAME",
                   help="with --stage1: also the reference's voxel loss terms per window (no names: pyramid ef ef_splitp "
                        "compensation; also pt match norml1 norml2): writes stage1_loss_result.csv and adds \"losses\" "
                        "to stage1_record.json")
    p.add_argument("--ef_type", default="c+cl", choices=("only_c", "cl", "c+cl"))
    p.add_argument("--add_base_loss", action="store_true", help="add the plain MSE to the pyramid loss")
    p.add_argument("--alpha_pyramid", type=float, default=1000)
    p.add_argument("--alpha_ef", type=float, default=0.5)
    p.add_argument("--alpha_efc", type=float, default=5)
    p.add_argument("--alpha_match", type=float, default=0.5)
    p.add_argument("--alpha_compensation", type=float, default=1)
    p.add_argument("--alpha_pt", type=float, default=1)
    p.add_argument("--alpha_norm", type=float, default=1e-5)
    p.add_argument("-o", "--out_folder", type=str, default="./results")
    p.add_argument("-l", "--log_level", type=str, default="info")
    return p


def load_events(path: str) -> np.ndarray:
    ev = np.load(path, allow_pickle=False)
    if isinstance(ev, np.lib.npyio.NpzFile):
        ev = ev["event_stream"]
    if ev.dtype.names is None or not {"timestamp", "x", "y", "polarity"} <= set(ev.dtype.names):
        raise ValueError(f"{path}: expected structured events with fields timestamp, x, y, polarity")
    return ev


def split_by_frames(events: np.ndarray, T: np.ndarray):
    """GT events in [T_i, T_{i+1}) belong to pair i (stable order inside a pair); returns (events, counts, dropped)."""
    P = T.size - 1
    idx = np.searchsorted(T, events["timestamp"], side="right") - 1
    keep = (idx >= 0) & (idx < P)
    order = np.argsort(idx[keep], kind="stable")
    kept = events[keep][order]
    counts = np.bincount(idx[keep], minlength=P).astype(np.int64)
    return kept, counts, int((~keep).sum())


def write_results(out_folder: str, summary: Dict[str, np.ndarray], records) -> None:
    """abbr_result.csv in the reference's layout (stage2_metrics.py:256-266: methods as rows, 3 digits, overflow as
    int) and full_record.json (per-pair values at full precision)."""
    os.makedirs(out_folder, exist_ok=True)
    with open(op.join(out_folder, "abbr_result.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["", "Avg Error", "#Overflow", "Pred GT Event # Ratio"])
        for m, v in summary.items():
            w.writerow([m, repr(round(float(v[0]), 3)), int(round(float(v[1]), 3)), repr(round(float(v[2]), 3))])
    with open(op.join(out_folder, "full_record.json"), "w") as f:
        json.dump({"summary": {m: [float(x) for x in v] for m, v in summary.items()}, "pairs": records}, f, indent=1)


def main(argv=None):
    args = build_parser().parse_args(argv)
    logging.basicConfig(level=getattr(logging, args.log_level.upper()))
    if args.pred_events is not None:
        return _main_pred_events(args)
    from . import glue, synth
    from .v2ce import get_trained_mode, read_image_folder
    from .v2ce_3d import V2ce3d
    if str(args.device).startswith("cuda") and torch.device(args.device).index is not None:
        torch.cuda.set_device(torch.device(args.device))
    sources = [args.image_folder, args.npy_frames, args.synthetic or None]
    assert sum(s is not None for s in sources) == 1, "specify exactly one frame source"
    if args.image_folder is not None:
        frames = read_image_folder(args.image_folder, args.max_frame_num)
    elif args.npy_frames is not None:
        frames = np.load(args.npy_frames)[:args.max_frame_num]
    else:
        frames = synth.synthetic_frames(args.synthetic, args.height, args.width)
    if args.synthetic_weights is not None:
        model = V2ce3d(precision=args.precision)
        model.load_state_dict(synth.make_state_dict(args.synthetic_weights))
        model = model.eval().to(args.device)
    else:
        model = get_trained_mode(args.model_path, args.device, args.precision)
    voxels = glue.video_to_voxels(model, frames, seq_len=args.seq_len, width=args.width, height=args.height,
                                  batch_size=args.batch_size, device=args.device)
    n = int(voxels.shape[0]) + 1
    if args.frame_timestamps is not None:
        T = np.load(args.frame_timestamps).astype(np.int64).reshape(-1)
        if T.size < n:
            raise ValueError(f"{args.frame_timestamps}: {T.size} frame times for {n} frames")
        T = T[:n]
    else:
        T = np.array([glue.frame_offset_us(i, args.fps) for i in range(n)], dtype=np.int64)
    gt, counts, dropped = split_by_frames(load_events(args.gt_events), T)
    logger.info(f"{len(gt)} GT events in {n - 1} pairs; {dropped} outside [T_0, T_{n - 1}) dropped")
    summary, records = run_metric(voxels, gt, counts, T, args.evaluate_on, search_range=args.search_range,
                                  additional_events_strategy=args.additional_events_strategy,
                                  bidirectional=args.bidirectional, pooling_type=args.pooling_type, seed=args.seed)
    write_results(args.out_folder, summary, records)
    for m, v in summary.items():
        logger.info(f"{m}: avg error {v[0]:.3f}, overflow {v[1]:.3f}, pred/gt {v[2]:.3f}")
    print(op.join(args.out_folder, "abbr_result.csv"))
    if args.stage1:
        from .stage1_metrics import run_stage1_metric
        s1, r1 = run_stage1_metric(voxels, gt, counts, T, seq_len=args.seq_len, **_stage1_loss_args(args))
        _report_stage1(args.out_folder, s1, r1)


def _stage1_loss_args(args) -> dict:
    """--stage1_losses and its options as keywords of run_stage1_metric; nothing without the flag."""
    if args.stage1_losses is None:
        return {}
    if not args.stage1:
        raise SystemExit("--stage1_losses belongs to the stage-1 score: give --stage1")
    names = tuple(args.stage1_losses) or ("pyramid", "ef", "ef_splitp", "compensation")
    opts = {k: getattr(args, k) for k in ("ef_type", "add_base_loss", "alpha_pyramid", "alpha_ef", "alpha_efc",
                                          "alpha_match", "alpha_compensation", "alpha_pt", "alpha_norm")}
    return {"losses": names, "loss_options": opts}


def _report_stage1(out_folder, summary, records):
    from .stage1_metrics import write_stage1_results
    write_stage1_results(out_folder, summary, records)
    for k, v in summary.items():
        print(f"{k:22s} {v:.6f}")
    print(op.join(out_folder, "stage1_result.csv"))
    if "summary_losses" in records:
        for k, v in records["summary_losses"].items():
            print(f"{k:22s} {v}")
        print(op.join(out_folder, "stage1_loss_result.csv"))


def _main_pred_events(args):
    """--stage1 --pred_events: an event stream against the recording, both voxelised per pair (no model, no stage 2)."""
    from .stage1_metrics import run_stage1_metric
    if not args.stage1:
        raise SystemExit("--pred_events scores stage 1 only: give --stage1")
    if args.frame_timestamps is None:
        raise SystemExit("--pred_events needs --frame_timestamps")
    T = np.load(args.frame_timestamps).astype(np.int64).reshape(-1)
    gt, counts, dropped = split_by_frames(load_events(args.gt_events), T)
    pred, pcounts, pdropped = split_by_frames(load_events(args.pred_events), T)
    logger.info(f"{len(gt)} GT / {len(pred)} predicted events in {T.size - 1} pairs; {dropped} / {pdropped} dropped")
    dev = torch.device(args.device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    s1, r1 = run_stage1_metric(None, gt, counts, T, seq_len=args.seq_len, pred_events=pred, pred_counts=pcounts,
                               height=args.height, width=args.width, device=dev, **_stage1_loss_args(args))
    _report_stage1(args.out_folder, s1, r1)


if __name__ == "__main__":
    main()
