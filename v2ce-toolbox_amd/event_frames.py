"""The event-frame video's numeric stage on the device (csrc/event_frames.hip): the frames of
``write_event_frame_video`` (v2ce.py:241-280) without the clip's sums ever reaching the host.

Per batch ``EventFrameRenderer.add`` runs one kernel: the three sequential f32 sums of ``pipeline.event_frame_sums`` and
an integer histogram of the leading eleven bits of their positive values.  ``finish`` reads that histogram, finds the bin
of each of the two ranks ``np.percentile`` interpolates between, refines twice by ten bits over the stored sums (positive
floats order like their bit patterns, so the two order statistics are exact), evaluates the percentile on the host in
numpy (``percentile_from_order_stats``) and renders uint8 frames on the device: float64 arithmetic with polarity kept,
float32 in grey, as numpy's dtype rules make the reference do.  There is no CPU path."""
from __future__ import annotations

import logging

import numpy as np
import torch

from . import hip

logger = logging.getLogger("V2CE")


def _virtual_index(n, q, dtype):
    """np.percentile's (method 'linear') virtual index for n values of ``dtype``: (v, previous rank, next rank)."""
    quant = np.asanyarray(np.true_divide(int(q), dtype(100)))    # python int / f32 scalar stays f32
    v = np.asanyarray((n - 1) * quant)
    prev = np.floor(v)
    nxt = prev + 1
    if v >= n - 1:
        prev = nxt = n - 1
    if v < 0:
        prev = nxt = 0
    return v, int(prev), int(nxt)


def percentile_ranks(n, q, dtype):
    """The two 0-based ranks np.percentile(arr, q) reads from the sorted ``arr`` (len n, dtype float32 / float64)."""
    return _virtual_index(n, q, dtype)[1:]


def percentile_from_order_stats(n, q, kth, dtype):
    """np.percentile(arr, q) (method 'linear') from n = len(arr) and two order statistics: kth(i) = the i-th smallest,
    0-based; dtype = arr.dtype (np.float32 or np.float64).  Bit for bit, result dtype included, also beyond 2^24
    values of float32, where the float32 virtual index is coarse."""
    v, prev, nxt = _virtual_index(n, q, dtype)
    gamma = np.asanyarray(v - np.floor(v), dtype=v.dtype)
    a = dtype(kth(prev))
    b = dtype(kth(nxt))
    d = np.subtract(b, a)
    r = np.asanyarray(np.add(a, d * gamma))
    if gamma >= 0.5:
        r = np.asanyarray(np.subtract(b, d * (1 - gamma)), dtype=r.dtype)
    return r[()]


def _bin_of_rank(hist, rank):
    """hist: int64 counts in value order -> (the bin that holds 0-based ``rank``, the rank inside that bin)."""
    c = np.cumsum(hist)
    b = int(np.searchsorted(c, rank, side="right"))
    return b, int(rank - (c[b - 1] if b else 0))


class EventFrameRenderer:
    """``add(first_pair, vox)`` per batch in any order, ``finish() -> (frames uint8 [L,H,W,3] RGB on the host, upper)``:
    the frames and the upper bound of ``v2ce.event_frame_images(event_frame_sums(clip), ceil, percentile,
    keep_polarity)``, byte for byte.  ``reset()`` starts the clip again."""

    def __init__(self, keep_polarity=True, ceil=10, upper_bound_percentile=98, height=260, width=346, device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise hip.V2ceHipError(f"EventFrameRenderer needs a HIP device (got {self.device}); there is no CPU path")
        self.keep_polarity = bool(keep_polarity)
        self.mode = hip.EVENT_FRAMES_POLARITY if self.keep_polarity else hip.EVENT_FRAMES_GREY
        self.ceil, self.q = ceil, upper_bound_percentile
        self.H = None if height is None else int(height)          # None: taken from the first batch (pano keeps the
        self.W = None if width is None else int(width)            # frame's own width, pipeline.resized_width)
        self.dtype = np.float64 if self.keep_polarity else np.float32
        self.mult = 1 if self.keep_polarity else 3                # grey: every value counts three times
        self._hist0 = None
        self._sums = []                                            # (first pair, [P,3,H,W] f32 on the device)
        self.last = {}                                             # n, ranks and order statistics of the last finish()

    def reset(self):
        self._sums = []
        if self._hist0 is not None:
            self._hist0.zero_()

    def add(self, first_pair, vox):
        """vox [P,2,10,H,W] f32 on the device; returns its sums [P,3,H,W] (kept until finish / reset)."""
        vox = hip.require_device_f32(vox, "vox")
        if vox.dim() == 5 and not self._sums:
            self.H = int(vox.shape[3]) if self.H is None else self.H
            self.W = int(vox.shape[4]) if self.W is None else self.W
        if vox.dim() != 5 or tuple(vox.shape[1:]) != (2, 10, self.H, self.W):
            raise ValueError(f"vox must be [P,2,10,{self.H},{self.W}], got {tuple(vox.shape)}")
        P = int(vox.shape[0])
        sums = torch.empty((P, 3, self.H, self.W), dtype=torch.float32, device=vox.device)
        if P == 0:
            return sums
        L = hip.lib()
        with torch.cuda.device(vox.device):
            if self._hist0 is None:
                self._hist0 = torch.zeros(L.v2ce_event_frames_hist_bytes(0) // 8, dtype=torch.int64, device=vox.device)
            hip.check(L.v2ce_event_frames_sums(vox.data_ptr(), P, self.H, self.W, self.mode, sums.data_ptr(),
                                               self._hist0.data_ptr(), hip.stream_ptr(vox.device)), "v2ce_event_frames_sums")
        self._sums.append((int(first_pair), sums))
        return sums

    def level0_histogram(self) -> np.ndarray:
        """int64 [2048]: the positive values of the mode's channels seen so far, by bits 30..20."""
        if self._hist0 is None:
            return np.zeros(hip.EVENT_FRAMES_LEVEL0_BINS, np.int64)
        return self._hist0.cpu().numpy()

    def refine_histogram(self, level, prefix_a, prefix_b) -> np.ndarray:
        """int64 [2, 1024] over the stored sums (v2ce_event_frames_refine); one host synchronisation."""
        L = hip.lib()
        dev = self._sums[0][1].device
        with torch.cuda.device(dev):
            h = torch.zeros((2, hip.EVENT_FRAMES_REFINE_BINS), dtype=torch.int64, device=dev)
            for _, s in self._sums:
                hip.check(L.v2ce_event_frames_refine(s.data_ptr(), int(s.shape[0]), self.H, self.W, self.mode, level,
                                                     prefix_a, prefix_b, h.data_ptr(), hip.stream_ptr(dev)),
                          "v2ce_event_frames_refine")
            return h.cpu().numpy()

    def order_statistics(self, rank_a, rank_b):
        """The values at two 0-based ranks of the positive values of the mode's channels (each counted once)."""
        ranks = (int(rank_a), int(rank_b))
        h0 = self.level0_histogram()
        prefix, inside = zip(*(_bin_of_rank(h0, r) for r in ranks))
        for level in (1, 2):
            h = self.refine_histogram(level, prefix[0], prefix[1])
            step = [_bin_of_rank(h[i], inside[i]) for i in range(2)]
            prefix = tuple((prefix[i] << 10) | step[i][0] for i in range(2))
            inside = tuple(s[1] for s in step)
        return tuple(np.array([p], np.uint32).view(np.float32)[0] for p in prefix)

    def upper_bound(self):
        """min(np.percentile(positive values, q), ceil) as the host computes it (v2ce.py:262-264)."""
        count = int(self.level0_histogram().sum()) if self._sums else 0
        n = count * self.mult
        if n == 0:
            np.percentile(np.empty(0, self.dtype), self.q)         # the host path's own error for an empty selection
            raise IndexError("no positive event-frame value in the clip")
        prev, nxt = percentile_ranks(n, self.q, self.dtype)
        a, b = self.order_statistics(prev // self.mult, nxt // self.mult)
        kth = {prev: a, nxt: b}
        pct = percentile_from_order_stats(n, self.q, kth.__getitem__, self.dtype)
        self.last = {"n": n, "ranks": (prev, nxt), "order_stats": (a, b), "percentile": pct}
        return min(pct, self.ceil)

    def finish(self):
        upper = self.upper_bound()
        logger.info(f"Upper bound of the event frame value during video writing: {upper}")
        batches = sorted(self._sums, key=lambda kv: kv[0])
        total, at = sum(int(s.shape[0]) for _, s in batches), 0
        for fp, s in batches:
            if fp != at:
                raise ValueError(f"the batches do not tile the clip: pair {at} is missing or doubled (next batch starts at {fp})")
            at += int(s.shape[0])
        L = hip.lib()
        dev = batches[0][1].device
        with torch.cuda.device(dev):
            frames = torch.empty((total, self.H, self.W, 3), dtype=torch.uint8, device=dev)
            for fp, s in batches:
                hip.check(L.v2ce_event_frames_render(s.data_ptr(), int(s.shape[0]), self.H, self.W, self.mode, float(upper),
                                                     fp, total, frames.data_ptr(), hip.stream_ptr(dev)),
                          "v2ce_event_frames_render")
            host = torch.empty(frames.shape, dtype=torch.uint8, pin_memory=True)
            host.copy_(frames, non_blocking=True)
            torch.cuda.current_stream(dev).synchronize()
        self.reset()
        return host.numpy(), upper
