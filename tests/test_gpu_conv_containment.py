"""Every conv entry of include/v2ce_hip.h stays inside its buffers and inside the logical width of its pitched rows.

One ROWS entry per C-ABI entry and kernel family, called through hip.lib() with raw pointers and a hand-built hip.ConvDesc
(V2ce3d._conv chooses neither pitches nor entries here).  Everything a call receives -- activations, index maps, weight
tables (written by the library's own pack entries, which tests/test_gpu_weight_prep.py covers), scale / shift / bias, the
residual, y, sc_y, pred_y and the range slots -- sits in a guarded, poisoned allocation (tests/guarded.py) of exactly the
byte size the header documents.  The padding columns of every pitched input row hold the run's poison; as f32 the two
poisons are about -2.9e-16 and 1.5e16, so a padding or guard value that enters any sum changes the result of the second run.

Every row runs under three PITCH SETS: "dense" (every pitch 0: the last row ends at the buffer's last byte), "production"
(V2ce3d._pitch(width) each) and "odd" (pairwise different pitches: Wout_pitch = Wout + 1, so column Wout is the first padding
column; the others width + 3, + 5, ...), and each pitch set three times: poisoned with POISON[0], with POISON[1], and with
POISON[0] and every buffer starting at the smallest offset past a 256-byte boundary that the header's alignment rule allows
(16 bytes for channels-last-16 tensors and weight tables, 4 bytes for everything else).  The range slots use
absmax_batch_stride = 3: [3b] and [3b + 1] zeroed by the caller, [3b + 2] poison.  verify() checks per row:

* containment: every guard byte of every buffer -- inputs, weights and maps included -- still holds its poison;
* inputs: every input holds its original bytes (padding poison included) after the call;
* written extent: the bytes equal in the two poisoned runs (guarded.written) are exactly the logical elements -- [..., :W] of
  every row, all 16 lanes of a channels-last-16 group -- of y, sc_y and pred_y; every padding column and every [3b + 2] float
  still holds its poison, in the misaligned run too;
* never read: the logical outputs of the three runs are bit-identical, and bit-identical across the three pitch sets;
* values: the logical outputs against an f64 evaluation (torch conv3d in double, once per row) at 1e-5 abs + 1e-5 rel;
* slots: [3b] equals max |y_b| over the logical elements bit for bit (0 with y == NULL); [3b + 1] is finite and > 0 for
  split-half launches and 0 for exact-f32 launches.

Shapes are the smallest at which the family still has ragged tiles on every axis: B = 2, T = 3 (odd: the last Winograd pair
is half empty; one row has T = 1), H = 9, a stride-1 width of 70 (production pitch 96), decoder rows 9 x 69 over a 5 x 35
source (odd sizes: the correction lists run), Cout of two channel tiles with the last one partial where the family's Cout
rule allows it (the Winograd-T kernel needs multiples of 64, the fused head and shortcut forms have 32 channels).  No output
exceeds 4 MB (a guarded allocation is 17x its size).  Out of scope, because the dispatch picks them only where a launch has
more tiles than one round of the persistent grid, which takes outputs beyond that size: the exact-f32 "large launch" instances
(conv3d_kernel<3,1,*,3|4,2,...> and <KS,S,*,4,...>: more than 512 boxes per channel tile and sequence), the 256-position
boxes of the >= 128-channel split-half forms (conv3d_f16x2_ws_kernel<3,1,2,2,4,...>; the rows reach their 192-position
siblings <3,1,2,2,3,...>), and the full-size decoder tiles conv3d_up_kernel<1,2,4,0> and <2,2,4,0> (the rows reach the half
tile <1,2,2,0> and the 32-channel forms).  tests/test_gpu_f32_conv.py, tests/test_gpu_tile_walk.py and
tests/test_gpu_upfold.py reach those with dense rows.

Not detectable here: a load that is masked out of the result but still reads past an allocation changes nothing that can be
observed without faulting.

test_rows_reach_their_instances (no GPU) checks every row's desc against the variant queries;
test_checker_catches_planted_violations proves verify() itself on a fake callee made of torch indexing;
test_stated_alignment_is_enforced puts each buffer the header wants 16-byte aligned 4 bytes off in turn: V2CE_ERR_BAD_ARG,
nothing written."""
import ctypes
import functools
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from guarded import POISON, Guarded, written

TOL = 1e-5
BAD_ARG = -1
B, T = 2, 3
STRIDE = 3                                       # absmax_batch_stride: [3b] max, [3b + 1] guard, [3b + 2] never touched
PITCH_SETS = ("dense", "production", "odd")
WS, F32 = "conv3d_f16x2_ws_kernel", "conv3d_kernel"


def _hip():
    from v2ce_toolbox_amd import hip
    return hip


class Row:
    """One launch.  H x W: the logical input plane (Hin x Win); src: (H0, W0) of x0 when it is resampled (index maps, or the
    2x source of the decoder entries); res: None | "full" | "low"; pred: (pred_cout, y is NULL); tail: dict(C0, C1, s, src)."""

    def __init__(self, name, entry, instance, C0, Cout, H=9, W=70, ks=3, s=1, split=True, C1=0, src=None, res=None, act="relu",
                 sc=False, pred=None, tail=None, c16_out=None, T=T):
        self.name, self.entry, self.instance = name, entry, instance
        self.C0, self.C1, self.Cout, self.H, self.W, self.ks, self.s, self.split, self.T = C0, C1, Cout, H, W, ks, s, split, T
        self.src, self.res, self.act, self.sc, self.pred, self.tail = src, res, act, sc, pred, tail
        self.in_c16 = split and entry != "head"
        self.out_c16 = split if c16_out is None else c16_out
        self.H0, self.W0 = src if src is not None else (H, W)
        p = ks // 2
        self.Hout, self.Wout = (H + 2 * p - ks) // s + 1, (W + 2 * p - ks) // s + 1
        self.mapped = src is not None and entry in ("fwd", "sc", "pred", "tail")
        if tail is not None:
            ts = tail["s"]
            tail.setdefault("C1", 0)
            tail["Hin"], tail["Win"] = (self.Hout - 1) * ts + 1, (self.Wout - 1) * ts + 1
            tail["H0"], tail["W0"] = tail.get("src") or (tail["Hin"], tail["Win"])

    def __repr__(self):
        return self.name

    # ---- pitches ---------------------------------------------------------------------------------------------------------
    def widths(self):
        w = {"Wout": self.Wout, "W0": self.W0}
        if self.C1 and self.entry != "up2_part":
            w["Win"] = self.W
        if self.tail is not None:
            w["tW0"] = self.tail["W0"]
            if self.tail["C1"]:
                w["tWin"] = self.tail["Win"]
        if self.res == "low":
            w["res"] = (self.Wout + 1) // 2
        return w

    def pitches(self, pset):
        """{key: row pitch in floats} of the pitch set."""
        from v2ce_toolbox_amd.v2ce_3d import V2ce3d
        w = self.widths()
        if pset == "dense":
            return dict(w)
        if pset == "production":
            return {k: V2ce3d._pitch(v) for k, v in w.items()}
        out, used, add = {"Wout": w["Wout"] + 1}, {w["Wout"] + 1}, 3
        for k in w:
            if k == "Wout":
                continue
            while w[k] + add in used:
                add += 2
            out[k] = w[k] + add
            used.add(out[k])
            add += 2
        assert len(set(out.values())) == len(out) and all(out[k] > w[k] for k in w)
        return out

    def descs(self, pset):
        """(desc, tail desc or None, pitches) of the pitch set; a dense pitch is passed as 0 = "the width itself"."""
        hip = _hip()
        P = self.pitches(pset)
        f = (lambda k: 0) if pset == "dense" else (lambda k: P.get(k, 0))
        act = {"none": hip.ACT_NONE, "relu": hip.ACT_RELU, "leaky": hip.ACT_LEAKY}[self.act]
        d = hip.ConvDesc(B=B, T=self.T, C0=self.C0, H0=self.H0, W0=self.W0, C1=self.C1, Hin=self.H, Win=self.W, Cout=self.Cout,
                         Hout=self.Hout, Wout=self.Wout, ksize=self.ks, stride_hw=self.s, act=act, tile_t=0, tile_h=0, tile_w=0,
                         precision=hip.PRECISION_F16X2 if self.split else hip.PRECISION_F32, W0_pitch=f("W0"), Win_pitch=f("Win"),
                         Wout_pitch=f("Wout"), layout=hip.LAYOUT_C16 if self.out_c16 else hip.LAYOUT_PLANAR, absmax_batch_stride=STRIDE)
        td = None
        if self.tail is not None:
            t = self.tail
            td = hip.ConvDesc(B=B, T=self.T, C0=t["C0"], H0=t["H0"], W0=t["W0"], C1=t["C1"], Hin=t["Hin"], Win=t["Win"], Cout=self.Cout,
                              Hout=self.Hout, Wout=self.Wout, ksize=1, stride_hw=t["s"], act=hip.ACT_NONE, tile_t=0, tile_h=0, tile_w=0,
                              precision=hip.PRECISION_F16X2, W0_pitch=f("tW0"), Win_pitch=f("tWin"), Wout_pitch=f("Wout"),
                              layout=hip.LAYOUT_C16, absmax_batch_stride=STRIDE)
        return d, td, P

    def variant(self, pset="dense"):
        hip = _hip()
        d = self.descs(pset)[0]
        if self.entry == "head":
            return "conv3d_head_f16x2_kernel"             # (one kernel per input channel count; the entry has no variant query)
        if self.entry in ("wt", "wt_tail"):
            return hip.conv_wt_variant(d, (3 if self.res else 2) if self.entry == "wt_tail" else int(bool(self.res)))
        if self.entry in ("up2", "up2_part"):
            return hip.conv_up2_variant(d, self.sc)
        fuse = {"fwd": 0, "pred": 1, "sc": 2, "tail": 3}[self.entry]
        return hip.conv_variant(d, self.mapped, fuse + (4 if self.res else 0))


ROWS = [
    # ---- v2ce_conv3d_fwd, split-half
    Row("fwd-ws-3x3x3", "fwd", f"{WS}<3,1,1,2,4,3,0,0,0>", 32, 96),
    Row("fwd-ws-3x3x3-res", "fwd", f"{WS}<3,1,1,2,4,3,0,2,0>", 32, 96, res="full"),
    Row("fwd-ws-3x3x3-res-c160", "fwd", f"{WS}<3,1,2,2,3,3,0,2,0>", 16, 160, res="full"),
    Row("fwd-ws-3x3x3-s2", "fwd", f"{WS}<3,2,2,1,2,3,0,2,0>", 16, 96, W=139, s=2),
    Row("fwd-ws-1x1x1", "fwd", f"{WS}<1,1,1,2,4,3,0,2,0>", 32, 96, ks=1),
    Row("fwd-ws-1x1x1-s2", "fwd", f"{WS}<1,2,1,2,4,3,0,2,0>", 16, 96, W=139, ks=1, s=2),
    Row("fwd-ws-3x3x3-maps", "fwd", f"{WS}<3,1,1,2,4,3,0,0,0>", 16, 96, C1=16, src=(4, 30)),
    # ---- v2ce_conv3d_fwd, exact f32
    Row("fwd-f32-3x3x3-res", "fwd", f"{F32}<3,1,2,2,4,8,1,0>", 6, 72, split=False, res="full"),
    Row("fwd-f32-3x3x3-s2", "fwd", f"{F32}<3,2,2,2,2,14,1,0>", 6, 72, W=139, s=2, split=False),
    Row("fwd-f32-1x1x1-maps", "fwd", f"{F32}<1,1,2,2,8,2,2,1>", 8, 72, ks=1, C1=5, src=(4, 30), split=False),
    Row("fwd-f32-head", "fwd", "conv3d_head_kernel", 2, 32, split=False, act="leaky"),
    Row("fwd-f32-head-bridge", "fwd", "conv3d_head_kernel", 2, 32, split=False, act="leaky", c16_out=True),
    # ---- v2ce_conv3d_fwd_sc
    Row("sc-s2", "sc", f"{WS}<3,2,2,1,2,9,2,0,0>", 16, 96, W=139, s=2, sc=True),
    Row("sc-s1-c32", "sc", f"{WS}<3,1,1,1,4,3,2,0,0>", 32, 32, sc=True),
    # ---- v2ce_conv3d_fwd_pred
    Row("pred-y-res-20", "pred", f"{WS}<3,1,1,1,4,9,1,1,1>", 32, 32, res="full", pred=(20, False)),
    Row("pred-null-20", "pred", f"{WS}<3,1,1,1,4,9,1,0,1>", 32, 32, pred=(20, True)),
    Row("pred-null-res-7", "pred", f"{WS}<3,1,1,1,4,9,1,1,1>", 32, 32, res="full", pred=(7, True)),
    Row("pred-y-7", "pred", f"{WS}<3,1,1,1,4,9,1,0,1>", 32, 32, pred=(7, False)),
    # ---- v2ce_conv3d_fwd_tail
    Row("tail-s2", "tail", f"{WS}<3,1,1,2,4,3,3,0,0>", 32, 96, tail=dict(C0=16, s=2)),
    Row("tail-maps-c160", "tail", f"{WS}<3,1,2,2,3,3,3,0,0>", 16, 160, tail=dict(C0=32, C1=16, s=1, src=(5, 35))),
    # ---- v2ce_conv3d_fwd_up2 / _up2_part
    Row("up2", "up2", "conv3d_up_kernel<1,2,2,0>", 16, 96, W=69, C1=16, src=(5, 35)),
    Row("up2-c32", "up2", "conv3d_up_kernel<1,1,4,0>", 16, 32, W=69, C1=16, src=(5, 35)),
    Row("up2-sc", "up2", "conv3d_up_kernel<1,1,4,2>", 16, 32, W=69, C1=16, src=(5, 35), sc=True),
    Row("up2-part-c160", "up2_part", "conv3d_up_kernel<1,2,2,0>", 32, 160, W=69, C1=32, src=(5, 35), act="none"),
    # ---- v2ce_conv3d_fwd_wt / _wt_tail
    Row("wt", "wt", "conv3d_wt_kernel<2,4,0,0>", 32, 128),
    Row("wt-res", "wt", "conv3d_wt_kernel<2,4,1,0>", 32, 128, res="full"),
    Row("wt-T1", "wt", "conv3d_wt_kernel<2,4,0,0>", 32, 128, T=1),
    Row("wt-tail", "wt_tail", "conv3d_wt_kernel<2,4,0,1>", 32, 128, tail=dict(C0=64, s=1)),
    Row("wt-tail-res", "wt_tail", "conv3d_wt_kernel<2,4,1,1>", 32, 128, res="full", tail=dict(C0=64, s=1)),
    Row("wt-tail-lowres-maps", "wt_tail", "conv3d_wt_kernel<2,4,1,1>", 32, 128, res="low", tail=dict(C0=64, s=1, src=(5, 35))),
    # ---- v2ce_conv3d_head_f16x2
    Row("head-c2", "head", "conv3d_head_f16x2_kernel", 2, 32, act="leaky"),
    Row("head-c3", "head", "conv3d_head_f16x2_kernel", 3, 32, act="leaky"),
]
ENTRY_EXPORT = {"fwd": "v2ce_conv3d_fwd", "sc": "v2ce_conv3d_fwd_sc", "pred": "v2ce_conv3d_fwd_pred", "tail": "v2ce_conv3d_fwd_tail",
                "up2": "v2ce_conv3d_fwd_up2", "up2_part": "v2ce_conv3d_fwd_up2_part", "wt": "v2ce_conv3d_fwd_wt",
                "wt_tail": "v2ce_conv3d_fwd_wt_tail", "head": "v2ce_conv3d_head_f16x2"}


# ---------------------------------------------------------------------------------------------------------------------
# layouts: logical [B, T, C, H, W] <-> the bytes of a pitched planar / channels-last-16 buffer
# ---------------------------------------------------------------------------------------------------------------------
def to_buf(x, c16, pitch, poison):
    """f32 buffer [B][T][C][H][pitch] or [B][T][C/16][H][pitch][16] of the logical tensor; padding columns poisoned."""
    b, t, c, h, w = x.shape
    a = np.empty((b, t, c // 16, h, pitch, 16) if c16 else (b, t, c, h, pitch), np.float32)
    a.view(np.uint8)[...] = poison
    if c16:
        a[:, :, :, :, :w, :] = x.reshape(b, t, c // 16, 16, h, w).transpose(0, 1, 2, 4, 5, 3)
    else:
        a[..., :w] = x
    return a


def from_buf(body, shape, c16, pitch):
    """(logical [B, T, C, H, W] f32, byte mask of the logical elements) of a buffer's bytes."""
    b, t, c, h, w = shape
    a = body.view(np.float32).reshape((b, t, c // 16, h, pitch, 16) if c16 else (b, t, c, h, pitch))
    m = np.zeros(a.shape, bool)
    if c16:
        m[:, :, :, :, :w, :] = True
        x = a[:, :, :, :, :w, :].transpose(0, 1, 2, 5, 3, 4).reshape(b, t, c, h, w)
    else:
        m[..., :w] = True
        x = a[..., :w]
    return np.ascontiguousarray(x), np.repeat(m.ravel(), 4)


class Buf:
    def __init__(self, kind, g, orig=None, meta=None):
        self.kind, self.g, self.orig, self.meta = kind, g, orig, meta          # kind: "in" | "out" | "slots"
        self.intact = self.body = None


class Exec:
    """One execution: hands out the guarded buffers; collect() reads them back."""

    def __init__(self, poison, misalign=False, shift=None):
        self.poison, self.misalign, self.shift, self.bufs, self.align = poison, misalign, shift, {}, {}

    def _guarded(self, name, n, align):
        """misalign: the smallest offset past a 256-byte boundary the stated alignment allows; shift: buffer `shift` 4 bytes
        past a 256-byte boundary, whatever its alignment."""
        self.align[name] = align
        return Guarded(n, self.poison, 4 if name == self.shift else (align if self.misalign else 0))

    def inp(self, name, arr, align=4):
        arr = np.ascontiguousarray(arr)
        g = self._guarded(name, arr.nbytes, align)
        g.fill(arr)
        self.bufs[name] = Buf("in", g, arr.view(np.uint8).ravel().copy())
        return g.ptr

    def act(self, name, x, c16, pitch):
        return self.inp(name, to_buf(x, c16, pitch, self.poison), 16 if c16 else 4)

    def out(self, name, shape, c16, pitch):
        b, t, c, h, w = shape
        g = self._guarded(name, b * t * c * h * pitch * 4, 16 if c16 else 4)
        self.bufs[name] = Buf("out", g, meta=(shape, c16, pitch))
        return g.ptr

    def _slots(self, maxes):
        s = np.empty((B, STRIDE), np.float32)
        s.view(np.uint8)[...] = self.poison
        s[:, 0], s[:, 1] = maxes, 0.0
        return s

    def slots_in(self, name, x):
        return self.inp(name, self._slots(np.abs(x).reshape(B, -1).max(axis=1)))

    def slots_out(self, name):
        g = self._guarded(name, B * STRIDE * 4, 4)
        g.fill(self._slots(0.0))
        self.bufs[name] = Buf("slots", g)
        self.bufs[name].orig_slots = self._slots(0.0).view(np.uint8).ravel()
        return g.ptr

    def collect(self):
        torch.cuda.synchronize()
        for b in self.bufs.values():
            b.intact, b.body = b.g.read()
        return self


# ---------------------------------------------------------------------------------------------------------------------
# inputs, packed weights, the f64 value
# ---------------------------------------------------------------------------------------------------------------------
def nearest(n_in, n_out):
    from v2ce_toolbox_amd.v2ce_3d import _nearest_map
    return _nearest_map(n_in, n_out)


@functools.lru_cache(maxsize=None)
def inputs(r):
    """Logical f32 tensors [B, T, C, H, W] and parameters of the row (CPU numpy), seeded by its name."""
    rng = np.random.default_rng(zlib.crc32(r.name.encode()))
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    cin = r.C0 + r.C1
    I = {"x0": f(B, r.T, r.C0, r.H0, r.W0)}
    if r.entry == "head":
        I["x0"] = (rng.random((B, r.T, r.C0, r.H0, r.W0)) * 6.0 - 0.93).astype(np.float32)
        I["bias"] = 0.3 * f(32)
    if r.C1 and r.entry != "up2_part":
        I["x1"] = f(B, r.T, r.C1, r.H, r.W)
    I["w"] = f(r.Cout, cin, r.ks ** 3) * np.float32((2.0 / (cin * r.ks ** 3)) ** 0.5)
    I["scale"] = (rng.random(r.Cout) + 0.5).astype(np.float32)
    I["shift"] = 0.3 * f(r.Cout)
    if r.res:
        hw = ((r.Hout + 1) // 2, (r.Wout + 1) // 2) if r.res == "low" else (r.Hout, r.Wout)
        I["res"] = f(B, r.T, r.Cout, *hw)
    if r.sc:
        I["wd"] = f(r.Cout, cin, 1) * np.float32((1.0 / cin) ** 0.5)
        I["scale2"] = (rng.random(r.Cout) + 0.5).astype(np.float32)
        I["shift2"] = 0.3 * f(r.Cout)
    if r.tail is not None:
        t = r.tail
        tc = t["C0"] + t["C1"]
        I["tx0"] = f(B, r.T, t["C0"], t["H0"], t["W0"])
        if t["C1"]:
            I["tx1"] = f(B, r.T, t["C1"], t["Hin"], t["Win"])
        I["wd"] = f(r.Cout, tc, 1) * np.float32((1.0 / tc) ** 0.5)
    if r.pred is not None:
        I["wp"] = 0.2 * f(r.pred[0], 32)
        I["bp"] = np.zeros(32, np.float32)
        I["bp"][:r.pred[0]] = 0.1 * f(r.pred[0])
    if r.src is not None:
        I["hmap"], I["wmap"] = nearest(r.H0, r.H), nearest(r.W0, r.W)
        if r.entry in ("up2", "up2_part"):                 # the decoder entries imply src = dst >> 1
            assert np.array_equal(I["hmap"], np.arange(r.H) >> 1) and np.array_equal(I["wmap"], np.arange(r.W) >> 1)
    if r.tail is not None and r.tail.get("src"):
        I["thmap"], I["twmap"] = nearest(r.tail["H0"], r.tail["Hin"]), nearest(r.tail["W0"], r.tail["Win"])
    return I


def _virtual(x0, x1, hmap, wmap):
    """The virtual input as f64 [B, C, T, H, W]: x0 through the index maps ++ x1."""
    x = torch.from_numpy(x0).double()
    if hmap is not None:
        x = x[:, :, :, torch.from_numpy(hmap).long()][..., torch.from_numpy(wmap).long()]
    if x1 is not None:
        x = torch.cat([x, torch.from_numpy(x1).double()], dim=2)
    return x.permute(0, 2, 1, 3, 4)


@functools.lru_cache(maxsize=None)
def want(r):
    """f64 outputs of the row, logical [B, T, C, H, W]: {"y", "sc_y", "pred_y"}."""
    I = inputs(r)
    col = lambda v: torch.from_numpy(v).double().view(1, -1, 1, 1, 1)
    x = _virtual(I["x0"], I.get("x1"), I.get("hmap"), I.get("wmap"))
    w = torch.from_numpy(I["w"]).double().reshape(r.Cout, r.C0 + r.C1, r.ks, r.ks, r.ks)
    if r.entry == "up2_part":                              # the upsampled channels' share alone
        w = w[:, :r.C0]
    acc = F.conv3d(x, w, None, (1, r.s, r.s), r.ks // 2)
    if r.tail is not None:
        t = r.tail
        tx = _virtual(I["tx0"], I.get("tx1"), I.get("thmap"), I.get("twmap"))[..., ::t["s"], ::t["s"]]
        acc = acc + F.conv3d(tx, torch.from_numpy(I["wd"]).double().reshape(r.Cout, -1, 1, 1, 1))
    y = acc * col(I["scale"]) + col(I["shift"]) if r.entry != "head" else acc + col(I["bias"])
    if r.res:
        res = torch.from_numpy(I["res"]).double().permute(0, 2, 1, 3, 4)
        if r.res == "low":
            res = res[..., torch.arange(r.Hout) >> 1, :][..., torch.arange(r.Wout) >> 1]
        y = y + res
    y = {"none": y, "relu": torch.relu(y), "leaky": F.leaky_relu(y, 0.01)}[r.act]
    out = {"y": y}
    if r.sc:
        wd = torch.from_numpy(I["wd"]).double().reshape(r.Cout, -1, 1, 1, 1)
        out["sc_y"] = F.conv3d(x, wd, None, (1, r.s, r.s)) * col(I["scale2"]) + col(I["shift2"])
    if r.pred is not None:
        pc = r.pred[0]
        wp = torch.from_numpy(I["wp"]).double().view(pc, 32, 1, 1, 1)
        out["pred_y"] = torch.relu(F.conv3d(y, wp) + col(I["bp"][:pc]))
    return {k: v.permute(0, 2, 1, 3, 4).contiguous().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def packed(r):
    """The weight tables of the row as the library's pack entries write them (bytes; one device round trip per row)."""
    hip = _hip()
    L, st, I = hip.lib(), hip.stream_ptr(), inputs(r)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def run(nbytes, call):
        out = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        hip.check(call(out.data_ptr()), "pack")
        torch.cuda.synchronize()
        return out.cpu().numpy()
    cin, k3 = r.C0 + r.C1, r.ks ** 3
    w = dev(I["w"])
    P = {}
    if r.entry == "head":
        if r.C0 == 2:
            P["w"] = run(L.v2ce_pack_head_weights_f16x2_bytes(), lambda o: L.v2ce_pack_head_weights_f16x2(w.data_ptr(), o, st))
        else:
            P["w"] = run(L.v2ce_pack_head_weights_f16x2_c3_bytes(), lambda o: L.v2ce_pack_head_weights_f16x2_c3(w.data_ptr(), o, st))
    elif r.entry in ("wt", "wt_tail"):
        P["w"] = run(L.v2ce_pack_weights_f16x2_wt_bytes(r.Cout, cin), lambda o: L.v2ce_pack_weights_f16x2_wt(w.data_ptr(), r.Cout, cin, None, o, st))
    elif r.entry in ("up2", "up2_part"):
        P["w"] = run(L.v2ce_pack_weights_f16x2_up_bytes(r.Cout, r.C0, r.C1),
                     lambda o: L.v2ce_pack_weights_f16x2_up(w.data_ptr(), r.Cout, r.C0, r.C1, None, o, st))
    elif r.split:
        P["w"] = run(L.v2ce_pack_weights_f16x2_bytes(r.Cout, cin, k3), lambda o: L.v2ce_pack_weights_f16x2(w.data_ptr(), r.Cout, cin, k3, None, o, st))
    else:
        P["w"] = run(r.Cout * cin * k3 * 4, lambda o: L.v2ce_pack_weights(w.data_ptr(), r.Cout, cin, k3, None, o, st))
    if "wd" in I:
        wd, c = dev(I["wd"]), I["wd"].shape[1]
        P["wd"] = run(L.v2ce_pack_weights_f16x2_bytes(r.Cout, c, 1), lambda o: L.v2ce_pack_weights_f16x2(wd.data_ptr(), r.Cout, c, 1, None, o, st))
    if r.pred is not None:
        wp = dev(I["wp"])
        P["wp"] = run(L.v2ce_pack_pred_weights_f16x2_bytes(), lambda o: L.v2ce_pack_pred_weights_f16x2(wp.data_ptr(), r.pred[0], 32, o, st))
    return P


# ---------------------------------------------------------------------------------------------------------------------
# one launch
# ---------------------------------------------------------------------------------------------------------------------
def library_call(r, e, d, td, a):
    """The row's entry on the buffers `a` (name -> device address or None) of execution e."""
    hip = _hip()
    L, st, by = hip.lib(), hip.stream_ptr(), ctypes.byref
    g = a.get
    if r.entry == "fwd":
        return L.v2ce_conv3d_fwd(by(d), g("x0"), g("x1"), g("hmap"), g("wmap"), g("w"), g("scale"), g("shift"), g("res"), g("y"),
                                 g("x0_absmax"), g("x1_absmax"), g("y_absmax"), st)
    if r.entry == "pred":
        return L.v2ce_conv3d_fwd_pred(by(d), g("x0"), g("x1"), g("hmap"), g("wmap"), g("w"), g("scale"), g("shift"), g("res"), g("y"),
                                      g("x0_absmax"), g("x1_absmax"), g("y_absmax"), g("wp"), g("bp"), r.pred[0], g("pred_y"), st)
    if r.entry == "sc":
        return L.v2ce_conv3d_fwd_sc(by(d), g("x0"), g("x1"), g("hmap"), g("wmap"), g("w"), g("scale"), g("shift"), g("y"), g("x0_absmax"),
                                    g("x1_absmax"), g("y_absmax"), g("wd"), g("scale2"), g("shift2"), g("sc_y"), st)
    if r.entry == "tail":
        return L.v2ce_conv3d_fwd_tail(by(d), g("x0"), g("x1"), g("hmap"), g("wmap"), g("w"), g("scale"), g("shift"), g("y"), g("x0_absmax"),
                                      g("x1_absmax"), g("y_absmax"), by(td), g("tx0"), g("tx1"), g("thmap"), g("twmap"), g("wd"),
                                      g("tx0_absmax"), g("tx1_absmax"), st)
    if r.entry == "head":
        return L.v2ce_conv3d_head_f16x2(by(d), g("x0"), g("w"), g("bias"), g("y"), g("x0_absmax"), g("y_absmax"), st)
    if r.entry == "up2":
        return L.v2ce_conv3d_fwd_up2(by(d), g("x0"), g("x1"), g("w"), g("scale"), g("shift"), g("y"), g("x0_absmax"), g("x1_absmax"),
                                     g("y_absmax"), g("wd"), g("scale2"), g("shift2"), g("sc_y"), st)
    if r.entry == "up2_part":
        return L.v2ce_conv3d_fwd_up2_part(by(d), g("x0"), g("w"), g("scale"), g("shift"), g("y"), g("x0_absmax"), g("x1_absmax"),
                                          g("y_absmax"), st)
    if r.entry == "wt":
        return L.v2ce_conv3d_fwd_wt(by(d), g("x0"), g("w"), g("scale"), g("shift"), g("res"), g("y"), g("x0_absmax"), g("y_absmax"), st)
    assert r.entry == "wt_tail"
    return L.v2ce_conv3d_fwd_wt_tail(by(d), g("x0"), g("w"), g("scale"), g("shift"), g("y"), g("x0_absmax"), g("y_absmax"), by(td), g("tx0"),
                                     g("tx1"), g("thmap"), g("twmap"), g("wd"), g("tx0_absmax"), g("tx1_absmax"), g("res"),
                                     (r.Hout + 1) // 2 if r.res == "low" else 0, a["_res_pitch"] if r.res == "low" else 0, st)


def execute(r, pset, poison, misalign=False, callee=library_call, tables=None, shift=None):
    """One execution of the row under a pitch set: every buffer guarded, the callee run, everything read back.  shift: the
    name of a buffer to put 4 bytes past a 256-byte boundary; the call must then be refused with V2CE_ERR_BAD_ARG."""
    hip = _hip()
    I, e = inputs(r), Exec(poison, misalign, shift)
    d, td, P = r.descs(pset)
    tables = packed(r) if tables is None else tables
    a = {"x0": e.act("x0", I["x0"], r.in_c16, P["W0"])}
    if "x1" in I:
        a["x1"] = e.act("x1", I["x1"], r.in_c16, P["Win"])
    for k in ("hmap", "wmap", "thmap", "twmap"):
        if k in I and (k[0] == "t" or r.mapped):
            a[k] = e.inp(k, I[k])
    for k in ("w", "wd", "wp"):
        if k in tables:
            a[k] = e.inp(k, tables[k], 16)
    for k in ("scale", "shift", "scale2", "shift2", "bias", "bp"):
        if k in I and not (r.entry == "head" and k in ("scale", "shift")):
            a[k] = e.inp(k, I[k])
    if r.res:
        a["res"] = e.act("res", I["res"], r.out_c16, P["res"] if r.res == "low" else P["Wout"])
        a["_res_pitch"] = P.get("res", 0)
    if r.tail is not None:
        a["tx0"] = e.act("tx0", I["tx0"], True, P["tW0"])
        if "tx1" in I:
            a["tx1"] = e.act("tx1", I["tx1"], True, P["tWin"])
    if r.split:                                            # (the exact-f32 kernels ignore the input slots: NULL)
        a["x0_absmax"] = e.slots_in("x0_absmax", I["x0"])
        if r.C1:
            a["x1_absmax"] = e.slots_in("x1_absmax", I["x1"] if "x1" in I else I["x0"])
        if r.tail is not None:
            a["tx0_absmax"] = e.slots_in("tx0_absmax", I["tx0"])
            if "tx1" in I:
                a["tx1_absmax"] = e.slots_in("tx1_absmax", I["tx1"])
    oshape = (B, r.T, r.Cout, r.Hout, r.Wout)
    if r.pred is None or not r.pred[1]:
        a["y"] = e.out("y", oshape, r.out_c16, P["Wout"])
    if r.sc:
        a["sc_y"] = e.out("sc_y", oshape, r.out_c16, P["Wout"])
    if r.pred is not None:
        a["pred_y"] = e.out("pred_y", (B, r.T, r.pred[0], r.Hout, r.Wout), False, r.Wout)      # always planar and dense
    a["y_absmax"] = e.slots_out("y_absmax")
    rc = callee(r, e, d, td, a)
    if shift is not None:
        msg = hip.lib().v2ce_last_error().decode()
        assert rc == BAD_ARG and "16-byte aligned" in msg, f"{r.name} [{pset}]: {shift} 4 bytes off a 16-byte boundary: rc {rc}: {msg}"
        return e.collect()
    assert rc == 0, f"{r.name} [{pset}]: rc {rc}: {hip.lib().v2ce_last_error().decode()}"
    return e.collect()


# ---------------------------------------------------------------------------------------------------------------------
# the checks
# ---------------------------------------------------------------------------------------------------------------------
def verify(r, wanted, runs):
    """runs: {pitch set: (POISON[0] run, POISON[1] run, misaligned POISON[0] run)} of row r; wanted: its f64 outputs."""
    tag = lambda pset, i: f"{r.name} [{pset}, {('POISON[0]', 'POISON[1]', 'misaligned')[i]}]"
    # containment and inputs
    for pset, trio in runs.items():
        for i, e in enumerate(trio):
            for name, b in e.bufs.items():
                assert b.intact, f"{tag(pset, i)}: {name}: write outside the buffer, a guard byte changed ({b.g.n} bytes, {b.kind})"
                if b.kind == "in":
                    assert np.array_equal(b.body, b.orig), f"{tag(pset, i)}: {name}: a const input changed"
    first, report = None, []
    for pset, (A, Bb, M) in runs.items():
        logical = {}
        for name, a in A.bufs.items():
            if a.kind == "slots":                          # [3b + 2] is never touched
                for i, e in enumerate((A, Bb, M)):
                    s = e.bufs[name].body.reshape(B, STRIDE, 4)
                    assert np.all(s[:, 2:] == e.poison), f"{tag(pset, i)}: {name}: the floats between the slots [{STRIDE}b + 2] were written"
                continue
            if a.kind != "out":
                continue
            shape, c16, pitch = a.meta
            xa, mask = from_buf(a.body, shape, c16, pitch)
            xb, _ = from_buf(Bb.bufs[name].body, shape, c16, pitch)
            xm, _ = from_buf(M.bufs[name].body, shape, c16, pitch)
            wr = written(a.body, Bb.bufs[name].body)
            extra, missing = np.flatnonzero(wr & ~mask), np.flatnonzero(~wr & mask)
            assert extra.size == 0, (f"{tag(pset, 0)}: {name}: {extra.size} bytes written outside the logical extent (a padding column), "
                                     f"first at byte {extra[0]} of {a.body.size} (row pitch {pitch}, width {shape[4]})")
            assert missing.size == 0, (f"{tag(pset, 0)}: {name}: {missing.size} logical bytes left unwritten, first at byte {missing[0]} "
                                       f"of {a.body.size} (row pitch {pitch}, width {shape[4]})")
            assert np.all(M.bufs[name].body[~mask] == M.poison), f"{tag(pset, 2)}: {name}: a padding column was written"
            # never read: poison, guard contents and alignment do not reach the result
            for i, x in ((1, xb), (2, xm)):
                assert np.array_equal(x.view(np.int32), xa.view(np.int32)), \
                    f"{tag(pset, i)}: {name}: differs from the POISON[0] run (a padding or guard value was read)"
            logical[name] = xa
            report.append(f"{pset}/{name} {int(wr.sum())}/{a.body.size} bytes")
        # the same bits under every pitch set
        if first is None:
            first = (pset, logical)
        for name, x in logical.items():
            assert np.array_equal(x.view(np.int32), first[1][name].view(np.int32)), f"{r.name}: {name}: [{pset}] differs from [{first[0]}]"
        # the range slots
        for i, e in enumerate((A, Bb, M)):
            s = e.bufs["y_absmax"].body.view(np.float32).reshape(B, STRIDE)
            for b in range(B):
                ymax = np.float32(np.abs(logical["y"][b]).max()) if "y" in logical else np.float32(0.0)
                assert s[b, 0].view(np.int32) == ymax.view(np.int32), f"{tag(pset, i)}: slot [{STRIDE * b}] = {s[b, 0]!r}, max |y_{b}| = {ymax!r}"
                if r.split:
                    assert np.isfinite(s[b, 1]) and s[b, 1] > 0, f"{tag(pset, i)}: range-guard slot [{STRIDE * b + 1}] = {s[b, 1]!r}"
                else:
                    assert s[b, 1] == 0, f"{tag(pset, i)}: exact-f32 launch wrote the range-guard slot: {s[b, 1]!r}"
    # values (the same bits under every pitch set: once)
    worst = 0.0
    for name, x in first[1].items():
        w = wanted[name]
        assert x.shape == w.shape, (name, x.shape, w.shape)
        d = np.abs(x.astype(np.float64) - w)
        excess = d - TOL * np.abs(w)
        k = np.unravel_index(np.argmax(excess), excess.shape)
        print(f"conv containment {r.name}: {name} max |d| = {d.max():.3e}, max excess over rel = {excess[k]:.3e}")
        assert excess[k] <= TOL, f"{r.name}: {name} at (b, t, c, h, w) = {k}: got {x[k]!r}, want {w[k]!r}"
        worst = max(worst, float(d.max()))
    print(f"conv containment {r.name} -> {r.instance}: {'; '.join(report)}; guards intact, max |d| = {worst:.3e}")


# ---------------------------------------------------------------------------------------------------------------------
# the tests
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", ROWS, ids=lambda r: r.name)
def test_rows_reach_their_instances(r):
    """Every row's desc is accepted by the variant query of its entry under every pitch set and names the row's instance; the
    odd pitches are pairwise different with Wout_pitch = Wout + 1, the production pitch of a stride-1 row differs from its width."""
    for pset in PITCH_SETS:
        assert r.variant(pset) == r.instance, (pset, r.variant(pset))
    P = r.pitches("odd")
    assert P["Wout"] == r.Wout + 1 and len(set(P.values())) == len(P)
    assert r.pitches("production")["Wout"] > r.Wout >= 64 and r.Wout % 32


def test_table_covers_every_conv_entry():
    from test_gpu_containment import COVERED_ELSEWHERE
    hip = _hip()
    here = {ENTRY_EXPORT[r.entry] for r in ROWS}
    assert here == set(ENTRY_EXPORT.values()) and here <= set(hip.EXPORTS)
    for name in here:
        assert COVERED_ELSEWHERE[name].startswith("tests/test_gpu_conv_containment.py::test_conv_containment"), name
    assert len({r.name for r in ROWS}) == len(ROWS)


@pytest.mark.gpu
@pytest.mark.parametrize("r", ROWS, ids=lambda r: r.name)
def test_conv_containment(r):
    runs = {pset: (execute(r, pset, POISON[0]), execute(r, pset, POISON[1]), execute(r, pset, POISON[0], misalign=True))
            for pset in PITCH_SETS}
    verify(r, want(r), runs)


@pytest.mark.gpu
@pytest.mark.parametrize("r", ROWS, ids=lambda r: r.name)
def test_stated_alignment_is_enforced(r):
    """Each buffer the header wants 16-byte aligned (channels-last-16 tensors, weight buffers), in turn 4 bytes off: the call is
    refused with V2CE_ERR_BAD_ARG and the alignment's message, and nothing was written -- outputs all poison, slots as the caller
    left them, guards intact."""
    plain = execute(r, "odd", POISON[0])
    names = [n for n, al in plain.align.items() if al == 16]
    assert "w" in names and ("y" in names) == (r.out_c16 and "y" in plain.bufs)
    for name in names:
        e = execute(r, "odd", POISON[0], shift=name)
        for n, b in e.bufs.items():
            assert b.intact, f"{r.name}: {n}: a refused call wrote outside the buffer"
            if b.kind == "out":
                assert np.all(b.body == e.poison), f"{r.name}: {n} written by a call refused for the alignment of {name}"
            elif b.kind == "slots":
                assert np.array_equal(b.body, plain.bufs[n].orig_slots), f"{r.name}: {n} written by a refused call"
            else:
                assert np.array_equal(b.body, b.orig), f"{r.name}: {n}: a const input changed"
    print(f"\nconv containment {r.name}: refused with V2CE_ERR_BAD_ARG, nothing written: {', '.join(names)} 4 bytes off")


FAKE = Row("fake", "fwd", None, 16, 32, H=3, W=5)


def _fake_callee(violation):
    """Writes the f64 value (rounded to f32) into the guarded, pitched y of the FAKE row with torch indexing, and the slots;
    plus one planted violation.  Every write stays inside the buffer's own allocation."""
    def callee(r, e, d, td, a):
        w = want(r)["y"].astype(np.float32)
        yb, sb = e.bufs["y"], e.bufs["y_absmax"]
        shape, c16, pitch = yb.meta
        g = yb.g
        full = g.t[g.front - 4:g.front + g.n + 4].view(torch.float32)           # one float of each guard zone, and the buffer
        y = full[1:-1].view(B, r.T, r.Cout // 16, r.Hout, pitch, 16)
        val = torch.from_numpy(to_buf(w, True, r.Wout, 0)).cuda()
        if violation == "unwritten":
            keep = y[1, 2, 1, 2, 3, 7].clone()
        y[:, :, :, :, :r.Wout, :] = val
        s = sb.g.t[sb.g.front:sb.g.front + sb.g.n].view(torch.float32).view(B, STRIDE)
        s[:, 0] = torch.from_numpy(np.abs(w).reshape(B, -1).max(axis=1)).cuda()
        s[:, 1] = 1e-7
        if violation == "padding":
            y[1, 2, 1, 2, r.Wout, 7] = 1.0
        elif violation == "front guard":
            full[0] = 1.0
        elif violation == "back guard":
            full[-1] = 1.0
        elif violation == "slot":
            s[1, 2] = 1.0
        elif violation == "unwritten":
            y[1, 2, 1, 2, 3, 7] = keep
        else:
            assert violation is None
        return 0
    return callee


@pytest.mark.gpu
def test_checker_catches_planted_violations():
    """verify() -- the function the rows use -- passes a correct fake callee and reports each planted violation: one float in
    a padding column, in the front guard, in the back guard, at [3b + 2], and one logical element left unwritten."""
    def runs(violation):
        c = _fake_callee(violation)
        return {"odd": tuple(execute(FAKE, "odd", p, m, callee=c, tables={}) for p, m in ((POISON[0], False), (POISON[1], False),
                                                                                           (POISON[0], True)))}
    verify(FAKE, want(FAKE), runs(None))
    reported = []
    for violation, message in (("padding", "written outside the logical extent"), ("front guard", "y: write outside the buffer"),
                               ("back guard", "y: write outside the buffer"), ("slot", r"floats between the slots"),
                               ("unwritten", "4 logical bytes left unwritten")):
        with pytest.raises(AssertionError, match=message) as info:
            verify(FAKE, want(FAKE), runs(violation))
        reported.append(f"{violation}: {str(info.value).splitlines()[0]}")
    print("\nplanted violations reported:\n  " + "\n  ".join(reported))
    assert len(reported) == 5
