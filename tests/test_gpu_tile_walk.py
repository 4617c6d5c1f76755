"""Split-half convolutions on MULTI-TILE persistent walks, against f64.

Every split-half conv kernel but the 2-channel head runs on a persistent grid (min(blocks, CUs) workgroups, each walking
virtual blocks vb, vb + grid, ...): the weight ring, the epilogue hand-over between tiles, the per-sequence power-of-two
pre-scales and the walk order all carry state from one tile to the next.  The other f64 tests mostly give each workgroup
one tile.  Every row of WALK_CASES is one kernel instance of the default dispatch, reached through the model's own entry
points, at a shape where

- the walk has several rounds: ceil(B T Hout Wout / POS_TILE) * ceil(Cout / CO_TILE) >= 3 x 256 CUs (Winograd-T: pairs of
  time steps instead of T), so every workgroup runs >= 3 tiles and the last round is ragged;
- the channel-tile count is not a power of two (3 or 5) wherever the form's Cout range allows it, so a workgroup's walk
  changes channel tile (with 2^n channel tiles and a grid of 256 every walk stays on one channel tile).  Exempt: the
  Cout <= 32 forms, and the 64-channel ws forms (Cout < 128: at most 2 tiles), which run Cout = 96 -- a partial last tile;
- the batch holds B = 3 sequences scaled by 2^-8, 1 and 2^8 (inputs, residual and tail inputs alike) with one range slot
  per sequence, so walks cross sequence boundaries and must switch pre-scale and slot.  The per-channel BN shift and the
  head bias are shared by the batch: they carry the 2^-8 scale, so sequence 0 is exactly 2^-8 times a unit problem;
- H and W are odd and divide no box; the Winograd-T rows have odd T (the last pair's second step is missing).

Checks: per sequence b, got_b / 2^k_b against the f64 value / 2^k_b at 1e-5 abs + 1e-5 rel; the sequence's range slot
holds max |y_b| of the returned tensor (not for the fused head, whose launch reports only the guard) and a finite guard
bound > 0; row b of the batched launch is bit-equal to the same launch on sequence b alone.

The f64 reference is evaluated at a position set, with all output channels (input patches gathered, one f64 matmul per
chunk): all positions of four time steps (first, last and both members of a Winograd pair), all positions on the first
two and last two rows and columns (the ragged boxes), and a seeded uniform 12 % of the rest.  A box away from the edges
holds >= 128 positions, so a box whose values are all wrong is missed with probability <= 0.88^128 < 1e-7.  Small
launches (< 1.2e10 multiply-adds) are evaluated in full.

test_walk_table (no GPU) checks the table against the dispatchers' variant queries and the rounds bound;
test_network_instances_are_covered (GPU) fails when the network launches an instance that has no row here."""
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conv_ref import at as _at, conv_at, positions

TOL = 1e-5
N_CU = 256                         # MI355X
SCALE_EXP = (-8, 0, 8)             # sequence b is 2^SCALE_EXP[b] times a unit-scale problem
HEAD_CH = 20                       # channels of the fused 1x1x1 head (the network's)


class Case:
    """One kernel instance on a walk.  H x W is the logical input plane (decoder kinds: the upsampled one = the output);
    C0: main input channels (up: the upsampled source), C1: skip channels (up kinds), tc: tail channels."""

    def __init__(self, name, kind, B, T, C0, Cout, H, W, ks=3, s=1, res=False, C1=0, tc=0):
        self.name, self.kind, self.B, self.T, self.C0, self.Cout, self.H, self.W = name, kind, B, T, C0, Cout, H, W
        self.ks, self.s, self.res, self.C1, self.tc = ks, s, res, C1, tc

    @property
    def out_hw(self):
        p = self.ks // 2
        return (self.H + 2 * p - self.ks) // self.s + 1, (self.W + 2 * p - self.ks) // self.s + 1

    def tiles(self):
        """(CO_TILE, POS_TILE, positions the walk covers) from the instance's template arguments."""
        a = [int(v) for v in self.name[self.name.index("<") + 1:-1].split(",")] if "<" in self.name else []
        Ho, Wo = self.out_hw
        if self.name.startswith("conv3d_f16x2_ws_kernel"):
            wco, co_fr, po_fr = a[2], a[3], a[4]
            return wco * co_fr * 32, (4 // wco) * po_fr * 32, self.B * self.T * Ho * Wo
        if self.name.startswith("conv3d_wt_kernel"):
            return a[0] * 32, a[1] * 32, self.B * ((self.T + 1) // 2) * Ho * Wo
        if self.name.startswith("conv3d_up_kernel"):
            wco, co_fr, po_fr = a[0], a[1], a[2]
            return wco * co_fr * 32, 4 * (po_fr // wco) * 32, self.B * self.T * Ho * Wo
        return None

    def co_tiles(self):
        t = self.tiles()
        return None if t is None else -(-self.Cout // t[0])

    def tile_bound(self):
        t = self.tiles()
        return None if t is None else -(-t[2] // t[1]) * self.co_tiles()

    def __repr__(self):
        return self.id

    @property
    def id(self):
        return f"{self.kind}-{self.name[self.name.index('<'):] if '<' in self.name else 'head'}"


WS = "conv3d_f16x2_ws_kernel"
WALK_CASES = [
    # -- 1x1x1 (shortcuts): stride 1 and 2, <= 32 / 64-channel / >= 128-channel forms
    Case(f"{WS}<1,1,1,1,4,3,0,2,0>", "ws", 3, 8, 32, 32, 101, 163, ks=1),
    Case(f"{WS}<1,1,1,2,4,3,0,2,0>", "ws", 3, 8, 32, 96, 91, 91, ks=1, res=True),
    Case(f"{WS}<1,1,2,2,4,3,0,2,0>", "ws", 3, 8, 64, 384, 51, 57, ks=1),
    Case(f"{WS}<1,2,1,1,4,3,0,2,0>", "ws", 3, 8, 16, 32, 201, 325, ks=1, s=2),
    Case(f"{WS}<1,2,1,2,4,3,0,2,0>", "ws", 3, 8, 16, 96, 181, 181, ks=1, s=2),
    Case(f"{WS}<1,2,2,2,4,3,0,2,0>", "ws", 3, 8, 32, 384, 101, 113, ks=1, s=2),
    # -- 3x3x3 stride 1, plain (RES 0) and with a residual
    Case(f"{WS}<3,1,1,1,4,3,0,0,0>", "ws", 3, 8, 32, 32, 101, 163),
    Case(f"{WS}<3,1,1,1,4,3,0,1,0>", "ws", 3, 8, 32, 32, 101, 163, res=True),
    Case(f"{WS}<3,1,1,2,4,3,0,0,0>", "ws", 3, 8, 32, 96, 91, 91),
    Case(f"{WS}<3,1,1,2,4,3,0,2,0>", "ws", 3, 8, 32, 96, 91, 91, res=True),
    Case(f"{WS}<3,1,2,2,4,3,0,0,0>", "ws", 3, 8, 32, 384, 67, 67),
    Case(f"{WS}<3,1,2,2,4,3,0,2,0>", "ws", 3, 8, 32, 384, 67, 67, res=True),
    Case(f"{WS}<3,1,2,2,3,3,0,0,0>", "ws", 3, 8, 32, 384, 51, 51),
    Case(f"{WS}<3,1,2,2,3,3,0,2,0>", "ws", 3, 8, 32, 384, 51, 51, res=True),
    # -- 3x3x3 stride 2
    Case(f"{WS}<3,2,1,1,1,3,0,2,0>", "ws", 3, 8, 16, 32, 145, 171, s=2),
    Case(f"{WS}<3,2,2,1,2,3,0,2,0>", "ws", 3, 8, 16, 96, 125, 157, s=2, res=True),
    Case(f"{WS}<3,2,4,1,4,3,0,2,0>", "ws", 3, 8, 32, 384, 73, 113, s=2),
    # -- fused 1x1x1 shortcut (second output)
    Case(f"{WS}<3,1,1,1,4,3,2,0,0>", "sc", 3, 8, 32, 32, 101, 163),
    Case(f"{WS}<3,2,1,1,1,3,2,0,0>", "sc", 3, 8, 16, 32, 145, 171, s=2),
    Case(f"{WS}<3,2,2,1,2,9,2,0,0>", "sc", 3, 8, 16, 96, 125, 157, s=2),
    Case(f"{WS}<3,2,4,1,4,3,2,0,0>", "sc", 3, 8, 32, 384, 73, 113, s=2),
    # -- fused 1x1x1 head (shared epilogue, PEPI)
    Case(f"{WS}<3,1,1,1,4,9,1,1,1>", "pred", 3, 8, 32, 32, 101, 163, res=True),
    Case(f"{WS}<3,1,1,1,4,9,1,0,1>", "pred", 3, 8, 32, 32, 101, 163),
    # -- folded 1x1x1 tail (FUSE 3)
    Case(f"{WS}<3,1,1,2,4,3,3,0,0>", "tail", 3, 8, 32, 96, 91, 91, tc=32),
    Case(f"{WS}<3,1,2,2,4,3,3,0,0>", "tail", 3, 8, 32, 384, 67, 67, tc=64),
    Case(f"{WS}<3,1,2,2,3,3,3,0,0>", "tail", 3, 8, 32, 384, 51, 51, tc=64),
    # -- Winograd-T (pairs of time steps; odd T)
    Case("conv3d_wt_kernel<2,4,0,0>", "wt", 3, 5, 32, 320, 45, 49),
    Case("conv3d_wt_kernel<2,4,1,0>", "wt", 3, 7, 32, 192, 53, 55, res=True),
    Case("conv3d_wt_kernel<2,4,0,1>", "wt_tail", 3, 5, 32, 320, 45, 49, tc=64),
    Case("conv3d_wt_kernel<2,4,1,1>", "wt_tail", 3, 7, 32, 192, 53, 55, res=True, tc=64),
    # -- phase-folded decoder conv1 (upsample 2x ++ skip)
    Case("conv3d_up_kernel<1,1,4,2>", "up_sc", 3, 8, 16, 32, 101, 163, C1=16),
    Case("conv3d_up_kernel<1,1,4,0>", "up", 3, 8, 16, 32, 101, 163, C1=16),
    Case("conv3d_up_kernel<1,2,4,0>", "up", 3, 8, 16, 320, 59, 59, C1=16),
    Case("conv3d_up_kernel<1,2,2,0>", "up", 3, 8, 16, 320, 43, 65, C1=16),
    Case("conv3d_up_kernel<2,2,4,0>", "up_part", 3, 8, 32, 384, 49, 57, C1=32),
    # -- the network's head (not persistent: one block per tile)
    Case("conv3d_head_f16x2_kernel", "head", 3, 5, 2, 32, 67, 93),
]


def _desc(c, B=None):
    from v2ce_toolbox_amd import hip
    Ho, Wo = c.out_hw
    up = c.kind.startswith("up")
    return hip.ConvDesc(B=c.B if B is None else B, T=c.T, C0=c.C0, H0=(c.H + 1) // 2 if up else c.H, W0=(c.W + 1) // 2 if up else c.W,
                        C1=c.C1, Hin=c.H, Win=c.W, Cout=c.Cout, Hout=Ho, Wout=Wo, ksize=c.ks, stride_hw=c.s,
                        act=hip.ACT_NONE if c.kind == "up_part" else hip.ACT_RELU, tile_t=0, tile_h=0, tile_w=0,
                        precision=hip.PRECISION_F16X2, W0_pitch=0, Win_pitch=0, Wout_pitch=0, layout=hip.LAYOUT_C16, absmax_batch_stride=2)


def _variant(c):
    from v2ce_toolbox_amd import hip
    d = _desc(c)
    if c.kind == "head":
        return "conv3d_head_f16x2_kernel"
    if c.kind in ("wt", "wt_tail"):
        return hip.conv_wt_variant(d, (3 if c.res else 2) if c.kind == "wt_tail" else int(c.res))
    if c.kind.startswith("up"):
        return hip.conv_up2_variant(d, c.kind == "up_sc")
    fuse = {"ws": 0, "sc": 2, "pred": 1, "tail": 3}[c.kind]
    return hip.conv_variant(d, False, fuse + (4 if c.res else 0))


@pytest.mark.parametrize("case", WALK_CASES, ids=lambda c: c.id)
def test_walk_table(case):
    """The row's instance is what the default dispatch picks for its shape, and the walk has the properties the
    module docstring lists (variant queries launch nothing: no GPU needed)."""
    assert _variant(case) == case.name
    assert case.B >= 3 and case.H % 2 == 1 and case.W % 2 == 1
    if case.kind == "head":
        return
    assert case.tile_bound() >= 3 * N_CU, case.tile_bound()
    n_co = case.co_tiles()
    if case.Cout > 32:
        if case.kind.startswith(("wt", "up")) or case.tiles()[0] == 128:
            assert n_co in (3, 5), n_co
        else:                                              # the 64-channel ws forms: a partial last channel tile
            assert case.Cout == 96 and n_co == 2
    if case.kind.startswith("wt"):
        assert case.T % 2 == 1


def test_instances_are_unique():
    assert len({c.name for c in WALK_CASES}) == len(WALK_CASES)


# ------------------------------------------------------------------------------------------------
# inputs and the f64 reference
# ------------------------------------------------------------------------------------------------
def _inputs(c):
    """CPU float32 tensors (NCDHW) of the case; sequence b carries the factor 2^SCALE_EXP[b]."""
    g = torch.Generator().manual_seed(zlib.crc32(c.name.encode()) & 0x7FFFFFFF)
    B, T, Cout = c.B, c.T, c.Cout
    Ho, Wo = c.out_hw
    k = torch.tensor([2.0 ** SCALE_EXP[b] for b in range(B)]).view(B, 1, 1, 1, 1)
    I = {"k": k}
    if c.kind == "head":
        I["x"] = (torch.rand(B, 2, T, c.H, c.W, generator=g) * 6.0 - 0.93) * k
        I["w"] = torch.randn(32, 2, 3, 3, 3, generator=g) * (2.0 / 54) ** 0.5
        I["bias"] = 0.3 * torch.randn(32, generator=g) * 2.0 ** SCALE_EXP[0]
        return I
    up = c.kind.startswith("up")
    cin = c.C0 + c.C1
    I["x0"] = torch.randn(B, c.C0, T, *(((c.H + 1) // 2, (c.W + 1) // 2) if up else (c.H, c.W)), generator=g) * k
    if up:
        I["x1"] = torch.randn(B, c.C1, T, c.H, c.W, generator=g) * k
    I["w"] = torch.randn(Cout, cin, c.ks, c.ks, c.ks, generator=g) * (2.0 / (cin * c.ks ** 3)) ** 0.5
    I["scale"] = torch.rand(Cout, generator=g) + 0.5
    I["shift"] = 0.3 * torch.randn(Cout, generator=g) * 2.0 ** SCALE_EXP[0]
    if c.res:
        lo = c.kind == "wt_tail"                         # a low-resolution residual read at (h >> 1, w >> 1)
        I["res"] = torch.randn(B, Cout, T, *(((Ho + 1) // 2, (Wo + 1) // 2) if lo else (Ho, Wo)), generator=g) * k
    if c.kind in ("sc", "up_sc"):
        I["wd"] = torch.randn(Cout, cin, 1, 1, 1, generator=g) * (1.0 / cin) ** 0.5
        I["scale2"] = torch.rand(Cout, generator=g) + 0.5
        I["shift2"] = 0.3 * torch.randn(Cout, generator=g) * 2.0 ** SCALE_EXP[0]
    if c.tc:
        I["tx"] = torch.randn(B, c.tc, T, Ho, Wo, generator=g) * k
        I["wd"] = torch.randn(Cout, c.tc, 1, 1, 1, generator=g) * (1.0 / c.tc) ** 0.5
    if c.kind == "pred":
        I["wp"] = torch.randn(HEAD_CH, 32, generator=g) * 0.2
        I["bp"] = torch.randn(HEAD_CH, generator=g) * 0.1 * 2.0 ** SCALE_EXP[0]
    return I


def _upsample(x0, hw):
    from oracle import unet as U
    return U.upsample_nearest_hw(x0, hw).double()


def reference(c, I, pos):
    """f64 outputs of the case at the positions: {"y": [N, C], "y2": [N, C] (the fused shortcut)}."""
    col = lambda v: v.double().view(1, -1)
    if c.kind == "head":
        return {"y": F.leaky_relu(conv_at(I["x"], I["w"], 1, pos) + col(I["bias"]), 0.01)}
    x = I["x0"].double()
    if c.kind.startswith("up"):
        x = torch.cat([_upsample(I["x0"], (c.H, c.W)), I["x1"].double()], dim=1)
    w = I["w"]
    if c.kind == "up_part":                   # the upsampled channels' share only
        w = w.clone()
        w[:, c.C0:] = 0
    acc = conv_at(x, w, c.s, pos)
    if c.tc:
        acc = acc + conv_at(I["tx"], I["wd"], 1, pos)
    y = acc * col(I["scale"]) + col(I["shift"])
    if c.res:
        b, t, h, ww = pos
        r = I["res"].double()
        y = y + (r[b, :, t, h >> 1, ww >> 1] if c.kind == "wt_tail" else r[b, :, t, h, ww])
    out = {"y": y if c.kind == "up_part" else torch.relu(y)}
    if c.kind in ("sc", "up_sc"):
        out["y2"] = conv_at(x, I["wd"], c.s, pos) * col(I["scale2"]) + col(I["shift2"])
    if c.kind == "pred":
        out["y"] = torch.relu(out["y"] @ I["wp"].double().t() + col(I["bp"]))
    return out


def test_conv_at_equals_conv3d():
    """The gathered-patch f64 reference equals F.conv3d (double) at every position, 3x3x3 and 1x1x1, strides 1 and 2."""
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 16, 5, 9, 11, generator=g)
    for k, s in ((3, 1), (3, 2), (1, 1), (1, 2)):
        w = torch.randn(8, 16, k, k, k, generator=g)
        full = F.conv3d(x.double(), w.double(), None, (1, s, s), k // 2)
        B, C, T, Ho, Wo = full.shape
        pos = tuple(torch.from_numpy(v.ravel()) for v in np.meshgrid(np.arange(B), np.arange(T), np.arange(Ho), np.arange(Wo), indexing="ij"))
        assert torch.allclose(conv_at(x, w, s, pos), _at(full, pos), rtol=1e-12, atol=1e-12)
    p = positions(3, 16, 20, 30, 0)
    assert all(v.numel() == p[0].numel() for v in p) and set(p[0].tolist()) == {0, 1, 2}


# ------------------------------------------------------------------------------------------------
# the launches, through the model's entry points
# ------------------------------------------------------------------------------------------------
def _btchw(x):
    return x.permute(0, 2, 1, 3, 4).contiguous()


def _model(B):
    from v2ce_toolbox_amd.v2ce_3d import V2ce3d
    m = V2ce3d.__new__(V2ce3d)
    torch.nn.Module.__init__(m)
    m._maps, m.precision, m._slot = {}, "f16x2", 0
    m._prep = {"absmax": torch.zeros((4, B, 2), device="cuda")}       # one range slot per sequence
    m.profile = []
    return m


def _dev(x, pitch=False):
    """CPU NCDHW -> device channels-last-16 with per-sequence max |x| slots ([B, 2], max in column 0); pitch: rows of the
    activations' row pitch (padding zero)."""
    from v2ce_toolbox_amd.v2ce_3d import V2ce3d
    d = V2ce3d.to_c16(_btchw(x).cuda())
    W = x.shape[-1]
    Wp = V2ce3d._pitch(W)
    if pitch and Wp != W:
        p = torch.zeros((*d.shape[:4], Wp, 16), device="cuda")
        p[:, :, :, :, :W] = d
        p.lw, p.c16 = W, True
        d = p
    am = torch.zeros((x.shape[0], 2))
    am[:, 0] = x.abs().amax(dim=(1, 2, 3, 4))
    d.absmax = am.cuda()
    return d


def _pred_table(wp):
    from v2ce_toolbox_amd import hip
    tab = torch.empty(hip.lib().v2ce_pack_pred_weights_f16x2_bytes() // 2, dtype=torch.float16, device="cuda")
    wpd = wp.cuda().contiguous()
    hip.check(hip.lib().v2ce_pack_pred_weights_f16x2(wpd.data_ptr(), wp.shape[0], 32, tab.data_ptr(), hip.stream_ptr(wpd.device)), "pack")
    return tab, torch.zeros(32, device="cuda")


def launch(c, I):
    """Runs the case's launch on the batch in I: {"y": NCDHW float32 numpy, "y2": (fused shortcut), "slot": [B, 2] of the
    output's range slot, "names": the profile's launches}."""
    from v2ce_toolbox_amd import hip
    from v2ce_toolbox_amd.v2ce_3d import V2ce3d
    B = I["k"].shape[0]
    m = _model(B)
    cu = lambda v: v.cuda().contiguous()
    relu = hip.ACT_RELU
    planar = lambda y: V2ce3d.to_planar(y).permute(0, 2, 1, 3, 4).cpu().numpy()
    out_slot = 0
    y2 = None
    if c.kind == "head":
        tab = torch.empty(hip.lib().v2ce_pack_head_weights_f16x2_bytes() // 2, dtype=torch.float16, device="cuda")
        hip.check(hip.lib().v2ce_pack_head_weights_f16x2(cu(I["w"]).data_ptr(), tab.data_ptr(), hip.stream_ptr("cuda")), "pack")
        y = planar(V2ce3d._head_split(m, cu(_btchw(I["x"])), tab, cu(I["bias"])))
        out_slot = 1
    elif c.kind.startswith("up"):
        buf = V2ce3d._split_buffer(c.Cout, c.C0 + c.C1, 27, "cuda", up_c0=c.C0)
        wq = V2ce3d._pack(m, cu(I["w"]), None, buf, split=True)
        x0, x1 = _dev(I["x0"]), _dev(I["x1"])
        if c.kind == "up_part":
            y = planar(V2ce3d._conv_up_part(m, x0, x1, wq, cu(I["scale"]), cu(I["shift"]), c.Cout, (c.H, c.W)))
        else:
            sc = (V2ce3d._pack(m, cu(I["wd"]), split=True), cu(I["scale2"]), cu(I["shift2"])) if c.kind == "up_sc" else None
            r = V2ce3d._conv(m, x0, x1, wq, cu(I["scale"]), cu(I["shift"]), c.Cout, 3, 1, relu, up_to=(c.H, c.W), split=True,
                             dense_out=True, sc=sc)
            y, y2 = (planar(r[0]), planar(r[1])) if sc is not None else (planar(r), None)
    else:
        wt = c.kind.startswith("wt")
        if wt:
            buf = V2ce3d._split_buffer(c.Cout, c.C0, 27, "cuda", wt=True)
            wq = V2ce3d._pack(m, cu(I["w"]), None, buf, split=True)
        else:
            wq = V2ce3d._pack(m, cu(I["w"]), split=True)
        pred = c.kind == "pred"
        kw = dict(split=True, dense_out=not pred)
        if c.res:
            kw["residual"] = _dev(I["res"], pitch=pred)
            kw["residual_up"] = c.kind == "wt_tail"
        if c.tc:
            kw["tail"] = (_dev(I["tx"]), None, None, 1, V2ce3d._pack(m, cu(I["wd"]), split=True))
        if c.kind == "sc":
            kw["sc"] = (V2ce3d._pack(m, cu(I["wd"]), split=True), cu(I["scale2"]), cu(I["shift2"]))
        if pred:
            tab, bias = _pred_table(I["wp"])
            bias[:HEAD_CH] = cu(I["bp"])
            kw["pred"] = (tab, bias, HEAD_CH)
        r = V2ce3d._conv(m, _dev(I["x0"], pitch=pred), None, wq, cu(I["scale"]), cu(I["shift"]), c.Cout, c.ks, c.s, relu, **kw)
        if c.kind == "sc":
            y, y2 = planar(r[0]), planar(r[1])
        elif pred:
            y = r.permute(0, 2, 1, 3, 4).cpu().numpy()
        else:
            y = planar(r)
    torch.cuda.synchronize()
    return {"y": y, "y2": y2, "slot": m._prep["absmax"][out_slot].cpu().numpy(), "names": [p[0] for p in m.profile]}


def _sub(I, b):
    """The inputs of sequence b alone (shared tensors as they are)."""
    return {k: (v[b:b + 1].contiguous() if k in ("k", "x", "x0", "x1", "res", "tx") else v) for k, v in I.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("case", WALK_CASES, ids=lambda c: c.id)
def test_walk_vs_f64(case, capfd, monkeypatch):
    if case.kind.startswith("wt"):
        monkeypatch.setenv("V2CE_WT_VERBOSE", "1")     # the box line: tiles and positions, for the walk order below
    I = _inputs(case)
    got = launch(case, I)
    assert got["names"] == [case.name], got["names"]
    Ho, Wo = case.out_hw
    B, T = case.B, case.T
    full = B * T * Ho * Wo * case.Cout * (case.C0 + case.C1) * case.ks ** 3 < 1.2e10
    pos = positions(B, T, Ho, Wo, zlib.crc32(case.name.encode()) & 0xFFFF, frac=1.0 if full else 0.12)
    want = reference(case, I, pos)
    k = I["k"].view(-1).double()[pos[0]].view(-1, 1)
    worst, dmax = -1.0, 0.0
    for key in ("y", "y2"):
        if key not in want:
            continue
        a = torch.from_numpy(got[key]).double()
        g_, w_ = _at(a, pos) / k, want[key] / k
        assert g_.shape == w_.shape
        d = (g_ - w_).abs()
        excess = d - TOL * w_.abs()
        i = int(torch.argmax(excess.max(dim=1).values))
        j = int(torch.argmax(excess[i]))
        where = (int(pos[0][i]), j, int(pos[1][i]), int(pos[2][i]), int(pos[3][i]))
        assert float(excess[i, j]) <= TOL, (f"{case.id} {key}: max excess at (b, c, t, h, w) = {where}: got {float(g_[i, j])!r} "
                                            f"want {float(w_[i, j])!r} (unit scale)")
        worst, dmax = max(worst, float(excess[i, j])), max(dmax, float(d.max()))
    # the range slots: max |y| of each sequence (where the launch materialises y) and a finite guard bound
    slot = got["slot"]
    for b in range(B):
        assert np.isfinite(slot[b, 1]) and slot[b, 1] > 0, (b, slot[b])
        if case.kind != "pred":
            ymax = float(np.abs(got["y"][b]).max())
            assert abs(float(slot[b, 0]) - ymax) <= 1e-6 * ymax, (b, float(slot[b, 0]), ymax)
    if case.kind.startswith("wt"):
        # the walk order the dispatcher took: channel-tile-major (xcd_remap 2) where the weights outweigh the XCD's input
        line = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("[wt<")][-1]
        n_pos = int(line.split("(")[1].split(" of ")[0])
        blocks = int(line.rsplit(",", 1)[1].split()[0])
        n_co = case.co_tiles()
        per_xcd = blocks // (8 * n_co)
        remap = 2 if 64 * case.C0 * 36 * 4 * n_co > per_xcd * n_pos * 2 * case.C0 * 4 else 1
        assert remap == (2 if case.Cout == 320 else 1), line
    # batch invariance: each sequence alone gives its rows bit for bit
    for b in range(B):
        alone = launch(case, _sub(I, b))
        for key in ("y", "y2"):
            if got[key] is not None:
                assert np.array_equal(alone[key][0].view(np.int32), got[key][b].view(np.int32)), (case.id, key, b)
    print(f"WALK {case.id} {case.name} tiles>={case.tile_bound()} co_tiles={case.co_tiles()} "
          f"positions={pos[0].numel()}/{B * T * Ho * Wo} max|d|={dmax:.3e} max_excess={worst:.3e}")


@pytest.mark.gpu
def test_network_instances_are_covered():
    """One default forward at 346 x 260, T = 16, B = 1, 4, 8 (8: the per-tile batch of the panorama config): every conv
    instance it launches has a row in WALK_CASES -- a new or renamed instance fails here until it gets one."""
    from oracle import glue as OG
    from v2ce_toolbox_amd import synth
    from v2ce_toolbox_amd.v2ce_3d import V2ce3d
    table = {c.name for c in WALK_CASES}
    x1 = OG.preprocess(synth.synthetic_frames(17, 260, 346, seed=9))
    m = V2ce3d()
    m.load_state_dict(synth.make_state_dict(0))
    m = m.eval().to("cuda")
    for B in (1, 4, 8):
        x = torch.from_numpy(np.stack([x1] * B)).cuda()
        m.profile = []
        with torch.no_grad():
            m(x)
        torch.cuda.synchronize()
        names = {p[0] for p in m.profile}
        assert names and names <= table, (B, sorted(names - table))
