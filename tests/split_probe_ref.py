"""Exact-arithmetic probes of the split-half forward convolutions: the case table, the data, a restatement of
the split-half evaluation in f64, and the f64 truth.  tests/test_split_probe_cpu.py proves the data's conditions and shows on
the restatement which probe catches which fault; tests/test_gpu_split_probes.py runs the kernels.

A split-half launch pre-scales every f32 operand by a power of two, splits it into two fp16 halves hi = fp16(v s),
lo = fp16(v s - hi), forms w_h x_h + w_h x_l + w_l x_h on the fp16 MFMA and sums in f32.  On data with

  (a) every operand that a kernel or packer splits exactly hi + lo (at most 22 significant bits below the tensor's maximum),
  (b) in every product one factor with a zero lo half (the dropped w_l x_l is then zero),
  (c) for every output  sum |w| |x| + |shift| + |res|  below 2^24 units of its smallest bit,

every product and every partial sum is an exact f32 in any order, so the launch must return the f64 truth rounded to f32 --
which IS the truth -- in every element.  The operands are the ones the kernels really split: the Winograd-T D_j / G_j and
the tail's half sums and differences (4.1g), the phase-folded weight sums and their odd-size correction lists (4.1e), the
fused head's intermediate y at its per-position pre-scale (4.1j).

PROBE_CASES has one row per row of test_gpu_tile_walk.WALK_CASES: the same instance, kind, kernel size, stride, channel
counts and residual flag, T = 3 (a Winograd pair and a half pair), B = 2 with sequence 1 = 2^8 x sequence 0, and the
smallest odd plane (searched over (n, n + 2), (n + 2, n), (n, n + 4)) at which the dispatcher keeps the instance and every
box the host side can choose (candidate_boxes restates conv3d.hip choose_tile, conv3d_wt.hip choose_wt_box and the
rounds / blocks filter of conv3d_up.hip choose_up_cfg, whose last tie-break on LDS conflicts is not restated: all its
candidates are checked) gives at least two boxes along H and along W with ragged last ones.

Probes (seeded per row).  scale / scale2 cycle through 0.5, 1, 2, 4 per channel (a wrong channel index in the epilogue
changes the value); shift, bias and the residual are small signed integers.  The BN shift and the head bias are shared by
the batch, so they are multiples of 2^8: an integer of sequence 1's units (at unit size they would sit eight bits below
sequence 1's products and cost condition (c) those eight bits).  The check "sequence 1 = 2^8 x sequence 0" therefore runs
against a launch of sequence 0 whose shift is scaled down by 2^8 (inputs_p0_unit_shift): that is the scaled problem.
  P1  x and w dense signed integers of three bits, no zero in w: only hi halves.
  P2  x odd integers of 12-18 bits (per-row width, widths()), every x_l != 0; w in {-1, 0, +1}, a fixed number of non-zeros
      per output channel whose positions tile (channel, tap) so that every (tap, input channel) is hit.
  P3  w (and wd, wp, the head's weights) odd integers of 12-18 bits; x in {-1, 0, +1} at a density that keeps (c).  The
      fused head (pred) multiplies its intermediate y by wp: for (b) y must have a zero lo half, so the pred rows keep w
      in [-3, 3] without a BN shift and put the wide integers into wp alone.
  P3w the pred rows' second half of P3: w odd integers of 12-13 bits, x as in P3, wp in {-1, 0, +1} (four per head channel):
      the lo plane of the main packed weight and the w_l x_h stream of the two pred instances themselves.
  P4  standard normals, shift = bias = 0, the same unit data at 2^-8, 1, 2^8 (p4_batches): rows bitwise scaled.

Head (conv3d_head.hip, read for this): y = acc * inv + bias, then fmaxf(y, slope * y) + 0 with slope the f32 0.01f -- the
arithmetic of apply_act.  The truth's negative side is therefore the exact pre-activation times float32(0.01), rounded once."""
import math
import os
import sys
import zlib

import numpy as np
import torch
import torch.nn.functional as F

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
for p in (TESTS, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

from conv_ref import conv_at  # noqa: E402
from test_gpu_f32_conv import choose_tile  # noqa: E402
from test_gpu_tile_walk import HEAD_CH, N_CU, WALK_CASES, Case, _sub, _variant, launch, reference  # noqa: E402,F401

T_PROBE, B_PROBE, SEQ_EXP = 3, 2, 8
P4_EXP = (-8, 0, 8)
SCALES = (0.5, 1.0, 2.0, 4.0)
SLOPE = float(np.float32(0.01))

# instance -> (H, W) of the probe (the search described above; test_split_probe_cpu.test_probe_table checks every row)
WS = "conv3d_f16x2_ws_kernel"
PROBE_HW = {
    WS + "<1,1,1,1,4,3,0,2,0>": (45, 43),
    WS + "<1,1,1,2,4,3,0,2,0>": (45, 43),
    WS + "<1,1,2,2,4,3,0,2,0>": (29, 33),
    WS + "<1,2,1,1,4,3,0,2,0>": (127, 129),
    WS + "<1,2,1,2,4,3,0,2,0>": (127, 129),
    WS + "<1,2,2,2,4,3,0,2,0>": (75, 73),
    WS + "<3,1,1,1,4,3,0,0,0>": (29, 31),
    WS + "<3,1,1,1,4,3,0,1,0>": (29, 31),
    WS + "<3,1,1,2,4,3,0,0,0>": (29, 31),
    WS + "<3,1,1,2,4,3,0,2,0>": (29, 31),
    WS + "<3,1,2,2,4,3,0,0,0>": (53, 55),
    WS + "<3,1,2,2,4,3,0,2,0>": (53, 55),
    WS + "<3,1,2,2,3,3,0,0,0>": (31, 33),
    WS + "<3,1,2,2,3,3,0,2,0>": (31, 33),
    WS + "<3,2,1,1,1,3,0,2,0>": (51, 49),
    WS + "<3,2,2,1,2,3,0,2,0>": (51, 49),
    WS + "<3,2,4,1,4,3,0,2,0>": (51, 49),
    WS + "<3,1,1,1,4,3,2,0,0>": (29, 31),
    WS + "<3,2,1,1,1,3,2,0,0>": (51, 49),
    WS + "<3,2,2,1,2,9,2,0,0>": (51, 49),
    WS + "<3,2,4,1,4,3,2,0,0>": (51, 49),
    WS + "<3,1,1,1,4,9,1,1,1>": (29, 27),
    WS + "<3,1,1,1,4,9,1,0,1>": (29, 27),
    WS + "<3,1,1,2,4,3,3,0,0>": (29, 31),
    WS + "<3,1,2,2,4,3,3,0,0>": (53, 55),
    WS + "<3,1,2,2,3,3,3,0,0>": (31, 33),
    "conv3d_wt_kernel<2,4,0,0>": (5, 7),
    "conv3d_wt_kernel<2,4,1,0>": (7, 9),
    "conv3d_wt_kernel<2,4,0,1>": (5, 7),
    "conv3d_wt_kernel<2,4,1,1>": (7, 9),
    "conv3d_up_kernel<1,1,4,2>": (33, 37),
    "conv3d_up_kernel<1,1,4,0>": (33, 37),
    # conv3d_up_kernel<1,2,4,0>: with T = 3 the dispatcher takes <1,2,2,0> at every plane: the row keeps its walk shape
    "conv3d_up_kernel<1,2,2,0>": (63, 65),
    "conv3d_up_kernel<2,2,4,0>": (43, 45),
    "conv3d_head_f16x2_kernel": (7, 67),
}

FULL_WALK_P1 = ("conv3d_f16x2_ws_kernel<3,1,2,2,4,3,0,2,0>", "conv3d_wt_kernel<2,4,1,1>", "conv3d_up_kernel<1,1,4,2>")


# ---------------------------------------------------------------------------------------------------------------------
# the boxes the host side can take

def _args(c):
    return [int(v) for v in c.name[c.name.index("<") + 1:-1].split(",")] if "<" in c.name else []


def choose_wt_box(B, T, H, W, n_co, n_cu, pos_tile, slot=256):
    """conv3d_wt.hip choose_wt_box: (pairs, th, tw, flat)."""
    pairs = (T + 1) // 2
    best, best_cost = (0, 0, 0, 0), 1e30
    for pp in range(1, min(pairs, 16) + 1):
        n_max = pos_tile // pp
        if n_max < 1:
            break
        nR = -(-H * W // n_max)
        n = -(-H * W // nR)
        rows = min(H, (W - 1 + n - 1) // W + 1)
        if pp * (rows + 2) * (W + 2) > slot:
            continue
        nsp = B * -(-pairs // pp) * nR
        blocks = 8 * -(-nsp // 8) * n_co
        cost = float(-(-blocks // n_cu)) * (1.0 + 0.15 * pp * (rows + 2) * (W + 2) / slot) + 1e-3 * blocks / n_cu
        if cost < best_cost:
            best_cost, best = cost, (pp, rows, W, n)
    for pp in range(1, min(pairs, 16) + 1):
        for th in range(1, min(H, 64) + 1):
            for tw in range(1, min(W, 128) + 1):
                if pp * th * tw > pos_tile or pp * (th + 2) * (tw + 2) > slot:
                    continue
                nsp = B * -(-pairs // pp) * -(-H // th) * -(-W // tw)
                blocks = 8 * -(-nsp // 8) * n_co
                cost = float(-(-blocks // n_cu)) * (1.0 + 0.15 * pp * (th + 2) * (tw + 2) / slot) + 1e-3 * blocks / n_cu
                if cost < best_cost - 1e-9:
                    best_cost, best = cost, (pp, th, tw, 0)
    return best


def up_candidates(B, T, Ho, Wo, n_sub_max, n_co, n_cu):
    """conv3d_up.hip choose_up_cfg up to its tie-break: the (tt, TH, TW) boxes with the fewest rounds and within 3 % of the
    fewest blocks (the LDS-conflict search picks one of them)."""
    cands = []
    tt = 1
    while tt <= 16 and tt <= (2 * T - 1 if T > 1 else 1):
        sh = 1
        while sh <= 64 and 2 * (sh - 1) < Ho:
            sw = 1
            while sw <= 64 and 2 * (sw - 1) < Wo:
                if tt * sh * sw > n_sub_max or (tt + 2) * (2 * sh + 2) * (2 * sw + 2) > 1152:
                    break
                nsp = B * -(-T // tt) * -(-Ho // (2 * sh)) * -(-Wo // (2 * sw))
                blocks = 8 * -(-nsp // 8) * n_co
                cands.append((-(-blocks // n_cu), blocks, tt, 2 * sh, 2 * sw))
                sw += 1
            sh += 1
        tt *= 2
    rounds = min(k[0] for k in cands)
    blocks = min(k[1] for k in cands if k[0] == rounds)
    return [k[2:] for k in cands if k[0] == rounds and k[1] * 100 <= blocks * 103]


def candidate_boxes(c):
    """Every (tt, th, tw) output box the launch of the row can take (th = 0: flat ranges of the plane)."""
    a = _args(c)
    Ho, Wo = c.out_hw
    if c.kind == "head":
        return [(4, 4, 64)]
    if c.name.startswith("conv3d_f16x2_ws_kernel"):
        ks, s, wco, po_fr, opt = a[0], a[1], a[2], a[4], a[8]
        return [choose_tile(c.T, Ho, Wo, ks, 1 if ks == 1 else s, (4 // wco) * po_fr * 32, 1152 if opt else 1280)]
    if c.name.startswith("conv3d_wt_kernel"):
        pp, th, tw, flat = choose_wt_box(c.B, c.T, Ho, Wo, -(-c.Cout // (a[0] * 32)), N_CU, a[1] * 32)
        return [(2 * pp, 0 if flat else th, tw)]
    wco, co_fr, po_fr = a[0], a[1], a[2]
    return up_candidates(c.B, c.T, Ho, Wo, (po_fr // wco) * 32, -(-c.Cout // (wco * co_fr * 32)), N_CU)


def boxes_ok(c):
    """At least two boxes along H and along W, the last ones ragged, whichever candidate box the host takes."""
    Ho, Wo = c.out_hw
    return all(th > 0 and -(-Ho // th) >= 2 and -(-Wo // tw) >= 2 and Ho % th and Wo % tw for _, th, tw in candidate_boxes(c))


def _probe_row(c):
    H, W = PROBE_HW.get(c.name, (c.H, c.W))
    small = (H, W) != (c.H, c.W)
    return Case(c.name, c.kind, B_PROBE if small else c.B, T_PROBE if small else c.T, c.C0, c.Cout, H, W, ks=c.ks, s=c.s, res=c.res,
                C1=c.C1, tc=c.tc)


def probes_of(c):
    """The exact probes a row runs."""
    return ("P1", "P2", "P3", "P3w") if c.kind == "pred" else ("P1", "P2", "P3")


def probe_cases():
    return [_probe_row(c) for c in WALK_CASES]


# ---------------------------------------------------------------------------------------------------------------------
# data

def _seed(c, probe):
    return zlib.crc32(f"{c.name}/{probe}".encode()) & 0x7FFFFFFF


def shapes(c, U):
    """name -> shape of the case's tensors for U sequences (NCDHW; weights as the launch takes them)."""
    Ho, Wo = c.out_hw
    T = c.T
    if c.kind == "head":
        return {"x": (U, 2, T, c.H, c.W), "w": (32, 2, 3, 3, 3), "bias": (32,)}
    up = c.kind.startswith("up")
    cin = c.C0 + c.C1
    s = {"x0": (U, c.C0, T) + (((c.H + 1) // 2, (c.W + 1) // 2) if up else (c.H, c.W)), "w": (c.Cout, cin, c.ks, c.ks, c.ks),
         "scale": (c.Cout,), "shift": (c.Cout,)}
    if up:
        s["x1"] = (U, c.C1, T, c.H, c.W)
    if c.res:
        s["res"] = (U, c.Cout, T) + (((Ho + 1) // 2, (Wo + 1) // 2) if c.kind == "wt_tail" else (Ho, Wo))
    if c.kind in ("sc", "up_sc"):
        s.update(wd=(c.Cout, cin, 1, 1, 1), scale2=(c.Cout,), shift2=(c.Cout,))
    if c.tc:
        s.update(tx=(U, c.tc, T, Ho, Wo), wd=(c.Cout, c.tc, 1, 1, 1))
    if c.kind == "pred":
        s.update(wp=(HEAD_CH, 32), bp=(HEAD_CH,))
    return s


ACT = ("x", "x0", "x1", "tx")            # activations: wide in P2
WGT = ("w", "wd", "wp")                  # weights: wide in P3
AMP = {"wt": 8, "wt_tail": 8, "up": 2, "up_sc": 2, "up_part": 2}      # sum |operand products| over sum |w| |x| (transforms, folds)


def nnz_of(cout, k):
    """Non-zeros per output channel of a P2 weight: enough to tile all k (channel, tap) columns over the output channels."""
    return max(3, -(-k // cout))


def widths(c):
    """Per-row widths and densities (chosen from the term counts so that (a)-(c) hold; the CPU test proves they do)."""
    k = (c.C0 + c.C1) * c.ks ** 3 if c.kind != "head" else 54
    amp = AMP.get(c.kind, 1)
    n2 = nnz_of(c.Cout, k) + (nnz_of(c.Cout, c.tc) if c.tc else 0)
    hi2 = min(18, 21 - math.ceil(math.log2(n2 * amp)))
    hits = 6.0                                           # expected non-zero x per output in P3
    if c.kind in ("sc", "up_sc"):                        # the shortcut sees one tap: four of its cin columns are to be live
        hits = 4.0 * c.ks ** 3
    n3 = hits + 6.0 * hits ** 0.5 + (6.0 if c.tc else 0.0)
    hi3 = min(18, 21 - math.ceil(math.log2(n3 * amp)))
    live = k                                             # columns an output really sees: 12 folded taps per upsampled channel
    if c.kind.startswith("up"):
        live = 12 * c.C0 + (0 if c.kind == "up_part" else 27 * c.C1)
    w = {"p2": (max(12, hi2 - 4), hi2), "p3": (max(12, hi3 - 4), hi3), "rho": min(0.5, hits / live), "rho_t": min(0.5, 3.0 / max(c.tc, 1))}
    if c.kind == "pred":                                 # y <= 2^20 into a second stage of four non-zeros; wp wide alone in P3
        w["p2"] = (12, 14)
        w["p3"] = (12, 13)
    return w


def _ints(g, shape, lo, hi, nonzero=False):
    v = torch.randint(lo, hi + 1, shape, generator=g)
    if nonzero:
        v = torch.where(v == 0, torch.full_like(v, hi), v)
    return v.float()


def _wide(g, shape, bits):
    """Odd integers of bits[0] .. bits[1] significant bits, random sign."""
    b = torch.randint(bits[0], bits[1] + 1, shape, generator=g)
    top = torch.ones_like(b) << (b - 1)
    m = top + (torch.rand(shape, generator=g, dtype=torch.float64) * top.double()).long().clamp_(max=(1 << 24))
    m = torch.minimum(m, 2 * top - 1) | 1
    sign = torch.randint(0, 2, shape, generator=g) * 2 - 1
    return (m * sign).float()


def _sparse_pm1(g, shape, nnz=None):
    """{-1, 0, +1} weights [Cout, ...]: nnz non-zeros per output channel, placed as consecutive windows of a seeded permutation
    of the K columns, so that the Cout windows cover every column."""
    cout, k = shape[0], int(np.prod(shape[1:]))
    nnz = nnz_of(cout, k) if nnz is None else nnz
    perm = torch.randperm(k, generator=g)
    idx = perm[(torch.arange(cout).view(-1, 1) * nnz + torch.arange(nnz).view(1, -1)) % k]
    sign = (torch.randint(0, 2, idx.shape, generator=g) * 2 - 1).float()
    return torch.zeros(cout, k).scatter_(1, idx, sign).view(shape)


def _trits(g, shape, rho):
    u = torch.rand(shape, generator=g)
    return torch.where(u < rho / 2, -1.0, torch.where(u < rho, 1.0, 0.0)).float()


def _batch(I, k):
    """Unit sequences -> the batch: sequence b is unit sequence (b mod U) times k[b]."""
    kk = torch.tensor(k, dtype=torch.float32).view(-1, 1, 1, 1, 1)
    out = {"k": kk}
    for name, v in I.items():
        if name in ACT + ("res",):
            v = torch.cat([v[b % v.shape[0]:b % v.shape[0] + 1] for b in range(len(k))]) * kk
        out[name] = v.contiguous()
    return out


def unit_inputs(c, probe, U=1):
    """The probe's CPU float32 tensors for U unit-scale sequences (P1-P3)."""
    g = torch.Generator().manual_seed(_seed(c, probe))
    wd = widths(c)
    I = {}
    for name, shp in shapes(c, U).items():
        if name in ("scale", "scale2"):
            off = 0 if name == "scale" else 1
            I[name] = torch.tensor([SCALES[(i + off) % 4] for i in range(shp[0])])
        elif name == "shift" and c.kind == "pred" and probe == "P3":
            I[name] = torch.zeros(shp)                   # (2^8 in each of y's 32 channels times a 13-bit wp would break (c))
        elif name in ("shift", "shift2", "bias", "bp"):
            I[name] = _ints(g, shp, -3, 3) * 2.0 ** SEQ_EXP
        elif name == "res":
            I[name] = _ints(g, shp, -3, 3)
        elif probe == "P1":
            I[name] = _ints(g, shp, -7, 7, nonzero=name in WGT)
        elif probe == "P2":
            if name in ACT:
                I[name] = _wide(g, shp, wd["p2"])
            else:
                I[name] = _sparse_pm1(g, shp, 4 if name == "wp" else None)
        else:                                             # P3; P3w (pred rows): w wide and wp in {-1, 0, +1} instead
            assert probe == "P3" or (probe == "P3w" and c.kind == "pred"), probe
            narrow_w = c.kind == "pred" and name == "w" and probe == "P3"
            if name in ACT:
                I[name] = _trits(g, shp, wd["rho_t"] if name == "tx" else wd["rho"])
            elif narrow_w:
                I[name] = _ints(g, shp, -3, 3, nonzero=True)
            elif probe == "P3w" and name == "wp":
                I[name] = _sparse_pm1(g, shp, 4)
            else:
                I[name] = _wide(g, shp, wd["p3"])
    return I


def inputs(c, probe):
    """The batch of P1-P3: B = 2, sequence 1 = 2^8 x sequence 0 (rows at their walk shape: independent unit sequences at
    1, 2^8, 1, so that a walk switches pre-scale twice)."""
    if c.B == B_PROBE:
        return _batch(unit_inputs(c, probe, 1), [1.0, 2.0 ** SEQ_EXP])
    return _batch(unit_inputs(c, probe, c.B), [2.0 ** (SEQ_EXP * (b % 2)) for b in range(c.B)])


def inputs_p0_unit_shift(c, probe):
    """Sequence 0 alone with every shared additive term divided by 2^8: 2^-8 times the problem of sequence 1."""
    I = _sub(inputs(c, probe), 0)
    return {k: (v * 2.0 ** -SEQ_EXP if k in ("shift", "shift2", "bias", "bp") else v) for k, v in I.items()}


def p4_batches(c):
    """The exponent tuples of P4's launches.  The dispatch depends on the batch size, so a row of B = 2 runs (2^-8, 1) and
    (1, 2^8) in two launches of its own batch size: each holds the unit row."""
    return [P4_EXP] if c.B == len(P4_EXP) else [P4_EXP[:2], P4_EXP[1:]]


def inputs_p4(c, exps=P4_EXP):
    """Standard normals at the walk's weight scaling, no additive terms; sequence b = unit data x 2^exps[b]."""
    g = torch.Generator().manual_seed(_seed(c, "P4"))
    I = {}
    for name, shp in shapes(c, 1).items():
        if name in ("scale", "scale2"):
            I[name] = torch.rand(shp, generator=g) + 0.5
        elif name in ("shift", "shift2", "bias", "bp"):
            I[name] = torch.zeros(shp)
        elif name in WGT:
            I[name] = torch.randn(shp, generator=g) * (2.0 / int(np.prod(shp[1:]))) ** 0.5
        else:
            I[name] = torch.randn(shp, generator=g)
    return _batch(I, [2.0 ** e for e in exps])


# ---------------------------------------------------------------------------------------------------------------------
# truth

def all_positions(B, T, Ho, Wo, device="cpu"):
    g = torch.meshgrid(torch.arange(B), torch.arange(T), torch.arange(Ho), torch.arange(Wo), indexing="ij")
    return tuple(v.reshape(-1).to(device) for v in g)


def truth(c, I, device="cpu"):
    """f64 outputs of the batch at every position: {"y": [B, C, T, Ho, Wo] (, "y2")} on `device`."""
    J = {k: v.to(device) for k, v in I.items()}
    B = J["k"].shape[0]
    Ho, Wo = c.out_hw
    pos = all_positions(B, c.T, Ho, Wo, device)
    if c.kind == "head":
        pre = conv_at(J["x"], J["w"], 1, pos) + J["bias"].double().view(1, -1)
        out = {"y": torch.where(pre < 0, pre * SLOPE, pre)}
    else:
        out = reference(c, J, pos)
    return {k: v.view(B, c.T, Ho, Wo, -1).permute(0, 4, 1, 2, 3).contiguous() for k, v in out.items()}


# ---------------------------------------------------------------------------------------------------------------------
# the restatement of the split-half evaluation (sequence 0 of a batch, every position, f64 holding exact f32 values)

def pow2_prescale(amax):
    """common.h pow2_prescale: the power of two s with amax * s in [2^14, 2^15)."""
    if not amax > 0:
        return 1.0
    return 2.0 ** (15 - math.frexp(float(np.float32(amax)))[1])


def split(v, s, hi_bits=11):
    """hi = fp16(v s), lo = fp16(v s - hi) as f64, and whether hi + lo == v s everywhere.  hi_bits = 10: the mutant whose hi
    plane keeps ten significant bits (lo is still formed against the 11-bit hi)."""
    vs = (v.double() * s).float()
    assert torch.equal(vs.double(), v.double() * s)
    hi = vs.half().float()
    lo = (vs - hi).half().float()
    exact = bool(torch.equal(hi + lo, vs)) and bool(torch.isfinite(hi).all())
    if hi_bits == 10:
        m, e = torch.frexp(hi.double())
        hi = torch.ldexp(torch.round(m * 1024.0) / 1024.0, e).float()
    return hi.double(), lo.double(), exact


def _lsb(v):
    """The smallest set bit over the non-zero elements (multiples of 1/4 here), 1 if all are zero."""
    q = (v.double().abs() * 4.0)
    assert torch.equal(q, q.round())
    q = q[q != 0].long()
    return float((q & -q).min()) / 4.0 if q.numel() else 1.0


class Model:
    """Accumulates the streams of one launch: acc (at unit scale), sum |w| |x|, the smallest product bit, the conditions."""

    def __init__(self, mut=None):
        self.mut = mut or {}
        self.a = self.b = True
        self.unit = 1.0
        self.lo_x = self.lo_w = 0           # operand elements with a non-zero lo half
        self.notes = []

    def mm(self, W, X, ws, xs, k3, main=False, lo_swap=None):
        """X [N, K] against W [Cout, K] (column = channel * k3 + tap): (acc, sum |w| |x|) [N, Cout]."""
        bits = 10 if self.mut.get("hi10") else 11
        wh, wl, ea = split(W, ws, bits)
        xh, xl, eb = split(X, xs, bits)
        if lo_swap is not None:
            wl = split(lo_swap, ws, bits)[1]
        self.a = self.a and ea and eb
        if not (ea and eb):
            self.notes.append(("a", tuple(W.shape), tuple(X.shape), ea, eb))
        if bool(((xl != 0).double() @ (wl != 0).double().t()).any()):
            self.b = False
        self.lo_x += int((xl != 0).sum())
        self.lo_w += int((wl != 0).sum())
        self.unit = min(self.unit, _lsb(W) * _lsb(X))
        col = torch.arange(W.shape[1])
        if main and "drop_whxl_chunk" in self.mut:
            xl = xl * ((col // k3) // 16 != self.mut["drop_whxl_chunk"]).double()
        if main and "drop_wlxh_tap" in self.mut:
            wl = wl * (col % k3 != self.mut["drop_wlxh_tap"] % k3).double()
        acc = (xh @ wh.t() + xl @ wh.t() + xh @ wl.t()) / (ws * xs)
        return acc, X.double().abs() @ W.double().abs().t()


def _gather(x, k, stride, pos, pad=None):
    """x [C, T, H, W] -> [N, C * k^3] patches at the output positions (t, h, w), zero padded."""
    p = k // 2 if pad is None else pad
    xp = F.pad(x.double(), (p, p, p, p, p, p))
    t, h, w = pos
    cols = torch.stack([xp[:, t + dt, h * stride + dh, w * stride + dw] for dt in range(k) for dh in range(k) for dw in range(k)], dim=2)
    return cols.permute(1, 0, 2).reshape(t.numel(), -1)


def _amax(*v):
    return max(float(t.abs().max()) for t in v)


def _fold2(w, axis, phase):
    """Phase fold of a 3-tap axis into 2 (4.1e): even phase {w[-1], w[0] + w[+1]}, odd phase {w[-1] + w[0], w[+1]} (f32 sums)."""
    a, b, c = (w.select(axis, i).float() for i in range(3))
    return torch.stack([a, b + c] if phase == 0 else [a + b, c], dim=axis)


def model(c, I, mut=None):
    """The launch of sequence 0 of the batch I as the kernels evaluate it: {"y": [C, T, Ho, Wo] f64 (, "y2"), "cond": {...}}.
    mut (the CPU test's mutants): "hi10" acts on every split of the launch; "drop_whxl_chunk" / "drop_wlxh_tap" on the main
    K loop only (not on a tail, a fused shortcut, the correction lists or the fused head's second stage); "swap_G12_lo" on the
    Winograd-T weights."""
    M = Model(mut)
    J = _sub(I, 0)
    Ho, Wo = c.out_hw
    T = c.T
    pos = tuple(v for v in all_positions(1, T, Ho, Wo)[1:])
    col = lambda v: v.double().view(1, -1)
    res_abs = 0.0
    y2 = None
    if c.kind == "head":
        x, w = J["x"][0], J["w"]
        acc, s = M.mm(w.reshape(32, -1), _gather(x, 3, 1, pos), pow2_prescale(_amax(w)), pow2_prescale(_amax(x)), 27, main=True)
        scale, shift = torch.ones(32), J["bias"]
    elif c.kind.startswith("wt"):
        x, w = J["x0"][0], J["w"]
        ws, xs = pow2_prescale(1.5 * _amax(w)), pow2_prescale(2.0 * _amax(x))
        if c.tc:
            tx, wd = J["tx"][0], J["wd"].reshape(c.Cout, -1)
            wts, ts = pow2_prescale(_amax(wd)), pow2_prescale(_amax(tx))
            S = min(xs * ws, ts * wts)               # one accumulator scale for both parts
            xs, ts = S / ws, S / wts
        g0, g1, g2 = (w[:, :, i].float() for i in range(3))
        G = [g0, ((g0 + g1) + g2) * 0.5, ((g0 - g1) + g2) * 0.5, g2]
        Gl = [G[0], G[2], G[1], G[3]] if M.mut.get("swap_G12_lo") else G
        pairs = (T + 1) // 2
        xp = F.pad(x.float(), (0, 0, 0, 0, 1, 2))                        # time steps -1 .. T + 1
        acc = torch.zeros(T + 1, Ho * Wo, c.Cout, dtype=torch.float64)
        s = torch.zeros_like(acc)
        hw = tuple(v.reshape(-1) for v in torch.meshgrid(torch.arange(Ho), torch.arange(Wo), indexing="ij"))
        z = torch.zeros_like(hw[0])

        def plane(v):                                                # [C, H, W] -> [Ho Wo, C * 9]: the 3 x 3 (H, W) patches
            vp = F.pad(v.double(), (1, 1, 1, 1))
            return torch.stack([vp[:, hw[0] + dh, hw[1] + dw] for dh in range(3) for dw in range(3)], dim=2).permute(1, 0, 2).reshape(z.numel(), -1)

        for p in range(pairs):
            d = [xp[:, 2 * p + i] for i in range(4)]
            D = [d[0] - d[2], d[1] + d[2], d[2] - d[1], d[1] - d[3]]
            m, sa = [], 0.0
            for j in range(4):
                a_, s_ = M.mm(G[j].reshape(c.Cout, -1), plane(D[j]), ws, xs, 9, main=True, lo_swap=Gl[j].reshape(c.Cout, -1) if Gl is not G else None)
                m.append(a_)
                sa = sa + s_
            if c.tc:
                h = c.tc // 2
                ta, tb = tx[:, 2 * p].float(), tx[:, min(2 * p + 1, T - 1)].float() * (1.0 if 2 * p + 1 < T else 0.0)
                ops = [(wd[:, :h], ta[:h]), (wd[:, h:], (ta[h:] + tb[h:]) * 0.5), (wd[:, h:], (ta[h:] - tb[h:]) * 0.5), (wd[:, :h], -tb[:h])]
                for j, (wj, xj) in enumerate(ops):
                    a_, s_ = M.mm(wj, xj.reshape(xj.shape[0], -1).t(), wts, ts, 1)
                    m[j] = m[j] + a_
                    sa = sa + s_
            acc[2 * p], acc[2 * p + 1] = m[0] + m[1] + m[2], m[1] - m[2] - m[3]
            s[2 * p] = s[2 * p + 1] = sa
        acc, s = acc[:T].reshape(-1, c.Cout), s[:T].reshape(-1, c.Cout)
        scale, shift = J["scale"], J["shift"]
    elif c.kind.startswith("up"):
        x0, x1, w = J["x0"][0], J["x1"][0], J["w"]
        C0 = c.C0
        w0 = w[:, :C0]
        H, W = c.H, c.W
        odd_h, odd_w = H % 2 == 1, W % 2 == 1
        folded = [_fold2(_fold2(w0, 3, ph), 4, pw) for ph in (0, 1) for pw in (0, 1)]          # [Cout, C0, 3, 2, 2] each
        corr_h = [-_fold2(w0[:, :, :, 2:3], 4, pw) for pw in (0, 1)]                             # [Cout, C0, 3, 1, 2]: -w[+1] rows
        corr_w = [-_fold2(w0[:, :, :, :, 2:3], 3, ph) for ph in (0, 1)]                          # [Cout, C0, 3, 2, 1]
        corner = w0[:, :, :, 2:3, 2:3].float()
        ws = pow2_prescale(max([_amax(w)] + [_amax(f) for f in folded]))
        xs = pow2_prescale(_amax(x0, x1))
        acc = torch.zeros(T, H, W, c.Cout, dtype=torch.float64)
        s = torch.zeros_like(acc)
        x0p = F.pad(x0.double(), (1, 1, 1, 1, 1, 1))

        def low(ti, ii, jj, offs):                                    # low-resolution patches: [N, C0 * len(offs)]
            cols = torch.stack([x0p[:, ti + dt, ii + a, jj + b] for dt, a, b in offs], dim=2)
            return cols.permute(1, 0, 2).reshape(ti.numel(), -1)

        for ph in (0, 1):
            for pw in (0, 1):
                ni, nj = (H - ph + 1) // 2, (W - pw + 1) // 2
                ti, ii, jj = (v.reshape(-1) for v in torch.meshgrid(torch.arange(T), torch.arange(ni), torch.arange(nj), indexing="ij"))
                offs = [(dt, a + ph, b + pw) for dt in range(3) for a in range(2) for b in range(2)]
                a_, s_ = M.mm(folded[2 * ph + pw].reshape(c.Cout, -1), low(ti, ii, jj, offs), ws, xs, 12, main=True)
                hh, ww = 2 * ii + ph, 2 * jj + pw
                acc[ti, hh, ww] += a_
                s[ti, hh, ww] += s_
                if ph == 0 and odd_h:                                # the last row: its +1 neighbour is padding
                    k = ii == ni - 1
                    offs = [(dt, 1, b + pw) for dt in range(3) for b in range(2)]
                    a_, s_ = M.mm(corr_h[pw].reshape(c.Cout, -1), low(ti[k], ii[k], jj[k], offs), ws, xs, 6)
                    acc[ti[k], hh[k], ww[k]] += a_
                    s[ti[k], hh[k], ww[k]] += s_
                if pw == 0 and odd_w:
                    k = jj == nj - 1
                    offs = [(dt, a + ph, 1) for dt in range(3) for a in range(2)]
                    a_, s_ = M.mm(corr_w[ph].reshape(c.Cout, -1), low(ti[k], ii[k], jj[k], offs), ws, xs, 6)
                    acc[ti[k], hh[k], ww[k]] += a_
                    s[ti[k], hh[k], ww[k]] += s_
                if ph == 0 and pw == 0 and odd_h and odd_w:
                    k = (ii == ni - 1) & (jj == nj - 1)
                    a_, s_ = M.mm(corner.reshape(c.Cout, -1), low(ti[k], ii[k], jj[k], [(dt, 1, 1) for dt in range(3)]), ws, xs, 3)
                    acc[ti[k], hh[k], ww[k]] += a_
                    s[ti[k], hh[k], ww[k]] += s_
        acc, s = acc.reshape(-1, c.Cout), s.reshape(-1, c.Cout)
        if c.kind != "up_part":
            a_, s_ = M.mm(w[:, C0:].reshape(c.Cout, -1), _gather(x1, 3, 1, pos), ws, xs, 27)
            acc, s = acc + a_, s + s_
        if c.kind == "up_sc":
            wd = J["wd"].reshape(c.Cout, -1)
            up = x0[:, :, torch.arange(H) // 2][:, :, :, torch.arange(W) // 2]
            xc = torch.cat([up, x1])
            a2, s2 = M.mm(wd, _gather(xc, 1, 1, pos), pow2_prescale(_amax(wd)), xs, 1)
            y2 = (a2 * col(J["scale2"]) + col(J["shift2"]), s2 * col(J["scale2"]).abs() + col(J["shift2"]).abs(), col(J["scale2"]))
        scale, shift = J["scale"], J["shift"]
    else:
        x, w = J["x0"][0], J["w"]
        k3 = c.ks ** 3
        ws, xs = pow2_prescale(_amax(w)), pow2_prescale(_amax(x))
        acc, s = M.mm(w.reshape(c.Cout, -1), _gather(x, c.ks, c.s, pos), ws, xs, k3, main=True)
        if c.tc:
            tx, wd = J["tx"][0], J["wd"].reshape(c.Cout, -1)
            a_, s_ = M.mm(wd, _gather(tx, 1, 1, pos), pow2_prescale(_amax(wd)), pow2_prescale(_amax(tx)), 1)
            acc, s = acc + a_, s + s_
        if c.kind == "sc":
            wd = J["wd"].reshape(c.Cout, -1)
            a2, s2 = M.mm(wd, _gather(x, 1, c.s, pos), pow2_prescale(_amax(wd)), xs, 1)
            y2 = (a2 * col(J["scale2"]) + col(J["shift2"]), s2 * col(J["scale2"]).abs() + col(J["shift2"]).abs(), col(J["scale2"]))
        scale, shift = J["scale"], J["shift"]
    y = acc * col(scale) + col(shift)
    s = s * col(scale).abs() + col(shift).abs()
    if c.res:
        r = J["res"][0].double()
        t, h, w_ = pos
        r = r[:, t, h >> 1, w_ >> 1] if c.kind == "wt_tail" else r[:, t, h, w_]
        y, s = y + r.t(), s + r.t().abs()
    unit = torch.minimum(col(scale).abs() * M.unit, torch.ones(1, dtype=torch.float64))
    c_ok = bool((s < 0.98 * 2.0 ** 24 * unit).all())
    if y2 is not None:
        c_ok = c_ok and bool((y2[1] < 0.98 * 2.0 ** 24 * torch.minimum(y2[2].abs() * M.unit, torch.ones(1, dtype=torch.float64))).all())
    nonzero_sums = float((acc != 0).double().mean())
    if c.kind == "head":
        y = torch.where(y < 0, (y * SLOPE).float().double(), y)
    elif c.kind != "up_part":
        y = torch.relu(y)
    if c.kind == "pred":                            # the fused head on the y still in registers: a power of two per position
        wp = J["wp"]
        pws = pow2_prescale(_amax(wp))
        vs = torch.tensor([pow2_prescale(float(v)) for v in y.abs().amax(dim=1)], dtype=torch.float64).view(-1, 1)
        M2 = Model(mut)
        bits = 10 if M.mut.get("hi10") else 11
        yh, yl, ea = split(y, vs, bits)
        ph_, pl_, eb = split(wp, pws, bits)
        M2.a = ea and eb
        M2.b = not bool(((yl != 0).double() @ (pl_ != 0).double().t()).any())
        a2 = ((yh @ ph_.t() + yl @ ph_.t() + yh @ pl_.t()) / (vs * pws))
        s2 = y.abs() @ wp.double().abs().t() + col(J["bp"]).abs()
        unit2 = min(1.0, _lsb(wp) * min(_lsb(y), 1.0))
        c_ok = c_ok and bool((s2 < 0.98 * 2.0 ** 24 * unit2).all())
        M.a, M.b = M.a and M2.a, M.b and M2.b
        M.lo_w += int((pl_ != 0).sum())
        M.lo_x += int((yl != 0).sum())
        nonzero_sums = float((a2 != 0).double().mean())
        y = torch.relu(a2 + col(J["bp"]))
    out = {"y": y.t().reshape(-1, T, Ho, Wo)}
    if y2 is not None:
        out["y2"] = y2[0].t().reshape(-1, T, Ho, Wo)
    out["cond"] = {"a": M.a, "b": M.b, "c": c_ok, "lo_x": M.lo_x, "lo_w": M.lo_w, "nonzero_sums": nonzero_sums, "notes": M.notes}
    return out
