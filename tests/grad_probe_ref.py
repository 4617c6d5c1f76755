"""What the probe tests of the eleven gradient kernels share (tests/test_grad_probe_cpu.py, tests/test_gpu_grad_probes.py): the
case table, the data builders of the four probes, the share arithmetic of the weight-gradient grids, the three assertions of
the absorption probe and a numpy model of one output element of a hypothetical weight-gradient kernel.  No GPU.

The truths are the f64 restatements the suite already has (tests/grad_walk_ref.py, convn_ref.py, convupn_ref.py): nothing is
rounded there.  A case is (kind, channels):

  wgrad    (cin, cout)       v2ce_conv32_wgrad at (32, 32), v2ce_convn_wgrad at convn_ref.PAIRS      x, y, upstream
  upwgrad  (c0, c1, cout)    v2ce_convup_wgrad at (64, 32, 32), v2ce_convupn_wgrad at convupn_ref.TRIPLES   x0, x1, g1, gd
  dgrad    (cin, cout)       v2ce_conv32_dgrad at (32, 32), v2ce_convn_dgrad at convn_ref.PAIRS      weight, y, upstream
  updgrad  (64, 32, 32)      v2ce_convup_dgrad                                                      weight, short, g1, gd
  head     (cout,)           v2ce_pred_head_grads at grad_walk_ref.HEAD_COUTS                       feat, y, upstream, weight
  wgrad    (cin, cout)       v2ce_convc_wgrad at WIDE_PAIRS = (128, 128), (512, 32), (32, 512), (512, 512)   x, y, upstream
  dgrad    (cin, cout)       v2ce_convc_dgrad at WIDE_PAIRS                                         weight, y, upstream
  updgrad  (c0, c1, cout)    v2ce_convupn_dgrad at convupn_ref.TRIPLES                              weight, short, g1, gd

(the last three rows are appended to CASES behind the others, whose indices seed their data: `is_new`) with the inputs in
the reference's layouts as f32 tensors on the CPU under the names on the right.  In every kind one operand is a gradient coming from behind (role "up": upstream, g1, gd) and the other one is what it is multiplied with (role "other").

Probe 1, wide integers.  Sparse upstream gradients, dense other operands, every value an odd integer of 12 significant bits
(2049 .. 2895, either sign), so a product is an odd integer of 23 significant bits below 2^23 and an element's two terms sum
below 2^24: every f32 order of every sum is exact, while a product formed at less than f32 precision is not.  The one element
that collects more is d_x0 of v2ce_convup_dgrad (the 2 x 2 pool: up to four terms): the weights of its 64 channels are odd
integers of 11 bits (1025 .. 1447), products of 22 bits.  The appended cases need up to 512 positions, or 256 with disjoint
3 x 3 x 3 neighbourhoods: they have a shape, [2, 4, 5, 131], and slot tables of their own (p1w_slots).

Probe 2, absorption.  Ones everywhere and one anchor of 2^24, 2^32 or 2^36: what an f32 chain, an f32 partial slot or an f32
finish loses next to the anchor is an integer that the header's sentences bound.

Probe 3, power-of-two scale equivariance: per-channel exponents for the normal data of the walks (the appended cases:
[1, 3, 20, 70], 60 tiles with a ragged second tile column).

Probe 4, the underflow term: the same normal data scaled so that products lie at the lower end of f32's normal range."""
import numpy as np
import torch

from tests import convn_ref as R
from tests import convupn_ref as RU
from tests import grad_walk_ref as G
from tests.last_conv_ref import ulp32

CASES = [("wgrad", (32, 32))] + [("wgrad", p) for p in R.PAIRS] + [("upwgrad", RU.OLD)] + [("upwgrad", t) for t in RU.TRIPLES] + \
        [("dgrad", (32, 32))] + [("dgrad", p) for p in R.PAIRS] + [("updgrad", RU.OLD)] + [("head", (c,)) for c in G.HEAD_COUTS]
# appended, never inserted: a case's index seeds its data.  (128, 128) is the model's layer and the first width at which the
# input gradient fetches its weights again per tile, the asymmetric pairs catch a transposed or truncated group index,
# 512 -> 512 is 256 pairs: a default grid of one share
N_OLD = len(CASES)
WIDE_PAIRS = ((128, 128), (512, 32), (32, 512), (512, 512))
CASES += [("wgrad", p) for p in WIDE_PAIRS] + [("dgrad", p) for p in WIDE_PAIRS] + [("updgrad", t) for t in RU.TRIPLES]
WGRAD_CASES = [c for c in CASES if c[0] in ("wgrad", "upwgrad")]
CONV_CASES = [c for c in CASES if c[0] != "head"]


def case_id(case):
    return case[0] + "_" + "_".join(map(str, case[1]))


def is_new(case):
    """The appended cases: v2ce_convc_wgrad, v2ce_convc_dgrad and v2ce_convupn_dgrad."""
    return CASES.index(case) >= N_OLD


OUTPUTS = {"wgrad": ("weight", "shift"), "upwgrad": ("weight", "short", "short_bias"), "dgrad": ("x", "res"),
           "updgrad": ("x0", "x1"), "head": ("weight", "bias", "feat")}
# the outputs that are sums of products (the others are sums or copies of the "up" operand alone)
PRODUCTS = {"wgrad": ("weight",), "upwgrad": ("weight", "short"), "dgrad": ("x",), "updgrad": ("x0", "x1"),
            "head": ("weight", "feat")}
ROLES = {"wgrad": {"up": ("upstream",), "other": ("x",)}, "upwgrad": {"up": ("g1", "gd"), "other": ("x0", "x1")},
         "dgrad": {"up": ("upstream",), "other": ("weight",)}, "updgrad": {"up": ("g1", "gd"), "other": ("weight", "short")},
         "head": {"up": ("upstream",), "other": ("feat", "weight")}}


def updgrad_truth(c0, weight, short, g1, gd):
    """grad_walk_ref.convup_dgrad at any channel counts, c0 of the input channels upsampled: the per-tap f64 matmuls, the
    shortcut's matmul and the 2 x 2 pool (tests/test_grad_probe_cpu.py holds it to convupn_dgrad_ref.dgrad)."""
    g, s = G.f64(g1), G.f64(gd)
    w = G.f64(short).to(g.device).reshape(short.shape[0], -1)
    d, a = G._tap_transposed(weight, g)
    dX, aX = d + G.unrows(w.t() @ G.rows(s), s), a + G.unrows(w.abs().t() @ G.rows(s).abs(), s)
    return {"d_x0": G.pooled(dX[:, :c0]), "d_x1": dX[:, c0:].contiguous(), "abs_x0": G.pooled(aX[:, :c0]),
            "abs_x1": aX[:, c0:].contiguous()}


def truth(kind, z, ch=None):
    """The f64 truth of a case's outputs on the device of its inputs, under the kernel's output names.  ch: the channel
    triple of an updgrad case other than (64, 32, 32), which the tensors alone do not tell."""
    if kind == "wgrad":
        t = G.conv32_wgrad(z["x"], z.get("y"), z["upstream"])
        return {"weight": t["d_weight"], "shift": t["d_shift"]}
    if kind == "upwgrad":
        t = RU.wgrad_truth(z["x0"], z["x1"], z["g1"], z["gd"])
        return {"weight": t["d_weight"], "short": t["d_short"], "short_bias": t["d_short_bias"]}
    if kind == "dgrad":
        t = G.conv32_dgrad(z["weight"], z.get("y"), z["upstream"])
        return {"x": t["d_x"], "res": t["d_res"]}
    if kind == "updgrad":
        t = G.convup_dgrad(z["weight"], z["short"], z["g1"], z["gd"]) if ch in (None, RU.OLD) else \
            updgrad_truth(ch[0], z["weight"], z["short"], z["g1"], z["gd"])
        return {"x0": t["d_x0"], "x1": t["d_x1"]}
    t = G.pred_head_grads(z["feat"], z.get("y"), z["upstream"], z["weight"])
    return {"weight": t["d_weight"], "bias": t["d_bias"], "feat": t["d_feat"]}


def abs_truth(kind, z, ch=None):
    """An element's sum of |terms|: the truth of the absolute values, the mask applied first."""
    a = {k: v.abs() for k, v in z.items() if k != "y" and v is not None}
    if z.get("y") is not None:
        a["upstream"] = G.masked(z["y"], z["upstream"]).abs()
    return truth(kind, a, ch)


def n_terms_updgrad(shape):
    """[H0, W0]: the output positions of each source pixel of v2ce_convup_dgrad (1, 2 or 4), the factor of its term count."""
    return G.pooled(torch.ones((1, 1, 1, shape[2], shape[3]), dtype=torch.float64))[0, 0, 0].numpy()


# ---------------------------------------------------------------------------------------------------------------------
# the grids of the weight-gradient kernels (the max_workgroups paragraphs of v2ce_hip_convgrad.h, v2ce_hip_convupgrad.h,
# v2ce_hip_convngrad.h and v2ce_hip_convupngrad.h)

CAP = 256                                     # workgroups of a default grid at most


def pairs_of(kind, ch):
    """Workgroups per share: one per (32 output channels, 32 input channels)."""
    return (ch[-1] // 32) * (sum(ch[:-1]) // 32)


def wgrad_shares(kind, ch, tiles, max_workgroups=0):
    """The four headers' share count: one share per tile, at most 256 / pairs shares (256; 85; 256 / pairs); n > 0 caps the
    shares at max(n / pairs, 1)."""
    p = pairs_of(kind, ch)
    s = min(tiles, CAP // p)
    return min(s, max(max_workgroups // p, 1)) if max_workgroups > 0 else s


def share_positions(kind, ch, shape, max_workgroups, position=0):
    """Positions of the share that holds the tile with `position` (a flat index of full tiles: every tile has 128)."""
    tiles = G.conv_tiles(*shape)
    assert shape[2] % G.TILE_H == 0 and shape[3] % G.TILE_W == 0
    sizes = G.share_sizes(tiles, wgrad_shares(kind, ch, tiles, max_workgroups))
    tile, first = position // (G.TILE_H * G.TILE_W), 0
    for n in sizes:
        if tile < first + n:
            return n * G.TILE_H * G.TILE_W
        first += n
    raise ValueError(position)


# ---------------------------------------------------------------------------------------------------------------------
# probe 1: wide integers

P1_SHAPE = (2, 3, 5, 131)                     # 54 tiles: three tile rows (the last of one row), three tile columns (the last of 3)
P1_SEED = 1201
WIDE = (2048, 2896)                           # odd integers 2049 .. 2895: 12 bits, a product of two below 2^23
POOLED = (1024, 1448)                         # 1025 .. 1447: 11 bits; four products with a WIDE one sum below 2^24


def odd_integers(gen, shape, lo_hi=WIDE):
    """Seeded odd integers lo + 1 .. hi - 1 of either sign as f32."""
    lo, hi = lo_hi
    v = torch.randint(lo // 2, hi // 2, shape, generator=gen) * 2 + 1
    return (v * (torch.randint(0, 2, shape, generator=gen) * 2 - 1)).to(torch.float32)


def p1_slots():
    """66 positions (b, l, h, w) of P1_SHAPE whose columns are 4 apart within a batch element, so that no input-gradient
    element and no 2 x 2 pool of them reaches two: slot 0 is (0, 0, 0, 0), the first position of the first tile and a corner
    of the first frame; the last one is (1, 2, 4, 128) in the one-row, three-column last tile of the last frame."""
    return [(i % 2, (i // 2) % 3, (2 * (i // 2)) % 5, 4 * (i // 2)) for i in range(66)]


def p1_pick(n, of=None):
    """n of the slots, the first and the last among them, spread evenly."""
    of = list(range(66)) if of is None else of
    idx = sorted({round(k * (len(of) - 1) / (n - 1)) for k in range(n)})
    assert len(idx) == n
    return [p1_slots()[of[i]] for i in idx]


def p1_late(n, half=False):
    """[B, n] bool: is column w (of the source of the upsampled channels: half) of batch element b within a tap of a slot of
    the second half of every pick, 2 j + b > 32 with j the slot whose columns 4 j - 1 .. 4 j + 1 hold it."""
    j = (torch.arange(n) + 1) // (2 if half else 4)
    return (2 * j.view(1, -1) + torch.arange(P1_SHAPE[0]).view(-1, 1)) > 32


def p1_dense(gen, shape, late):
    """Odd integers of 12 bits in two classes: 2049 .. 2471 where `late` (which broadcasts against the shape) is false,
    2473 .. 2895 where it is true."""
    mid = (WIDE[0] + WIDE[1]) // 2
    return torch.where(late, odd_integers(gen, shape, (mid, WIDE[1])), odd_integers(gen, shape, (WIDE[0], mid)))


def p1_sparse(gen, channels, positions, per_pos, shape=P1_SHAPE):
    """[B, channels, L, H, W] of zeros with `per_pos` odd integers at each position: slot s = k per_pos + j of position k is
    channel s mod channels, so len(positions) per_pos / channels positions feed every channel.  The two terms of an element
    come from slots j = 0 and j = 1 of one position (input gradients, the head's d_feat) or from positions k and
    k + len / 2 (weight gradients), and a slot's value is of the quarter 2 (k >= len / 2) + j of the 12-bit range.  The other
    operand's classes (p1_dense) follow the same order -- columns near the second half's positions and odd output channels
    hold the larger class -- so of an element's two terms the second has the larger |up|, the larger |other| and the larger
    |up| + |other|: neither the rounding errors of an 11-bit operand nor the dropped low bits of the two terms can cancel."""
    B, L, H, W = shape
    assert (len(positions) * per_pos) % channels == 0 and per_pos in (1, 2)
    out = torch.zeros((B, channels, L, H, W), dtype=torch.float32)
    q = (WIDE[1] - WIDE[0]) // 4
    vals = [odd_integers(gen, (len(positions), per_pos), (WIDE[0] + i * q, WIDE[0] + (i + 1) * q)) for i in range(4)]
    for k, (b, l, h, w) in enumerate(positions):
        for j in range(per_pos):
            out[b, (k * per_pos + j) % channels, l, h, w] = vals[2 * (2 * k >= len(positions)) + j][k, j]
    return out


def p1_y(gen, upstream):
    """A normal y with signed zeros that is positive wherever the upstream gradient is not zero."""
    y = G.signed_zero_normals(gen, tuple(upstream.shape))
    return torch.where(upstream != 0, y.abs() + 0.5, y)


def p1_inputs(case):
    """The inputs of probe 1.  Weight gradients: cout positions x 2 channels, every output channel at two positions, every
    element of d_weight and d_short a sum of two products (one where a tap leaves the tensor).  Input gradients: cout / 2
    positions x 2 channels, every d_x element a sum of two products or zero.  v2ce_convup_dgrad: g1 at 32 positions and gd at
    32 others, one channel each: a d_x1 element is one product, a d_x0 element up to four.  Head: cout positions x 2."""
    if is_new(case):
        return p1w_inputs(case)
    kind, ch = case
    B, L, H, W = P1_SHAPE
    gen = torch.Generator().manual_seed(P1_SEED + 31 * CASES.index(case))
    act = lambda c: (B, c, L, H, W)
    cols, cols0 = p1_late(W).view(B, 1, 1, 1, W), p1_late((W + 1) // 2, half=True).view(B, 1, 1, 1, (W + 1) // 2)
    odd_co = lambda cout, dims: (torch.arange(cout) % 2 == 1).view([cout] + [1] * dims)
    if kind == "wgrad":
        cin, cout = ch
        up = p1_sparse(gen, cout, p1_pick(cout), 2)
        return {"x": p1_dense(gen, act(cin), cols), "upstream": up, "y": p1_y(gen, up)}
    if kind == "upwgrad":
        c0, c1, cout = ch
        return {"x0": p1_dense(gen, (B, c0, L, (H + 1) // 2, (W + 1) // 2), cols0), "x1": p1_dense(gen, act(c1), cols),
                "g1": p1_sparse(gen, cout, p1_pick(cout), 2), "gd": p1_sparse(gen, cout, p1_pick(cout), 2)}
    if kind == "dgrad":
        cin, cout = ch
        up = p1_sparse(gen, cout, p1_pick(cout // 2), 2)
        return {"weight": p1_dense(gen, (cout, cin, 3, 3, 3), odd_co(cout, 4)), "upstream": up, "y": p1_y(gen, up)}
    if kind == "updgrad":
        c0, c1, cout = ch
        even = [i for i in range(66) if (i // 2) % 2 == 0]
        odd = [i for i in range(66) if (i // 2) % 2 == 1]
        w = odd_integers(gen, (cout, c0 + c1, 3, 3, 3))
        w[:, :c0] = odd_integers(gen, (cout, c0, 3, 3, 3), POOLED)
        return {"weight": w, "short": odd_integers(gen, (cout, c0 + c1)), "g1": p1_sparse(gen, cout, p1_pick(cout, even), 1),
                "gd": p1_sparse(gen, cout, p1_pick(cout, odd), 1)}
    cout, = ch
    up = p1_sparse(gen, cout, p1_pick(cout), 2)
    return {"feat": p1_dense(gen, act(G.C), cols), "upstream": up, "y": p1_y(gen, up).abs(),
            "weight": p1_dense(gen, (cout, G.C), odd_co(cout, 1))}


# the appended cases: up to 512 positions

P1W_SHAPE = (2, 4, 5, 131)                    # 72 tiles: three tile rows (the last of one row), three tile columns (the last of 3)
P1W_STEP = {"wgrad": 3, "dgrad": 3, "updgrad": 4}


def p1_shape(case):
    return P1W_SHAPE if is_new(case) else P1_SHAPE


def p1w_slots(kind):
    """The positions (b, l, h, w) of P1W_SHAPE that a sparse gradient of the appended cases may use, column by column.
    dgrad: frames 0 and 3, rows 0 and 3, every third column -- 352 positions whose 3 x 3 x 3 neighbourhoods are disjoint,
    so that no input-gradient element reaches two.  updgrad: every fourth column of the same frames and rows -- 264
    positions of which no 2 x 2 pool of output positions (rows 2 h0 - 1 .. 2 h0 + 2 and as many columns of a neighbourhood)
    reaches two.  wgrad, whose elements sum over the positions whatever they are: every frame and every row of every third
    column, 1760 positions.  Slot 0 is (0, 0, 0, 0), the first position of the first tile and a corner of the first frame;
    the last one lies in the three-column last tile of the last frame (wgrad: in its one-row last tile row)."""
    B, L, H, W = P1W_SHAPE
    frames, lines = (range(L), range(H)) if kind == "wgrad" else ((0, 3), (0, 3))
    return [(b, l, h, w) for w in range(0, W, P1W_STEP[kind]) for b in range(B) for l in frames for h in lines]


def p1w_pick(kind, n):
    """n of the slots: the first n / 2 and the last n / 2, so that the two halves share no column and a column within a tap
    of the one half is within a tap of no position of the other -> (positions, the first column of the later half)."""
    slots = p1w_slots(kind)
    first, second = slots[:n // 2], slots[len(slots) - n // 2:]
    assert n % 2 == 0 and n <= len(slots) and first[-1][3] + 3 <= second[0][3]
    return first + second, second[0][3]


def p1w_inputs(case):
    """The inputs of probe 1 of an appended case at P1W_SHAPE, in the scheme of p1_inputs.  wgrad: cout positions x 2
    channels, the two terms of an element at positions k and k + cout / 2, x of the larger class in the columns from one
    before the later half's first.  dgrad: cout / 2 positions x 2 channels, every output channel once, the odd ones with
    the larger gradients and the larger weights.  updgrad: g1 at cout positions and gd at cout others, one channel each: a
    d_x1 element is one product, a d_x0 element up to four products of one gradient value with four taps of one (co, ci).
    The weights of the c0 upsampled channels are 11-bit integers 4 m + 1 (1025 .. 1445) whose sign depends on (co, ci)
    alone: the four terms have one sign, and what an operand loses at 11 bits (the gradient), at 10 bits (these weights:
    every one of them rounds towards zero by one) or with its lowest bit has one sign in all four, so it cannot cancel."""
    kind, ch = case
    B, L, H, W = P1W_SHAPE
    gen = torch.Generator().manual_seed(P1_SEED + 31 * CASES.index(case))
    if kind == "wgrad":
        cin, cout = ch
        at, later = p1w_pick(kind, cout)
        up = p1_sparse(gen, cout, at, 2, P1W_SHAPE)
        late = (torch.arange(W) >= later - 1).view(1, 1, 1, 1, W)
        return {"x": p1_dense(gen, (B, cin, L, H, W), late), "upstream": up, "y": p1_y(gen, up)}
    if kind == "dgrad":
        cin, cout = ch
        up = p1_sparse(gen, cout, p1w_pick(kind, cout // 2)[0], 2, P1W_SHAPE)
        odd_co = (torch.arange(cout) % 2 == 1).view(cout, 1, 1, 1, 1)
        return {"weight": p1_dense(gen, (cout, cin, 3, 3, 3), odd_co), "upstream": up, "y": p1_y(gen, up)}
    assert kind == "updgrad"
    c0, c1, cout = ch
    at = p1w_pick(kind, 2 * cout)[0]
    mine = [sum(p) % 2 == 0 for p in at]        # a checkerboard (the columns are even): either gets every batch element, frame and row
    w = odd_integers(gen, (cout, c0 + c1, 3, 3, 3))
    sign = torch.randint(0, 2, (cout, c0, 1, 1, 1), generator=gen) * 2 - 1
    quarter = torch.randint(POOLED[0] // 4, POOLED[1] // 4, (cout, c0, 3, 3, 3), generator=gen)
    w[:, :c0] = (sign * (quarter * 4 + 1)).to(torch.float32)
    return {"weight": w, "short": odd_integers(gen, (cout, c0 + c1)),
            "g1": p1_sparse(gen, cout, [p for p, m in zip(at, mine) if m], 1, P1W_SHAPE),
            "gd": p1_sparse(gen, cout, [p for p, m in zip(at, mine) if not m], 1, P1W_SHAPE)}


def round_to_bits(t, bits):
    """Every element rounded (to nearest, ties to even) to `bits` significant bits: what an operand of an 11-bit format
    keeps."""
    m, e = torch.frexp(t.to(torch.float64))
    return torch.ldexp(torch.round(m * 2.0 ** bits) / 2.0 ** bits, e).to(torch.float32)


def drop_lowest_bit(t):
    """Every integer element with its lowest set bit cleared: the low half of a two-way split, whose product with the other
    operand's low half a three-product scheme leaves out."""
    a = t.abs().to(torch.int64)
    return (torch.sign(t) * (a - (a & -a)).to(torch.float32)).to(torch.float32)


def with_role(kind, z, role, f):
    """The inputs with f applied to the tensors of one role ("up", "other") or of both ("both")."""
    names = ROLES[kind]["up"] + ROLES[kind]["other"] if role == "both" else ROLES[kind][role]
    return {k: (f(v) if k in names else v) for k, v in z.items()}


# ---------------------------------------------------------------------------------------------------------------------
# probe 2: absorption

P2_SHAPE = (1, 4, 26, 128)                    # 104 full tiles, 13312 positions: three chains of 32 tiles and eight tiles more
P2_UP_CHANNEL, P2_IN_CHANNEL, P2_X0_CHANNEL = 5, 7, 9
P2_TILE = 40                                  # the tile of the input anchor: frame 1, rows 14 .. 15, columns 0 .. 63
P2_AT = (1, 14, 30)                           # an interior position of it; its source pixel is (7, 15)
HEAD_ANCHOR = 2.0 ** 30


def p2_inputs(case, anchor, where):
    """Ones in every value tensor, y None (the head: ones).  where "up": the anchor at position (b, l, h, w) = 0 of channel
    5 of every 32-channel group of the upstream gradient (g1 and gd); "input": at P2_AT of channel 7 of every 32-channel
    group of x; the upsample kernels: of channel 7 of x1, and at the source pixel of P2_AT of channel 9 of x0."""
    kind, ch = case
    B, L, H, W = P2_SHAPE
    one = lambda c, h=H, w=W: torch.ones((B, c, L, h, w), dtype=torch.float32)
    assert G.tile_of(P2_SHAPE, P2_TILE)[1:] == (1, 14, 16, 0, 64) and where in ("up", "input")
    if kind == "head":
        z = {"feat": one(G.C), "y": one(ch[0]), "upstream": one(ch[0]), "weight": torch.ones((ch[0], G.C))}
        z["upstream"][0, 3, 0, 0, 0] = anchor
        return z
    if kind == "wgrad":
        z = {"x": one(ch[0]), "y": None, "upstream": one(ch[1])}
        ups, ins = [z["upstream"]], [z["x"]]
    else:
        z = {"x0": one(ch[0], (H + 1) // 2, (W + 1) // 2), "x1": one(ch[1]), "g1": one(ch[2]), "gd": one(ch[2])}
        ups, ins = [z["g1"], z["gd"]], []
    if where == "up":
        for t in ups:
            t[0, P2_UP_CHANNEL::32, 0, 0, 0] = anchor
    elif kind == "wgrad":
        z["x"][0, P2_IN_CHANNEL::32, P2_AT[0], P2_AT[1], P2_AT[2]] = anchor
    else:
        z["x1"][0, P2_IN_CHANNEL, P2_AT[0], P2_AT[1], P2_AT[2]] = anchor
        z["x0"][0, P2_X0_CHANNEL, P2_AT[0], P2_AT[1] // 2, P2_AT[2] // 2] = anchor
    return z


def header_bound(exact, abs_terms, n_pos, chain):
    """The weight-gradient headers' bound, elementwise."""
    return R.wgrad_bound(np.asarray(exact), np.asarray(abs_terms), n_pos, chain)


def share_bound(exact, positions):
    """What the headers' sentences leave an element whose terms are ones beside one anchor: every sum above the f32 chain
    is f64 and exact on integers of this size, the chain that holds the anchor has at most `positions` terms and loses less
    than that, and the store rounds once."""
    return ulp32(np.asarray(exact)) + positions


def is_round32(got, exact):
    """The bytes of an f64-throughout output: the exact value rounded once."""
    want = np.asarray(exact, np.float64).astype(np.float32)
    return np.array_equal(np.asarray(got, np.float32).view(np.int32), want.view(np.int32))


def model_element(products, shares, chain, acc=np.float32, partial=np.float64, finish=np.float64):
    """One output element of a hypothetical weight-gradient kernel: `products` in walk order; a workgroup sums the products
    of its share [s0, s1) in `acc` chains of at most `chain` positions (None: never flushed), adds each chain into a partial
    slot of dtype `partial`, the finish adds the slots in share order in dtype `finish` and rounds once to f32.  (The
    products here are exact in f32, so an fmaf is an addition.)  The contract's kernel is chain 4096, f64, f64."""
    products = np.asarray(products, np.float64)
    total = finish(0)
    for s0, s1 in shares:
        slot = partial(0)
        step = (s1 - s0) if chain is None else chain
        for c0 in range(s0, s1, max(step, 1)):
            seg = products[c0:min(c0 + step, s1)].astype(acc)
            slot = partial(slot + partial(np.cumsum(seg, dtype=acc)[-1]))            # cumsum: sequential adds in acc
        total = finish(total + finish(slot))
    return np.float32(total)


def boundaries(sizes, tile=G.TILE_H * G.TILE_W):
    """Share sizes in tiles -> [(first position, end position)]."""
    out, at = [], 0
    for n in sizes:
        out.append((at, at + n * tile))
        at += n * tile
    return out


# ---------------------------------------------------------------------------------------------------------------------
# probes 3 and 4: the normal data of the walks

P3_SHAPE = R.WALK                             # [2, 3, 43, 131]: 396 ragged tiles
P3W_SHAPE = (1, 3, 20, 70)                    # the appended cases: 60 tiles, a ragged second tile column (a per-element property
                                              # needs no long walk); one share of a weight gradient flushes mid-walk
P3_SEED = 709                                 # (707 and 708 draw an exact 0.0, which no exponent scales)
P3_MAX_EXP = 16
P3_RANGE = (2.0 ** -60, 2.0 ** 40)
P4_SHAPE = (1, 2, 5, 70)
P4_SEED = 808


def p3_shape(case):
    return P3W_SHAPE if is_new(case) else P3_SHAPE


def normal_inputs(case, shape, seed):
    """The suite's seeded standard normals of a case at `shape` under this file's names.  The appended cases draw up to
    7e6 weights, among which an exact 0.0 is likely (f32 normals hold one in about 2^-24 draws): there a 0.0 of a value
    tensor becomes 1.0, so that every value has an exponent to scale."""
    z = _normal_inputs(case, shape, seed)
    if is_new(case):
        z = {k: (v if k == "y" else torch.where(v == 0, torch.ones_like(v), v)) for k, v in z.items()}
    return z


def _normal_inputs(case, shape, seed):
    kind, ch = case
    if kind == "updgrad" and ch != RU.OLD:                              # (convupn_ref.inputs has the gradients, no weights)
        z = RU.inputs(shape, *ch, False, seed)
        gen = torch.Generator().manual_seed(seed + 31 * CASES.index(case))
        return {"weight": G.normals(gen, (ch[2], ch[0] + ch[1], 3, 3, 3)), "short": G.normals(gen, (ch[2], ch[0] + ch[1])),
                "g1": z["g1"], "gd": z["gd"]}
    if kind == "head":
        z = G.head_inputs(shape, False, seed, ch[0])
        return {"feat": z["feat"], "y": z["y_head"], "upstream": z["up_head"], "weight": z["w_head"]}
    if kind in ("wgrad", "dgrad"):
        z = G.walk_inputs(shape, False, seed) if ch == (32, 32) else R.inputs(shape, ch[0], ch[1], False, seed)
        other = "x" if kind == "wgrad" else "weight"
        return {other: z[other], "y": z["y"], "upstream": z["upstream"]}
    z = G.walk_inputs(shape, False, seed) if ch == RU.OLD else RU.inputs(shape, *ch, False, seed)
    if kind == "upwgrad":
        return {k: z[k] for k in ("x0", "x1", "g1", "gd")}
    return {"weight": z["weight_up"], "short": z["short"], "g1": z["g1"], "gd": z["gd"]}


def exponents(case, name, n):
    """Seeded exponents -16 .. 16, one per channel."""
    gen = torch.Generator().manual_seed(P3_SEED + 97 * CASES.index(case) + sum(map(ord, name)))
    return torch.randint(-P3_MAX_EXP, P3_MAX_EXP + 1, (n,), generator=gen, dtype=torch.int32)


def pow2(exps):
    """2^exps as f32 from the exponent bits, -126 <= exps <= 127: exact, which a pow() behind torch.ldexp need not be."""
    e = exps.to(torch.int32)
    assert int(e.min()) >= -126 and int(e.max()) <= 127
    return ((e + 127) << 23).view(torch.float32)


def scaled(t, exps, dim):
    """t with index i of dimension `dim` multiplied by 2^exps[i]: one exact f32 multiplication."""
    view = [1] * t.dim()
    view[dim] = -1
    return t * pow2(exps.to(t.device)).view(view)
