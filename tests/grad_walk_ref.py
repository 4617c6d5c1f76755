"""torch f64 restatement of the five gradient kernels' header formulas that runs at full-grid sizes, on whatever device
its inputs live on: conv32_wgrad / conv32_dgrad (include/v2ce_hip_convgrad.h, v2ce_hip_convdgrad.h), convup_wgrad /
convup_dgrad (v2ce_hip_convupgrad.h, v2ce_hip_convupdgrad.h) and pred_head_grads (v2ce_hip_train.h).

The numpy restatements (tests/last_conv_ref.py, last_conv_dgrad_ref.py, last_block_ref.py, last_block_dgrad_ref.py,
pred_head_ref.py) are the ones torch's f64 goldens validate; their einsums take minutes at 5e5 positions.  These ports
state the same sums as one f64 matmul per tap over zero-padded shifted views, return the same dictionaries (the ``abs_*``
sums of |terms| included) as f64 tensors, and are held to the numpy restatements by tests/test_grad_walk_cpu.py.  Tensors
are in the reference's layouts: activations [B, C, L, H, W], x0 [B, 64, L, H0, W0], weights as nn.Conv3d stores them.
Every product and sum is f64; nothing is rounded here.

The second half is what the walk tests (tests/test_grad_walk_cpu.py, tests/test_gpu_grad_walks.py) share: the walk table,
the share arithmetic of a persistent grid, the seeded inputs and the channels-last-16 packing on the device."""
import torch

C, C0, CIN = 32, 64, 96
TILE_H, TILE_W = 2, 64                        # a tile of the four convolution kernels: 2 rows x 64 columns of one frame
HEAD_TILE = 128                               # a tile of pred_head_grads: 128 consecutive positions


def f64(a):
    return torch.as_tensor(a).to(torch.float64)


def masked(y, upstream):
    """torch's relu backward on the result: upstream where y > 0, else 0 (a NaN in y gives 0); y None: upstream."""
    u = f64(upstream)
    return u if y is None else torch.where(torch.as_tensor(y).to(u.device) > 0, u, torch.zeros_like(u))


def padded(x):
    """[B, C, L, H, W] -> [B, C, L + 2, H + 2, W + 2] with a border of zeros: the convolution's zero padding."""
    return torch.nn.functional.pad(x, (1, 1, 1, 1, 1, 1))


def rows(x):
    """[B, C, L, H, W] -> [C, B L H W]: one row per channel, the positions in the tensor's own order."""
    return x.permute(1, 0, 2, 3, 4).reshape(x.shape[1], -1)


def unrows(r, like):
    """[C, B L H W] -> [B, C, L, H, W] with the position dimensions of `like`."""
    B, _, L, H, W = like.shape
    return r.reshape(r.shape[0], B, L, H, W).permute(1, 0, 2, 3, 4).contiguous()


def shifted_rows(xp, kt, kh, kw):
    """rows of x[b, c, l + kt - 1, h + kh - 1, w + kw - 1] (zeros outside the tensor) from xp = padded(x)."""
    L, H, W = xp.shape[2] - 2, xp.shape[3] - 2, xp.shape[4] - 2
    return rows(xp[:, :, kt:kt + L, kh:kh + H, kw:kw + W])


def _tap_sums(m, x):
    """d[co, ci, kt, kh, kw] = sum over the positions of m[co] x[ci] shifted by the tap, and the same on absolute values."""
    m2, xp = rows(m), padded(x)
    a2, ap = m2.abs(), xp.abs()
    d = torch.zeros((m.shape[1], x.shape[1], 3, 3, 3), dtype=torch.float64, device=m.device)
    a = torch.zeros_like(d)
    for kt in range(3):
        for kh in range(3):
            for kw in range(3):
                d[:, :, kt, kh, kw] = m2 @ shifted_rows(xp, kt, kh, kw).t()
                a[:, :, kt, kh, kw] = a2 @ shifted_rows(ap, kt, kh, kw).t()
    return d, a


def _tap_transposed(weight, m):
    """d[b, ci, l, h, w] = sum over co and the taps of weight[co, ci, tap] m[co][b, l - kt + 1, h - kh + 1, w - kw + 1], and
    the same on absolute values."""
    w, mp = f64(weight).to(m.device), padded(m)
    wa, ma = w.abs(), mp.abs()
    d = torch.zeros((w.shape[1], m.numel() // m.shape[1]), dtype=torch.float64, device=m.device)
    a = torch.zeros_like(d)
    for kt in range(3):
        for kh in range(3):
            for kw in range(3):
                d += w[:, :, kt, kh, kw].t() @ shifted_rows(mp, 2 - kt, 2 - kh, 2 - kw)
                a += wa[:, :, kt, kh, kw].t() @ shifted_rows(ma, 2 - kt, 2 - kh, 2 - kw)
    return unrows(d, m), unrows(a, m)


def conv32_wgrad(x, y, upstream):
    """tests/last_conv_ref.py: wgrad -> dict d_weight [32, 32, 3, 3, 3], d_shift [32], abs_weight, abs_shift."""
    m = masked(y, upstream)
    d, a = _tap_sums(m, f64(x))
    return {"d_weight": d, "d_shift": rows(m).sum(dim=1), "abs_weight": a, "abs_shift": rows(m).abs().sum(dim=1)}


def conv32_dgrad(weight, y, upstream):
    """tests/last_conv_dgrad_ref.py: dgrad -> dict d_x, d_res [B, 32, L, H, W], abs_x."""
    m = masked(y, upstream)
    d, a = _tap_transposed(weight, m)
    return {"d_x": d, "d_res": m, "abs_x": a}


def virtual_input(x0, x1):
    """X [B, 96, L, H, W]: X[ci] = x0[ci] at (h >> 1, w >> 1) for ci < 64, x1[ci - 64] behind them."""
    H, W = x1.shape[3], x1.shape[4]
    assert x0.shape[3] == (H + 1) // 2 and x0.shape[4] == (W + 1) // 2 and x0.shape[1] == C0 and x1.shape[1] == C
    ih, iw = torch.arange(H, device=x0.device) >> 1, torch.arange(W, device=x0.device) >> 1
    return torch.cat([x0[:, :, :, ih][:, :, :, :, iw], x1], dim=1)


def convup_wgrad(x0, x1, g1, gd):
    """tests/last_block_ref.py: wgrad -> dict d_weight [32, 96, 3, 3, 3], abs_weight (g1 not None), d_short [32, 96],
    d_short_bias [32], abs_short, abs_short_bias (gd not None)."""
    X = virtual_input(f64(x0), f64(x1))
    out = {}
    if g1 is not None:
        d, a = _tap_sums(f64(g1), X)
        out.update(d_weight=d, abs_weight=a)
    if gd is not None:
        g2, X2 = rows(f64(gd)), rows(X)
        out.update(d_short=g2 @ X2.t(), abs_short=g2.abs() @ X2.abs().t(), d_short_bias=g2.sum(dim=1),
                   abs_short_bias=g2.abs().sum(dim=1))
    return out


def pooled(d_up):
    """The backward of the nearest upsample at h >> 1, w >> 1: [B, C, L, H, W] -> [B, C, L, (H + 1) // 2, (W + 1) // 2], a
    source pixel collecting the output positions that exist (the 2 x 2 pool, ragged at an odd H or W)."""
    B, Cx, L, H, W = d_up.shape
    out = torch.zeros((B, Cx, L, (H + 1) // 2, (W + 1) // 2), dtype=d_up.dtype, device=d_up.device)
    for dh in range(2):
        for dw in range(2):
            part = d_up[:, :, :, dh::2, dw::2]
            out[:, :, :, :part.shape[3], :part.shape[4]] += part
    return out


def convup_dgrad(weight, short_weight, g1, gd):
    """tests/last_block_dgrad_ref.py: dgrad -> dict d_X [B, 96, L, H, W], d_x0 [B, 64, L, H0, W0], d_x1 [B, 32, L, H, W],
    abs_x0, abs_x1, n_x0 [H0, W0].  g1 or gd None: its share is left out."""
    ref = f64(g1 if g1 is not None else gd)
    B, _, L, H, W = ref.shape
    dX = torch.zeros((B, CIN, L, H, W), dtype=torch.float64, device=ref.device)
    aX = torch.zeros_like(dX)
    if g1 is not None:
        d, a = _tap_transposed(weight, f64(g1))
        dX += d
        aX += a
    if gd is not None:
        s, g = f64(short_weight).to(ref.device).reshape(C, CIN), f64(gd)
        dX += unrows(s.t() @ rows(g), g)
        aX += unrows(s.abs().t() @ rows(g).abs(), g)
    n = pooled(torch.ones((1, 1, 1, H, W), dtype=torch.float64, device=ref.device))[0, 0, 0]
    return {"d_X": dX, "d_x0": pooled(dX[:, :C0]), "d_x1": dX[:, C0:].contiguous(), "abs_x0": pooled(aX[:, :C0]),
            "abs_x1": aX[:, C0:].contiguous(), "n_x0": n}


def pred_head_grads(feat, y, upstream, weight):
    """tests/pred_head_ref.py: grads -> dict d_weight [Cout, 32], d_bias [Cout], d_feat [B, 32, L, H, W], abs_weight,
    abs_bias."""
    m = masked(y, upstream)
    f, w = f64(feat), f64(weight).to(m.device).reshape(-1, C)
    m2, f2 = rows(m), rows(f)
    return {"d_weight": m2 @ f2.t(), "d_bias": m2.sum(dim=1), "d_feat": unrows(w.t() @ m2, f),
            "abs_weight": m2.abs() @ f2.abs().t(), "abs_bias": m2.abs().sum(dim=1)}


# ---------------------------------------------------------------------------------------------------------------------
# the walk table: the smallest shapes at which every workgroup of the default grid walks an uneven share of the tiles

WALKS = {"wide": (3, 5, 75, 131),             # 1710 tiles: shares of 6-7 at 256 workgroups, of 20-21 at 85 shares
         "deep": (3, 8, 353, 65)}             # 8496 tiles: shares of 33-34 (one flush of the f32 chain) and 99-100 (three)
CAP_CONV32, CAP_UPWGRAD_SHARES, CAP_UPDGRAD, CAP_HEAD = 256, 85, 256, 512   # the headers' "at most" of the default grids
OTHER_GRID = 97                               # max_workgroups of the second run: uneven shares of another size
HEAD_COUTS = (20, 32)
INT_MAX = 3                                   # the exact check's integers are 1 .. INT_MAX


def pitch_of(w):
    """V2ce3d._pitch: rows of at least 64 floats are padded to a multiple of 32."""
    return w if w < 64 else (w + 31) // 32 * 32


def conv_tiles(B, L, H, W):
    return B * L * ((H + TILE_H - 1) // TILE_H) * ((W + TILE_W - 1) // TILE_W)


def head_tiles(B, L, H, W):
    return (B * L * H * W + HEAD_TILE - 1) // HEAD_TILE


def share_sizes(tiles, shares):
    """The sizes of the contiguous shares [b tiles / shares, (b + 1) tiles / shares) of a persistent grid."""
    return [(b + 1) * tiles // shares - b * tiles // shares for b in range(shares)]


def tile_of(shape, index):
    """-> (b, l, h0, h1, w0, w1): the positions of tile `index` in the kernels' order (frames, tile rows, tile columns)."""
    B, L, H, W = shape
    th, tw = (H + TILE_H - 1) // TILE_H, (W + TILE_W - 1) // TILE_W
    f, r = divmod(index, th * tw)
    i, j = divmod(r, tw)
    return f // L, f % L, i * TILE_H, min(i * TILE_H + TILE_H, H), j * TILE_W, min(j * TILE_W + TILE_W, W)


def integers(gen, shape):
    """Seeded integers 1 .. INT_MAX as f32 (on the CPU: the same values on every machine)."""
    return torch.randint(1, INT_MAX + 1, shape, generator=gen).to(torch.float32)


def normals(gen, shape):
    return torch.randn(shape, generator=gen, dtype=torch.float32)


def signed_zero_normals(gen, shape):
    """A normal tensor with about 1 % of its elements +0.0 and about 1 % -0.0: y > 0 is what decides the mask."""
    y = normals(gen, shape)
    u = torch.rand(shape, generator=gen)
    y[u < 0.01] = 0.0
    y[u > 0.99] = -0.0
    return y


def walk_inputs(shape, exact, seed):
    """The inputs of the four convolution kernels at [B, L, H, W] in the reference's layouts, f32 on the CPU.  exact:
    integers 1 .. 3 and a normal y with signed zeros (check A), else standard normals (check B)."""
    B, L, H, W = shape
    gen = torch.Generator().manual_seed(seed)
    draw = integers if exact else normals
    act, src = (B, C, L, H, W), (B, C0, L, (H + 1) // 2, (W + 1) // 2)
    return {"x": draw(gen, act), "upstream": draw(gen, act), "y": signed_zero_normals(gen, act) if exact else normals(gen, act),
            "weight": draw(gen, (C, C, 3, 3, 3)), "x0": draw(gen, src), "x1": draw(gen, act), "g1": draw(gen, act),
            "gd": draw(gen, act), "weight_up": draw(gen, (C, CIN, 3, 3, 3)), "short": draw(gen, (C, CIN))}


def head_inputs(shape, exact, seed, cout):
    """The inputs of pred_head_grads alike: feat [B, 32, L, H, W], y_head, up_head [B, cout, L, H, W], w_head [cout, 32]."""
    B, L, H, W = shape
    gen = torch.Generator().manual_seed(seed)
    draw = integers if exact else normals
    head = (B, cout, L, H, W)
    return {"feat": draw(gen, (B, C, L, H, W)), "up_head": draw(gen, head), "w_head": draw(gen, (cout, C)),
            "y_head": signed_zero_normals(gen, head) if exact else normals(gen, head)}


def to_c16(a, pitch):
    """[B, 16 G, L, H, W] -> channels-last-16 [B, L, G, H, pitch, 16] f32 on a's device, NaN in the padding columns, with
    ``.lw`` and ``.c16`` as the package's producers set them."""
    B, Cx, L, H, W = a.shape
    out = torch.full((B, L, Cx // 16, H, pitch, 16), float("nan"), dtype=torch.float32, device=a.device)
    out[:, :, :, :, :W, :] = a.reshape(B, Cx // 16, 16, L, H, W).permute(0, 3, 1, 4, 5, 2)
    out.lw, out.c16 = W, True
    return out


def from_c16(c, W):
    """channels-last-16 [B, L, G, H, pitch, 16] -> [B, 16 G, L, H, W] of the logical columns."""
    B, L, G, H, _, _ = c.shape
    return c[:, :, :, :, :W, :].permute(0, 2, 5, 1, 3, 4).reshape(B, G * 16, L, H, W).contiguous()


def to_dense(y):
    """[B, Cout, L, H, W] -> the head kernels' [B, L, Cout, H, W]."""
    return y.permute(0, 2, 1, 3, 4).contiguous()
