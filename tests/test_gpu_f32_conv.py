"""Exact-f32 convolutions against f64, one row per kernel instance, at the ragged edges of the ABI.

The exact-f32 kernels (conv3d_kernel<KS,S,CO_FR,PO_FR,CK,EPT,MW,IL> and conv3d_head_kernel) run every call made with
precision "f32", every call or clip that the split-half range guard reruns, and the reference side of several tests.
Every row of F32_CASES is one instance of the f32 dispatch (v2ce_conv3d_fwd with desc.precision = V2CE_PRECISION_F32),
reached through the model's own entry points (V2ce3d._pack, V2ce3d._conv) at a shape where

- the input channels are ragged: Cin % CK != 0, so the last chunk of CK channels is partial (CK = 4: residues 1 and 3;
  CK = 8: 1, 3 and 7; CK = 2: 1); the channel loop runs >= 3 chunks (each side of a concat: >= 3), so both LDS buffers are
  reused and the interleaved DMA forms (IL = 1) issue into a buffer that held an older chunk.  Exempt: the head row and
  the Cin = 3 row, which have one chunk;
- the output channels are ragged: Cout is a multiple of 4 but not of the channel tile (32 or 64), and the 64-channel forms
  have 3 channel tiles, with an XCD-remapped grid;
- H and W are odd (exempt: the row with W = 2, a stride-2 row on an even width), and some rows have T = 1 or H = 1;
- the batch holds B = 3 sequences scaled by 2^-8, 1 and 2^8 (inputs and residual; the shared BN shift carries 2^-8), so
  sequence 0 is exactly 2^-8 times a unit problem; every row has a residual and an activation.

Checks per row: got_b / 2^k_b against the f64 value / 2^k_b at 1e-5 abs + 1e-5 rel; every output finite; row b of the
batched launch bit-equal to the same launch on sequence b alone; the launch bit-equal under V2CE_XCD_REMAP=0 (another
grid, the same summation order).  test_f32_poisoned_surroundings runs the launch again with the packed weights at the
start of an allocation whose tail holds CK * K3 * Cout + 64 NaNs, and the inputs and the residual inside NaN-filled
allocations (a whole sequence of NaN before the first sequence and after the last): the output must be finite and
bit-equal to the plain launch.  This pins down what the partial last chunk relies on: its weight rows ci0 + ci >= Cin are
fetched with the chunk base in the scalar offset of the buffer load (issue_chunk), past the Cin * K3 * Cout packed
weights, and read 0 only because the descriptor's range check covers the scalar offset too (measured on gfx950: no NaN
reaches an output).  If it did not, they would read what follows the weights, and NaN there times the zero halo of those
channels is NaN.

The f64 reference is evaluated at the position set of conv_ref.positions() (every edge row, column and four time
steps, a seeded 12 % of the rest) when the launch has more than 1.2e10 multiply-adds, everywhere otherwise.

test_f32_table (no GPU) checks each row against the dispatcher's variant query and the properties above;
test_f32_table_covers_the_dispatch sweeps the variant query over shapes and fails on an instance that has no row;
test_f32_network_instances_are_covered (GPU) fails when an f32 forward of the network launches an instance without a row."""
import hashlib
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
if TESTS not in sys.path:                  # (the child process of the remap check runs this file as a script)
    sys.path.insert(0, TESTS)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from conv_ref import at, conv_at, positions  # noqa: E402

TOL = 1e-5
SCALE_EXP = (-8, 0, 8)                     # sequence b is 2^SCALE_EXP[b] times a unit-scale problem
RELU, LEAKY = 1, 2                         # hip.ACT_RELU, hip.ACT_LEAKY

# the instances of the f32 dispatch (conv3d.hip, the block behind V2CE_REQUIRE(d.precision == V2CE_PRECISION_F32 ...)):
# <KS, S, CO_FR, PO_FR, CK, EPT, MW, IL>, CO_TILE = 32 CO_FR, POS_TILE = 128 PO_FR, halo plane <= 256 EPT
F32_INSTANCES = [
    "conv3d_kernel<3,1,1,2,4,8,1,0>",      # 3x3x3 s1, <= 32 channels, small launch (per sequence)
    "conv3d_kernel<3,1,2,3,2,8,1,0>",      # 3x3x3 s1, 384-position boxes (small launch on 17x22-like planes, or large)
    "conv3d_kernel<3,1,2,2,4,8,1,0>",      # 3x3x3 s1, small launch
    "conv3d_kernel<3,1,1,3,2,8,1,0>",      # 3x3x3 s1, <= 32 channels, large launch, 384-position boxes
    "conv3d_kernel<3,1,1,4,2,8,2,1>",      # 3x3x3 s1, <= 32 channels, large launch, 512-position boxes, interleaved DMA
    "conv3d_kernel<3,1,2,4,2,8,2,1>",      # 3x3x3 s1, large launch, 512-position boxes, interleaved DMA
    "conv3d_kernel<3,2,2,3,2,14,1,0>",     # 3x3x3 s2, 384-position boxes
    "conv3d_kernel<3,2,2,2,2,14,1,0>",     # 3x3x3 s2
    "conv3d_kernel<3,2,1,2,2,14,1,0>",     # 3x3x3 s2, <= 32 channels, small launch
    "conv3d_kernel<3,2,1,4,2,14,1,0>",     # 3x3x3 s2, <= 32 channels, large launch
    "conv3d_kernel<1,1,1,4,8,2,2,1>",      # 1x1x1 s1, <= 32 channels, interleaved DMA
    "conv3d_kernel<1,1,2,2,8,2,2,1>",      # 1x1x1 s1, interleaved DMA
    "conv3d_kernel<1,2,1,2,8,8,1,0>",      # 1x1x1 s2, <= 32 channels, small launch
    "conv3d_kernel<1,2,1,4,8,8,1,0>",      # 1x1x1 s2, <= 32 channels, large launch
    "conv3d_kernel<1,2,2,2,8,8,1,0>",      # 1x1x1 s2, small launch
    "conv3d_kernel<1,2,2,4,8,8,1,0>",      # 1x1x1 s2, large launch
    "conv3d_head_kernel",                  # the UNet's head: 3x3x3 s1, 2 -> 32 channels
]


class Case:
    """One f32 launch.  H x W: the logical input plane; src: the low-resolution plane of source 0 of a virtual
    nearest-upsample + concat (C1 > 0), None otherwise."""

    def __init__(self, name, T, C0, Cout, H, W, ks=3, s=1, C1=0, src=None, act=LEAKY, B=3):
        self.name, self.T, self.C0, self.Cout, self.H, self.W = name, T, C0, Cout, H, W
        self.ks, self.s, self.C1, self.src, self.act, self.B = ks, s, C1, src, act, B

    @property
    def cin(self):
        return self.C0 + self.C1

    @property
    def out_hw(self):
        p = self.ks // 2
        return (self.H + 2 * p - self.ks) // self.s + 1, (self.W + 2 * p - self.ks) // self.s + 1

    @property
    def args(self):
        """The template arguments <KS, S, CO_FR, PO_FR, CK, EPT, MW, IL> (None: the head kernel)."""
        return [int(v) for v in self.name[self.name.index("<") + 1:-1].split(",")] if "<" in self.name else None

    @property
    def ck(self):
        return self.args[4]

    @property
    def co_tile(self):
        return 32 * self.args[2]

    def chunks(self):
        """Channel chunks per source: (C0 / CK, ceil(C1 / CK)) for a concat, (ceil(Cin / CK),) otherwise."""
        if self.C1:
            return self.C0 // self.ck, -(-self.C1 // self.ck)
        return (-(-self.C0 // self.ck),)

    def co_tiles(self):
        return -(-self.Cout // self.co_tile)

    def tile(self):
        """The box the launch takes (conv3d.hip choose_tile, restated)."""
        KS, S, CO_FR, PO_FR, CK, EPT = self.args[:6]
        return choose_tile(self.T, *self.out_hw, KS, S, 4 * PO_FR * 32, 256 * EPT)

    def n_spatial(self):
        tt, th, tw = self.tile()
        Ho, Wo = self.out_hw
        return self.B * -(-self.T // tt) * -(-Ho // th) * -(-Wo // tw)

    @property
    def id(self):
        return self.name[self.name.index("<"):] if "<" in self.name else "head"

    def __repr__(self):
        return self.id


def choose_tile(T, Ho, Wo, ks, s, pos_tile, max_plane):
    """conv3d.hip choose_tile: the (tt, th, tw) box of <= pos_tile positions and halo plane <= max_plane that maximises the
    fraction of MFMA lanes computing real outputs, then prefers wide rows and small halos."""
    best, best_eff, best_halo = (1, 1, 1), -1.0, 0
    tt = 1
    while tt <= T and tt <= 16:
        for th in range(1, min(Ho, 64) + 1):
            max_tw = pos_tile // (tt * th)
            if max_tw < 1:
                break
            for tw in range(1, min(Wo, max_tw) + 1):
                plane = (tt + ks - 1) * ((th - 1) * s + ks) * ((tw - 1) * s + ks)
                if plane > max_plane:
                    break
                ntiles = -(-T // tt) * -(-Ho // th) * -(-Wo // tw)
                eff = T * Ho * Wo / (ntiles * pos_tile)
                if eff > best_eff + 1e-9 or (eff > best_eff - 1e-9 and (tw > best[2] or (tw == best[2] and plane < best_halo))):
                    best, best_eff, best_halo = (tt, th, tw), eff, plane
        tt *= 2
    return best


K = "conv3d_kernel"
F32_CASES = [
    # -- 3x3x3 stride 1
    Case(f"{K}<3,1,1,2,4,8,1,0>", 1, 9, 12, 37, 53),                          # T = 1; Cin % 4 = 1
    Case(f"{K}<3,1,2,3,2,8,1,0>", 3, 8, 164, 55, 57, C1=5, src=(23, 21)),   # upsample 23x21 -> 55x57 (not 2x) ++ skip
    Case(f"{K}<3,1,2,2,4,8,1,0>", 5, 11, 140, 29, 41, act=RELU),             # Cin % 4 = 3
    Case(f"{K}<3,1,1,3,2,8,1,0>", 16, 7, 28, 65, 67),
    Case(f"{K}<3,1,1,4,2,8,2,1>", 16, 7, 20, 63, 73),
    Case(f"{K}<3,1,2,4,2,8,2,1>", 16, 5, 164, 39, 39),
    # -- 3x3x3 stride 2
    Case(f"{K}<3,2,2,3,2,14,1,0>", 3, 5, 180, 25, 41, s=2),
    Case(f"{K}<3,2,2,2,2,14,1,0>", 3, 7, 148, 25, 31, s=2, act=RELU),
    Case(f"{K}<3,2,1,2,2,14,1,0>", 5, 5, 4, 301, 2, s=2),                    # W = 2: even width, one output column
    Case(f"{K}<3,2,1,4,2,14,1,0>", 16, 7, 24, 129, 129, s=2),
    # -- 1x1x1
    Case(f"{K}<1,1,1,4,8,2,2,1>", 4, 24, 20, 19, 27, ks=1, C1=17, src=(10, 14)),   # upsample 2x ++ skip
    Case(f"{K}<1,1,2,2,8,2,2,1>", 7, 23, 164, 1, 301, ks=1, act=RELU),       # H = 1; Cin % 8 = 7
    Case(f"{K}<1,2,1,2,8,8,1,0>", 4, 3, 28, 45, 57, ks=1, s=2),             # Cin = 3: one chunk
    Case(f"{K}<1,2,1,4,8,8,1,0>", 16, 17, 8, 129, 129, ks=1, s=2),
    Case(f"{K}<1,2,2,2,8,8,1,0>", 3, 23, 180, 27, 39, ks=1, s=2),
    Case(f"{K}<1,2,2,4,8,8,1,0>", 8, 17, 172, 105, 105, ks=1, s=2, act=RELU),
    # -- the head
    Case("conv3d_head_kernel", 5, 2, 32, 67, 93),
]


def _desc(c, B=None):
    from v2ce_toolbox_amd import hip
    Ho, Wo = c.out_hw
    H0, W0 = c.src if c.src else (c.H, c.W)
    return hip.ConvDesc(B=c.B if B is None else B, T=c.T, C0=c.C0, H0=H0, W0=W0, C1=c.C1, Hin=c.H, Win=c.W, Cout=c.Cout,
                        Hout=Ho, Wout=Wo, ksize=c.ks, stride_hw=c.s, act=c.act, tile_t=0, tile_h=0, tile_w=0,
                        precision=hip.PRECISION_F32, W0_pitch=0, Win_pitch=0, Wout_pitch=0, layout=hip.LAYOUT_PLANAR,
                        absmax_batch_stride=0)


@pytest.mark.parametrize("case", F32_CASES, ids=lambda c: c.id)
def test_f32_table(case):
    """The row's instance is what the f32 dispatch picks for its shape (the variant query launches nothing: no GPU
    needed), and the row has the properties the module docstring lists."""
    from v2ce_toolbox_amd import hip
    assert (RELU, LEAKY) == (hip.ACT_RELU, hip.ACT_LEAKY)
    assert hip.conv_variant(_desc(case), case.src is not None, 0) == case.name
    for B in (1, 2):                  # the choice is made per sequence: the same instance for any batch
        assert hip.conv_variant(_desc(case, B), case.src is not None, 0) == case.name
    assert case.B == 3
    if case.name == "conv3d_head_kernel":
        return
    assert case.Cout % 4 == 0 and case.Cout % case.co_tile != 0, (case.Cout, case.co_tile)
    if case.co_tile == 64:
        assert case.co_tiles() == 3
    assert case.W <= 2 or (case.H % 2 == 1 and case.W % 2 == 1)
    assert (case.C1 == 0) == (case.src is None)
    if case.C1:
        assert case.C0 % case.ck == 0 and all(n >= 3 for n in case.chunks()), case.chunks()
        assert case.C1 % case.ck != 0
    elif case.cin > 3:
        assert case.chunks()[0] >= 3 and case.cin % case.ck != 0, (case.cin, case.ck)
    else:
        assert case.cin % case.ck != 0


def test_f32_table_edges():
    """The edges the table covers as a whole."""
    rows = [c for c in F32_CASES if c.name != "conv3d_head_kernel"]
    assert sorted(c.name for c in F32_CASES) == sorted(F32_INSTANCES)
    for ck in (2, 4, 8):                           # ragged residues of the last chunk: 1 and CK - 1
        res = {(c.C1 or c.cin) % c.ck for c in rows if c.ck == ck}
        assert {1, ck - 1} <= res, (ck, res)
    assert any(c.C1 == 0 and c.cin in (2, 3) for c in rows)
    assert any(c.T == 1 for c in rows) and any(c.W <= 2 for c in rows) and any(c.H == 1 for c in rows)
    assert any(c.s == 2 and c.W % 2 == 0 for c in rows)
    assert any(c.n_spatial() % 8 != 0 and c.co_tiles() > 1 for c in rows)
    ups = [c for c in rows if c.C1]
    assert {(c.ks, c.s) for c in ups} == {(3, 1), (1, 1)}
    assert any(c.src != ((c.H + 1) // 2, (c.W + 1) // 2) for c in ups)         # a ratio that is not 2
    assert any(c.args[7] == 1 and c.ks == 3 for c in rows) and any(c.args[7] == 1 and c.ks == 1 for c in rows)


def test_f32_table_covers_the_dispatch():
    """The f32 dispatch over a sweep of shapes (kernel sizes, strides, channel counts, the network's planes and ragged
    ones, T 1..16, with and without a virtual concat) picks no instance outside F32_INSTANCES, and reaches every one."""
    from v2ce_toolbox_amd import hip
    seen = set()
    planes = ((1, 1), (2, 2), (1, 301), (9, 11), (17, 22), (33, 44), (37, 53), (39, 39), (65, 87), (63, 73), (130, 173),
              (129, 129), (255, 263), (260, 346))
    for ks, s in ((3, 1), (3, 2), (1, 1), (1, 2)):
        for cout in (4, 20, 32, 36, 64, 100, 164, 256):
            for T in (1, 2, 4, 16):
                for H, W in planes:
                    for cin, c1 in ((2, 0), (3, 0), (17, 0), (64, 0), (32, 32)):
                        c = Case("sweep", T, cin, cout, H, W, ks=ks, s=s, C1=c1,
                                 src=((H + 1) // 2, (W + 1) // 2) if c1 else None)
                        d = _desc(c)
                        if T * cout * c.out_hw[0] * c.out_hw[1] >= 1 << 29:
                            continue
                        seen.add(hip.conv_variant(d, c1 > 0, 0))
    assert seen == set(F32_INSTANCES), (sorted(seen - set(F32_INSTANCES)), sorted(set(F32_INSTANCES) - seen))


# ------------------------------------------------------------------------------------------------
# inputs and the f64 reference
# ------------------------------------------------------------------------------------------------
def _inputs(c):
    """CPU float32 tensors (NCDHW) of the case; sequence b carries the factor 2^SCALE_EXP[b]."""
    g = torch.Generator().manual_seed(zlib.crc32(c.name.encode()) & 0x7FFFFFFF)
    B, T, Cout = c.B, c.T, c.Cout
    Ho, Wo = c.out_hw
    k = torch.tensor([2.0 ** SCALE_EXP[b] for b in range(B)]).view(B, 1, 1, 1, 1)
    H0, W0 = c.src if c.src else (c.H, c.W)
    I = {"k": k, "x0": torch.randn(B, c.C0, T, H0, W0, generator=g) * k}
    if c.C1:
        I["x1"] = torch.randn(B, c.C1, T, c.H, c.W, generator=g) * k
    I["w"] = torch.randn(Cout, c.cin, c.ks, c.ks, c.ks, generator=g) * (2.0 / (c.cin * c.ks ** 3)) ** 0.5
    I["scale"] = torch.rand(Cout, generator=g) + 0.5
    I["shift"] = 0.3 * torch.randn(Cout, generator=g) * 2.0 ** SCALE_EXP[0]
    I["res"] = torch.randn(B, Cout, T, Ho, Wo, generator=g) * k
    return I


def reference(c, I, pos):
    """f64 output of the case at the positions: [N, Cout]."""
    from oracle import unet as U
    col = lambda v: v.double().view(1, -1)
    x = I["x0"].double()
    if c.C1:
        x = torch.cat([U.upsample_nearest_hw(I["x0"], (c.H, c.W)).double(), I["x1"].double()], dim=1)
    y = conv_at(x, I["w"], c.s, pos) * col(I["scale"]) + col(I["shift"]) + at(I["res"].double(), pos)
    return torch.relu(y) if c.act == RELU else F.leaky_relu(y, 0.01)


# ------------------------------------------------------------------------------------------------
# the launches, through the model's entry points
# ------------------------------------------------------------------------------------------------
def _btchw(x):
    return x.permute(0, 2, 1, 3, 4).contiguous()


def _device(x, poison):
    """CPU tensor -> device; poison: inside a NaN-filled allocation with one sequence's worth of NaN on either side."""
    if not poison:
        return x.cuda()
    pad = max(4096, x[0].numel())
    buf = torch.full((2 * pad + x.numel(),), float("nan"), device="cuda")
    v = buf[pad:pad + x.numel()].view(x.shape)
    v.copy_(x.cuda())
    return v


def launch(c, I, poison=False):
    """The case's launch on the batch in I: {"y": NCDHW float32 numpy, "names": the profile's launches}."""
    from v2ce_toolbox_amd.v2ce_3d import V2ce3d
    m = V2ce3d.__new__(V2ce3d)
    torch.nn.Module.__init__(m)
    m._maps, m.precision, m.profile = {}, "f32", []
    w = I["w"].cuda().contiguous()
    n = w.numel()
    wp = None
    if poison:                       # the packed weights, then >= one chunk's worth of NaN
        ck = c.ck if c.args else 2
        buf = torch.full((n + ck * c.ks ** 3 * c.Cout + 64,), float("nan"), device="cuda")
        wp = buf[:n]
    wp = V2ce3d._pack(m, w, out=wp)
    x0 = _device(_btchw(I["x0"]), poison)
    x1 = _device(_btchw(I["x1"]), poison) if c.C1 else None
    res = _device(_btchw(I["res"]), poison)
    y = V2ce3d._conv(m, x0, x1, wp, I["scale"].cuda(), I["shift"].cuda(), c.Cout, c.ks, c.s, c.act, residual=res,
                     up_to=(c.H, c.W) if c.C1 else None, dense_out=True)
    torch.cuda.synchronize()
    return {"y": y.permute(0, 2, 1, 3, 4).cpu().numpy(), "names": [p[0] for p in m.profile]}


def _sub(I, b):
    """The inputs of sequence b alone (shared tensors as they are)."""
    return {k: (v[b:b + 1].contiguous() if k in ("k", "x0", "x1", "res") else v) for k, v in I.items()}


def _digest(y):
    return hashlib.sha256(np.ascontiguousarray(y).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def remap_off():
    """{case id: digest of the output} of every row's launch in a child process with V2CE_XCD_REMAP=0 (the switch is
    read once per process)."""
    env = dict(os.environ, V2CE_XCD_REMAP="0")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__)]
    r = subprocess.run(cmd, env=env, cwd=ROOT, timeout=600, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
@pytest.mark.parametrize("case", F32_CASES, ids=lambda c: c.id)
def test_f32_vs_f64(case, remap_off):
    I = _inputs(case)
    got = launch(case, I)
    assert got["names"] == [case.name], got["names"]
    y = got["y"]
    assert np.isfinite(y).all(), f"{case.id}: {int((~np.isfinite(y)).sum())} outputs are not finite"
    Ho, Wo = case.out_hw
    B, T = case.B, case.T
    full = B * T * Ho * Wo * case.Cout * case.cin * case.ks ** 3 < 1.2e10
    pos = positions(B, T, Ho, Wo, zlib.crc32(case.name.encode()) & 0xFFFF, frac=1.0 if full else 0.12)
    want = reference(case, I, pos)
    k = I["k"].view(-1).double()[pos[0]].view(-1, 1)
    g_, w_ = at(torch.from_numpy(y).double(), pos) / k, want / k
    assert g_.shape == w_.shape
    d = (g_ - w_).abs()
    excess = d - TOL * w_.abs()
    i = int(torch.argmax(excess.max(dim=1).values))
    j = int(torch.argmax(excess[i]))
    where = (int(pos[0][i]), j, int(pos[1][i]), int(pos[2][i]), int(pos[3][i]))
    assert float(excess[i, j]) <= TOL, (f"{case.id}: max excess at (b, c, t, h, w) = {where}: got {float(g_[i, j])!r} "
                                        f"want {float(w_[i, j])!r} (unit scale)")
    # batch invariance: each sequence alone gives its rows bit for bit
    for b in range(B):
        alone = launch(case, _sub(I, b))["y"]
        assert np.array_equal(alone[0].view(np.int32), y[b].view(np.int32)), (case.id, b)
    # the grid without the XCD remap: the same summation order, the same bits
    assert remap_off[case.id] == _digest(y), f"{case.id}: V2CE_XCD_REMAP=0 changes the output"
    print(f"F32 {case.id} tile={case.tile() if case.args else None} co_tiles={case.co_tiles() if case.args else 1} "
          f"positions={pos[0].numel()}/{B * T * Ho * Wo} max|d|={float(d.max()):.3e} max_excess={float(excess[i, j]):.3e}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", F32_CASES, ids=lambda c: c.id)
def test_f32_poisoned_surroundings(case):
    """NaN after the packed weights (>= one chunk of CK input channels: the rows of a partial last chunk must not be
    read from there), around the inputs and the residual: the output is finite and equals the plain launch bit for bit."""
    I = _inputs(case)
    plain = launch(case, I)["y"]
    got = launch(case, I, poison=True)["y"]
    bad = ~np.isfinite(got)
    assert not bad.any(), (f"{case.id}: {int(bad.sum())} outputs are not finite, in channels "
                           f"{sorted(set(np.nonzero(bad)[1].tolist()))[:16]}")
    assert np.array_equal(plain.view(np.int32), got.view(np.int32)), case.id


@pytest.mark.gpu
def test_f32_network_instances_are_covered():
    """One f32 forward at 346 x 260, T = 16, B = 1, 4, 8: every conv instance it launches has a row in F32_CASES (the
    range guard reruns a call at the same shapes on these kernels)."""
    from oracle import glue as OG
    from v2ce_toolbox_amd import synth
    from v2ce_toolbox_amd.v2ce_3d import V2ce3d
    table = {c.name for c in F32_CASES}
    x1 = OG.preprocess(synth.synthetic_frames(17, 260, 346, seed=9))
    m = V2ce3d(precision="f32")
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


if __name__ == "__main__":
    # the child of the remap_off fixture: the digest of every row's launch, as one JSON line
    print(json.dumps({c.id: _digest(launch(c, _inputs(c))["y"]) for c in F32_CASES}))
