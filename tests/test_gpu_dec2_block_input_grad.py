"""The third decoder block as a complete autograd node (dec2_block.py: Dec2ConvsThrough(input_grads=True),
Dec2BlockThrough) on the GPU, on the exact-f32 model and the [1, 2, 2, 16, 16] synthetic input of
tests/test_gpu_dec2_block_model.py: the gradients with respect to the block's two sources h1 [1, 2, 8, 4, 4, 16] and s2
[1, 2, 4, 8, 8, 16].

The layer's gradients are the bytes of a direct ``convupn_dgrad`` call; only the sources that need one are asked for.

Against torch's f64 autograd on a replica of the block's first half built from the layer's own tensors -- W = W_bar / sigma
with sigma = u . (W_bar v) of the layer's u, v after the forward's power iteration, the frozen statistics, F.interpolate +
cat + conv3d -- the bound is the chain tests/test_gpu_last_block_input_grad.py documents, with the gradients of (z1, zd)
given exactly (so nothing is carried).  With eps = 2^-24, Wf1 = rs1 W and Wfd = rsd Wd the folded weights, S1 / Sd the f64
sums of |Wf1| |g1| and |Wfd| |gd| over an element's terms, S = S1 + Sd, n the element's term count (V2CE_UPNDGRAD_TERMS(64)
for d_s2, times its 1, 2 or 4 output positions for d_h1):
  kernel   the header of v2ce_convupn_dgrad on the folded weights: (n + 1) eps S + n 2^-126
  folds    Wf1 and Wfd are f32 products (one rounding per term) of rs = 1 / sqrt(var + eps_bn), itself three f32 roundings:
           8 eps S covers both with room
  W        W_bar / sigma derived in f32: 4 (rows + cols) kappa eps = 4 (64 + 5184) kappa eps relative, on S1 alone, with
           kappa = sum |u_i| |W_bar_ij| |v_j| / |sigma|
plus one f32 ulp of the truth.  Every result is printed as a fraction of its bound."""
import numpy as np
import pytest
import torch
from torch import nn

from test_gpu_dec2_block_model import sources
from test_gpu_last_block_autograd import teacher
from test_gpu_last_conv_autograd import EPS32, make_model, x_dev
from tests import convupn_dgrad_ref as R
from v2ce_toolbox_amd import dec2_block, losses
from v2ce_toolbox_amd.dec2_block import Dec2Block, Dec2BlockThrough, Dec2ConvsThrough
from v2ce_toolbox_amd.last_block import LastBlock
from v2ce_toolbox_amd.pred_head import PredHead

pytestmark = pytest.mark.gpu

C, C0, C1 = 64, 128, 64
ROWS, COLS = 64, 192 * 27


def leaf(t, requires_grad=True):
    """A copy of a source as a leaf of its own, with the attributes a channels-last-16 tensor carries."""
    c = t.detach().clone().requires_grad_(requires_grad)
    c.lw, c.c16 = t.lw, True
    return c


def upstream(z, seed):
    """A seeded gradient for a channels-last-16 output: standard normals in the logical columns, zeros in the padding."""
    g = torch.randn(z.shape, generator=torch.Generator().manual_seed(seed)).cuda()
    g[:, :, :, :, z.lw:, :] = 0
    return g


def logical(t, lw):
    """channels-last-16 on the device -> [B, 16 G, L, H, lw] f64; the padding columns are zeros."""
    a = t.detach().cpu().numpy()
    assert not np.isnan(a).any() and not a[:, :, :, :, lw:, :].any()
    return R.from_c16(a, lw).astype(np.float64)


def first_half(m, need0=True, need1=True):
    """Dec2ConvsThrough on the model's sources, backward from seeded gradients of (z1, zd) -> (layer, h1, s2, g1, gd)."""
    h1, s2, _ = sources(m, x_dev())
    convs = Dec2ConvsThrough.from_model(m, input_grads=True)
    h1, s2 = leaf(h1, need0), leaf(s2, need1)
    z1, zd = convs(h1, s2)
    g1, gd = upstream(z1, 11), upstream(zd, 12)
    torch.autograd.backward([z1, zd], [g1, gd])
    return convs, h1, s2, g1, gd


def test_backward_fills_both_sources_with_the_bytes_of_a_direct_call(monkeypatch):
    m = make_model("f32")
    calls = []
    real = dec2_block.convupn_dgrad

    def spy(*a, **k):
        calls.append((a, dict(k)))
        return real(*a, **k)
    monkeypatch.setattr(dec2_block, "convupn_dgrad", spy)
    convs, h1, s2, g1, gd = first_half(m)
    assert convs.input_grads is True and len(calls) == 1
    for t, planes in ((h1, 8), (s2, 4)):
        assert t.grad is not None and t.grad.shape == t.shape and t.shape[2] == planes
        a = t.grad.cpu().numpy()
        assert not np.isnan(a).any() and not a[:, :, :, :, t.lw:, :].any()
        assert np.count_nonzero(a[:, :, :, :, :t.lw, :]) > a[:, :, :, :, :t.lw, :].size // 2
    assert (h1.lw, s2.lw) == (4, 8)
    (a, k), = calls
    assert tuple(k["want"]) == ("x0", "x1") and set(k["out"]) == {"x0"} and tuple(k["out"]["x0"].shape) == tuple(h1.shape)
    assert tuple(a[0].shape) == (C, C0 + C1, 3, 3, 3) and tuple(a[1].shape) == (C, C0 + C1)
    direct = real(*a, want=("x0", "x1"))
    assert torch.equal(direct["x0"], h1.grad) and torch.equal(direct["x1"], s2.grad)
    assert direct["x0"].lw == 4 and direct["x1"].lw == 8
    # the layer's own parameters got their gradients in the same backward
    assert all(p.grad is not None and float(p.grad.abs().max()) > 0 for p in convs.parameters())
    # only the sources that need a gradient are asked for, and nothing is launched when neither does
    both0, both1 = h1.grad.clone(), s2.grad.clone()
    calls.clear()
    _, h1, s2, _, _ = first_half(m, need1=False)
    assert [tuple(k["want"]) for _, k in calls] == [("x0",)] and s2.grad is None and torch.equal(h1.grad, both0)
    calls.clear()
    _, h1, s2, _, _ = first_half(m, need0=False)
    assert [tuple(k["want"]) for _, k in calls] == [("x1",)] and calls[0][1]["out"] is None and h1.grad is None
    assert torch.equal(s2.grad, both1)
    calls.clear()
    convs, h1, s2, _, _ = first_half(m, need0=False, need1=False)
    assert not calls and h1.grad is None and s2.grad is None and convs.weight_bar.grad is not None


def test_source_gradients_match_torch_f64_autograd_on_a_replica_of_the_first_half():
    m = make_model("f32")
    convs, h1, s2, g1, gd = first_half(m)
    f64 = lambda t: t.detach().cpu().double()
    wb, u, v = f64(convs.weight_bar), f64(convs.weight_u), f64(convs.weight_v)      # u, v: after the forward's iteration
    sigma = u.dot(wb.view(ROWS, COLS).mv(v))
    kappa = float((u.abs()[:, None] * wb.view(ROWS, COLS).abs() * v.abs()[None, :]).sum() / sigma.abs())
    W = wb / sigma
    rs1 = 1.0 / torch.sqrt(f64(convs.bn1_var) + float(convs.eps))
    rsd = 1.0 / torch.sqrt(f64(convs.bnd_var) + float(convs.eps))
    x0 = torch.from_numpy(logical(h1, 4)).requires_grad_(True)
    x1 = torch.from_numpy(logical(s2, 8)).requires_grad_(True)
    G1, GD = torch.from_numpy(logical(g1, 8)), torch.from_numpy(logical(gd, 8))
    B, _, L, H, Wd = x1.shape
    X = torch.cat([nn.functional.interpolate(x0, size=(L, H, Wd), mode="nearest"), x1], dim=1)
    bc = lambda p: p.view(1, C, 1, 1, 1)
    z1 = (nn.functional.conv3d(X, W, padding=1) - bc(f64(convs.bn1_mean))) * bc(rs1)
    zd = (nn.functional.conv3d(X, f64(convs.short_weight), bias=f64(convs.short_bias)) - bc(f64(convs.bnd_mean))) * bc(rsd)
    ((z1 * G1).sum() + (zd * GD).sum()).backward()
    # S1, Sd and the restated gradient on the folded weights
    wf1, wfd = (rs1.view(C, 1, 1, 1, 1) * W).numpy(), (rsd.view(C, 1) * f64(convs.short_weight).view(C, C0 + C1)).numpy()
    s1 = R.dgrad(C0, C1, C, wf1, None, G1.numpy(), None)
    sd = R.dgrad(C0, C1, C, None, wfd, None, GD.numpy())
    n = {"x0": R.terms(C) * R.pooled(np.ones((1, 1, 1, H, Wd))), "x1": R.terms(C)}
    print(f"kappa = {kappa:.3f}")
    for k, got, want in (("x0", logical(h1.grad, 4), x0.grad.numpy()), ("x1", logical(s2.grad, 8), x1.grad.numpy())):
        S1, Sd = s1[f"abs_{k}"], sd[f"abs_{k}"]
        assert np.abs(s1[f"d_{k}"] + sd[f"d_{k}"] - want).max() <= 1e-11 * np.abs(want).max()       # the replica is the header's sum
        bound = R.dgrad_bound(S1 + Sd, n[k]) + 8 * EPS32 * (S1 + Sd) + 4 * (ROWS + COLS) * kappa * EPS32 * S1 + R.ulp32(want)
        err = np.abs(got - want)
        print(f"d_{'h1' if k == 'x0' else 's2'}: max error {err.max():.3e}, {float((err / bound).max()):.4f} of its bound")
        assert got.shape == want.shape and np.all(err <= bound), (k, float(err.max()))
        assert np.abs(want).max() > 0


def step(m, cls, need):
    """One cls -> LastBlock -> PredHead -> calculate_loss -> backward on fresh layers -> (modules, h1, s2)."""
    x = x_dev()
    gt = teacher(m, x)
    h1, s2, x1 = sources(m, x)
    mods = (cls.from_model(m), LastBlock.from_model(m), PredHead.from_model(m))
    h1, s2 = leaf(h1, need), leaf(s2, need)
    dec2, block, head = mods
    losses.calculate_loss(head(block(dec2(h1, s2), x1)), gt)[0].backward()
    return mods, h1, s2


def test_whole_chain_gives_source_gradients_and_keeps_the_parameter_gradients_bytes():
    m = make_model("f32")
    through, h1, s2 = step(m, Dec2BlockThrough, True)
    assert isinstance(through[0].convs, Dec2ConvsThrough) and through[0].convs.input_grads is True
    assert len(list(through[0].parameters())) == 10
    assert all(p.grad is not None and float(p.grad.abs().max()) > 0 for mod in through for p in mod.parameters())
    for t in (h1, s2):
        assert t.grad is not None and t.grad.shape == t.shape and float(t.grad.abs().max()) > 0
        assert not t.grad[:, :, :, :, t.lw:, :].any()
    plain, p1, p2 = step(m, Dec2Block, False)
    assert p1.grad is None and p2.grad is None
    for a, b in zip(through, plain):
        pa, pb = dict(a.named_parameters()), dict(b.named_parameters())
        assert list(pa) == list(pb)
        for k in pa:
            assert torch.equal(pa[k].grad, pb[k].grad), k           # asking for input gradients changes nothing else
    assert list(through[0].state_dict()) == list(plain[0].state_dict())
    plain[0].load_state_dict(through[0].state_dict())
    # the split: the older class refuses what the new one takes
    with pytest.raises(ValueError, match="no gradient with respect to x0 and x1"):
        Dec2Block.from_model(m)(leaf(h1), leaf(s2, False))


class Affine(nn.Module):
    """A per-channel scale and shift on a channels-last-16 tensor with 16 G channels: a layer of the caller's own."""

    def __init__(self, planes):
        super().__init__()
        self.scale = nn.Parameter(torch.ones(planes, 1, 1, 16))
        self.shift = nn.Parameter(torch.zeros(planes, 1, 1, 16))

    def forward(self, t):
        y = t * self.scale + self.shift
        y = torch.cat([y[..., :t.lw, :], torch.zeros_like(y[..., t.lw:, :])], dim=-2)      # (padding columns stay zeros)
        y.lw, y.c16 = t.lw, True
        return y


def test_a_layer_in_front_of_h1_trains_through_the_block():
    """Plain gradient descent on the affine layer alone, the three blocks rebuilt from the model at every step (so their
    spectral-norm vectors start from the same state and the loss is one fixed function of the affine parameters).  The step
    size comes from the first gradient: lr = 0.02 loss / |grad|^2 takes about 2 % off the loss per step to first order.
    Deterministic, because the kernels are."""
    m = make_model("f32")
    x = x_dev()
    gt = teacher(m, x)
    h1, s2, x1 = sources(m, x)
    mine = Affine(8).cuda()
    loss, lr = [], None
    for _ in range(4):
        dec2, block, head = Dec2BlockThrough.from_model(m), LastBlock.from_model(m), PredHead.from_model(m)
        mine.zero_grad()
        total = losses.calculate_loss(head(block(dec2(mine(h1), s2), x1)), gt)[0]
        loss.append(float(total.detach()))
        total.backward()
        grads = [p.grad for p in mine.parameters()]
        assert all(g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in grads)
        if lr is None:
            lr = 0.02 * loss[0] / float(sum((g.double() ** 2).sum() for g in grads))
        with torch.no_grad():
            for p in mine.parameters():
                p.sub_(lr * p.grad)
    print(f"affine layer in front of h1: lr {lr:.3e}, losses {loss}")
    assert loss[3] < loss[0] and all(np.isfinite(loss))
    assert float((mine.scale.detach() - 1).abs().max()) > 0 and float(mine.shift.detach().abs().max()) > 0
