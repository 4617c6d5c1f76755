"""The last decoder block as a complete autograd node (last_block.py: TailConvs(input_grads=True), LastBlock) on the GPU:
the gradients with respect to the block's two sources against the reference block's own f64 autograd
(tests/golden/.lastblock_dgrad/NAME.layer.*.npz), on an exact-f32 model.

The bound is a first-order propagation of the kernels' contracts on top of the chain of
tests/test_gpu_last_block_autograd.py (whose E_g1 and E_gd -- the errors of the device's gradients of z1 and zd -- are
formed here by the same expressions), not something the code gave.  With eps = 2^-24, Wf1 = rs1 W1 and Wfd = rsd Wd the
folded weights, S1 / Sd the f64 sums of |Wf1| |g1| and |Wfd| |gd| over an element's terms, S = S1 + Sd, n the element's
term count (V2CE_UPDGRAD_TERMS for d_x1, times its 1, 2 or 4 output positions for d_x0):
  kernel   the header of v2ce_convup_dgrad on the folded weights: (n + 1) eps S + n 2^-126
  folds    Wf1 and Wfd are f32 products (one rounding per term) of rs = 1 / sqrt(var + eps_bn), itself three f32 roundings:
           8 eps S covers both with room
  W1       W_bar1 / sigma1 derived in f32: 4 (rows + cols) kappa1 eps = 4 * 2624 kappa1 eps relative, on S1 alone -- the
           term the existing chain test uses
  carried  the kernel's sums are linear in (g1, gd): the same sums on (|Wf1|, |Wfd|) and (E_g1, E_gd)
plus one f32 ulp of the truth.  Every result is printed as a fraction of its bound next to the reference's own f32 deviation."""
import numpy as np
import pytest
import torch

from test_gpu_last_block_autograd import chain_bounds, close, kappa_of, layers_from_golden, src_dev, teacher
from test_gpu_last_conv_autograd import EPS32, c16_dev, f32_model, x_dev
from tests import last_block_dgrad_ref as D
from tests import last_block_ref as R
from tests import last_conv_dgrad_ref as D2
from tests.make_last_block_goldens import CASES, KERNEL_ONLY
from v2ce_toolbox_amd import hip, last_block, losses
from v2ce_toolbox_amd.last_block import LastBlock
from v2ce_toolbox_amd.pred_head import PredHead

pytestmark = pytest.mark.gpu

LAYER_CASES = [n for n in sorted(CASES) if n not in KERNEL_ONLY]
PARAM_GRADS = ("convs.weight_bar", "convs.short_weight", "convs.short_bias", "norms.bn1_weight", "norms.bn1_bias", "norms.bnd_weight",
               "norms.bnd_bias", "conv.weight_bar", "conv.bn_weight", "conv.bn_bias")


def block_from_golden(z, model, input_grads=True):
    convs, norms, conv = layers_from_golden(z, model)
    convs.input_grads = input_grads
    return LastBlock(convs, norms, conv)


def param_grads(block):
    named = dict(block.named_parameters())
    assert set(named) == set(PARAM_GRADS)
    return {k: named[k].grad for k in PARAM_GRADS}


def source_logical(t, lw):
    """channels-last-16 [B, L, G, H, pitch, 16] on the device -> [B, 16 G, L, H, lw] f64; the padding columns are zeros."""
    a = t.detach().cpu().numpy()
    assert not np.isnan(a).any() and not a[:, :, :, :, lw:, :].any()
    B, L, G, H, _, _ = a.shape
    return np.ascontiguousarray(a[:, :, :, :, :lw, :].transpose(0, 2, 5, 1, 3, 4).reshape(B, G * 16, L, H, lw)).astype(np.float64)


def input_grad_bounds(z, p, f, g):
    """The module docstring's bounds of (d_x0, d_x1), without the final ulp."""
    k1 = kappa_of(p["weight_bar1"], f["u1a"], f["v1a"], f["sigma1"])
    k2 = kappa_of(p["weight_bar2"], f["u2a"], f["v2a"], f["sigma2"])
    # E_g1, E_gd: the expressions of tests/test_gpu_last_block_autograd.py::chain_bounds
    mask_t = f["pre1"] > 0
    aw1 = R.bc(np.abs(p["bn1_weight"]))
    S2 = g["abs_d_t"]
    e_dt = D2.dgrad_bound(S2, hip.DGRAD_TERMS) + (4 * 896 * k2 + 8) * EPS32 * S2
    e_g1 = np.where(mask_t, aw1 * e_dt, 0.0) + EPS32 * np.abs(g["g1"])
    e_gd = EPS32 * np.abs(g["gd"])
    wf1 = f["rs1"][:, None, None, None, None] * f["W1"]
    wfd = f["rsd"][:, None] * np.asarray(p["short_weight"], np.float64).reshape(32, 96)
    s1, sd = D.dgrad(wf1, None, g["g1"], None), D.dgrad(None, wfd, None, g["gd"])
    carried = D.dgrad(np.abs(wf1), np.abs(wfd), e_g1, e_gd)
    H, W = g["g1"].shape[3], g["g1"].shape[4]
    n = {"x0": hip.UPDGRAD_TERMS * D.pooled(np.ones((1, 1, 1, H, W))), "x1": hip.UPDGRAD_TERMS}
    out = {}
    for k in ("x0", "x1"):
        S1, Sd = s1[f"abs_{k}"], sd[f"abs_{k}"]
        out[k] = D.dgrad_bound(S1 + Sd, n[k]) + 8 * EPS32 * (S1 + Sd) + 4 * 2624 * k1 * EPS32 * S1 + carried[f"d_{k}"]
    return out, {"x0": s1["d_x0"] + sd["d_x0"], "x1": s1["d_x1"] + sd["d_x1"]}


@pytest.mark.parametrize("name", LAYER_CASES)
def test_block_input_gradients_match_the_reference_blocks_autograd(name):
    z = D.load_case(name)
    p = {k: z[k] for k in R.PARAMS}
    block = block_from_golden(z, f32_model())
    x0, x1 = src_dev(z["x0"]).requires_grad_(True), c16_dev(z["x1"]).requires_grad_(True)   # (padding columns hold NaN)
    feat = block(x0, x1)
    assert feat.grad_fn is not None and feat.lw == z["x1"].shape[-1]
    feat.backward(c16_dev(z["upstream"]))
    assert x0.grad.shape == x0.shape and x1.grad.shape == x1.shape
    f = R.block_forward(z["x0"], z["x1"], p)
    g = R.block_grads(z["x0"], z["x1"], p, z["upstream"], f)
    bounds, restated = input_grad_bounds(z, p, f, g)
    for k, t, lw in (("x0", x0.grad, z["x0"].shape[-1]), ("x1", x1.grad, z["x1"].shape[-1])):
        want = z[f"ref64_layer_d_{k}"]
        assert np.abs(restated[k] - want).max() <= 1e-11 * max(np.abs(want).max(), 1e-300)
        got = source_logical(t, lw)
        err, bound = np.abs(got - want), bounds[k] + R.ulp32(want)
        print(f"{name}: d_{k}: max error {err.max():.3e}, {float((err / bound).max()):.4f} of its bound; reference f32 "
              f"{float(z[f'ref32_dev_layer_d_{k}']):.3e}")
        assert got.shape == want.shape and np.all(err <= bound), (name, k, float(err.max()))
        if name == "zero":
            assert not got.any()
        else:
            assert np.abs(got).max() > 0
    # the ten parameter gradients of the same backward, under the existing chain's bounds
    pb, _ = chain_bounds(z["x0"], z["x1"], p, f, g, z["upstream"])
    got = param_grads(block)
    for mine, theirs in zip(PARAM_GRADS, R.BLOCK_GRADS):
        close(name, theirs, got[mine], z[f"ref64_{theirs}"], pb[theirs], z[f"ref32_dev_{theirs}"])


def test_parameter_gradients_keep_their_bytes_and_only_the_needed_outputs_are_requested(monkeypatch):
    z = D.load_case("b2_l3_5x7")
    calls, m = [], f32_model()
    real = last_block.convup_dgrad
    monkeypatch.setattr(last_block, "convup_dgrad", lambda *a, **k: calls.append(tuple(k["want"])) or real(*a, **k))

    def backward(input_grads, need0, need1):
        block = block_from_golden(z, m, input_grads)
        x0, x1 = src_dev(z["x0"]).requires_grad_(need0), c16_dev(z["x1"]).requires_grad_(need1)
        block(x0, x1).backward(c16_dev(z["upstream"]))
        return {k: v.cpu().numpy().tobytes() for k, v in param_grads(block).items()}, x0.grad, x1.grad

    plain, _, _ = backward(False, False, False)
    assert calls == []
    off, g0, g1 = backward(True, False, False)               # nothing requires grad: nothing new is launched
    assert calls == [] and g0 is None and g1 is None and off == plain
    both, b0, b1 = backward(True, True, True)
    assert calls == [("x0", "x1")] and both == plain
    only1, g0, g1 = backward(True, False, True)
    assert calls[1:] == [("x1",)] and g0 is None and only1 == plain
    only0, h0, h1 = backward(True, True, False)
    assert calls[2:] == [("x0",)] and h1 is None and only0 == plain
    # an output's bytes do not depend on whether the other one was asked for
    assert torch.equal(g1, b1) and torch.equal(h0, b0)
    # the default layer refuses as before
    with pytest.raises(ValueError, match="no gradient with respect to x0 and x1"):
        block_from_golden(z, m, False)(src_dev(z["x0"]).requires_grad_(True), c16_dev(z["x1"]))


def test_a_layer_in_front_of_the_block_trains_through_it():
    """A learnable per-channel scale on x0 in plain torch in front of LastBlock, through PredHead and calculate_loss: its
    gradient is sum d_x0 x0 per channel, formed here in f64 from the d_x0 the block returned.  torch's own f32 product and
    sum over the n elements of a channel is within (n + 2) 2^-24 of the sum of |terms|."""
    m = f32_model()
    x = x_dev()
    gt = teacher(m, x)
    snap = m.sn_snapshot()
    x0, x1 = m.forward_tail_sources(x)
    m.sn_restore(snap)
    block, head = LastBlock.from_model(m), PredHead.from_model(m)
    rng = np.random.default_rng(5)
    scale = torch.from_numpy((1 + 0.1 * rng.standard_normal(64)).astype(np.float32)).cuda().requires_grad_(True)
    xs = x0 * scale.view(4, 1, 1, 16)                        # channel 16 g + j of [B, L, g, H0, column, j]
    xs.lw, xs.c16 = x0.lw, True
    xs.retain_grad()
    pred = head(block(xs, x1))
    total, _ = losses.calculate_loss(pred, gt)
    total.backward()
    assert xs.grad is not None and xs.grad.shape == x0.shape and x1.grad is None
    assert all(q.grad is not None and float(q.grad.abs().max()) > 0 for q in block.parameters())
    d = xs.grad.detach().cpu().numpy().astype(np.float64)
    assert not d[:, :, :, :, x0.lw:, :].any() and np.abs(d).max() > 0
    terms = d * x0.detach().cpu().numpy().astype(np.float64)
    want = terms.sum(axis=(0, 1, 3, 4)).reshape(64)
    n = terms.size // 64
    bound = (n + 2) * EPS32 * np.abs(terms).sum(axis=(0, 1, 3, 4)).reshape(64) + R.ulp32(want)
    err = np.abs(scale.grad.detach().cpu().numpy().astype(np.float64) - want)
    print(f"scale in front of LastBlock: max error {err.max():.3e}, {float((err / bound).max()):.4f} of its bound")
    assert np.all(err <= bound) and np.abs(want).max() > 0
