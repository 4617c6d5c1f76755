"""TailConvs as an autograd layer (last_block.py), V2ce3d.forward_tail_sources and finetune.fit_last_block on the GPU.

Against the reference block's own f64 autograd (tests/golden/.lastblock/NAME.layer.npz and companions) the whole chain
TailConvs -> TailNorms -> LastConv runs on an exact-f32 model.  Every bound is a first-order propagation of the kernels'
contracts (tests/last_block_ref.py), not something the code gave.  With eps = 2^-24, |.| elementwise, conv(|a|, |b|) the
same sums on absolute values, and kappa = sum |u_i W_ij v_j| / |sigma| the condition of a spectral norm whose sigma, u, v
are f32 products of rows + cols terms (sigma enters squared, u and v once each: 4 (rows + cols) kappa eps relative):

forward (the masks are pinned by the goldens' MARGIN; values carry these errors into the sums that read them)
  c1     an fmaf chain of 2592 terms on W1 = W_bar1 / sigma1:  E_c1 = (2592 + 4 + 4 * 2624 kappa1) eps conv(|X|, |W1|)
  z1     E_z1 = rs1 E_c1 + 6 eps rs1 (conv(|X|, |W1|) + |mean1|);   zd: E_zd = (96 + 8) eps rsd (conv(|X|, |Wd|) + |bias_d| + |mean_d|)
  t      E_t = mask_t (|w1| E_z1 + 3 eps (|w1 z1| + |b1|));  res is not read by any gradient
backward
  d_t    the header of the input-gradient kernel on the folded weight Wf = scale2 W2: E_dt = (864 + 1) eps S + 864 2^-126
         + (4 * 896 kappa2 + 8) eps S with S = sum |Wf| |m| (the fold and W2's own derivation in f32);  d_res is a copy
  g1     = w1 mask_t d_t:  E_g1 = |w1| mask_t E_dt + eps |g1|;   gd = wd d_res:  E_gd = eps |gd|
  dM1, dMd, sum gd   the header of v2ce_convup_wgrad on the device's (g1, gd), plus the same sums on (E_g1, E_gd) in the
         places of (|g1|, |gd|): the kernel's outputs are linear in them
  conv1, shortcut    the closed forms (last_block_ref.conv_grads) are linear in dM1, dMd and the sum: the bound is the same
         form on absolute values (conv_bounds); on top torch evaluates them in f32: (82 944 + 2592 + 4 * 2624 kappa1 + 16) eps
         times the closed form on absolute values for weight_bar1, 4 eps for the shortcut's
  bn1, bnd   d_weight = sum g z, d_bias = sum g over the n positions of a channel: E_dt through |z|, E_z through |g|, and
         (n + 4) eps times the sum of |terms| for torch's f32 evaluation
  conv2, bn2   the header of the 32-channel weight-gradient kernel on the device's t, plus sum |m| E_t; then
         last_conv_ref.param_bounds and the f32 slack of tests/test_gpu_last_conv_autograd.py
each plus one f32 ulp of the truth.  Every result is printed as a fraction of its bound next to the reference's own f32
deviation (ref32_dev).  The model-level tests use synth.make_state_dict."""
import functools

import numpy as np
import pytest
import torch

from test_gpu_last_conv_autograd import EPS32, c16_dev, f32_model, make_model, planar, state_dict, x_dev
from tests import last_block_ref as R
from tests import last_conv_dgrad_ref as D
from tests import last_conv_ref as R2
from tests.make_last_block_goldens import CASES, KERNEL_ONLY
from v2ce_toolbox_amd import finetune, hip, last_block, losses, synth
from v2ce_toolbox_amd.last_block import TailConvs
from v2ce_toolbox_amd.last_conv import LastConv, TailNorms
from v2ce_toolbox_amd.pred_head import PredHead, pred_head_forward

pytestmark = pytest.mark.gpu

LAYER_CASES = [n for n in sorted(CASES) if n not in KERNEL_ONLY]
PRE = "UNet.decoders.3."
CONV_KEYS = {PRE + "conv1.module.weight_bar", PRE + "conv1.module.weight_u", PRE + "conv1.module.weight_v",
             PRE + "downsample.0.weight", PRE + "downsample.0.bias"}
TAIL_KEYS = {PRE + "conv2.module.weight_bar", PRE + "conv2.module.weight_u", PRE + "conv2.module.weight_v", PRE + "bn2.weight",
             PRE + "bn2.bias", "UNet.pred.conv3d.weight", "UNet.pred.conv3d.bias"}
NORM_STATE = {PRE + "bn1.weight", PRE + "bn1.bias", PRE + "downsample.1.weight", PRE + "downsample.1.bias"}


def src_dev(a):
    t = torch.from_numpy(R.src_to_c16(a, R.pitch_of(a.shape[-1]))).cuda()
    t.lw, t.c16 = a.shape[-1], True
    return t


def sn_state(m):
    return {k: v.clone() for k, v in m.state_dict().items() if k.endswith(("weight_u", "weight_v"))}


def layers_from_golden(z, model):
    """(TailConvs, TailNorms, LastConv) holding the golden block's constants."""
    convs, norms, conv = TailConvs(model).cuda(), TailNorms().cuda(), LastConv(model).cuda()
    put = lambda dst, key: dst.copy_(torch.from_numpy(np.asarray(z[key])))
    with torch.no_grad():
        for mod, pairs in ((convs, (("weight_bar", "weight_bar1"), ("weight_u", "u1"), ("weight_v", "v1"), ("short_weight", "short_weight"),
                                    ("short_bias", "short_bias"), ("bn1_mean", "bn1_mean"), ("bn1_var", "bn1_var"),
                                    ("bnd_mean", "bnd_mean"), ("bnd_var", "bnd_var"))),
                           (norms, (("bn1_weight", "bn1_weight"), ("bn1_bias", "bn1_bias"), ("bnd_weight", "bnd_weight"),
                                    ("bnd_bias", "bnd_bias"))),
                           (conv, (("weight_bar", "weight_bar2"), ("weight_u", "u2"), ("weight_v", "v2"), ("bn_weight", "bn2_weight"),
                                   ("bn_bias", "bn2_bias"), ("running_mean", "bn2_mean"), ("running_var", "bn2_var")))):
            for name, key in pairs:
                put(getattr(mod, name), key)
        convs.eps.fill_(float(z["eps"]))
        conv.eps.fill_(float(z["eps"]))
    return convs, norms, conv


def kappa_of(weight_bar, u, v, sigma):
    wb = np.abs(np.asarray(weight_bar, np.float64).reshape(32, -1))
    return float((np.abs(u)[:, None] * wb * np.abs(v)[None, :]).sum() / abs(sigma))


def check_uv(got_u, got_v, weight_bar, u0, u1_ref, v1_ref, label):
    """The iterated vectors against another f32 evaluation of the same iteration: the argument of
    tests/test_gpu_last_conv_autograd.py::check_uv for a [rows, cols] matrix.  Two f32 evaluations of an n-term product, in
    any order, differ by at most 2 (n + 2) 2^-24 times its sum of |terms|; a norm of n components carries (n + 4) 2^-24
    relative; an error of the raw vector moves the normalised one by at most itself over the norm, plus its norm over the
    norm along the vector; v's error enters u through |W|."""
    W = np.asarray(weight_bar, np.float64).reshape(32, -1)
    rows, cols = W.shape
    aW, u0 = np.abs(W), np.asarray(u0, np.float64)
    v1, u1 = np.asarray(v1_ref, np.float64), np.asarray(u1_ref, np.float64)
    nv = np.linalg.norm(W.T @ u0)
    d_raw_v = 2 * (rows + 2) * EPS32 * (aW.T @ np.abs(u0))
    d_v = d_raw_v / nv + (np.linalg.norm(d_raw_v) / nv + 2 * (cols + 4) * EPS32) * np.abs(v1) + 2.0 ** -149
    nu = np.linalg.norm(W @ v1)
    d_raw_u = 2 * (cols + 2) * EPS32 * (aW @ np.abs(v1)) + aW @ d_v
    d_u = d_raw_u / nu + (np.linalg.norm(d_raw_u) / nu + 2 * (rows + 4) * EPS32) * np.abs(u1) + 2.0 ** -149
    for got, want, bound, k in ((got_v, v1, d_v, "v"), (got_u, u1, d_u, "u")):
        err = np.abs(got.detach().cpu().numpy().astype(np.float64) - want)
        print(f"{label}: {k} after the call: max error {err.max():.3e}, {float((err / bound).max()):.4f} of its bound")
        assert np.all(err <= bound), (label, k)


def close(label, k, got, want, bound, dev32=None):
    a = got.detach().cpu().numpy().astype(np.float64)
    err = np.abs(a - want)
    bound = bound + R.ulp32(want)
    tail = "" if dev32 is None else f"; reference f32 {float(dev32):.3e}"
    print(f"{label}: {k}: max error {err.max():.3e}, {float((err / bound).max()):.4f} of its bound{tail}")
    assert a.shape == want.shape and not np.isnan(a).any() and np.all(err <= bound), (label, k, float(err.max()))


def chain_bounds(x0, x1, p, f, g, upstream):
    """The module docstring's bounds for the ten gradients of last_block_ref.BLOCK_GRADS (without the final ulp), from the
    f64 forward `f` (block_forward) and backward `g` (block_grads) of the block."""
    s5 = lambda a: a.sum(axis=(0, 2, 3, 4))
    n = x1.size // 32
    aX = np.abs(f["X"])
    k1 = kappa_of(p["weight_bar1"], f["u1a"], f["v1a"], f["sigma1"])
    k2 = kappa_of(p["weight_bar2"], f["u2a"], f["v2a"], f["sigma2"])
    # forward
    mag1 = R2.conv(aX, np.abs(f["W1"]))
    e_z1 = R.bc(f["rs1"]) * ((2592 + 4 + 4 * 2624 * k1) * EPS32 * mag1 + 6 * EPS32 * (mag1 + R.bc(np.abs(p["bn1_mean"]))))
    magd = R.conv1x1(aX, np.abs(p["short_weight"])) + R.bc(np.abs(p["short_bias"])) + R.bc(np.abs(p["bnd_mean"]))
    e_zd = (96 + 8) * EPS32 * R.bc(f["rsd"]) * magd
    mask_t = f["pre1"] > 0
    aw1 = R.bc(np.abs(p["bn1_weight"]))
    e_t = np.where(mask_t, aw1 * e_z1 + 3 * EPS32 * (aw1 * np.abs(f["z1"]) + R.bc(np.abs(p["bn1_bias"]))), 0.0)
    # backward: conv2's input gradient, the norms' multiplications, the new kernel, the closed forms
    S = g["abs_d_t"]
    e_dt = D.dgrad_bound(S, hip.DGRAD_TERMS) + (4 * 896 * k2 + 8) * EPS32 * S
    e_g1 = np.where(mask_t, aw1 * e_dt, 0.0) + EPS32 * np.abs(g["g1"])
    e_gd = EPS32 * np.abs(g["gd"])
    carried = R.wgrad(x0, x1, e_g1, e_gd)                  # the kernel's sums with the errors in the gradients' places
    e_dM1 = R.wgrad_bound(g["dM1"], g["abs_dM1"], n, hip.UPWGRAD_CHAIN) + carried["abs_weight"]
    e_dMd = R.wgrad_bound(g["dMd"], g["abs_dMd"], n, hip.UPWGRAD_CHAIN) + carried["abs_short"]
    e_sum = R.ulp32(g["d_sum"]) + carried["abs_short_bias"]
    cargs = (p["weight_bar1"], f["u1a"], f["v1a"], f["sigma1"], f["rs1"], f["rsd"])
    out = R.conv_bounds(e_dM1, e_dMd, e_sum, *cargs)
    size = R.conv_bounds(np.abs(g["dM1"]), np.abs(g["dMd"]), np.abs(g["d_sum"]), *cargs)
    out["d_weight_bar1"] = out["d_weight_bar1"] + (82944 + 2592 + 4 * 2624 * k1 + 16) * EPS32 * size["d_weight_bar1"]
    out["d_short_weight"] = out["d_short_weight"] + 4 * EPS32 * size["d_short_weight"]
    out["d_short_bias"] = out["d_short_bias"] + 4 * EPS32 * size["d_short_bias"]
    # the two BatchNorms' affine parts
    g_t = np.where(mask_t, g["d_t"], 0.0)
    e_gt = np.where(mask_t, e_dt, 0.0)
    az1, azd, ares = np.abs(f["z1"]), np.abs(f["zd"]), np.abs(g["d_res"])
    out["d_bn1_weight"] = s5(e_gt * az1) + s5(np.abs(g_t) * e_z1) + (n + 4) * EPS32 * s5(np.abs(g_t) * az1)
    out["d_bn1_bias"] = s5(e_gt) + (n + 4) * EPS32 * s5(np.abs(g_t))
    out["d_bnd_weight"] = s5(ares * e_zd) + (n + 4) * EPS32 * s5(ares * azd)
    out["d_bnd_bias"] = (n + 4) * EPS32 * s5(ares)
    # conv2 and bn2: the kernel on the device's t
    e_dM2 = R2.wgrad_bound(g["dM2"], g["abs_dM2"], n, hip.WGRAD_CHAIN) + R2.wgrad(e_t, f["feat"], np.abs(upstream))["abs_weight"]
    pargs = (p["weight_bar2"], f["u2a"], f["v2a"], f["sigma2"], f["scale2"], p["bn2_mean"], p["bn2_var"], float(p["eps"]))
    c2 = R2.param_bounds(e_dM2, R.ulp32(g["d_shift2"]), *pargs)
    size2 = R2.param_bounds(np.abs(g["dM2"]), np.abs(g["d_shift2"]), *pargs)
    rel2 = (27648 + 864 + 4 * 896 * k2 + 16) * EPS32
    for mine, theirs in (("d_weight_bar2", "d_weight_bar"), ("d_bn2_weight", "d_bn_weight"), ("d_bn2_bias", "d_bn_bias")):
        out[mine] = c2[theirs] + rel2 * size2[theirs]
    return out, (k1, k2)


@pytest.mark.parametrize("name", LAYER_CASES)
def test_chain_matches_the_reference_blocks_autograd(name):
    z = R.load_case(name)
    p = {k: z[k] for k in R.PARAMS}
    convs, norms, conv = layers_from_golden(z, f32_model())
    x0, x1 = src_dev(z["x0"]), c16_dev(z["x1"])           # (their padding columns hold NaN: it must not reach a result)
    z1, zd = convs(x0, x1)
    assert z1.grad_fn is not None and zd.grad_fn is not None and z1.lw == zd.lw == z["x1"].shape[-1]
    assert z1.shape == zd.shape == (x1.shape[0], x1.shape[1], 2, x1.shape[3], R.pitch_of(z1.lw), 16)
    check_uv(convs.weight_u, convs.weight_v, z["weight_bar1"], z["u1"], z["ref32_u1_after"], z["ref32_v1_after"], name + " conv1")
    t, res = norms(z1, zd)
    feat = conv(t, res)
    check_uv(conv.weight_u, conv.weight_v, z["weight_bar2"], z["u2"], z["ref32_u2_after"], z["ref32_v2_after"], name + " conv2")
    assert np.array_equal(planar(t) > 0, z["mask_t"]) and np.array_equal(planar(feat) > 0, z["mask_y"])   # the reference's masks
    feat.backward(c16_dev(z["upstream"]))
    f = R.block_forward(z["x0"], z["x1"], p)
    g = R.block_grads(z["x0"], z["x1"], p, z["upstream"], f)
    bounds, (k1, k2) = chain_bounds(z["x0"], z["x1"], p, f, g, z["upstream"])
    print(f"{name}: kappa1 {k1:.1f}, kappa2 {k2:.1f}")
    got = {"d_weight_bar1": convs.weight_bar.grad, "d_short_weight": convs.short_weight.grad, "d_short_bias": convs.short_bias.grad,
           "d_bn1_weight": norms.bn1_weight.grad, "d_bn1_bias": norms.bn1_bias.grad, "d_bnd_weight": norms.bnd_weight.grad,
           "d_bnd_bias": norms.bnd_bias.grad, "d_weight_bar2": conv.weight_bar.grad, "d_bn2_weight": conv.bn_weight.grad,
           "d_bn2_bias": conv.bn_bias.grad}
    assert set(got) == set(R.BLOCK_GRADS)
    for k in R.BLOCK_GRADS:
        close(name, k, got[k], z[f"ref64_{k}"], bounds[k], z[f"ref32_dev_{k}"])
    if name == "zero":
        assert not any(v.any() for v in got.values())
    else:
        assert all(float(v.abs().max()) > 0 for v in got.values())


@pytest.mark.parametrize("precision", ["f16x2", "f32"])
def test_tail_sources_and_tail_convs_reproduce_the_normed_pair(precision):
    m = make_model(precision)
    x = x_dev()
    snap = m.sn_snapshot()
    x0, x1 = m.forward_tail_sources(x)
    assert m.calls == 1 and x0.shape == (1, 2, 4, 8, 8, 16) and x1.shape == (1, 2, 2, 16, 16, 16) and x0.lw == 8 and x1.lw == 16
    assert x0.c16 and x1.c16 and not x0.requires_grad and x0.grad_fn is None and x1.grad_fn is None
    after = sn_state(m)
    m.sn_restore(snap)
    layer = TailConvs.from_model(m)                          # u, v from before the call: the layer iterates them itself
    z1, zd = layer(x0, x1)
    assert z1.grad_fn is not None and zd.grad_fn is not None
    want1, wantd = m.forward_tail_normed(x)
    now = sn_state(m)
    assert len(now) == 24 and all(torch.equal(after[k], now[k]) for k in after)          # the same power iteration
    assert m.calls == 1 and z1.shape == want1.shape and z1.lw == zd.lw == want1.lw == 16
    for got, want, k in ((z1, want1, "z1"), (zd, wantd, "zd")):
        err = (got.detach() - want).abs()[:, :, :, :, :16, :]
        print(f"{precision}: TailConvs(forward_tail_sources) vs forward_tail_normed: {k}: max |d| = {float(err.max()):.3e}")
        assert bool((err <= 1e-5 + 1e-5 * want.abs()[:, :, :, :, :16, :]).all())
    # the shortcut: the same weights through the same pack, the same epilogue vectors, the same launch on the same range slots --
    # its bytes are the model's (conv1's differ: the layer packs W_bar / sigma, the model W_bar with 1 / sigma in the scale)
    assert torch.equal(zd.detach()[:, :, :, :, :16, :], wantd[:, :, :, :, :16, :])
    inner = m.UNet.decoders[-1].conv1.module               # both advanced conv1's vectors by one iteration
    sd = state_dict()
    pre = PRE + "conv1.module."
    check_uv(layer.weight_u, layer.weight_v, sd[pre + "weight_bar"].numpy(), sd[pre + "weight_u"].numpy(),
             inner.weight_u.cpu().numpy(), inner.weight_v.cpu().numpy(), precision)
    if precision == "f16x2":
        assert 0.0 < float(layer.guard) <= m.RANGE_GUARD_LIMIT


def test_a_gradient_of_the_sources_is_refused_and_nothing_is_launched_without_trainable_parameters(monkeypatch):
    m = f32_model()
    z = R.load_case("b2_l3_5x7")
    convs, norms, conv = layers_from_golden(z, m)
    x0, x1 = src_dev(z["x0"]), c16_dev(z["x1"])
    with pytest.raises(ValueError, match="no gradient with respect to x0 and x1"):
        convs(src_dev(z["x0"]).requires_grad_(True), x1)
    x1g = c16_dev(z["x1"]).requires_grad_(True)
    assert x1g.lw == x1.lw
    with pytest.raises(ValueError, match="no gradient with respect to x0 and x1"):
        convs(x0, x1g)
    # only the shortcut trains: d_weight is not asked for; nothing trains: the kernel is not called
    calls = []
    real = last_block.convup_wgrad
    monkeypatch.setattr(last_block, "convup_wgrad", lambda *a, **k: calls.append(k["want"]) or real(*a, **k))
    convs.weight_bar.requires_grad_(False)
    feat = conv(*norms(*convs(x0, x1)))
    feat.backward(c16_dev(z["upstream"]))
    assert calls == [("short", "short_bias")] and convs.weight_bar.grad is None and convs.short_weight.grad is not None
    for q in convs.parameters():
        q.requires_grad_(False)
    conv(*norms(*convs(x0, x1))).backward(c16_dev(z["upstream"]))
    assert len(calls) == 1


def tail_chain(m, x, gt):
    """-> the four modules and the loss after one forward / backward of the whole block through calculate_loss."""
    snap = m.sn_snapshot()
    x0, x1 = m.forward_tail_sources(x)
    m.sn_restore(snap)
    convs, norms, conv, head = TailConvs.from_model(m), TailNorms.from_model(m), LastConv.from_model(m), PredHead.from_model(m)
    pred = head(conv(*norms(*convs(x0, x1))))
    total, _ = losses.calculate_loss(pred, gt)
    total.backward()
    return convs, norms, conv, head, x0, x1, pred, total


def teacher(m, x, seed=9):
    """Ground truth for a fit: the model's own features through a perturbed head."""
    snap = m.sn_snapshot()
    feat = m.forward_features(x)
    m.sn_restore(snap)
    head = PredHead.from_model(m)
    rng = np.random.default_rng(seed)
    w = head.weight.detach() + 0.3 * head.weight.detach().abs().mean() * torch.from_numpy(
        rng.standard_normal(tuple(head.weight.shape)).astype(np.float32)).cuda()
    return pred_head_forward(feat, w.contiguous(), head.bias.detach())


def test_write_back_then_the_model_runs_the_tuned_block():
    m = make_model()
    x = x_dev()
    convs, norms, conv, head, x0, x1, pred, _ = tail_chain(m, x, teacher(m, x))
    mods = (convs, norms, conv, head)
    assert all(p.grad is not None and float(p.grad.abs().max()) > 0 for mod in mods for p in mod.parameters())
    with torch.no_grad():
        for mod in mods:
            for p in mod.parameters():
                p.sub_(0.05 * p.grad / (p.grad.abs().max() + 1e-30) * p.abs().max())
    before = {k: v.clone() for k, v in m.state_dict().items()}
    for mod in mods:
        mod.write_back(m)
    assert m._prep is None
    changed = {k for k, v in m.state_dict().items() if not torch.equal(before[k], v)}
    assert changed == CONV_KEYS | TAIL_KEYS | NORM_STATE
    # the model's next call iterates every spectral-norm layer once: the ten frozen ones as in forward_tail_sources, the two
    # tuned ones from the vectors the layers left -- as the layers' own next forward does
    want = m(x)
    have = head(conv(*norms(*convs(x0, x1)))).detach()
    err = (have - want).abs()
    print(f"write_back: tuned block vs model(x): max |d| = {float(err.max()):.3e}")
    assert bool((err <= 1e-5 + 1e-5 * want.abs()).all())
    assert float((have - pred.detach()).abs().max()) > 1e-4          # the update did change the output


@functools.lru_cache(maxsize=None)
def recording():
    """Two windows [1, 4, 2, 32, 48] of a synthetic recording with a teacher's voxels."""
    m = make_model()
    xs, gs = [], []
    for seed in (3, 4):
        fr = synth.synthetic_frames(5, 32, 48, seed=seed).astype(np.float32) / 255
        x = np.stack([fr[:-1], fr[1:]], axis=1)
        x = torch.from_numpy(((x - np.float32(0.153)) / np.float32(0.165))[None]).to("cuda:0")
        xs.append(x)
        gs.append(teacher(m, x))                             # one teacher for both windows: an update on one serves the other
    return xs, gs


# plain gradient descent.  The step size is checked, not assumed: the assertions are that the loss falls.  Every forward of the
# two trained convolutions also advances their spectral-norm u / v (synthetic weights: the iteration has not converged), which
# moves the loss by itself; so next to the plain statement -- the loss after four updates is below the loss at step 0 -- the
# fit is compared step by step with the same fit at lr = 0, which makes the same forwards and no update
FIT_LR = 1e-5


def test_fit_last_block_lowers_the_loss_and_restores_the_rest():
    xs, gs = recording()
    m = make_model()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    calls = m.calls
    hist = finetune.fit_last_block(m, xs, gs, steps=6, lr=FIT_LR, optimizer="sgd")
    loss = [h["loss"] for h in hist]
    still = [h["loss"] for h in finetune.fit_last_block(make_model(), xs, gs, steps=6, lr=0.0, optimizer="sgd")]
    print(f"fit_last_block: losses {loss}; without updates {still}")
    assert len(hist) == 6 and all(set(h) == {"loss", "loss_dict"} for h in hist) and all(np.isfinite(loss))
    assert loss[4] < loss[0]                               # window 0 at step 0 and after four updates
    assert loss[0] == still[0] and all(a < b for a, b in zip(loss[1:], still[1:]))   # every update lowered what followed
    after = m.state_dict()
    changed = {k for k in before if not torch.equal(before[k], after[k])}
    assert changed == CONV_KEYS | TAIL_KEYS | NORM_STATE and m.calls == calls and m._prep is None
    # only the two new groups: the layers behind them keep their bytes (conv2's u / v keep the fit's iterations)
    m2 = make_model()
    h2 = finetune.fit_last_block(m2, xs, gs, train=("conv1", "convd"), steps=2, lr=FIT_LR, optimizer="sgd")
    changed = {k for k, v in m2.state_dict().items() if not torch.equal(before[k], v)}
    assert changed == CONV_KEYS | {PRE + "conv2.module.weight_u", PRE + "conv2.module.weight_v"}
    assert h2[0]["loss"] == hist[0]["loss"]                # the same first step: identical kernels on identical bytes
    # a window beyond the cache budget is recomputed from the entry state: the same history
    m3 = make_model()
    h3 = finetune.fit_last_block(m3, xs, gs, steps=6, lr=FIT_LR, optimizer="sgd", cache_bytes=0)
    assert h3 == hist and all(torch.equal(after[k], v) for k, v in m3.state_dict().items())


def test_fit_last_block_without_the_new_groups_is_fit_tail_norms():
    xs, gs = recording()
    a, b = make_model(), make_model()
    ha = finetune.fit_tail_norms(a, xs, gs, train=finetune.TAIL_NORM_GROUPS, steps=3, lr=1e-3)
    hb = finetune.fit_last_block(b, xs, gs, train=finetune.TAIL_NORM_GROUPS, steps=3, lr=1e-3)
    assert ha == hb and len(ha) == 3
    sa, sb = a.state_dict(), b.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa) and a.calls == b.calls
