"""LastConv as an autograd layer (last_conv.py), V2ce3d.forward_tail_inputs and finetune.fit_tail on the GPU.

Against the reference block's own f64 autograd (tests/golden/.lastconv/) the layer runs on an exact-f32 model; the
bounds are derived from the arithmetic, not from what the code gives:
  dM, d_shift      the kernel's bound (tests/test_gpu_convgrad.py): E = ulp32 + V2CE_WGRAD_CHAIN 2^-24 abs_terms + N 2^-52
                   abs_terms, and one f32 ulp;
  the closed forms dW = scale dM, d_scale = <W, dM>, d_weight_bar = dW / sigma - (<dW, W_bar> / sigma^2) u v^T, d_bn_weight =
                   (d_scale - mean d_shift) rsqrt(var + eps) are linear in dM and d_shift, so E is carried through them on
                   absolute values (last_conv_ref.param_bounds); on top, torch evaluates them in f32: any order of an
                   n-term f32 sum is within n 2^-24 of its sum of |terms| (n = 27 648 for <dW, W_bar>, 864 for a row), and
                   sigma, u and v come from f32 products of 896 terms whose relative error is at most 896 2^-24 times the
                   condition number kappa = sum |u_i W_ij v_j| / |sigma|; sigma enters squared and u, v once each.  So
                   slack = (27 648 + 864 + 4 * 896 kappa + 16) 2^-24 times the closed form on absolute values.
The model-level tests use synth.make_state_dict at x [1, 2, 2, 16, 16] and compare with the numpy restatement
(tests/last_conv_ref.py, itself checked against the reference block without a GPU) under the same bounds."""
import functools

import numpy as np
import pytest
import torch

from tests import last_conv_ref as R
from tests.make_last_conv_goldens import CASES, KERNEL_ONLY
from v2ce_toolbox_amd import finetune, hip, losses, synth
from v2ce_toolbox_amd.last_conv import LastConv
from v2ce_toolbox_amd.pred_head import PredHead, pred_head_forward
from v2ce_toolbox_amd.v2ce_3d import V2ce3d

pytestmark = pytest.mark.gpu

SHAPE = (1, 2, 2, 16, 16)
LAYER_CASES = [n for n in sorted(CASES) if n not in KERNEL_ONLY]
EPS32 = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def state_dict(seed=0):
    return synth.make_state_dict(seed)


def make_model(precision="f16x2", seed=0):
    m = V2ce3d(precision=precision)
    m.load_state_dict(state_dict(seed))
    return m.eval().to("cuda:0")


@functools.lru_cache(maxsize=None)
def image_units():
    fr = synth.synthetic_frames(SHAPE[1] + 1, SHAPE[3], SHAPE[4], seed=3).astype(np.float32) / 255
    x = np.stack([fr[:-1], fr[1:]], axis=1)
    return ((x - np.float32(0.153)) / np.float32(0.165))[None]


def x_dev():
    return torch.from_numpy(image_units()).to("cuda:0")


def c16_dev(a):
    t = torch.from_numpy(R.to_c16(a, R.pitch_of(a.shape[-1]))).cuda()
    t.lw, t.c16 = a.shape[-1], True
    return t


def planar(t):
    return R.from_c16(t.detach().cpu().numpy(), t.lw)


def consts(layer):
    """The layer's tensors as numpy: what the closed forms are evaluated on."""
    g = lambda n: getattr(layer, n).detach().cpu().numpy()
    return {k: g(k) for k in ("weight_bar", "weight_u", "weight_v", "bn_weight", "bn_bias", "running_mean", "running_var")} | \
        {"eps": float(layer.eps)}


def check_param_grads(layer, c, u1, v1, truth, dM, d_shift, abs_dM, n_pos, label):
    """layer.*.grad against `truth` {d_weight_bar, d_bn_weight, d_bn_bias} under the module docstring's bounds; c: the
    constants (weight_bar, bn, statistics), u1 / v1: the iterated vectors in f64, dM / d_shift / abs_dM: f64 truth."""
    W, sigma, scale, shift = R.effective(c["weight_bar"], u1, v1, c["bn_weight"], c["bn_bias"], c["running_mean"],
                                         c["running_var"], c["eps"])
    e_dM = R.wgrad_bound(dM, abs_dM, n_pos, hip.WGRAD_CHAIN)
    e_shift = R.ulp32(d_shift)
    carried = R.param_bounds(e_dM, e_shift, c["weight_bar"], u1, v1, sigma, scale, c["running_mean"], c["running_var"], c["eps"])
    kappa = (np.abs(u1)[:, None] * np.abs(np.asarray(c["weight_bar"], np.float64).reshape(32, -1)) * np.abs(v1)[None, :]).sum() / abs(sigma)
    rel = (27648 + 864 + 4 * 896 * kappa + 16) * EPS32
    size = R.param_bounds(np.abs(dM), np.abs(d_shift), c["weight_bar"], u1, v1, sigma, scale, c["running_mean"],
                          c["running_var"], c["eps"])
    got = {"d_weight_bar": layer.weight_bar.grad, "d_bn_weight": layer.bn_weight.grad, "d_bn_bias": layer.bn_bias.grad}
    for k, g in got.items():
        a = g.detach().cpu().numpy().astype(np.float64)
        err = np.abs(a - truth[k])
        bound = carried[k] + rel * size[k] + R.ulp32(truth[k])
        print(f"{label}: {k}: max error {err.max():.3e}, {float((err / bound).max()):.4f} of its bound (kappa {kappa:.1f})")
        assert a.shape == truth[k].shape and np.all(err <= bound), (label, k, float(err.max()))


def check_uv(layer, weight_bar, u0, u1_ref, v1_ref, label):
    """layer.weight_u / weight_v against another f32 evaluation of the same iteration.  Two f32 evaluations of an n-term
    product, in any order, differ by at most 2 (n + 2) 2^-24 times its sum of |terms|; a norm of n components carries
    (n + 4) 2^-24 relative; an error of the raw vector moves the normalised one by at most itself over the norm, plus its
    norm over the norm along the vector; v's error enters u through |W|."""
    W = np.asarray(weight_bar, np.float64).reshape(32, -1)
    aW, u0 = np.abs(W), np.asarray(u0, np.float64)
    v1, u1 = np.asarray(v1_ref, np.float64), np.asarray(u1_ref, np.float64)
    nv = np.linalg.norm(W.T @ u0)
    d_raw_v = 2 * 34 * EPS32 * (aW.T @ np.abs(u0))
    d_v = d_raw_v / nv + (np.linalg.norm(d_raw_v) / nv + 2 * 868 * EPS32) * np.abs(v1) + 2.0 ** -149
    nu = np.linalg.norm(W @ v1)
    d_raw_u = 2 * 866 * EPS32 * (aW @ np.abs(v1)) + aW @ d_v
    d_u = d_raw_u / nu + (np.linalg.norm(d_raw_u) / nu + 2 * 36 * EPS32) * np.abs(u1) + 2.0 ** -149
    for got, want, bound, k in ((layer.weight_v, v1, d_v, "v"), (layer.weight_u, u1, d_u, "u")):
        err = np.abs(got.detach().cpu().numpy().astype(np.float64) - want)
        print(f"{label}: {k} after the call: max error {err.max():.3e}, {float((err / bound).max()):.4f} of its bound")
        assert np.all(err <= bound), (label, k)


def layer_from_golden(z, model):
    layer = LastConv(model).cuda()
    with torch.no_grad():
        for name, key in (("weight_bar", "weight_bar"), ("weight_u", "u"), ("weight_v", "v"), ("bn_weight", "bn_weight"),
                          ("bn_bias", "bn_bias"), ("running_mean", "running_mean"), ("running_var", "running_var")):
            getattr(layer, name).copy_(torch.from_numpy(z[key]))
        layer.eps.fill_(float(z["eps"]))
    return layer


@functools.lru_cache(maxsize=None)
def f32_model():
    return make_model("f32")


@pytest.mark.parametrize("name", LAYER_CASES)
def test_layer_matches_the_reference_blocks_autograd(name):
    z = R.load_case(name)
    layer = layer_from_golden(z, f32_model())
    t, res = c16_dev(z["t"]), c16_dev(z["res"])
    feat = layer(t, res)
    assert feat.grad_fn is not None and feat.lw == z["t"].shape[-1] and feat.shape == t.shape
    # u and v after the call are the reference's: f32 products of 32 and 864 terms in another order
    check_uv(layer, z["weight_bar"], z["u"], z["ref32_u_after"], z["ref32_v_after"], name)
    # the forward on the exact-f32 convolution: an fmaf chain of 864 terms, the epilogue's operations, one store, on W, scale
    # and shift that the device derived in f32 (sigma: the kappa term)
    wb = np.abs(z["weight_bar"].astype(np.float64).reshape(32, -1))
    u1, v1 = R.power_iteration(z["weight_bar"], z["u"], z["v"])
    W64, sigma, scale64, shift64 = R.effective(z["weight_bar"], u1, v1, z["bn_weight"], z["bn_bias"], z["running_mean"],
                                               z["running_var"], z["eps"])
    mag = R.conv(np.abs(z["t"]), np.abs(W64)) * np.abs(scale64)[None, :, None, None, None] + \
        np.abs(shift64)[None, :, None, None, None] + np.abs(z["res"])
    kappa = (np.abs(u1)[:, None] * wb * np.abs(v1)[None, :]).sum() / abs(sigma)
    got = planar(feat).astype(np.float64)
    err = np.abs(got - z["ref64_feat"])
    bound = R.ulp32(z["ref64_feat"]) + (864 + 8 + 4 * 896 * kappa) * EPS32 * mag
    print(f"{name}: feat: max error {err.max():.3e}, {float((err / bound).max()):.4f} of its bound; reference f32 "
          f"{float(z['ref32_dev_feat']):.3e}")
    assert np.all(err <= bound)
    assert np.array_equal(got > 0, z["y"] > 0)              # the relu mask is the reference's
    feat.backward(c16_dev(z["upstream"]))                   # (its padding columns hold NaN: they are not read)
    truth = {k: z[f"ref64_{k}"] for k in ("d_weight_bar", "d_bn_weight", "d_bn_bias")}
    c = {k: z[k] for k in ("weight_bar", "bn_weight", "bn_bias", "running_mean", "running_var")} | {"eps": float(z["eps"])}
    check_param_grads(layer, c, u1, v1, truth, z["ref64_dM"], z["ref64_d_shift"], z["abs_terms_dM"], z["t"].size // 32, name)
    if name == "inactive":
        assert not layer.weight_bar.grad.any() and not layer.bn_weight.grad.any() and not layer.bn_bias.grad.any()
    else:
        assert layer.weight_bar.grad.abs().max() > 0


@pytest.mark.parametrize("precision", ["f16x2", "f32"])
def test_tail_inputs_and_layer_reproduce_forward_features(precision):
    m = make_model(precision)
    x = x_dev()
    snap = m.sn_snapshot()
    t, res = m.forward_tail_inputs(x)
    assert m.calls == 1 and t.shape == res.shape == (1, 2, 2, 16, 16, 16) and t.lw == res.lw == 16
    assert not t.requires_grad and t.grad_fn is None and float(t.min()) >= 0.0
    m.sn_restore(snap)
    layer = LastConv.from_model(m)                           # u, v from before the call: the layer iterates them itself
    feat = layer(t, res)
    want = m.forward_features(x)
    err = (feat.detach() - want).abs()
    print(f"{precision}: LastConv(forward_tail_inputs) vs forward_features: max |d| = {float(err.max()):.3e}")
    assert bool((err <= 1e-5 + 1e-5 * want.abs()).all())
    inner = m.UNet.decoders[-1].conv2.module               # both advanced conv2's vectors by one iteration
    sd = state_dict()
    pre = "UNet.decoders.3.conv2.module."
    check_uv(layer, sd[pre + "weight_bar"].numpy(), sd[pre + "weight_u"].numpy(), inner.weight_u.cpu().numpy(),
             inner.weight_v.cpu().numpy(), precision)


def chain(m, x, gt_seed=5):
    """-> (layer, head, t, res, feat, pred, gt) after one forward / backward of the tail through calculate_loss."""
    snap = m.sn_snapshot()
    t, res = m.forward_tail_inputs(x)
    m.sn_restore(snap)
    layer, head = LastConv.from_model(m), PredHead.from_model(m)
    before = consts(layer)
    feat = layer(t, res)
    feat.retain_grad()
    rng = np.random.default_rng(gt_seed)
    w = head.weight.detach() + 0.3 * head.weight.detach().abs().mean() * torch.from_numpy(
        rng.standard_normal(tuple(head.weight.shape)).astype(np.float32)).cuda()
    fd = feat.detach()
    fd.lw = feat.lw
    gt = pred_head_forward(fd, w.contiguous(), head.bias.detach())
    pred = head(feat)
    total, _ = losses.calculate_loss(pred, gt)
    total.backward()
    return layer, head, t, res, feat, pred, gt, before


def restated_grads(layer, before, t, feat):
    """The closed forms on the device's own upstream gradient (feat.grad) -> (truth, u1, v1, dM, d_shift, abs_dM, n)."""
    up = R.from_c16(feat.grad.cpu().numpy(), feat.lw)
    tt = planar(t)
    g = R.wgrad(tt, planar(feat), up)
    u1, v1 = R.power_iteration(before["weight_bar"], before["weight_u"], before["weight_v"])
    W, sigma, scale, shift = R.effective(before["weight_bar"], u1, v1, before["bn_weight"], before["bn_bias"],
                                         before["running_mean"], before["running_var"], before["eps"])
    truth = R.param_grads(g["d_weight"], g["d_shift"], before["weight_bar"], u1, v1, sigma, scale, before["running_mean"],
                          before["running_var"], before["eps"])
    return truth, u1, v1, g["d_weight"], g["d_shift"], g["abs_weight"], tt.size // 32


def test_backward_through_the_head_and_calculate_loss_matches_the_restatement():
    m = make_model("f32")
    layer, head, t, res, feat, pred, gt, before = chain(m, x_dev())
    assert feat.grad is not None and float(feat.grad.abs().max()) > 0 and t.grad is None
    assert head.weight.grad is not None and float(head.weight.grad.abs().max()) > 0
    truth, u1, v1, dM, d_shift, abs_dM, n = restated_grads(layer, before, t, feat)
    check_param_grads(layer, before, u1, v1, truth, dM, d_shift, abs_dM, n, "tail through the loss")
    assert layer.weight_bar.grad.abs().max() > 0 and layer.bn_weight.grad.abs().max() > 0


def test_write_back_then_the_model_runs_the_tuned_tail():
    m = make_model()
    x = x_dev()
    layer, head, t, res, feat, pred, gt, _ = chain(m, x)
    with torch.no_grad():
        for p in list(layer.parameters()) + list(head.parameters()):
            p.sub_(0.05 * p.grad / (p.grad.abs().max() + 1e-30) * p.abs().max())
    before = {k: v.clone() for k, v in m.state_dict().items()}
    layer.write_back(m)
    head.write_back(m)
    changed = {k for k, v in m.state_dict().items() if not torch.equal(before[k], v)}
    pre = "UNet.decoders.3."
    assert changed == {pre + "conv2.module.weight_bar", pre + "conv2.module.weight_u", pre + "conv2.module.weight_v",
                       pre + "bn2.weight", pre + "bn2.bias", "UNet.pred.conv3d.weight", "UNet.pred.conv3d.bias"}
    # the model's next call iterates every spectral-norm layer once: the eleven frozen ones as in forward_tail_inputs, the
    # tuned one from the vectors the layer left -- as the layer's own next forward does
    want = m(x)
    have = head(layer(t, res)).detach()
    err = (have - want).abs()
    print(f"write_back: tuned tail vs model(x): max |d| = {float(err.max()):.3e}")
    assert bool((err <= 1e-5 + 1e-5 * want.abs()).all())
    assert float((have - pred.detach()).abs().max()) > 1e-4          # the update did change the output


def fit_data(m):
    x = x_dev()
    feat = m.forward_features(x)
    head = PredHead.from_model(m)
    rng = np.random.default_rng(9)
    w = head.weight.detach() + 0.3 * head.weight.detach().abs().mean() * torch.from_numpy(
        rng.standard_normal(tuple(head.weight.shape)).astype(np.float32)).cuda()
    return x, pred_head_forward(feat, w.contiguous(), head.bias.detach())


def test_fit_tail_on_the_head_alone_is_fit_head():
    a, b = make_model(), make_model()
    x, gt = fit_data(make_model())
    ha = finetune.fit_head(a, x, gt, steps=3, lr=1e-3)
    hb = finetune.fit_tail(b, x, gt, train=("pred",), steps=3, lr=1e-3)
    assert ha == hb and len(ha) == 3
    sa, sb = a.state_dict(), b.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa) and a.calls == b.calls


def test_one_sgd_step_of_fit_tail_is_the_manual_step_and_the_rest_is_restored():
    lr = 1e-3
    m = make_model("f32")
    x, gt = fit_data(make_model("f32"))
    before = {k: v.clone() for k, v in m.state_dict().items()}
    calls = m.calls
    hist = finetune.fit_tail(m, x, gt, steps=1, lr=lr, optimizer="sgd")
    assert len(hist) == 1 and set(hist[0]) == {"loss", "loss_dict"} and hist[0]["loss"] > 0 and m.calls == calls
    after = m.state_dict()
    changed = {k for k in before if not torch.equal(before[k], after[k])}
    pre = "UNet.decoders.3."
    assert changed == {pre + "conv2.module.weight_bar", pre + "conv2.module.weight_u", pre + "conv2.module.weight_v",
                       pre + "bn2.weight", pre + "bn2.bias", "UNet.pred.conv3d.weight", "UNet.pred.conv3d.bias"}
    # the same step by hand on a second instance, from the restated gradients
    ref = make_model("f32")
    snap = ref.sn_snapshot()
    t, res = ref.forward_tail_inputs(x)
    ref.sn_restore(snap)
    layer, head = LastConv.from_model(ref), PredHead.from_model(ref)
    c0 = consts(layer)
    feat = layer(t, res)
    feat.retain_grad()
    total, _ = losses.calculate_loss(head(feat), gt)
    total.backward()
    assert float(total.detach()) == hist[0]["loss"]
    truth, u1, v1, dM, d_shift, abs_dM, n = restated_grads(layer, c0, t, feat)
    check_param_grads(layer, c0, u1, v1, truth, dM, d_shift, abs_dM, n, "fit_tail's step")
    torch.optim.SGD(list(layer.parameters()) + list(head.parameters()), lr=lr).step()
    for key, p in ((pre + "conv2.module.weight_bar", layer.weight_bar), (pre + "bn2.weight", layer.bn_weight),
                   (pre + "bn2.bias", layer.bn_bias), ("UNet.pred.conv3d.weight", head.weight), ("UNet.pred.conv3d.bias", head.bias)):
        assert torch.equal(after[key], p.detach().reshape(after[key].shape)), key   # the same kernels on the same bytes
    assert torch.equal(after[pre + "conv2.module.weight_u"], layer.weight_u)
    # only 'bn2': the convolution and the head keep their bytes
    m2 = make_model("f32")
    finetune.fit_tail(m2, x, gt, train=("bn2",), steps=2, lr=lr, optimizer="sgd")
    changed = {k for k, v in m2.state_dict().items() if not torch.equal(before[k], v)}
    assert changed == {pre + "conv2.module.weight_u", pre + "conv2.module.weight_v", pre + "bn2.weight", pre + "bn2.bias"}
