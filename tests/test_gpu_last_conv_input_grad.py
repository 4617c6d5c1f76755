"""LastConv's input gradients (v2ce_conv32_dgrad), V2ce3d.forward_tail_normed, TailNorms and finetune.fit_tail_norms on the
GPU.

Against the reference block's own f64 autograd (tests/golden/.lastconv_dgrad/NAME.block.*.npz) the layers run on an exact-f32
model; the bounds are derived from the arithmetic, not from what the code gives.  With Wf = scale[co] W[co] (the weight with
bn2's scale folded in), m the masked upstream and S = sum |Wf| |m| over an element's 864 terms:
  d_t          E_t = (V2CE_DGRAD_TERMS + 1) 2^-24 S + V2CE_DGRAD_TERMS 2^-126 (the kernel's bound on the folded weight) + 2^-24 S
               (the fold: one f32 rounding of every scale[co] W[co] product);
  d_res        a copy: the bytes of the masked upstream;
  bn1, bn_d    d_weight = sum over the n positions of a channel of g z, d_bias = sum of g, with g = d_t where t > 0 (bn1) or
               d_res (bn_d).  They are linear in g, so E_t is carried through them on absolute values
               (last_conv_dgrad_ref.tail_bounds; d_res is exact); on top, torch evaluates them in f32 on the f32-rounded z:
               one rounding of z, one of the product, and any order of an n-term f32 sum is within n 2^-24 of its sum of
               |terms|.  So slack = (n + 4) 2^-24 times the sum of |terms|, plus one f32 ulp of the result.
The model-level tests use synth.make_state_dict at x [1, 2, 2, 16, 16] and compare with the numpy restatement
(tests/last_conv_dgrad_ref.py, itself checked against the reference block without a GPU) under the same bounds."""
import numpy as np
import pytest
import torch

from test_gpu_last_conv_autograd import (EPS32, LAYER_CASES, c16_dev, check_param_grads, consts, f32_model, fit_data,
                                         layer_from_golden, make_model, planar, restated_grads, x_dev)
from tests import last_conv_dgrad_ref as D
from tests import last_conv_ref as R
from v2ce_toolbox_amd import finetune, hip, last_conv, losses
from v2ce_toolbox_amd.last_conv import LastConv, TailNorms
from v2ce_toolbox_amd.pred_head import PredHead

pytestmark = pytest.mark.gpu

NORM_KEYS = ("bn1_weight", "bn1_bias", "bnd_weight", "bnd_bias")
PRE = "UNet.decoders.3."
TAIL_KEYS = {PRE + "conv2.module.weight_bar", PRE + "conv2.module.weight_u", PRE + "conv2.module.weight_v", PRE + "bn2.weight",
             PRE + "bn2.bias", "UNet.pred.conv3d.weight", "UNet.pred.conv3d.bias"}
NORM_STATE = {PRE + "bn1.weight", PRE + "bn1.bias", PRE + "downsample.1.weight", PRE + "downsample.1.bias"}


def norms_from_golden(z):
    layer = TailNorms().cuda()
    with torch.no_grad():
        for k in NORM_KEYS:
            getattr(layer, k).copy_(torch.from_numpy(z[k]))
    return layer


def golden_inputs(z):
    """-> (z1, zd) in f64 and as the device's f32 channels-last-16 tensors (padding columns NaN)."""
    eps = float(z["eps"])
    z1, zd = D.normed(z["c1"], z["bn1_mean"], z["bn1_var"], eps), D.normed(z["cd"], z["bnd_mean"], z["bnd_var"], eps)
    return z1, zd, c16_dev(z1.astype(np.float32)), c16_dev(zd.astype(np.float32))


def folded(c, u1, v1):
    """scale[co] W[co] in f64 from the layer's constants."""
    W, sigma, scale, shift = R.effective(c["weight_bar"], u1, v1, c["bn_weight"], c["bn_bias"], c["running_mean"],
                                         c["running_var"], c["eps"])
    return scale[:, None, None, None, None] * W


def input_grad_bound(Wf, y, upstream):
    """E_t of the module docstring, per element."""
    S = D.dgrad(np.abs(Wf), y, np.abs(upstream))["abs_x"]
    return D.dgrad_bound(S, hip.DGRAD_TERMS) + EPS32 * S


def check_input_grads(t, res, truth_t, truth_res, e_t, label):
    W = t.lw
    for g in (t.grad, res.grad):
        a = g.cpu().numpy()
        assert g.shape == t.shape and not np.isnan(a).any() and not a[:, :, :, :, W:, :].any(), label
    err = np.abs(planar_grad(t) - truth_t)
    print(f"{label}: d_t: max error {err.max():.3e}, {float((err / e_t).max()):.4f} of its bound")
    assert np.all(err <= e_t), (label, float(err.max()))
    assert planar_grad(res).astype(np.float32).tobytes() == truth_res.astype(np.float32).tobytes(), label


def planar_grad(t):
    return R.from_c16(t.grad.cpu().numpy(), t.lw).astype(np.float64)


def check_norm_grads(norms, z1, zd, w1, b1, d_t, d_res, e_t, truth, label, active=None):
    """norms.*.grad against `truth` (None: the restatement's) under the module docstring's bounds; z1 / zd, d_t / d_res: f64
    truth; active: the device's own relu mask t > 0 where no golden pins it."""
    n = z1.size // 32
    g = D.tail_grads(z1, zd, w1, b1, d_t, d_res, active)
    carried = D.tail_bounds(z1, zd, w1, b1, e_t, np.zeros_like(e_t), active)
    for k in NORM_KEYS:
        got = getattr(norms, k).grad.detach().cpu().numpy().astype(np.float64)
        want = g["d_" + k] if truth is None else truth["d_" + k]
        err = np.abs(got - want)
        bound = carried["d_" + k] + (n + 4) * EPS32 * g["abs_d_" + k] + R.ulp32(want)
        print(f"{label}: d_{k}: max error {err.max():.3e}, {float((err / bound).max()):.4f} of its bound")
        assert got.shape == (32,) and not np.isnan(got).any() and np.all(err <= bound), (label, k, float(err.max()))


@pytest.mark.parametrize("name", LAYER_CASES)
def test_input_and_norm_gradients_match_the_reference_blocks_autograd(name):
    z = D.load_case(name)
    layer, norms = layer_from_golden(z, f32_model()), norms_from_golden(z)
    z1, zd, z1_dev, zd_dev = golden_inputs(z)            # (their padding columns hold NaN: it must not reach a gradient)
    t, res = norms(z1_dev, zd_dev)
    assert t.grad_fn is not None and t.lw == res.lw == z["c1"].shape[-1] and t.shape == z1_dev.shape
    assert not t.detach()[:, :, :, :, t.lw:, :].any() and not res.detach()[:, :, :, :, t.lw:, :].any()
    t.retain_grad()
    res.retain_grad()
    feat = layer(t, res)
    assert np.array_equal(planar(feat) > 0, z["y_block"] > 0)          # the relu mask is the reference's
    feat.backward(c16_dev(z["upstream"]))
    c = {k: z[k] for k in ("weight_bar", "bn_weight", "bn_bias", "running_mean", "running_var")} | {"eps": float(z["eps"])}
    u1, v1 = R.power_iteration(z["weight_bar"], z["u"], z["v"])
    e_t = input_grad_bound(folded(c, u1, v1), z["y_block"], z["upstream"])
    check_input_grads(t, res, z["ref64_d_t"], z["ref64_d_res"], e_t, name)
    truth = {f"d_{k}": z[f"ref64_d_{k}"] for k in NORM_KEYS}
    check_norm_grads(norms, z1, zd, z["bn1_weight"], z["bn1_bias"], z["ref64_d_t"], z["ref64_d_res"], e_t, truth, name)
    if name == "inactive":
        assert not t.grad.any() and not res.grad.any() and not any(getattr(norms, k).grad.any() for k in NORM_KEYS)
    else:
        assert all(float(getattr(norms, k).grad.abs().max()) > 0 for k in NORM_KEYS)


@pytest.mark.parametrize("name", ["b2_l3_5x7", "b1_l2_3x70"])
def test_parameter_gradients_keep_their_bytes_and_nothing_new_is_launched_without_input_gradients(name, monkeypatch):
    z = R.load_case(name)
    grads = {}
    for with_inputs in (True, False):
        layer = layer_from_golden(z, f32_model())
        t, res = c16_dev(z["t"]), c16_dev(z["res"])
        if with_inputs:
            t.requires_grad_(True)
            res.requires_grad_(True)
        else:
            def refuse(*a, **k):
                raise AssertionError("conv32_dgrad was called though no input requires grad")
            monkeypatch.setattr(last_conv, "conv32_dgrad", refuse)
        layer(t, res).backward(c16_dev(z["upstream"]))
        assert (t.grad is not None) == with_inputs and (res.grad is not None) == with_inputs
        grads[with_inputs] = [p.grad.clone() for p in layer.parameters()]
    assert all(torch.equal(a, b) for a, b in zip(grads[True], grads[False])) and len(grads[True]) == 3
    # one input alone: the other's gradient is not produced, the bytes are those of the joint call
    monkeypatch.undo()
    layer = layer_from_golden(z, f32_model())
    t, res = c16_dev(z["t"]), c16_dev(z["res"]).requires_grad_(True)
    res.lw, res.c16 = t.lw, True
    layer(t, res).backward(c16_dev(z["upstream"]))
    assert t.grad is None
    want = np.where(z["y"] > 0, z["upstream"], np.float32(0))
    assert R.from_c16(res.grad.cpu().numpy(), t.lw).tobytes() == want.tobytes()


def tail_chain(m, x, gt=None):
    """-> the modules and tensors after one forward / backward of TailNorms -> LastConv -> PredHead -> calculate_loss."""
    snap = m.sn_snapshot()
    z1, zd = m.forward_tail_normed(x)
    m.sn_restore(snap)
    norms, layer, head = TailNorms.from_model(m), LastConv.from_model(m), PredHead.from_model(m)
    before = consts(layer)
    t, res = norms(z1, zd)
    t.retain_grad()
    res.retain_grad()
    feat = layer(t, res)
    feat.retain_grad()
    if gt is None:
        gt = fit_data(make_model("f32"))[1]
    total, _ = losses.calculate_loss(head(feat), gt)
    total.backward()
    return norms, layer, head, z1, zd, t, res, feat, before, total


def check_chain_against_the_restatement(norms, layer, z1, zd, t, res, feat, before, label):
    up = R.from_c16(feat.grad.cpu().numpy(), feat.lw)
    u1, v1 = R.power_iteration(before["weight_bar"], before["weight_u"], before["weight_v"])
    Wf = folded(before, u1, v1)
    g = D.dgrad(Wf, planar(feat), up)
    e_t = input_grad_bound(Wf, planar(feat), up)
    check_input_grads(t, res, g["d_x"], g["d_res"], e_t, label)
    w1, b1 = (getattr(norms, k).detach().cpu().numpy() for k in ("bn1_weight", "bn1_bias"))
    z1p, zdp = planar(z1).astype(np.float64), planar(zd).astype(np.float64)
    active = planar(t) > 0                                 # the device's own mask, as feat's is for conv2
    pre1 = D.tail_forward(z1p, zdp, w1, b1, w1, b1)[2]
    assert np.array_equal(active, pre1 > 0) or np.abs(pre1[active != (pre1 > 0)]).max() <= 1e-6
    check_norm_grads(norms, z1p, zdp, w1, b1, g["d_x"], g["d_res"], e_t, None, label, active)


def test_backward_through_the_loss_matches_the_restatement_on_the_devices_own_upstream():
    m = make_model("f32")
    norms, layer, head, z1, zd, t, res, feat, before, _ = tail_chain(m, x_dev())
    assert float(feat.grad.abs().max()) > 0 and float(t.grad.abs().max()) > 0 and float(res.grad.abs().max()) > 0
    check_chain_against_the_restatement(norms, layer, z1, zd, t, res, feat, before, "tail norms through the loss")
    truth, u1, v1, dM, d_shift, abs_dM, n = restated_grads(layer, before, t, feat)
    check_param_grads(layer, before, u1, v1, truth, dM, d_shift, abs_dM, n, "tail norms through the loss")
    assert all(float(getattr(norms, k).grad.abs().max()) > 0 for k in NORM_KEYS)


def sn_state(m):
    return {k: v.clone() for k, v in m.state_dict().items() if k.endswith(("weight_u", "weight_v"))}


@pytest.mark.parametrize("precision", ["f16x2", "f32"])
def test_normed_pair_and_tail_norms_reproduce_the_tail_inputs(precision):
    m = make_model(precision)
    x = x_dev()
    snap = m.sn_snapshot()
    t, res = m.forward_tail_inputs(x)
    assert m.calls == 1
    after = sn_state(m)
    m.sn_restore(snap)
    z1, zd = m.forward_tail_normed(x)
    assert m.calls == 1 and z1.shape == zd.shape == t.shape and z1.lw == zd.lw == t.lw == 16 and z1.c16 and zd.c16
    assert not z1.requires_grad and z1.grad_fn is None and float(z1.min()) < 0.0        # no relu, no gradient
    now = sn_state(m)
    assert len(now) == 24 and all(torch.equal(after[k], now[k]) for k in after)          # the same power iteration
    assert all(not torch.equal(p, v) for p, v in snap[0])                                # ... of all twelve layers
    got_t, got_res = TailNorms.from_model(m)(z1, zd)
    for got, want, k in ((got_t, t, "t"), (got_res, res, "res")):
        err = (got.detach() - want).abs()[:, :, :, :, :16, :]
        print(f"{precision}: TailNorms(forward_tail_normed) vs forward_tail_inputs: {k}: max |d| = {float(err.max()):.3e}")
        assert bool((err <= 1e-5 + 1e-5 * want.abs()[:, :, :, :, :16, :]).all())
    m.forward_tail_normed(x)
    assert m.calls == 2


def test_fit_tail_norms_without_the_norms_is_fit_tail():
    a, b = make_model(), make_model()
    x, gt = fit_data(make_model())
    ha = finetune.fit_tail(a, x, gt, train=("pred", "conv2", "bn2"), steps=3, lr=1e-3)
    hb = finetune.fit_tail_norms(b, x, gt, train=("pred", "conv2", "bn2"), steps=3, lr=1e-3)
    assert ha == hb and len(ha) == 3
    sa, sb = a.state_dict(), b.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa) and a.calls == b.calls


def test_one_sgd_step_of_fit_tail_norms_is_the_manual_step_and_the_rest_is_restored():
    lr = 1e-3
    m = make_model("f32")
    x, gt = fit_data(make_model("f32"))
    before = {k: v.clone() for k, v in m.state_dict().items()}
    calls = m.calls
    hist = finetune.fit_tail_norms(m, x, gt, steps=1, lr=lr, optimizer="sgd")
    assert len(hist) == 1 and set(hist[0]) == {"loss", "loss_dict"} and hist[0]["loss"] > 0 and m.calls == calls
    after = m.state_dict()
    changed = {k for k in before if not torch.equal(before[k], after[k])}
    assert changed == TAIL_KEYS | NORM_STATE and len(changed) == 11
    # the same step by hand on a second instance, checked against the restated gradients
    ref = make_model("f32")
    norms, layer, head, z1, zd, t, res, feat, c0, total = tail_chain(ref, x, gt)
    assert float(total.detach()) == hist[0]["loss"]
    check_chain_against_the_restatement(norms, layer, z1, zd, t, res, feat, c0, "fit_tail_norms' step")
    torch.optim.SGD(list(head.parameters()) + list(layer.parameters()) + list(norms.parameters()), lr=lr).step()
    for key, p in ((PRE + "conv2.module.weight_bar", layer.weight_bar), (PRE + "bn2.weight", layer.bn_weight),
                   (PRE + "bn2.bias", layer.bn_bias), ("UNet.pred.conv3d.weight", head.weight), ("UNet.pred.conv3d.bias", head.bias),
                   (PRE + "bn1.weight", norms.bn1_weight), (PRE + "bn1.bias", norms.bn1_bias),
                   (PRE + "downsample.1.weight", norms.bnd_weight), (PRE + "downsample.1.bias", norms.bnd_bias)):
        assert torch.equal(after[key], p.detach().reshape(after[key].shape)), key   # the same kernels on the same bytes
    assert torch.equal(after[PRE + "conv2.module.weight_u"], layer.weight_u)
    # only 'bn1' and 'bnd': the convolution, its bn2 and the head keep their bytes
    m2 = make_model("f32")
    finetune.fit_tail_norms(m2, x, gt, train=("bn1", "bnd"), steps=2, lr=lr, optimizer="sgd")
    changed = {k for k, v in m2.state_dict().items() if not torch.equal(before[k], v)}
    assert changed == NORM_STATE | {PRE + "conv2.module.weight_u", PRE + "conv2.module.weight_v"}


def test_write_back_then_the_model_runs_the_tuned_norms():
    m = make_model()
    x = x_dev()
    norms, layer, head, z1, zd, t, res, feat, _, _ = tail_chain(m, x, fit_data(make_model())[1])
    pred = head(feat).detach()
    with torch.no_grad():
        for p in list(norms.parameters()) + list(layer.parameters()) + list(head.parameters()):
            p.sub_(0.05 * p.grad / (p.grad.abs().max() + 1e-30) * p.abs().max())
    before = {k: v.clone() for k, v in m.state_dict().items()}
    for mod in (norms, layer, head):
        mod.write_back(m)
    changed = {k for k, v in m.state_dict().items() if not torch.equal(before[k], v)}
    assert changed == TAIL_KEYS | NORM_STATE
    # the model's next call iterates every spectral-norm layer once: the eleven frozen ones as in forward_tail_normed, the
    # tuned one from the vectors the layer left -- as the layer's own next forward does
    want = m(x)
    have = head(layer(*norms(z1, zd))).detach()
    err = (have - want).abs()
    print(f"write_back: tuned norms and tail vs model(x): max |d| = {float(err.max()):.3e}")
    assert bool((err <= 1e-5 + 1e-5 * want.abs()).all())
    assert float((have - pred).abs().max()) > 1e-4                   # the update did change the output
