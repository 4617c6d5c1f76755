"""PredHead as an autograd layer on the features of V2ce3d.forward_features, and finetune.fit_head, on the GPU: the
model at x [1, 2, 2, 16, 16] with synth.make_state_dict, against the numpy restatements (tests/pred_head_ref.py,
tests/voxlossgrads_ref.py, tests/voxlosses_ref.py).  The kernel bounds are those of tests/test_gpu_pred_head.py."""
import functools

import numpy as np
import pytest
import torch

from test_gpu_pred_head import check_against
from tests import pred_head_ref as R
from tests import voxlosses_ref as VL
from tests import voxlossgrads_ref as G
from v2ce_toolbox_amd import finetune, losses, synth
from v2ce_toolbox_amd.pred_head import PredHead, pred_head_forward
from v2ce_toolbox_amd.v2ce_3d import V2ce3d

pytestmark = pytest.mark.gpu

SHAPE = (1, 2, 2, 16, 16)
PYRAMID = dict(loss=("pyramid",), add_base_loss=True)


def make_model(seed=0):
    m = V2ce3d()
    m.load_state_dict(synth.make_state_dict(seed))
    return m.eval().to("cuda:0")


@functools.lru_cache(maxsize=None)
def image_units():
    fr = synth.synthetic_frames(SHAPE[1] + 1, SHAPE[3], SHAPE[4], seed=3).astype(np.float32) / 255
    x = np.stack([fr[:-1], fr[1:]], axis=1)
    return ((x - np.float32(0.153)) / np.float32(0.165))[None]


def x_dev():
    return torch.from_numpy(image_units()).to("cuda:0")


def planar(feat):
    """channels-last-16 device features -> [B, 32, L, H, W] numpy."""
    return R.from_c16(feat.cpu().numpy(), feat.lw)


def params(head):
    return head.weight.detach().cpu().numpy().reshape(-1, 32), head.bias.detach().cpu().numpy()


def perturbed(head, seed, scale):
    """A copy of the head with every parameter moved by a relative `scale` (and the bias by an absolute one)."""
    rng = np.random.default_rng(seed)
    other = PredHead(head.weight.shape[0]).to(head.weight.device)
    with torch.no_grad():
        w, b = head.weight.detach().cpu().numpy(), head.bias.detach().cpu().numpy()
        sw = np.abs(w).mean()
        other.weight.copy_(torch.from_numpy((w + scale * sw * rng.standard_normal(w.shape)).astype(np.float32)))
        other.bias.copy_(torch.from_numpy((b + scale * sw * rng.standard_normal(b.shape)).astype(np.float32)))
    return other


def test_forward_features_and_head_match_the_restatement_and_the_fused_forward():
    m = make_model()
    x = x_dev()
    feat = m.forward_features(x)
    assert feat.dim() == 6 and tuple(feat.shape[:4]) == (1, 2, 2, 16) and feat.shape[5] == 16 and feat.lw == 16
    assert not feat.requires_grad and feat.grad_fn is None and m.calls == 1
    head = PredHead.from_model(m)
    pred = head(feat)
    assert pred.shape == (1, 2, 20, 16, 16) and pred.grad_fn is not None and pred.is_contiguous()
    w, b = params(head)
    got = {"y": R.from_dense(pred.detach().cpu().numpy())}
    check_against(got, R.forward(planar(feat), w, b), None, 0, "head on forward_features")
    assert (got["y"] > 0).mean() > 0.05                              # the fixture has active units
    # a second instance from the same state dict: its first call runs the same spectral-norm iteration, head fused
    want = make_model()(x).cpu().numpy()
    have = pred.detach().cpu().numpy()
    err = np.abs(have - want)
    print(f"head on features vs fused forward: max |d| = {err.max():.3e}")
    assert np.all(err <= 1e-5 + 1e-5 * np.abs(want)), err.max()


def test_backward_through_calculate_loss_matches_the_restatement():
    m = make_model()
    feat = m.forward_features(x_dev())
    head = PredHead.from_model(m)
    gt = pred_head_forward(feat, *[p.detach() for p in perturbed(head, 5, 0.3).parameters()])
    pred = head(feat)
    pred.retain_grad()
    total, d = losses.calculate_loss(pred, gt)
    total.backward()
    assert head.weight.grad.shape == head.weight.shape and head.bias.grad.shape == head.bias.shape
    up = R.from_dense(pred.grad.cpu().numpy())                       # the gradient the device produced
    assert np.abs(up).max() > 0
    w, _ = params(head)
    f = planar(feat)
    want = R.grads(f, R.from_dense(pred.detach().cpu().numpy()), up, w)
    got = {"y": np.zeros(1, np.float32), "d_weight": head.weight.grad.cpu().numpy().reshape(-1, 32),
           "d_bias": head.bias.grad.cpu().numpy()}
    check_against(got, np.zeros(1), want, R.positions(f), "autograd")
    assert np.abs(got["d_weight"]).max() > 0 and np.abs(got["d_bias"]).max() > 0
    # the features need no gradient: none was computed
    assert feat.grad is None


def test_gradients_are_exactly_zero_at_the_ground_truth():
    m = make_model()
    feat = m.forward_features(x_dev())
    head = PredHead.from_model(m)
    gt = head(feat).detach().clone()
    total, _ = losses.calculate_loss(head(feat), gt, **PYRAMID)
    total.backward()
    assert float(total.detach()) == 0.0
    assert (head.weight.grad == 0).all() and (head.bias.grad == 0).all()


def test_write_back_then_the_fused_forward_runs_the_tuned_head():
    m = make_model()
    x = x_dev()
    snap = m.sn_snapshot()
    feat = m.forward_features(x)
    m.sn_restore(snap)                                               # the next call repeats that spectral-norm iteration
    before = m(x).cpu().numpy()
    m.sn_restore(snap)
    head = perturbed(PredHead.from_model(m), 9, 0.5)
    own = head(feat).detach().cpu().numpy()
    assert np.abs(own - before).max() > 1e-3                         # the perturbed head computes something else
    head.write_back(m)
    after = m(x).cpu().numpy()
    err = np.abs(after - own)
    print(f"write_back: max |d| = {err.max():.3e}")
    assert np.all(err <= 1e-5 + 1e-5 * np.abs(own)), err.max()


def restated_fit(f, gt32, w, b, lr, steps):
    """The steps of fit_head in f64: pred -> rounded to f32 as the device hands it to the loss -> the loss and its
    gradient (voxlosses_ref, voxlossgrads_ref) -> the head's gradients (pred_head_ref) -> plain SGD."""
    w, b = w.astype(np.float64), b.astype(np.float64)
    hist = []
    for k in range(steps + 1):
        p32 = R.to_dense(R.forward(f, w, b)).astype(np.float32)
        value, _ = VL.loss_values([VL.total(VL.batch_stats(p32, gt32, terms=("pyramid",)))], **PYRAMID)
        hist.append(float(value))
        if k == steps:                                             # the loss after the last update; no further step
            break
        up, _ = G.grad(p32, gt32, **PYRAMID)
        g = R.grads(f, R.from_dense(p32), R.from_dense(up), w)
        w, b = w - lr * g["d_weight"], b - lr * g["d_bias"]
    return hist, w, b


STEPS = 4
# max |device parameter - restated parameter| / max |parameter| after STEPS steps, measured once against the restatement
# on an MI355X: 5.165e-08 (the parameters moved by 1.682e-02 on that scale).  The bound is 4 x that, for the f32
# roundings of every step (pred, pred.grad, the head's gradients, the update): about one f32 epsilon per step
MEASURED_PARAM_DEV = 5.165e-08
PARAM_TOL = 4 * MEASURED_PARAM_DEV


def test_fit_head_follows_the_restatement_and_leaves_the_trunk_alone():
    m = make_model()
    x = x_dev()
    snap = m.sn_snapshot()
    feat = m.forward_features(x)
    m.sn_restore(snap)
    assert m.calls == 0
    head = PredHead.from_model(m)
    gt = pred_head_forward(feat, *[p.detach() for p in perturbed(head, 11, 0.3).parameters()])
    f, gt32 = planar(feat), gt.cpu().numpy()
    w0, b0 = params(head)
    # the step: 1 / (an upper bound of the loss's curvature in the parameters).  The loss is alpha / 3 (mse + the mse of
    # three average pools); a pool is a contraction, so its curvature in pred is at most 2 alpha 4 / (3 n); a channel's
    # output is linear in its 33 parameters with rows [feat(pos), 1], whose Gram matrix is bounded by its trace S
    n = gt32.size
    S = float((f.astype(np.float64) ** 2).sum() + R.positions(f))
    lr = 1.0 / (8.0 * 1000 / (3.0 * n) * S)
    hist, w_ref, b_ref = restated_fit(f, gt32, w0, b0, lr, STEPS)
    print(f"lr = {lr:.4e}; restated losses {hist}")
    # the step size is checked, not assumed: the restatement decreases at every step, by far more than f32 resolves
    assert all(b < a * (1 - 1e-5) for a, b in zip(hist, hist[1:])), hist
    state = {k: v.clone() for k, v in m.state_dict().items()}
    history = finetune.fit_head(m, x, gt, steps=STEPS, lr=lr, optimizer="sgd", **PYRAMID)
    dev = [h["loss"] for h in history]
    print(f"device losses {dev}")
    assert len(history) == STEPS and all(set(h) == {"loss", "loss_dict"} and "pyramid_loss" in h["loss_dict"] for h in history)
    assert all(b < a for a, b in zip(dev, dev[1:])), dev
    assert np.allclose(dev, hist[:STEPS], rtol=1e-5, atol=0), (dev, hist)
    # the model afterwards: the head moved, nothing else did
    after = m.state_dict()
    head_keys = {"UNet.pred.conv3d.weight", "UNet.pred.conv3d.bias"}
    changed = {k for k in state if not torch.equal(state[k], after[k])}
    assert changed == head_keys, changed
    assert m.calls == 0 and m._prep is None
    w1, b1 = after["UNet.pred.conv3d.weight"].cpu().numpy().reshape(-1, 32), after["UNet.pred.conv3d.bias"].cpu().numpy()
    scale = max(np.abs(w_ref).max(), np.abs(b_ref).max())
    dev_w = max(np.abs(w1 - w_ref).max(), np.abs(b1 - b_ref).max()) / scale
    moved = max(np.abs(w1 - w0).max(), np.abs(b1 - b0).max()) / scale
    print(f"parameters: moved {moved:.3e}, deviation from the restatement {dev_w:.3e} (relative to max |parameter|)")
    assert moved > 100 * dev_w
    assert dev_w <= PARAM_TOL, (dev_w, PARAM_TOL)


def test_fit_head_adam_recomputes_features_beyond_the_cache_budget():
    m = make_model()
    x = x_dev()
    snap = m.sn_snapshot()
    feat = m.forward_features(x)
    m.sn_restore(snap)
    head = PredHead.from_model(m)
    gt = pred_head_forward(feat, *[p.detach() for p in perturbed(head, 13, 0.3).parameters()])
    state = {k: v.clone() for k, v in m.state_dict().items()}
    cached = finetune.fit_head(m, [x, x], [gt, gt], steps=4, lr=1e-3, optimizer="adam")
    tuned = {k: v.clone() for k, v in m.state_dict().items()}
    m.load_state_dict(state)
    m.to("cuda:0")
    again = finetune.fit_head(m, [x, x], [gt, gt], steps=4, lr=1e-3, optimizer="adam", cache_bytes=0)
    assert cached == again                                           # recomputed features are the cached ones
    assert all(torch.equal(tuned[k], v) for k, v in m.state_dict().items())
    assert m.calls == 0 and all(np.isfinite(h["loss"]) for h in cached)
    assert any(not torch.equal(tuned[k], state[k]) for k in ("UNet.pred.conv3d.weight", "UNet.pred.conv3d.bias"))


def test_command_line_writes_a_state_dict_the_inference_loader_takes(tmp_path):
    import json

    from v2ce_toolbox_amd.LDATI import EVENT_DTYPE
    from v2ce_toolbox_amd.v2ce import get_trained_mode
    H, W, frames = 32, 48, 6                                         # 5 pairs: one window of 4 and one of 1
    rng = np.random.default_rng(21)
    n = 4000
    ev = np.zeros(n, EVENT_DTYPE)
    ev["timestamp"] = np.sort(rng.integers(0, int((frames - 1) / 30 * 1e6), n))
    ev["x"], ev["y"], ev["polarity"] = rng.integers(0, W, n), rng.integers(0, H, n), rng.integers(0, 2, n)
    gt_path, out = str(tmp_path / "gt.npy"), str(tmp_path / "tuned.pt")
    np.save(gt_path, ev)
    finetune.main(["--synthetic", str(frames), "--synthetic_weights", "0", "--height", str(H), "--width", str(W),
                   "--seq_len", "4", "--gt_events", gt_path, "--steps", "3", "--lr", "1e-3", "--optimizer", "adam",
                   "--stage1_losses", "pyramid", "ef", "--add_base_loss", "-o", out, "-l", "warning"])
    hist = json.load(open(out + ".history.json"))
    assert hist["windows"] == 2 and len(hist["history"]) == 3 and hist["loss"] == ["pyramid", "ef"]
    assert all(np.isfinite(h["loss"]) and set(h["loss_dict"]) == {"ef_loss", "pyramid_loss"} for h in hist["history"])
    tuned = get_trained_mode(out, "cuda:0").state_dict()            # the unchanged loader of v2ce.py -m
    base = synth.make_state_dict(0)
    changed = {k for k in base if not torch.equal(torch.as_tensor(base[k]), tuned[k].cpu())}
    assert changed == {"UNet.pred.conv3d.weight", "UNet.pred.conv3d.bias"}, changed
