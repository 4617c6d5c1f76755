"""V2ce3d.forward_dec1_inputs, Dec1Conv on the model's own tensors, finetune.fit_dec1_conv and ``v2ce_finetune.py --train
dec1_conv2`` on the GPU (dec1_conv.py, finetune.py), on the [1, 2, 2, 16, 16] synthetic input of the other model tests.

Model.  With precision 'f32' ``Dec1Conv`` on the accessor's pair reproduces ``forward_dec2_sources``'s h1 byte for byte (the
same launch on the same bytes: the model's power iteration kernel, the model's pack of W_bar with its sigma, the model's
fold of bn2), s2 and x1 have the accessor's bytes, and both paths leave the same power-iteration state.  In 'f16x2' the
prediction through ``Dec1Conv -> Dec2BlockThrough -> LastBlock -> PredHead`` is within the project's parity tolerance of
``model.forward`` (1e-5 abs + 1e-5 rel), ``forward`` returns its bytes before and after the accessor has run, and the
layer's guard value is inside the limit.

Launch counts.  No convc_dgrad call when neither input requires grad, no convc_wgrad call when no parameter does, and the
64-channel entries of dec2_conv are never called by the new layer.

Fit.  The loss falls on the synthetic recording, ``train`` without the two new groups is fit_dec2_block step for step,
write_back -> state_dict -> the inference loader runs, the command line writes its two files."""
import json

import numpy as np
import pytest
import torch

from test_gpu_dec2_block_model import ALL_KEYS as DEC2_ALL_KEYS
from test_gpu_dec2_conv_model import same_bytes
from test_gpu_last_block_autograd import recording, sn_state, teacher
from test_gpu_last_conv_autograd import make_model, x_dev
from v2ce_toolbox_amd import dec1_conv, dec2_conv, finetune, losses, synth
from v2ce_toolbox_amd.dec1_conv import Dec1Conv
from v2ce_toolbox_amd.dec2_block import Dec2BlockThrough
from v2ce_toolbox_amd.last_block import LastBlock
from v2ce_toolbox_amd.pred_head import PredHead

pytestmark = pytest.mark.gpu

PRE1 = "UNet.decoders.1."
DEC1_KEYS = {PRE1 + "conv2.module.weight_bar", PRE1 + "conv2.module.weight_u", PRE1 + "conv2.module.weight_v",
             PRE1 + "bn2.weight", PRE1 + "bn2.bias"}
ALL_KEYS = DEC1_KEYS | DEC2_ALL_KEYS


def inputs(m, x):
    """-> (t1, res1, s2, x1) with the model's spectral-norm state put back: layers made afterwards iterate from the entry
    state."""
    snap = m.sn_snapshot()
    out = m.forward_dec1_inputs(x)
    m.sn_restore(snap)
    return out


def test_f32_accessor_and_dec1_conv_give_the_bytes_of_dec2s_source():
    m = make_model("f32")
    x = x_dev()
    snap = m.sn_snapshot()
    calls = m.calls
    t1, res1, s2, x1 = m.forward_dec1_inputs(x)
    assert m.calls == calls + 1
    for a in (t1, res1):
        assert a.shape[:4] == (1, 2, 8, 4) and a.shape[5] == 16 and a.lw == 4 and a.shape[4] >= 4
    assert s2.shape == (1, 2, 4, 8, 8, 16) and s2.lw == 8 and x1.shape == (1, 2, 2, 16, 16, 16) and x1.lw == 16
    assert all(a.c16 and not a.requires_grad and a.grad_fn is None for a in (t1, res1, s2, x1))
    after = sn_state(m)
    m.sn_restore(snap)
    conv = Dec1Conv.from_model(m)                           # u, v from before the call: the layer iterates them itself
    assert tuple(conv.weight_bar.shape) == (128, 128, 3, 3, 3) and conv.C == 128 and conv.INDEX == 3
    h1 = conv(t1, res1)
    assert h1.grad_fn is not None and h1.lw == 4 and h1.c16 and h1.shape == t1.shape
    want_h1, want_s2, want_x1 = m.forward_dec2_sources(x)
    now = sn_state(m)
    assert len(now) == 24 and all(torch.equal(after[k], now[k]) for k in after)          # the same power iteration
    assert m.calls == calls + 1                                                           # (sn_restore put the counter back)
    assert same_bytes(s2, want_s2) and same_bytes(x1, want_x1)
    lw = h1.lw
    assert same_bytes(h1.detach()[:, :, :, :, :lw, :], want_h1[:, :, :, :, :lw, :]), float((h1.detach() - want_h1).abs().max())
    inner = m.UNet.decoders[1].conv2.module                 # both advanced conv2's vectors by one iteration, by the same kernel
    assert torch.equal(conv.weight_u, inner.weight_u) and torch.equal(conv.weight_v, inner.weight_v)


def test_f16x2_prediction_through_the_layers_matches_forward_and_forward_keeps_its_bytes():
    m = make_model("f16x2")
    x = x_dev()
    snap = m.sn_snapshot()
    first = m(x).clone()
    m.sn_restore(snap)
    t1, res1, s2, x1 = inputs(m, x)
    assert hasattr(s2, "absmax") and hasattr(x1, "absmax")
    conv, dec2 = Dec1Conv.from_model(m), Dec2BlockThrough.from_model(m)
    block, head = LastBlock.from_model(m), PredHead.from_model(m)
    h1 = conv(t1, res1)
    assert hasattr(h1, "absmax") and tuple(h1.absmax.shape) == (1, 2) and h1.grad_fn is not None
    pred = head(block(dec2(h1, s2), x1))
    err = (pred.detach() - first).abs()
    print(f"f16x2: Dec1Conv -> Dec2BlockThrough -> LastBlock -> PredHead vs forward: max |d| = {float(err.max()):.3e}")
    assert bool((err <= 1e-5 + 1e-5 * first.abs()).all())
    print(f"f16x2: Dec1Conv guard {float(conv.guard):.3e} (limit {m.RANGE_GUARD_LIMIT:.1e})")
    assert 0.0 < float(conv.guard) <= m.RANGE_GUARD_LIMIT
    # the accessor left nothing behind: from the restored spectral-norm state forward returns its bytes
    m.sn_restore(snap)
    assert same_bytes(m(x), first)
    m.sn_restore(snap)
    m.forward_dec1_inputs(x)
    m.sn_restore(snap)
    assert same_bytes(m(x), first)


def test_launch_counts(monkeypatch):
    m = make_model("f32")
    x = x_dev()
    t1, res1, _, _ = inputs(m, x)
    conv = Dec1Conv.from_model(m)
    calls = []
    for mod, names in ((dec1_conv, ("convc_wgrad", "convc_dgrad")), (dec2_conv, ("convn_wgrad", "convn_dgrad"))):
        for n in names:
            real = getattr(mod, n)
            monkeypatch.setattr(mod, n, lambda *a, _n=n, _real=real, **k: calls.append((_n, tuple(k["want"]))) or _real(*a, **k))
    up = torch.randn(t1.shape, generator=torch.Generator().manual_seed(1)).cuda()
    conv(t1, res1).backward(up)                             # parameters alone: no input gradient
    assert calls == [("convc_wgrad", ("weight", "shift"))]
    assert all(p.grad is not None and float(p.grad.abs().max()) > 0 for p in conv.parameters()) and len(list(conv.parameters())) == 3
    calls.clear()
    tg, rg = t1.clone().requires_grad_(True), res1.clone().requires_grad_(True)
    tg.lw = rg.lw = t1.lw
    conv(tg, rg).backward(up)
    assert calls == [("convc_wgrad", ("weight", "shift")), ("convc_dgrad", ("x", "res"))]
    assert tg.grad.shape == t1.shape and not tg.grad[:, :, :, :, t1.lw:, :].any() and float(tg.grad.abs().max()) > 0
    calls.clear()
    for p in conv.parameters():
        p.requires_grad_(False)
    tg.grad = rg.grad = None
    conv(tg, res1).backward(up)                             # one input alone: no weight gradient
    assert calls == [("convc_dgrad", ("x",))] and tg.grad is not None
    calls.clear()
    out = conv(t1, res1)
    assert out.grad_fn is None and not out.requires_grad and not calls
    assert not any(n.startswith("convn") for n, _ in calls)


def test_write_back_then_the_model_runs_the_tuned_layers():
    m = make_model()
    x = x_dev()
    gt = teacher(m, x)
    t1, res1, s2, x1 = inputs(m, x)
    conv, dec2 = Dec1Conv.from_model(m), Dec2BlockThrough.from_model(m)
    block, head = LastBlock.from_model(m), PredHead.from_model(m)
    pred = head(block(dec2(conv(t1, res1), s2), x1))
    losses.calculate_loss(pred, gt)[0].backward()
    mods = (conv, dec2, block, head)
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
    assert changed == ALL_KEYS
    want = m(x)
    have = head(block(dec2(conv(t1, res1), s2), x1)).detach()
    err = (have - want).abs()
    print(f"write_back: tuned layers vs model(x): max |d| = {float(err.max()):.3e}")
    assert bool((err <= 1e-5 + 1e-5 * want.abs()).all())
    assert float((have - pred.detach()).abs().max()) > 1e-4          # the update did change the output
    # state_dict -> the inference loader
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    m2 = make_model()
    m2.load_state_dict(sd)
    m2 = m2.to("cuda:0")
    assert all(torch.equal(v, m.state_dict()[k]) for k, v in m2.state_dict().items())


FIT_LR = 1e-5                                                # plain gradient descent, as in the fit_dec2_block tests


def test_fit_dec1_conv_lowers_the_loss_and_restores_the_rest():
    xs, gs = recording()
    m = make_model()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    calls = m.calls
    hist = finetune.fit_dec1_conv(m, xs, gs, steps=6, lr=FIT_LR, optimizer="sgd")
    loss = [h["loss"] for h in hist]
    still = [h["loss"] for h in finetune.fit_dec1_conv(make_model(), xs, gs, steps=6, lr=0.0, optimizer="sgd")]
    print(f"fit_dec1_conv: losses {loss}; without updates {still}")
    assert len(hist) == 6 and all(set(h) == {"loss", "loss_dict"} for h in hist) and all(np.isfinite(loss))
    assert loss[4] < loss[0]                               # window 0 at step 0 and after four updates
    assert loss[0] == still[0] and all(a < b for a, b in zip(loss[1:], still[1:]))   # every update lowered what followed
    after = m.state_dict()
    changed = {k for k in before if not torch.equal(before[k], after[k])}
    assert changed == ALL_KEYS and m.calls == calls and m._prep is None
    # only the two new groups: the layers behind them keep their bytes (their convolutions' u / v keep the fit's iterations)
    m2 = make_model()
    finetune.fit_dec1_conv(m2, xs, gs, train=("dec1_conv2", "dec1_bn2"), steps=2, lr=FIT_LR, optimizer="sgd")
    changed = {k for k, v in m2.state_dict().items() if not torch.equal(before[k], v)}
    assert changed == DEC1_KEYS | {k for k in DEC2_ALL_KEYS if k.endswith(("weight_u", "weight_v"))}
    # a window beyond the cache budget is recomputed from the entry state: the same history
    m3 = make_model()
    h3 = finetune.fit_dec1_conv(m3, xs, gs, steps=6, lr=FIT_LR, optimizer="sgd", cache_bytes=0)
    assert h3 == hist and all(torch.equal(after[k], v) for k, v in m3.state_dict().items())


def test_fit_dec1_conv_without_the_new_groups_is_fit_dec2_block():
    xs, gs = recording()
    a, b = make_model(), make_model()
    ha = finetune.fit_dec2_block(a, xs, gs, train=finetune.DEC2_BLOCK_GROUPS, steps=3, lr=1e-3)
    hb = finetune.fit_dec1_conv(b, xs, gs, train=finetune.DEC2_BLOCK_GROUPS, steps=3, lr=1e-3)
    assert ha == hb and len(ha) == 3
    sa, sb = a.state_dict(), b.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa) and a.calls == b.calls
    assert finetune.DEC1_CONV_GROUPS == finetune.DEC2_BLOCK_GROUPS + ("dec1_conv2", "dec1_bn2")
    with pytest.raises(ValueError, match="train"):
        finetune.fit_dec1_conv(a, xs, gs, train=("dec0_conv2",), steps=1, lr=1e-3)


def test_command_line_trains_dec1_conv2_and_the_inference_loader_takes_the_result(tmp_path):
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
                   "--train", "dec1_conv2", "--stage1_losses", "pyramid", "ef", "--add_base_loss", "-o", out, "-l", "warning"])
    hist = json.load(open(out + ".history.json"))
    assert hist["windows"] == 2 and len(hist["history"]) == 3 and hist["loss"] == ["pyramid", "ef"]
    assert all(np.isfinite(h["loss"]) and set(h["loss_dict"]) == {"ef_loss", "pyramid_loss"} for h in hist["history"])
    model = get_trained_mode(out, "cuda:0")                          # the unchanged loader of v2ce.py -m
    tuned = model.state_dict()
    base = synth.make_state_dict(0)
    changed = {k for k in base if not torch.equal(torch.as_tensor(base[k]), tuned[k].cpu())}
    assert changed == ALL_KEYS, changed
    fr = synth.synthetic_frames(3, H, W, seed=5).astype(np.float32) / 255
    x = torch.from_numpy(((np.stack([fr[:-1], fr[1:]], axis=1) - np.float32(0.153)) / np.float32(0.165))[None]).to("cuda:0")
    assert bool(torch.isfinite(model(x)).all())
