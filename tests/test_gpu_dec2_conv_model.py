"""V2ce3d.forward_dec2_inputs, Dec2Conv on the model's own tensors, finetune.fit_dec2_conv and ``v2ce_finetune.py --train
dec2_conv2`` on the GPU (dec2_conv.py, finetune.py).

Model.  With precision 'f32' the layer on the accessor's pair reproduces ``forward_tail_sources``'s x0 byte for byte: the
same launches on the same bytes (conv1's and the shortcut's own launch in the accessor; in the layer the model's power
iteration kernel, the model's pack of W_bar / sigma and the model's BatchNorm fold).  With 'f16x2' the prediction through
Dec2Conv -> LastBlock -> PredHead matches ``model.forward`` at the project's parity tolerance (1e-5 abs + 1e-5 rel,
BASELINE.json north_star).  ``forward`` returns the same bytes before and after the accessor has run.

Launch count.  No convn_dgrad call when neither input requires grad, no convn_wgrad call when no parameter does.

Fit.  Modelled on the fit_last_block tests: the loss falls on a synthetic recording, ``train`` without the dec2 groups is
fit_last_block step for step, write_back -> state_dict -> the inference loader runs, the command line writes its two files."""
import json

import numpy as np
import pytest
import torch

from test_gpu_last_block_autograd import CONV_KEYS, NORM_STATE, TAIL_KEYS, recording, sn_state, teacher
from test_gpu_last_conv_autograd import make_model, x_dev
from v2ce_toolbox_amd import dec2_conv, finetune, losses, synth
from v2ce_toolbox_amd.dec2_conv import Dec2Conv
from v2ce_toolbox_amd.last_block import LastBlock
from v2ce_toolbox_amd.pred_head import PredHead

pytestmark = pytest.mark.gpu

PRE2 = "UNet.decoders.2."
DEC2_KEYS = {PRE2 + "conv2.module.weight_bar", PRE2 + "conv2.module.weight_u", PRE2 + "conv2.module.weight_v", PRE2 + "bn2.weight",
             PRE2 + "bn2.bias"}
HEAD_KEYS = {"UNet.pred.conv3d.weight", "UNet.pred.conv3d.bias"}


def same_bytes(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def test_f32_accessor_and_layer_give_the_bytes_of_the_tail_sources():
    m = make_model("f32")
    x = x_dev()
    snap = m.sn_snapshot()
    t2, res2, x1 = m.forward_dec2_inputs(x)
    assert m.calls == 1 and t2.shape == res2.shape == (1, 2, 4, 8, 8, 16) and x1.shape == (1, 2, 2, 16, 16, 16)
    assert t2.lw == res2.lw == 8 and x1.lw == 16 and t2.c16 and res2.c16 and x1.c16
    assert all(not a.requires_grad and a.grad_fn is None for a in (t2, res2, x1)) and float(t2.min()) >= 0.0
    after = sn_state(m)
    m.sn_restore(snap)
    layer = Dec2Conv.from_model(m)                          # u, v from before the call: the layer iterates them itself
    x0 = layer(t2, res2)
    assert x0.grad_fn is not None and x0.lw == 8 and x0.c16
    want0, want1 = m.forward_tail_sources(x)
    now = sn_state(m)
    assert len(now) == 24 and all(torch.equal(after[k], now[k]) for k in after)          # the same power iteration
    assert same_bytes(x1, want1)
    assert same_bytes(x0.detach(), want0), float((x0.detach() - want0).abs().max())
    inner = m.UNet.decoders[2].conv2.module                 # both advanced conv2's vectors by one iteration, by the same kernel
    assert torch.equal(layer.weight_u, inner.weight_u) and torch.equal(layer.weight_v, inner.weight_v)


def test_f16x2_prediction_through_the_layers_matches_forward_and_forward_keeps_its_bytes():
    m = make_model()
    x = x_dev()
    snap = m.sn_snapshot()
    first = m(x).clone()
    m.sn_restore(snap)
    t2, res2, x1 = m.forward_dec2_inputs(x)
    assert t2.shape == res2.shape == (1, 2, 4, 8, 8, 16) and hasattr(t2, "absmax") and hasattr(x1, "absmax")
    m.sn_restore(snap)
    layer, block, head = Dec2Conv.from_model(m), LastBlock.from_model(m), PredHead.from_model(m)
    x0 = layer(t2, res2)
    assert hasattr(x0, "absmax") and tuple(x0.absmax.shape) == (1, 2) and float(x0.absmax[0, 0]) == float(x0.detach().abs().max())
    pred = head(block(x0, x1))
    err = (pred.detach() - first).abs()
    print(f"f16x2: Dec2Conv -> LastBlock -> PredHead vs forward: max |d| = {float(err.max()):.3e}")
    assert bool((err <= 1e-5 + 1e-5 * first.abs()).all())
    assert 0.0 < float(layer.guard) <= m.RANGE_GUARD_LIMIT
    # the accessor left nothing behind: from the restored spectral-norm state forward returns its bytes
    m.sn_restore(snap)
    assert same_bytes(m(x), first)
    m.sn_restore(snap)
    m.forward_dec2_inputs(x)
    m.forward_tail_sources(x)
    m.sn_restore(snap)
    assert same_bytes(m(x), first)


def test_no_input_gradient_launch_without_inputs_that_need_one_and_no_weight_gradient_launch_without_parameters(monkeypatch):
    m = make_model("f32")
    x = x_dev()
    t2, res2, _ = m.forward_dec2_inputs(x)
    layer = Dec2Conv.from_model(m)
    calls = []
    real_w, real_d = dec2_conv.convn_wgrad, dec2_conv.convn_dgrad
    monkeypatch.setattr(dec2_conv, "convn_wgrad", lambda *a, **k: calls.append(("w", k["want"])) or real_w(*a, **k))
    monkeypatch.setattr(dec2_conv, "convn_dgrad", lambda *a, **k: calls.append(("d", k["want"])) or real_d(*a, **k))
    up = torch.randn(t2.shape, generator=torch.Generator().manual_seed(1)).cuda()
    layer(t2, res2).backward(up)
    assert calls == [("w", ("weight", "shift"))] and layer.weight_bar.grad is not None and layer.bn_bias.grad is not None
    calls.clear()
    layer.weight_bar.requires_grad_(False)
    layer.bn_weight.requires_grad_(False)
    layer(t2, res2).backward(up)
    assert calls == [("w", ("shift",))]
    calls.clear()
    layer.bn_bias.requires_grad_(False)
    tg = t2.clone().requires_grad_(True)
    tg.lw = t2.lw
    layer(tg, res2).backward(up)
    assert calls == [("d", ("x",))] and tg.grad is not None and tg.grad.shape == t2.shape
    calls.clear()
    rg = res2.clone().requires_grad_(True)
    rg.lw = res2.lw
    y = layer(tg, rg)
    y.backward(up)
    assert calls == [("d", ("x", "res"))]
    assert same_bytes(rg.grad, torch.where(y.detach() > 0, up, torch.zeros_like(up)))      # d_res: the masked upstream
    calls.clear()
    out = layer(t2, res2)
    assert out.grad_fn is None and not out.requires_grad and not calls


def test_write_back_then_the_model_runs_the_tuned_layers():
    m = make_model()
    x = x_dev()
    gt = teacher(m, x)
    snap = m.sn_snapshot()
    t2, res2, x1 = m.forward_dec2_inputs(x)
    m.sn_restore(snap)
    layer, block, head = Dec2Conv.from_model(m), LastBlock.from_model(m), PredHead.from_model(m)
    pred = head(block(layer(t2, res2), x1))
    losses.calculate_loss(pred, gt)[0].backward()
    mods = (layer, block, head)
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
    assert changed == DEC2_KEYS | CONV_KEYS | TAIL_KEYS | NORM_STATE
    want = m(x)
    have = head(block(layer(t2, res2), x1)).detach()
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


FIT_LR = 1e-5                                                # plain gradient descent, as in the fit_last_block tests


def test_fit_dec2_conv_lowers_the_loss_and_restores_the_rest():
    xs, gs = recording()
    m = make_model()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    calls = m.calls
    hist = finetune.fit_dec2_conv(m, xs, gs, steps=6, lr=FIT_LR, optimizer="sgd")
    loss = [h["loss"] for h in hist]
    still = [h["loss"] for h in finetune.fit_dec2_conv(make_model(), xs, gs, steps=6, lr=0.0, optimizer="sgd")]
    print(f"fit_dec2_conv: losses {loss}; without updates {still}")
    assert len(hist) == 6 and all(set(h) == {"loss", "loss_dict"} for h in hist) and all(np.isfinite(loss))
    assert loss[4] < loss[0]                               # window 0 at step 0 and after four updates
    assert loss[0] == still[0] and all(a < b for a, b in zip(loss[1:], still[1:]))   # every update lowered what followed
    after = m.state_dict()
    changed = {k for k in before if not torch.equal(before[k], after[k])}
    assert changed == DEC2_KEYS | CONV_KEYS | TAIL_KEYS | NORM_STATE | HEAD_KEYS and m.calls == calls and m._prep is None
    # only the two new groups: the layers behind them keep their bytes (their convolutions' u / v keep the fit's iterations)
    m2 = make_model()
    finetune.fit_dec2_conv(m2, xs, gs, train=("dec2_conv2", "dec2_bn2"), steps=2, lr=FIT_LR, optimizer="sgd")
    changed = {k for k, v in m2.state_dict().items() if not torch.equal(before[k], v)}
    assert changed == DEC2_KEYS | {k for k in CONV_KEYS | TAIL_KEYS if k.endswith(("weight_u", "weight_v"))}
    # a window beyond the cache budget is recomputed from the entry state: the same history
    m3 = make_model()
    h3 = finetune.fit_dec2_conv(m3, xs, gs, steps=6, lr=FIT_LR, optimizer="sgd", cache_bytes=0)
    assert h3 == hist and all(torch.equal(after[k], v) for k, v in m3.state_dict().items())


def test_fit_dec2_conv_without_the_dec2_groups_is_fit_last_block():
    xs, gs = recording()
    a, b = make_model(), make_model()
    ha = finetune.fit_last_block(a, xs, gs, train=finetune.LAST_BLOCK_GROUPS, steps=3, lr=1e-3)
    hb = finetune.fit_dec2_conv(b, xs, gs, train=finetune.LAST_BLOCK_GROUPS, steps=3, lr=1e-3)
    assert ha == hb and len(ha) == 3
    sa, sb = a.state_dict(), b.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa) and a.calls == b.calls
    assert finetune.DEC2_CONV_GROUPS == finetune.LAST_BLOCK_GROUPS + ("dec2_conv2", "dec2_bn2")
    with pytest.raises(ValueError, match="train"):
        finetune.fit_dec2_conv(a, xs, gs, train=("dec2_conv1",), steps=1, lr=1e-3)


def test_command_line_trains_dec2_conv2_and_the_inference_loader_takes_the_result(tmp_path):
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
                   "--train", "dec2_conv2", "--stage1_losses", "pyramid", "ef", "--add_base_loss", "-o", out, "-l", "warning"])
    hist = json.load(open(out + ".history.json"))
    assert hist["windows"] == 2 and len(hist["history"]) == 3 and hist["loss"] == ["pyramid", "ef"]
    assert all(np.isfinite(h["loss"]) and set(h["loss_dict"]) == {"ef_loss", "pyramid_loss"} for h in hist["history"])
    model = get_trained_mode(out, "cuda:0")                          # the unchanged loader of v2ce.py -m
    tuned = model.state_dict()
    base = synth.make_state_dict(0)
    changed = {k for k in base if not torch.equal(torch.as_tensor(base[k]), tuned[k].cpu())}
    assert changed == DEC2_KEYS | CONV_KEYS | TAIL_KEYS | NORM_STATE | HEAD_KEYS, changed
    fr = synth.synthetic_frames(3, H, W, seed=5).astype(np.float32) / 255
    x = torch.from_numpy(((np.stack([fr[:-1], fr[1:]], axis=1) - np.float32(0.153)) / np.float32(0.165))[None]).to("cuda:0")
    assert bool(torch.isfinite(model(x)).all())
