"""V2ce3d.forward_dec2_sources / forward_dec2_normed, Dec2Convs / Dec2Norms / Dec2Block on the model's own tensors,
finetune.fit_dec2_block and ``v2ce_finetune.py --train dec2_block`` on the GPU (dec2_block.py, finetune.py), on the
[1, 2, 2, 16, 16] synthetic input of tests/test_gpu_dec2_conv_model.py.

Model.  With precision 'f32' ``Dec2Convs`` on the accessor's sources reproduces ``forward_dec2_normed``'s pair byte for
byte: the same launches on the same bytes (the model's power iteration kernel, the model's pack of W_bar / sigma, epilogue
vectors built as ``_normed_epilogues`` builds them).  ``Dec2Norms`` of that, fed to ``Dec2Conv``, then ``LastBlock`` and
``PredHead``, reproduces ``model.forward`` within the project's parity tolerance (1e-5 abs + 1e-5 rel, BASELINE.json
north_star), in 'f32' and in 'f16x2'; the measured differences are printed.  ``forward`` returns the same bytes before and
after the accessors have run.

Launch count.  No convupn_wgrad call when no parameter of Dec2Convs requires grad.

Fit.  Modelled on the fit_dec2_conv tests: the loss falls on a synthetic recording, ``train`` without the four new groups is
fit_dec2_conv step for step, write_back -> state_dict -> the inference loader runs, the command line writes its two files."""
import json

import numpy as np
import pytest
import torch

from test_gpu_dec2_conv_model import DEC2_KEYS, HEAD_KEYS, same_bytes
from test_gpu_last_block_autograd import CONV_KEYS, NORM_STATE, TAIL_KEYS, recording, sn_state, teacher
from test_gpu_last_conv_autograd import make_model, x_dev
from v2ce_toolbox_amd import dec2_block, finetune, losses, synth
from v2ce_toolbox_amd.dec2_block import Dec2Block, Dec2Convs, Dec2Norms
from v2ce_toolbox_amd.dec2_conv import Dec2Conv
from v2ce_toolbox_amd.last_block import LastBlock
from v2ce_toolbox_amd.pred_head import PredHead

pytestmark = pytest.mark.gpu

PRE2 = "UNet.decoders.2."
DEC2_CONVS_KEYS = {PRE2 + "conv1.module.weight_bar", PRE2 + "conv1.module.weight_u", PRE2 + "conv1.module.weight_v",
                   PRE2 + "downsample.0.weight", PRE2 + "downsample.0.bias"}
DEC2_NORM_KEYS = {PRE2 + "bn1.weight", PRE2 + "bn1.bias", PRE2 + "downsample.1.weight", PRE2 + "downsample.1.bias"}
ALL_KEYS = DEC2_CONVS_KEYS | DEC2_NORM_KEYS | DEC2_KEYS | CONV_KEYS | TAIL_KEYS | NORM_STATE | HEAD_KEYS


def sources(m, x):
    """-> (h1, s2, x1) with the model's spectral-norm state put back: layers made afterwards iterate from the entry state."""
    snap = m.sn_snapshot()
    out = m.forward_dec2_sources(x)
    m.sn_restore(snap)
    return out


def test_f32_accessors_and_dec2_convs_give_the_bytes_of_the_normed_pair():
    m = make_model("f32")
    x = x_dev()
    snap = m.sn_snapshot()
    calls = m.calls
    h1, s2, x1 = m.forward_dec2_sources(x)
    assert m.calls == calls + 1
    assert h1.shape[:4] == (1, 2, 8, 4) and h1.shape[5] == 16 and h1.lw == 4 and h1.shape[4] >= 4
    assert s2.shape == (1, 2, 4, 8, 8, 16) and s2.lw == 8 and x1.shape == (1, 2, 2, 16, 16, 16) and x1.lw == 16
    assert all(a.c16 and not a.requires_grad and a.grad_fn is None for a in (h1, s2, x1))
    after = sn_state(m)
    m.sn_restore(snap)
    convs = Dec2Convs.from_model(m)                         # u, v from before the call: the layer iterates them itself
    z1, zd = convs(h1, s2)
    assert z1.grad_fn is not None and zd.grad_fn is not None and z1.lw == zd.lw == 8 and z1.c16 and zd.c16
    want1, wantd, want_x1 = m.forward_dec2_normed(x)
    now = sn_state(m)
    assert len(now) == 24 and all(torch.equal(after[k], now[k]) for k in after)          # the same power iteration
    assert m.calls == calls + 1 and same_bytes(x1, want_x1)                               # (sn_restore put the counter back)
    assert same_bytes(z1.detach(), want1), float((z1.detach() - want1).abs().max())
    assert same_bytes(zd.detach(), wantd), float((zd.detach() - wantd).abs().max())
    inner = m.UNet.decoders[2].conv1.module                 # both advanced conv1's vectors by one iteration, by the same kernel
    assert torch.equal(convs.weight_u, inner.weight_u) and torch.equal(convs.weight_v, inner.weight_v)
    # the norms turn the pair into forward_dec2_inputs's, up to the affine fold's rounding
    m.sn_restore(snap)
    t2, res2, _ = m.forward_dec2_inputs(x)
    t, res = Dec2Norms.from_model(m)(z1, zd)
    assert t.shape == t2.shape and not t[:, :, :, :, t.lw:, :].any() and hasattr(t, "absmax")
    for got, want, k in ((t, t2, "t2"), (res, res2, "res2")):
        err = (got.detach() - want).abs()
        print(f"f32: Dec2Norms(Dec2Convs(sources)) vs forward_dec2_inputs: {k}: max |d| = {float(err.max()):.3e}")
        assert bool((err <= 1e-5 + 1e-5 * want.abs()).all())


@pytest.mark.parametrize("precision", ["f32", "f16x2"])
def test_prediction_through_the_layers_matches_forward_and_forward_keeps_its_bytes(precision):
    m = make_model(precision)
    x = x_dev()
    snap = m.sn_snapshot()
    first = m(x).clone()
    m.sn_restore(snap)
    h1, s2, x1 = sources(m, x)
    if precision == "f16x2":
        assert hasattr(h1, "absmax") and hasattr(s2, "absmax") and hasattr(x1, "absmax")
    dec2, block, head = Dec2Block.from_model(m), LastBlock.from_model(m), PredHead.from_model(m)
    z1, zd = dec2.convs(h1, s2)
    want1, wantd, _ = m.forward_dec2_normed(x)
    m.sn_restore(snap)
    for got, want, k in ((z1, want1, "z1"), (zd, wantd, "zd")):
        err = (got.detach() - want).abs()[:, :, :, :, :8, :]
        print(f"{precision}: Dec2Convs(forward_dec2_sources) vs forward_dec2_normed: {k}: max |d| = {float(err.max()):.3e}")
        assert bool((err <= 1e-5 + 1e-5 * want.abs()[:, :, :, :, :8, :]).all())
    x0 = dec2.conv(*dec2.norms(z1, zd))
    if precision == "f16x2":
        assert hasattr(x0, "absmax") and tuple(x0.absmax.shape) == (1, 2)
        assert 0.0 < float(dec2.convs.guard) <= m.RANGE_GUARD_LIMIT
    pred = head(block(x0, x1))
    err = (pred.detach() - first).abs()
    print(f"{precision}: Dec2Block -> LastBlock -> PredHead vs forward: max |d| = {float(err.max()):.3e}")
    assert bool((err <= 1e-5 + 1e-5 * first.abs()).all())
    # the accessors left nothing behind: from the restored spectral-norm state forward returns its bytes
    m.sn_restore(snap)
    assert same_bytes(m(x), first)
    m.sn_restore(snap)
    m.forward_dec2_sources(x)
    m.forward_dec2_normed(x)
    m.forward_dec2_inputs(x)
    m.sn_restore(snap)
    assert same_bytes(m(x), first)


def test_sources_that_require_grad_are_refused_and_nothing_is_launched_without_trainable_parameters(monkeypatch):
    m = make_model("f32")
    x = x_dev()
    h1, s2, _ = sources(m, x)
    dec2 = Dec2Block.from_model(m)
    hg = h1.clone().requires_grad_(True)
    hg.lw = h1.lw
    with pytest.raises(ValueError, match="no gradient with respect to x0 and x1"):
        dec2(hg, s2)
    sg = s2.clone().requires_grad_(True)
    sg.lw = s2.lw
    with pytest.raises(ValueError, match="input gradient"):
        dec2.convs(h1, sg)
    calls = []
    real = dec2_block.convupn_wgrad
    monkeypatch.setattr(dec2_block, "convupn_wgrad", lambda *a, **k: calls.append(k["want"]) or real(*a, **k))
    up = torch.randn(s2.shape, generator=torch.Generator().manual_seed(1)).cuda()
    dec2(h1, s2).backward(up)
    assert calls == [("weight", "short", "short_bias")]
    assert all(p.grad is not None and float(p.grad.abs().max()) > 0 for p in dec2.parameters()) and len(list(dec2.parameters())) == 10
    calls.clear()
    dec2.convs.weight_bar.requires_grad_(False)
    dec2(h1, s2).backward(up)
    assert calls == [("short", "short_bias")]
    calls.clear()
    for q in dec2.convs.parameters():
        q.requires_grad_(False)
    dec2(h1, s2).backward(up)                               # the norms and conv2 still train
    assert not calls
    for q in dec2.parameters():
        q.requires_grad_(False)
    out = dec2(h1, s2)
    assert out.grad_fn is None and not out.requires_grad and not calls


def test_write_back_then_the_model_runs_the_tuned_layers():
    m = make_model()
    x = x_dev()
    gt = teacher(m, x)
    h1, s2, x1 = sources(m, x)
    dec2, block, head = Dec2Block.from_model(m), LastBlock.from_model(m), PredHead.from_model(m)
    pred = head(block(dec2(h1, s2), x1))
    losses.calculate_loss(pred, gt)[0].backward()
    mods = (dec2, block, head)
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
    have = head(block(dec2(h1, s2), x1)).detach()
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


def test_fit_dec2_block_lowers_the_loss_and_restores_the_rest():
    xs, gs = recording()
    m = make_model()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    calls = m.calls
    hist = finetune.fit_dec2_block(m, xs, gs, steps=6, lr=FIT_LR, optimizer="sgd")
    loss = [h["loss"] for h in hist]
    still = [h["loss"] for h in finetune.fit_dec2_block(make_model(), xs, gs, steps=6, lr=0.0, optimizer="sgd")]
    print(f"fit_dec2_block: losses {loss}; without updates {still}")
    assert len(hist) == 6 and all(set(h) == {"loss", "loss_dict"} for h in hist) and all(np.isfinite(loss))
    assert loss[4] < loss[0]                               # window 0 at step 0 and after four updates
    assert loss[0] == still[0] and all(a < b for a, b in zip(loss[1:], still[1:]))   # every update lowered what followed
    after = m.state_dict()
    changed = {k for k in before if not torch.equal(before[k], after[k])}
    assert changed == ALL_KEYS and m.calls == calls and m._prep is None
    # only the four new groups: the layers behind them keep their bytes (their convolutions' u / v keep the fit's iterations)
    m2 = make_model()
    finetune.fit_dec2_block(m2, xs, gs, train=("dec2_conv1", "dec2_convd", "dec2_bn1", "dec2_bnd"), steps=2, lr=FIT_LR, optimizer="sgd")
    changed = {k for k, v in m2.state_dict().items() if not torch.equal(before[k], v)}
    assert changed == DEC2_CONVS_KEYS | DEC2_NORM_KEYS | {k for k in DEC2_KEYS | CONV_KEYS | TAIL_KEYS if k.endswith(("weight_u", "weight_v"))}
    # a window beyond the cache budget is recomputed from the entry state: the same history
    m3 = make_model()
    h3 = finetune.fit_dec2_block(m3, xs, gs, steps=6, lr=FIT_LR, optimizer="sgd", cache_bytes=0)
    assert h3 == hist and all(torch.equal(after[k], v) for k, v in m3.state_dict().items())


def test_fit_dec2_block_without_the_new_groups_is_fit_dec2_conv():
    xs, gs = recording()
    a, b = make_model(), make_model()
    ha = finetune.fit_dec2_conv(a, xs, gs, train=finetune.DEC2_CONV_GROUPS, steps=3, lr=1e-3)
    hb = finetune.fit_dec2_block(b, xs, gs, train=finetune.DEC2_CONV_GROUPS, steps=3, lr=1e-3)
    assert ha == hb and len(ha) == 3
    sa, sb = a.state_dict(), b.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa) and a.calls == b.calls
    assert finetune.DEC2_BLOCK_GROUPS == finetune.DEC2_CONV_GROUPS + ("dec2_conv1", "dec2_convd", "dec2_bn1", "dec2_bnd")
    with pytest.raises(ValueError, match="train"):
        finetune.fit_dec2_block(a, xs, gs, train=("dec1_conv2",), steps=1, lr=1e-3)


def test_command_line_trains_dec2_block_and_the_inference_loader_takes_the_result(tmp_path):
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
                   "--train", "dec2_block", "--stage1_losses", "pyramid", "ef", "--add_base_loss", "-o", out, "-l", "warning"])
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
