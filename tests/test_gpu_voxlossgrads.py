"""GPU: the gradient of the stage-1 voxel losses (csrc/voxlossgrads.hip through v2ce_voxloss_grads /
v2ce_volume_loss_grads; losses.py) against the numpy f64 restatement (tests/voxlossgrads_ref.py) and, through
calculate_loss(...).backward() and the drop-in modules, against the reference's own autograd results
(tests/golden/.voxlossgrads/); the [N, D, H, W] entry against the 5-D entry, bit for bit; what stays unchanged without
grad; invariance to batching, repetition and alignment; NaN; refusals.

Bound, per element: |got - want| <= 2^-23 |want| + 1e-12 M, with M the sum of the absolute per-term contributions of
the restatement at that element: the one f32 rounding of the store, plus the project's allowance for f64 sums taken in
another order and for the device's exp / log."""
import numpy as np
import pytest
import torch

from tests import voxlossgrads_ref as G
from tests.test_voxlossgrads_cpu import GOLDENS, golden_specs, name_of
from v2ce_toolbox_amd import hip
from v2ce_toolbox_amd import losses as VL

pytestmark = pytest.mark.gpu
EACH = [(n,) for n in G.ALL_LOSS]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def voxels(rng, shape, density=0.3, scale=0.5):
    return (rng.exponential(scale, shape) * (rng.random(shape) < density)).astype(np.float32)


def pair(seed, shape):
    rng = np.random.default_rng(seed)
    p, g = voxels(rng, shape), voxels(rng, shape)
    thr = np.float32(0.01)
    p.reshape(-1)[::13] = thr                          # exactly at the threshold: not above it
    p.reshape(-1)[5::17] = np.nextafter(thr, np.float32(1))
    g.reshape(-1)[::29] = thr
    return p, g


def check(got, want, M, what=""):
    got = got.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(got) else got.astype(np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want)
    bound = 2.0 ** -23 * np.abs(want) + 1e-12 * M
    bad = err > bound
    print(f"{what}: max |d| {err.max():.3e}, max |want| {np.abs(want).max():.3e}, worst err / bound "
          f"{(err / np.maximum(bound, 1e-300)).max():.3f}")
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[0], err[bad].max(), bound[bad].min())


@pytest.mark.parametrize("B,L,H,W", [(1, 1, 8, 8), (1, 1, 9, 15), (2, 3, 11, 13), (1, 4, 16, 24), (3, 2, 8, 70),
                                     (1, 5, 17, 23), (2, 3, 7, 9)])
def test_gradient_matches_the_restatement(B, L, H, W):
    p, g = pair(B * 1000 + L * 100 + H, (B, L, 20, H, W))
    pd, gd = dev(p), dev(g)
    pyramid = min(H, W) >= 8
    lists = [t for t in EACH if pyramid or t != ("pyramid",)]
    lists += [tuple(n for n in G.DEFAULT_LOSS if pyramid or n != "pyramid"),
              tuple(n for n in G.ALL_LOSS if pyramid or n != "pyramid")]
    for loss in lists:
        for kw in (dict(), dict(ef_type="only_c", add_base_loss=True), dict(ef_type="cl")):
            if kw and len(loss) == 1 and loss[0] not in ("ef", "ef_splitp", "pyramid"):
                continue
            want, M = G.grad(p, g, loss, **kw)
            got = VL.voxel_loss_grads_batch(pd, gd, loss=loss, **kw)
            assert got.dtype == torch.float32 and got.shape == pd.shape and got.is_contiguous()
            check(got, want, M, f"{loss} {kw}")


def test_gradient_of_the_default_list_at_full_size():
    p, g = pair(77, (1, 16, 20, 260, 346))
    want, M = G.grad(p, g, G.DEFAULT_LOSS)
    check(VL.voxel_loss_grads_batch(dev(p), dev(g)), want, M, "default list at [1, 16, 20, 260, 346]")


def spec_kwargs(kw):
    kw = dict(kw)
    kw["loss"] = tuple(kw["loss"])
    return kw


@pytest.mark.parametrize("path", GOLDENS, ids=name_of)
def test_backward_of_calculate_loss_against_the_reference_autograd(path):
    for key, z, kw, stages, i in golden_specs(path):
        if i:                                          # the second stage is checked with the first
            continue
        kw = spec_kwargs(kw)
        g = dev(z["gt"])
        preds = [dev(z["pred"]).requires_grad_()] + ([dev(z["pred2"]).requires_grad_()] if stages == 2 else [])
        total, d = VL.calculate_loss(preds if stages == 2 else preds[0], g, **kw)
        assert total.grad_fn is not None and total.dtype == torch.float32 and total.dim() == 0 and total.is_cuda
        assert all(not v.requires_grad and not v.is_cuda for v in d.values())
        total.backward()
        for j, p in enumerate(preds):
            k = key if j == 0 else f"{key}_p2"
            _, M = G.grad(z["pred2"] if j else z["pred"], z["gt"], stages=stages, **kw)
            check(p.grad, z[f"ref64_grad_{k}"], M, f"{name_of(path)} {k}")
        assert g.grad is None


def test_backward_through_a_non_leaf_and_a_scaled_loss():
    z = np.load([p for p in GOLDENS if name_of(p) == "b2_l3_9x10"][0])
    kw = dict(loss=G.ALL_LOSS, ef_type="c+cl", add_base_loss=True)
    want = z["ref64_grad_full_c_cl_base1"]
    _, M = G.grad(z["pred"], z["gt"], **kw)
    g = dev(z["gt"])
    x = dev(z["pred"]).requires_grad_()
    p = x * 1
    assert not p.is_leaf
    VL.calculate_loss(p, g, **kw)[0].backward()
    check(x.grad, want, M, "non-leaf")
    x = dev(z["pred"]).requires_grad_()
    (3 * VL.calculate_loss(x, g, **kw)[0]).backward()              # the incoming gradient is read on the device
    check(x.grad, 3 * want, 3 * M, "3 * total")
    x = dev(z["pred"]).requires_grad_()
    total, _ = VL.calculate_loss(x, g, **kw)
    (gr,) = torch.autograd.grad(total, x)
    check(gr, want, M, "autograd.grad")
    with pytest.raises(RuntimeError):                               # once differentiable
        x = dev(z["pred"]).requires_grad_()
        (gr,) = torch.autograd.grad(VL.calculate_loss(x, g, **kw)[0], x, create_graph=True)
        gr.sum().backward()


def to_volumes(t):
    B, L, C, H, W = t.shape
    return t.reshape(B, L, 2, 10, H, W).permute(0, 2, 1, 3, 4, 5).reshape(B * 2, L * 10, H, W).contiguous()


def test_drop_in_modules_backpropagate():
    p, g = pair(21, (2, 3, 20, 9, 12))
    gd = dev(g)
    for module, loss, kw in ((VL.CompensationLoss(), ("compensation",), dict(alpha_compensation=1)),
                             (VL.MatchLoss(), ("match",), dict(alpha_match=1))):
        x = dev(p).requires_grad_()
        v = module(x, gd)
        assert v.grad_fn is not None and v.dim() == 0 and v.dtype == torch.float32
        with torch.no_grad():
            assert float(module(x, gd)) == float(v)
        v.backward()
        want, M = G.grad(p, g, loss, **kw)
        check(x.grad, want, M, type(module).__name__)
    rng = np.random.default_rng(22)
    for D in (8, 9, 11, 13, 25):                       # D % 3 = 2, 0, 2, 1, 1; partial last group of 8 planes
        pv, gv = voxels(rng, (2, D, 9, 10)), voxels(rng, (2, D, 9, 10))
        for module, loss, kw in ((VL.Pyramid3dLoss(add_base_loss=True), ("pyramid",), dict(add_base_loss=True)),
                                 (VL.Pyramid3dLoss(), ("pyramid",), dict()), (VL.PyramidTemporalLoss(), ("pt",), dict())):
            x = dev(pv).requires_grad_()
            v = module(x, dev(gv))
            assert v.grad_fn is not None
            with torch.no_grad():
                assert float(module(x, dev(gv))) == float(v)
            v.backward()
            want, M = G.volume_grad(pv, gv, loss, alpha_pyramid=1, **kw)
            check(x.grad, want, M, f"{type(module).__name__} D={D}")
    pv, gv = voxels(rng, (1, 5, 3, 3)), voxels(rng, (1, 5, 3, 3))    # the temporal term alone needs D >= 5 only
    x = dev(pv).requires_grad_()
    VL.PyramidTemporalLoss()(x, dev(gv)).backward()
    want, M = G.volume_grad(pv, gv, ("pt",), alpha_pyramid=1)
    check(x.grad, want, M, "PyramidTemporalLoss [1, 5, 3, 3]")


@pytest.mark.parametrize("B,L,H,W", [(2, 3, 11, 13), (1, 1, 8, 8), (1, 2, 9, 70)])
def test_volume_entry_equals_the_5d_entry_bit_for_bit(B, L, H, W):
    p, g = pair(31 + L, (B, L, 20, H, W))
    pd, gd = dev(p), dev(g)
    for loss, base in ((("pyramid", "pt"), True), (("pyramid",), False), (("pt",), False)):
        a = VL.voxel_loss_grads_batch(pd, gd, loss=loss, add_base_loss=base)
        b = VL.volume_loss_grads_batch(to_volumes(pd), to_volumes(gd), loss=loss, add_base_loss=base)
        assert b.shape == (2 * B, 10 * L, H, W)
        assert to_volumes(a).cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), loss
        assert a.abs().sum() > 0


def test_nothing_changes_without_grad():
    z = np.load([p for p in GOLDENS if name_of(p) == "b1_l1_8x8"][0])
    g = dev(z["gt"])
    for staged in (False, True):
        mk = lambda req: ([dev(z["pred"]).requires_grad_(req), dev(z["pred2"]).requires_grad_(req)] if staged
                          else dev(z["pred"]).requires_grad_(req))
        with_grad, d1 = VL.calculate_loss(mk(True), g, loss=G.ALL_LOSS)
        assert with_grad.grad_fn is not None
        plain, d2 = VL.calculate_loss(mk(False), g, loss=G.ALL_LOSS)
        with torch.no_grad():
            quiet, d3 = VL.calculate_loss(mk(True), g, loss=G.ALL_LOSS)
        for t in (plain, quiet):
            assert t.grad_fn is None and not t.requires_grad
            assert t.cpu().numpy().tobytes() == with_grad.detach().cpu().numpy().tobytes()
        assert list(d1) == list(d2) == list(d3)
        for k in d1:
            assert d1[k].numpy().tobytes() == d2[k].numpy().tobytes() == d3[k].numpy().tobytes(), k
            assert not d1[k].requires_grad and d1[k].grad_fn is None


def test_batch_equals_single_calls_and_repeats():
    p, g = pair(8, (3, 5, 20, 13, 18))
    sq = float((p.astype(np.float64) ** 2).sum())
    coef = VL.grad_coeffs(p.shape, G.ALL_LOSS, add_base_loss=True, pred_sq_sum=sq)
    a = VL.voxel_loss_grads_batch(dev(p), dev(g), coef=coef).cpu().numpy()
    b = VL.voxel_loss_grads_batch(dev(p), dev(g), coef=coef).cpu().numpy()
    assert a.tobytes() == b.tobytes()
    assert a.tobytes() == VL.voxel_loss_grads_batch(dev(p), dev(g), loss=G.ALL_LOSS, add_base_loss=True).cpu().numpy().tobytes()
    for i in range(3):
        one = VL.voxel_loss_grads_batch(dev(p[i:i + 1]), dev(g[i:i + 1]), coef=coef).cpu().numpy()
        assert one.tobytes() == a[i:i + 1].tobytes(), i
    pv, gv = to_volumes(dev(p)), to_volumes(dev(g))
    vc = VL.grad_coeffs(tuple(pv.shape), ("pyramid", "pt"), add_base_loss=True)
    a = VL.volume_loss_grads_batch(pv, gv, coef=vc).cpu().numpy()
    assert a.tobytes() == VL.volume_loss_grads_batch(pv, gv, coef=vc).cpu().numpy().tobytes()
    for i in (0, 5):
        one = VL.volume_loss_grads_batch(pv[i:i + 1].contiguous(), gv[i:i + 1].contiguous(), coef=vc).cpu().numpy()
        assert one.tobytes() == a[i:i + 1].tobytes(), i


def test_misaligned_bases():
    p, g = pair(5, (2, 3, 20, 9, 11))
    want = VL.voxel_loss_grads_batch(dev(p), dev(g), loss=G.ALL_LOSS).cpu().numpy()

    def off_by_one(a):                                 # contiguous, one element past a 256-byte boundary
        big = torch.zeros(64 + 1 + a.size, device="cuda")
        k = (-big.data_ptr() // 4) % 64 + 1
        v = big[k:k + a.size].view(a.shape)
        assert v.data_ptr() % 256 == 4
        v.copy_(dev(a))
        return v
    pv, gv, out = off_by_one(p), off_by_one(g), off_by_one(np.zeros_like(p))
    up = torch.ones(1, device="cuda")
    got = VL.voxel_loss_grads_batch(pv, gv, loss=G.ALL_LOSS, grad=out, upstream=up)
    assert got is out
    assert got.cpu().numpy().tobytes() == want.tobytes()
    vv = VL.volume_loss_grads_batch(to_volumes(dev(p)), to_volumes(dev(g))).cpu().numpy()
    tp, tg = off_by_one(to_volumes(dev(p)).cpu().numpy()), off_by_one(to_volumes(dev(g)).cpu().numpy())
    assert VL.volume_loss_grads_batch(tp, tg, grad=off_by_one(np.zeros_like(vv))).cpu().numpy().tobytes() == vv.tobytes()


@pytest.mark.parametrize("at", [(0, 1, 3, 2, 5), (1, 0, 14, 7, 11), (0, 1, 9, 8, 3)])
def test_nan_stays_inside_the_windows_it_falls_in(at):
    p, g = pair(6, (2, 2, 20, 9, 12))                  # column 11 and row 8 lie outside the floored k = 8 (and row 8: k = 2) extents
    p[at] = np.nan
    with np.errstate(invalid="ignore"):
        want, M = G.grad(p, g, ("pyramid",), add_base_loss=True)
    got = VL.voxel_loss_grads_batch(dev(p), dev(g), loss=("pyramid",), add_base_loss=True).cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want))
    n = int(np.isnan(want).sum())
    assert n == {5: 512, 11: 64, 3: 1}[at[4]], n       # the 8-window; the 4-window; the element alone
    ok = ~np.isnan(want)
    assert np.all(np.abs(got[ok] - want[ok]) <= 2.0 ** -23 * np.abs(want[ok]) + 1e-12 * M[ok])


def test_refusals():
    x = torch.zeros(1, 2, 20, 8, 8, device="cuda")
    y = torch.zeros(1, 2, 20, 8, 8, device="cuda")
    VL.voxel_loss_grads_batch(x, y, grad=torch.empty_like(x), upstream=torch.ones((), device="cuda"))
    with pytest.raises(ValueError, match="overlaps"):
        VL.voxel_loss_grads_batch(x, y, grad=x)
    with pytest.raises(ValueError, match="overlaps"):
        VL.voxel_loss_grads_batch(x, y, grad=y)
    both = torch.zeros(2 * x.numel() - 4, device="cuda")
    with pytest.raises(ValueError, match="overlaps"):                # the tail of grad is the head of pred
        VL.voxel_loss_grads_batch(both[x.numel() - 4:].view(x.shape), y, grad=both[:x.numel()].view(x.shape))
    with pytest.raises(ValueError, match="overlaps"):
        VL.voxel_loss_grads_batch(x, y, upstream=x.view(-1)[7:8])
    with pytest.raises(ValueError, match="overlaps"):
        VL.volume_loss_grads_batch(x[0], y[0], upstream=y.view(-1)[:1])
    with pytest.raises(ValueError, match="float32"):
        VL.voxel_loss_grads_batch(x, y, grad=torch.empty_like(x, dtype=torch.float64))
    with pytest.raises(ValueError, match="float32"):
        VL.voxel_loss_grads_batch(x, y, upstream=torch.ones(1, device="cuda", dtype=torch.float64))
    with pytest.raises(ValueError, match="float32"):
        VL.voxel_loss_grads_batch(x.double(), y.double())
    with pytest.raises(ValueError, match="contiguous"):
        VL.voxel_loss_grads_batch(x, y, grad=torch.zeros(1, 2, 20, 8, 16, device="cuda")[..., ::2])
    with pytest.raises(ValueError, match="contiguous"):
        VL.voxel_loss_grads_batch(torch.zeros(1, 2, 20, 8, 16, device="cuda")[..., ::2], y)
    with pytest.raises(ValueError, match="lives on"):
        VL.voxel_loss_grads_batch(x, y, grad=torch.empty(x.shape))
    with pytest.raises(ValueError, match="lives on"):
        VL.voxel_loss_grads_batch(x, y, upstream=torch.ones(1))
    with pytest.raises(ValueError, match="one element"):
        VL.voxel_loss_grads_batch(x, y, upstream=torch.ones(2, device="cuda"))
    with pytest.raises(ValueError, match="shape"):
        VL.voxel_loss_grads_batch(x, y, grad=torch.empty(1, 2, 20, 8, 9, device="cuda"))
    with pytest.raises(hip.V2ceHipError, match="no CPU path"):
        VL.voxel_loss_grads_batch(x.cpu(), y.cpu())
    with pytest.raises(hip.V2ceHipError, match="no CPU path"):
        VL.calculate_loss(x.cpu().requires_grad_(), y.cpu())
    small = torch.zeros(1, 2, 20, 7, 9, device="cuda")
    with pytest.raises(ValueError, match="smaller than kernel size"):
        VL.voxel_loss_grads_batch(small, small)
    with pytest.raises(ValueError, match="discriminator"):
        VL.calculate_loss(x.clone().requires_grad_(), y, loss=("pyramid", "gan"))
    with pytest.raises(ValueError, match="only"):
        VL.volume_loss_grads_batch(x[0], y[0], loss=("ef",))
