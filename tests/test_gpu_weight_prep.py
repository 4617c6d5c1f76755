"""The weight preparation stage against f64 and bit-exact restatements: the spectral-norm power iteration (v2ce_sn_power_iter,
v2ce_sn_update_batch in every mode) and the split-half packers (v2ce_pack_weights_f16x2 and its _up, _wt, _wt_slice, pred and
head forms, and the batched packs of csrc/sn.hip).  f64 helpers: tests/weight_ref.py.

* Power iteration: every step against an f64 half-step from the kernel's own previous vector (bars of a few f32 ulps derived
  from the kernel's roundings), and 64 steps against the f64 trajectory (sigma and the residual |W v - sigma u|).
* v2ce_sn_update_batch: one TABLE row per mode, each run twice on buffers poisoned with two patterns (a byte equal in both
  runs was written, a byte that differs was not), bit for bit against the per-layer calls the header promises it equals,
  against f64, and with the layers permuted.
* Packers: plain, pred and head planes bit for bit against numpy; folded (up) and Winograd-T planes within the split error
  of f64; the tail {bound, pre-scale} sound and tight; exactly the documented bytes written.
* The rejections of v2ce_sn_update_batch leave every device buffer unchanged.
* Every layer the model hands to v2ce_sn_update_batch has a TABLE row; 64 model calls against f64 and the oracle."""
import numpy as np
import pytest
import torch

from oracle import glue as OG
from oracle import unet as U
import weight_ref as R
from guarded import POISON, Guarded, written
from v2ce_toolbox_amd import synth

pytestmark = pytest.mark.gpu

OK, BAD_ARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -4
NO_PACK, NO_ITERATE = 1, 2
SIGMA_BAR = 8 * R.U32                            # f32 trajectory vs f64 trajectory, relative (f32 emulation: <= 2.2 ulps)


def L():
    from v2ce_toolbox_amd import hip
    return hip.lib()


def stream():
    from v2ce_toolbox_amd import hip
    return hip.stream_ptr()


def f32dev(x):
    return torch.as_tensor(np.ascontiguousarray(x, np.float32)).cuda()


def weights_dev(w):
    """w on the device with 28x its size of zeros behind it, so that a kernel reading another layer's rows or another kernel
    volume stays inside the allocation (and produces wrong values for the assertions to find)."""
    w = np.ascontiguousarray(w, np.float32).ravel()
    t = torch.zeros(28 * w.size + 65536, dtype=torch.float32, device="cuda")
    t[:w.size] = torch.from_numpy(w).cuda()
    return t


# ---------------------------------------------------------------------------------------------------------------------
# 1. per-layer power iteration
# ---------------------------------------------------------------------------------------------------------------------
SN_SHAPES = [(r, c) for r in (1, 15, 17, 32, 1056) for c in (1, 255, 257, 16 * 27, 512 * 27)]


def run_power_iter(W, u0, v0, steps, per_step=None):
    rows, cols = W.shape
    wd, ud, vd = f32dev(W), f32dev(u0), f32dev(v0)
    ws = torch.empty(L().v2ce_sn_workspace_bytes(rows, cols), dtype=torch.uint8, device="cuda")
    sig = torch.empty(1, device="cuda")
    for k in range(steps):
        u_prev = ud.cpu().numpy()
        assert L().v2ce_sn_power_iter(ud.data_ptr(), vd.data_ptr(), wd.data_ptr(), rows, cols, sig.data_ptr(), ws.data_ptr(),
                                      ws.numel(), stream()) == OK
        torch.cuda.synchronize()
        per_step(k, u_prev, vd.cpu().numpy(), ud.cpu().numpy(), float(sig.item()))


@pytest.mark.parametrize("rows,cols", SN_SHAPES, ids=[f"{r}x{c}" for r, c in SN_SHAPES])
def test_power_iter_vs_f64(rows, cols):
    rng = np.random.RandomState(rows * 7919 + cols)
    W = (rng.randn(rows, cols) * 0.05).astype(np.float32)
    u0 = rng.randn(rows).astype(np.float32)
    u0 = (u0 / np.linalg.norm(u0)).astype(np.float32)
    v0 = np.zeros(cols, np.float32)
    traj = R.trajectory(W, u0, 64)
    W64 = W.astype(np.float64)
    wsum = float(np.abs(W64).sum())
    st = {"ex": -np.inf, "v": 0.0, "u": 0.0, "s": 0.0, "traj": 0.0, "res": 0.0}

    def per_step(k, u_prev, v, u, sigma):
        ex, uv, uu, us = R.check_step(W64, u_prev, v, u, sigma)
        st["ex"], st["v"], st["u"], st["s"] = max(st["ex"], ex), max(st["v"], uv), max(st["u"], uu), max(st["s"], us)
        assert ex <= 0, f"step {k}: one-step excess {ex:.3e} (ulps v {uv:.2f} u {uu:.2f} sigma {us:.2f})"
        s64 = traj[k][2]
        st["traj"] = max(st["traj"], abs(sigma - s64) / s64 / R.U32)
        assert abs(sigma - s64) <= SIGMA_BAR * s64, (k, sigma, s64)
        res = float(np.linalg.norm(W64 @ v - sigma * u.astype(np.float64)))
        bar = 8 * R.U32 * sigma + 2.0 ** -48 * wsum
        st["res"] = max(st["res"], res / (R.U32 * sigma))
        assert res <= bar, (k, res, bar)
        if k == 63:
            st["drift_u"] = float(np.abs(u - traj[k][0]).max())
            st["drift_v"] = float(np.abs(v - traj[k][1]).max())

    run_power_iter(W, u0, v0, 64, per_step)
    print(f"sn {rows}x{cols}: worst ulps v {st['v']:.2f} u {st['u']:.2f} sigma {st['s']:.2f}, one-step excess {st['ex']:.2e}; "
          f"trajectory sigma {st['traj']:.2f} x 2^-24 rel, residual {st['res']:.2f} x 2^-24 sigma, "
          f"64-step drift u {st['drift_u']:.2e} v {st['drift_v']:.2e}")


# ---------------------------------------------------------------------------------------------------------------------
# packer checks (shared by the batched rows and the packer table)
# ---------------------------------------------------------------------------------------------------------------------
PACK_STATS = {}


def _stat(name, **kw):
    s = PACK_STATS.setdefault(name, {})
    for k, v in kw.items():
        s[k] = max(s.get(k, -np.inf), v)


def _tail_sound(name, hi, lo, tail0, scale):
    hi64, lo64 = hi.astype(np.float64), lo.astype(np.float64)
    assert np.all(np.isfinite(hi64)) and np.all(np.abs(hi64) <= R.F16_MAX), f"{name}: |hi| reaches fp16 overflow"
    assert scale == R.pow2_prescale(tail0), (name, tail0, scale)
    dec = np.abs(hi64 + lo64)
    # the planes hold the f32 values |v| <= tail[0] * pre-scale, up to the rounding of their lo halves
    over = float((dec - float(tail0) * float(scale) - R.split_err(lo)).max()) if dec.size else -1.0
    assert over <= 0, f"{name}: tail[0] {tail0!r} does not bound the planes (excess {over:.3e})"
    return dec


def check_plain(name, body, w, sigma, tail_words=2, scale_from_tail=False):
    """A v2ce_pack_weights_f16x2 buffer (or the plain part of an up buffer) of w [Cout][Cin][k3]: bit for bit."""
    Cout, Cin, k3 = w.shape
    n = Cout * Cin * k3
    hi, lo = R.decode(body, n)
    tail = R.tail_of(body, 4 * n, tail_words)
    q = R.quot32(w, sigma)
    amax = np.float32(np.abs(q).max())
    if scale_from_tail:                          # an up buffer: the folded sums may raise the common bound
        assert tail[0] >= amax, (name, tail[0], amax)
        s = R.pow2_prescale(tail[0])
    else:
        assert tail[0] == amax, f"{name}: tail[0] {tail[0]!r} != max |w / sigma| {amax!r}"
        s = R.pow2_prescale(amax)
    whi, wlo = R.split((q * s).astype(np.float32).reshape(Cout, Cin // 16, 16, k3).transpose(3, 1, 0, 2))
    for plane, got, want in (("hi", hi, whi.ravel()), ("lo", lo, wlo.ravel())):
        bad = np.nonzero(got.view(np.uint16) != want.view(np.uint16))[0]
        assert bad.size == 0, f"{name}: {bad.size} {plane} halves differ, first at {bad[0]}: got {got[bad[0]]!r} want {want[bad[0]]!r}"
    dec = _tail_sound(name, hi, lo, tail[0], tail[1])
    if not scale_from_tail and n:
        assert dec.max() >= float(tail[0]) * float(tail[1]) - R.split_err(lo).max()      # tight: equality up to the split
    if tail_words == 4:
        assert tail[2] == 0 and tail[3] == 0, (name, tail)
    _stat(name, bits=0.0)
    return tail


def _check_f64(name, hi, lo, val, mag, cnt, s):
    """hi + lo against s * (the f64 value) within the f32 evaluation's bound plus the split error."""
    shape = (-1,) + (1,) * (val.ndim - 1)
    bar = s * (cnt.reshape(shape) + 1) * R.U32 * mag + R.split_err(lo.reshape(val.shape))
    d = np.abs(hi.reshape(val.shape).astype(np.float64) + lo.reshape(val.shape).astype(np.float64) - float(s) * val)
    ex = float((d - bar).max())
    ratio = float((d / bar).max())
    _stat(name, excess=ex, ratio=ratio)
    assert ex <= 0, f"{name}: hi + lo off the f64 value by {ex:.3e} beyond the bar"


def check_up(name, body, w, C0, sigma):
    Cout, Cin, _ = w.shape
    n = Cout * Cin * 27
    tail = check_plain(name + "/plain", body[:4 * n + 16], w, sigma, tail_words=4, scale_from_tail=True)
    val, mag, cnt = R.up_fold_f64(w, sigma, C0)
    m = 108 * (C0 // 16) * Cout * 16
    fb = body[4 * n + 16:]
    assert fb.size == 4 * m
    hi, lo = fb[:2 * m].view(np.float16), fb[2 * m:].view(np.float16)
    _check_f64(name + "/fold", hi, lo, val, mag, cnt, tail[1])
    dec = _tail_sound(name + "/fold", hi, lo, tail[0], tail[1])
    q = np.abs(R.quot32(w, sigma)).max()
    # tail[0] = the larger of max |w / sigma| and the largest folded sum: tight up to the split and the sums' rounding
    top = max(float(q) * float(tail[1]), float(dec.max()) if dec.size else 0.0)
    assert float(tail[0]) * float(tail[1]) <= top * (1 + 8 * R.U32) + 2.0 ** -24, (name, tail, top)


def check_wt(name, body, w, ci0, cin, sigma):
    Cout, Ctot, _ = w.shape
    m = 36 * (cin // 16) * Cout * 16
    assert body.size == 4 * m + 16
    hi, lo = body[:2 * m].view(np.float16), body[2 * m:4 * m].view(np.float16)
    tail = R.tail_of(body, 4 * m, 4)
    want0 = np.float32(np.float32(1.5) * np.abs(R.quot32(w, sigma)).max())      # over the WHOLE tensor
    assert tail[0] == want0 and tail[2] == 0 and tail[3] == 0, (name, tail, want0)
    val, mag, cnt = R.wt_f64(w, sigma, ci0, cin)
    _check_f64(name, hi, lo, val, mag, cnt, tail[1])
    _tail_sound(name, hi, lo, tail[0], tail[1])


def check_pred(name, body, w, cout):
    hi, lo, s = R.pred_planes(w, cout)
    t = body[:4096].view(np.float16).reshape(2, 2, 32, 16)
    assert np.array_equal(t[:, 0].view(np.uint16), hi.view(np.uint16)), f"{name}: hi halves differ"
    assert np.array_equal(t[:, 1].view(np.uint16), lo.view(np.uint16)), f"{name}: lo halves differ"
    got_s = R.tail_of(body, 4096, 1)[0]
    assert got_s == s, (name, got_s, s)
    amax = np.float32(np.abs(np.asarray(w, np.float32)).max())
    _tail_sound(name, t[:, 0], t[:, 1], amax, got_s)
    _stat(name, bits=0.0)


def check_head(name, body, w):
    hi, lo, tail = R.head_planes(w)
    t = body[:8192].view(np.float16).reshape(4, 2, 32, 16)
    assert np.array_equal(t[:, 0].view(np.uint16), hi.view(np.uint16)), f"{name}: hi halves differ"
    assert np.array_equal(t[:, 1].view(np.uint16), lo.view(np.uint16)), f"{name}: lo halves differ"
    got = R.tail_of(body, 8192, 2)
    assert np.array_equal(got, tail), (name, got, tail)
    _tail_sound(name, t[:, 0], t[:, 1], got[0], got[1])
    _stat(name, bits=0.0)


# ---------------------------------------------------------------------------------------------------------------------
# 2. v2ce_sn_update_batch: one row per mode
# ---------------------------------------------------------------------------------------------------------------------
def plain_bytes(rows, cin, k3):
    return int(L().v2ce_pack_weights_f16x2_bytes(rows, cin, k3))


def up_bytes(rows, c0, c1):
    return int(L().v2ce_pack_weights_f16x2_up_bytes(rows, c0, c1))


def wt_bytes(rows, cin):
    return int(L().v2ce_pack_weights_f16x2_wt_bytes(rows, cin))


def lay(rows, cin, k3=27, up=0, wt=0, skip=False, flags=0, scale=False, inv=False, same_sign=False, g2_peak=False):
    return dict(rows=rows, cin=cin, k3=k3, up=up, wt=wt, skip=skip, flags=flags, scale=scale, inv=inv, same_sign=same_sign,
                g2_peak=g2_peak)


def key_of(flags, k3, up, wt, skip, scale):
    return (int(flags), int(k3), bool(up), int(wt), bool(skip), bool(scale))


TABLE = {
    "plain_k27": [lay(64, 32), lay(32, 48), lay(1056, 96)],
    "plain_k1": [lay(64, 32, k3=1), lay(96, 128, k3=1)],
    "mixed_k3": [lay(64, 32), lay(32, 48, k3=1), lay(96, 16), lay(64, 80, k3=1)],
    "up": [lay(64, 48, up=32, same_sign=True), lay(32, 48, up=16)],
    "up_skip": [lay(64, 48, up=32, skip=True, same_sign=True), lay(64, 96, up=64, skip=True)],
    "wt": [lay(64, 32, wt=1), lay(128, 64, wt=1, same_sign=True), lay(64, 48, wt=1, g2_peak=True)],
    "no_pack": [lay(64, 32, flags=NO_PACK), lay(32, 16, k3=1, flags=NO_PACK)],
    "no_pack_scale": [lay(64, 32, flags=NO_PACK, scale=True, inv=True), lay(32, 16, k3=1, flags=NO_PACK, scale=True, inv=True)],
    "no_pack_up_scale": [lay(64, 48, up=32, flags=NO_PACK, scale=True, inv=True),
                         lay(64, 48, up=32, skip=True, flags=NO_PACK, scale=True, inv=True)],
    "no_pack_wt_scale": [lay(64, 32, wt=1, flags=NO_PACK, scale=True, inv=True)],
    "no_iterate": [lay(64, 32, k3=1, flags=NO_ITERATE), lay(32, 48, flags=NO_ITERATE)],
    "sixteen": [lay(32, 16, k3=1), lay(64, 16), lay(32, 48, k3=1), lay(96, 32), lay(32, 272, k3=1), lay(64, 48, up=32),
                lay(32, 16), lay(64, 32, wt=1), lay(32, 400, k3=1), lay(32, 48, up=16, skip=True), lay(128, 16),
                lay(32, 80, k3=1), lay(64, 32, flags=0, same_sign=True), lay(32, 16, k3=1), lay(96, 48), lay(32, 144, k3=1)],
}
# (column counts of "sixteen": 16 .. 1296, most of them not multiples of 256, so every layer boundary of the column-block
# prefix falls behind a partial block; more than 1024 rows per layer are covered by test_power_iter_vs_f64)


def table_keys():
    return {key_of(s["flags"], s["k3"], s["up"], s["wt"], s["skip"], s["scale"]) for row in TABLE.values() for s in row}


def make_layers(specs, seed):
    rng = np.random.RandomState(seed)
    out = []
    for sp in specs:
        rows, cin, k3 = sp["rows"], sp["cin"], sp["k3"]
        w = rng.randn(rows, cin, k3) * 0.05
        if sp["same_sign"]:
            w = 0.05 * (0.9 + 0.1 * rng.random_sample(w.shape))
        if sp["g2_peak"]:                        # g0 = g2 = -g1 = max |w| at one (dh, dw): |G[2]| = 1.5 max |w|, above every |g|
            w[3, 5, [4, 13, 22]] = [0.4, -0.4, 0.4]
        u = rng.randn(rows)
        v = rng.randn(cin * k3)
        out.append(dict(sp, w=w.astype(np.float32), u=(u / np.linalg.norm(u)).astype(np.float32),
                        v=(v / np.linalg.norm(v)).astype(np.float32), bn=(0.5 + rng.random_sample(rows)).astype(np.float32)))
    return out


def pack_size(ly):
    rows, cin, k3 = ly["rows"], ly["cin"], ly["k3"]
    if ly["wt"]:
        return wt_bytes(rows, cin)
    if ly["up"]:
        return up_bytes(rows, ly["up"], cin - ly["up"])
    return plain_bytes(rows, cin, k3)


def run_batched(layers, poison, sigma_src=None):
    """One v2ce_sn_update_batch call on fresh device copies; returns per layer {u, v, packed, skip, scale, inv} (bytes)."""
    keep, res = [], []
    arr = (hip_layer() * len(layers))()
    for e, ly in zip(arr, layers):
        rows, cols = ly["rows"], ly["cin"] * ly["k3"]
        wd, ud, vd, bn = weights_dev(ly["w"]), f32dev(ly["u"]), f32dev(ly["v"]), f32dev(ly["bn"])
        pk = Guarded(pack_size(ly), poison)
        sk = Guarded(wt_bytes(rows, ly["cin"] - ly["up"]), poison) if ly["skip"] else None
        sc, iv = Guarded(4 * rows, poison), Guarded(4, poison)
        keep += [wd, ud, vd, bn]
        e.w_bar, e.u, e.v, e.packed = wd.data_ptr(), ud.data_ptr(), vd.data_ptr(), pk.ptr
        e.rows, e.cols, e.k3, e.up_c0, e.wt, e.flags = rows, cols, ly["k3"], ly["up"], ly["wt"], ly["flags"]
        e.packed_skip = sk.ptr if sk else None
        e.bn_scale = bn.data_ptr() if ly["scale"] else None
        e.scale_out = sc.ptr if ly["scale"] else None
        e.inv_sigma_out = iv.ptr if ly["inv"] else None
        if ly["flags"] & NO_ITERATE:
            e.sigma_src = sigma_src[ly["src"]]
            e.wmax = float(np.abs(ly["w"]).max())
        res.append(dict(ud=ud, vd=vd, pk=pk, sk=sk, sc=sc, iv=iv))
    nb = L().v2ce_sn_batch_workspace_bytes(arr, len(layers))
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    rc = L().v2ce_sn_update_batch(arr, len(layers), ws.data_ptr(), nb, stream())
    assert rc == OK, L().v2ce_last_error().decode()
    torch.cuda.synchronize()
    return [dict(u=r["ud"].cpu().numpy(), v=r["vd"].cpu().numpy(), packed=r["pk"].body(), skip=r["sk"].body() if r["sk"] else None,
                 scale=r["sc"].body(), inv=r["iv"].body()) for r in res]


def hip_layer():
    from v2ce_toolbox_amd import hip
    return hip.SnLayer


def run_per_layer(layers, sigma_src_host=None):
    """The per-layer calls the header promises the batch equals: power iteration, then the layer's own packer."""
    out = []
    for ly in layers:
        rows, cin, k3, cols = ly["rows"], ly["cin"], ly["k3"], ly["cin"] * ly["k3"]
        wd, ud, vd = weights_dev(ly["w"]), f32dev(ly["u"]), f32dev(ly["v"])
        sig = torch.empty(1, device="cuda")
        pk = Guarded(pack_size(ly), POISON[0])
        sk = Guarded(wt_bytes(rows, cin - ly["up"]), POISON[0]) if ly["skip"] else None
        st = stream()
        if ly["flags"] & NO_ITERATE:
            sig.fill_(float(sigma_src_host[ly["src"]]))
        else:
            ws = torch.empty(L().v2ce_sn_workspace_bytes(rows, cols), dtype=torch.uint8, device="cuda")
            assert L().v2ce_sn_power_iter(ud.data_ptr(), vd.data_ptr(), wd.data_ptr(), rows, cols, sig.data_ptr(), ws.data_ptr(),
                                          ws.numel(), st) == OK
        if not ly["flags"] & NO_PACK:
            if ly["wt"]:
                rc = L().v2ce_pack_weights_f16x2_wt(wd.data_ptr(), rows, cin, sig.data_ptr(), pk.ptr, st)
            elif ly["up"]:
                rc = L().v2ce_pack_weights_f16x2_up(wd.data_ptr(), rows, ly["up"], cin - ly["up"], sig.data_ptr(), pk.ptr, st)
            else:
                rc = L().v2ce_pack_weights_f16x2(wd.data_ptr(), rows, cin, k3, sig.data_ptr(), pk.ptr, st)
            assert rc == OK
            if sk:
                assert L().v2ce_pack_weights_f16x2_wt_slice(wd.data_ptr(), rows, cin, ly["up"], cin - ly["up"], sig.data_ptr(),
                                                            sk.ptr, st) == OK
        torch.cuda.synchronize()
        out.append(dict(u=ud.cpu().numpy(), v=vd.cpu().numpy(), sigma=np.float32(sig.item()), packed=pk.body(),
                        skip=sk.body() if sk else None))
    return out


def check_layer_f64(name, ly, sigma, packed, skip):
    """f64 / bit-exact checks of one layer's results (sigma: the per-layer call's, equal to the batch's)."""
    w = ly["w"]
    if ly["wt"]:
        check_wt(name, packed, w, 0, ly["cin"], sigma)
    elif ly["up"]:
        check_up(name, packed, w, ly["up"], sigma)
    else:
        check_plain(name, packed, w, sigma)
    if skip is not None:
        check_wt(name + "/skip", skip, w, ly["up"], ly["cin"] - ly["up"], sigma)


def check_row(name, layers, A, B, ref, sigma_src_host=None):
    for i, (ly, a, b, r) in enumerate(zip(layers, A, B, ref)):
        tag = f"{name}[{i}]"
        it = not ly["flags"] & NO_ITERATE
        pack = not ly["flags"] & NO_PACK
        for k in ("u", "v"):
            assert np.array_equal(a[k], b[k]) and np.array_equal(a[k].view(np.uint32), r[k].view(np.uint32)), (tag, k)
            if not it:
                assert np.array_equal(a[k], ly[k]), f"{tag}: a pack-only layer moved {k}"
        for k in ("packed", "skip"):
            if a[k] is None:
                continue
            wr = written(a[k], b[k])
            if pack:
                assert wr.all(), f"{tag}: {k}: {int((~wr).sum())} bytes of the destination not written"
                assert np.array_equal(a[k], r[k]), f"{tag}: {k} differs from the per-layer packer at {int(np.argmax(a[k] != r[k]))}"
            else:
                assert not wr.any(), f"{tag}: {k} written by a V2CE_SN_NO_PACK layer"
        sigma = r["sigma"]
        for k, want in (("scale", (ly["bn"] / sigma).astype(np.float32) if ly["scale"] else None),
                        ("inv", np.array([np.float32(1) / sigma], np.float32) if ly["inv"] else None)):
            wr = written(a[k], b[k])
            if want is None:
                assert not wr.any(), f"{tag}: {k} written without being asked for"
            else:
                assert wr.all() and np.array_equal(a[k].view(np.float32).view(np.uint32), want.view(np.uint32)), (tag, k)
        if it:
            ex, uv, uu, us = R.check_step(ly["w"].reshape(ly["rows"], -1), ly["u"], a["v"], a["u"], sigma)
            _stat("batch_sn", excess=ex, ulps_v=uv, ulps_u=uu, ulps_sigma=us)
            assert ex <= 0, f"{tag}: one-step excess {ex:.3e} (ulps v {uv:.2f} u {uu:.2f} sigma {us:.2f})"
        if pack:
            check_layer_f64(tag, ly, sigma, a["packed"], a["skip"])


def run_row(name, layers):
    sigma_src = sigma_host = None
    if any(ly["flags"] & NO_ITERATE for ly in layers):
        # sigma_src: inv_sigma_out of a PREVIOUS call (a NO_PACK call on layers of the same shapes, as the model does)
        pre = make_layers([lay(ly["rows"], ly["cin"], ly["k3"], flags=NO_PACK, inv=True) for ly in layers], 99)
        inv = run_batched(pre, POISON[0])
        srcs = [torch.from_numpy(r["inv"].view(np.float32).copy()).cuda() for r in inv]
        sigma_src = [s.data_ptr() for s in srcs]
        sigma_host = [np.float32(s.item()) for s in srcs]
        assert all(s > 0 for s in sigma_host)
        for i, ly in enumerate(layers):
            ly["src"] = i
    A = run_batched(layers, POISON[0], sigma_src)
    B = run_batched(layers, POISON[1], sigma_src)
    ref = run_per_layer(layers, sigma_host)
    check_row(name, layers, A, B, ref, sigma_host)
    return A


@pytest.mark.parametrize("row", list(TABLE))
def test_batch_row(row):
    layers = make_layers(TABLE[row], 17 + list(TABLE).index(row))
    PACK_STATS.clear()
    A = run_row(row, layers)
    print(f"batch {row}: {PACK_STATS}")
    # a layer's bytes do not depend on its position in the batch
    perm = np.random.RandomState(5).permutation(len(layers))
    if np.array_equal(perm, np.arange(len(layers))):
        perm = perm[::-1].copy()
    if len(layers) > 1 and not any(ly["flags"] & NO_ITERATE for ly in layers):
        P = run_batched([layers[i] for i in perm], POISON[0])
        for j, i in enumerate(perm):
            for k in ("u", "v", "packed", "skip", "scale", "inv"):
                if A[i][k] is not None:
                    assert np.array_equal(A[i][k], P[j][k]), f"{row}: layer {i} at position {j}: {k} differs"


# ---------------------------------------------------------------------------------------------------------------------
# 3. packers
# ---------------------------------------------------------------------------------------------------------------------
def edge_weights(case, shape, seed):
    rng = np.random.RandomState(seed)
    top = np.float32(2.0 ** -3)
    if case == "zeros":
        return np.zeros(shape, np.float32)
    if case in ("pow2", "below_pow2"):
        w = rng.randn(*shape)
        w = (w / np.abs(w).max() * 0.999).astype(np.float32) * top
        w.flat[rng.randint(w.size)] = top if case == "pow2" else np.nextafter(top, np.float32(0))
        return w.astype(np.float32)
    if case in ("binades13", "binades20"):
        b = 13 if case == "binades13" else 20
        return (np.sign(rng.randn(*shape)) * 2.0 ** rng.uniform(-b, 0, shape) * top).astype(np.float32)
    if case == "same_sign":
        return (top * (0.9 + 0.1 * rng.random_sample(shape))).astype(np.float32)
    return (rng.randn(*shape) * 0.05).astype(np.float32)            # "normal", "sigma_null"


CASES = ["zeros", "pow2", "below_pow2", "binades13", "binades20", "same_sign", "sigma_null"]
PACKERS = ["plain27", "plain27_cout40", "plain1_cout7", "up", "wt", "wt_slice", "pred", "pred_cout20", "head"]


def sigma_for(case):
    # a power of two keeps max |w / sigma| exactly at / below the binade edge; 1.7 makes every quotient a rounding
    return None if case == "sigma_null" else (np.float32(2.0) if case in ("pow2", "below_pow2") else np.float32(1.7))


def run_packer(packer, w, sigma, poison):
    sg = None if sigma is None else f32dev([sigma])
    wd = f32dev(w)
    sp = None if sg is None else sg.data_ptr()
    st = stream()
    if packer.startswith("plain"):
        Cout, Cin, k3 = w.shape
        g = Guarded(plain_bytes(Cout, Cin, k3), poison)
        rc = L().v2ce_pack_weights_f16x2(wd.data_ptr(), Cout, Cin, k3, sp, g.ptr, st)
    elif packer == "up":
        g = Guarded(up_bytes(w.shape[0], 32, w.shape[1] - 32), poison)
        rc = L().v2ce_pack_weights_f16x2_up(wd.data_ptr(), w.shape[0], 32, w.shape[1] - 32, sp, g.ptr, st)
    elif packer == "wt":
        g = Guarded(wt_bytes(w.shape[0], w.shape[1]), poison)
        rc = L().v2ce_pack_weights_f16x2_wt(wd.data_ptr(), w.shape[0], w.shape[1], sp, g.ptr, st)
    elif packer == "wt_slice":
        g = Guarded(wt_bytes(w.shape[0], 32), poison)
        rc = L().v2ce_pack_weights_f16x2_wt_slice(wd.data_ptr(), w.shape[0], w.shape[1], 16, 32, sp, g.ptr, st)
    elif packer.startswith("pred"):
        g = Guarded(int(L().v2ce_pack_pred_weights_f16x2_bytes()), poison)
        rc = L().v2ce_pack_pred_weights_f16x2(wd.data_ptr(), w.shape[0], 32, g.ptr, st)
    else:
        g = Guarded(int(L().v2ce_pack_head_weights_f16x2_bytes()), poison)
        rc = L().v2ce_pack_head_weights_f16x2(wd.data_ptr(), g.ptr, st)
    assert rc == OK, L().v2ce_last_error().decode()
    torch.cuda.synchronize()
    return g.body()


PACKER_SHAPES = {"plain27": (64, 32, 27), "plain27_cout40": (40, 32, 27), "plain1_cout7": (7, 48, 1), "up": (64, 48, 27),
                 "wt": (64, 32, 27), "wt_slice": (64, 48, 27), "pred": (32, 32), "pred_cout20": (20, 32), "head": (32, 2, 27)}
# documented bytes: pred writes its 2 x 2 x 32 x 16 halves and { pre-scale }; head its halves and { max |w|, pre-scale }; the
# rest of their *_bytes() is padding that stays untouched.  Every other buffer is written in full.
DOC_BYTES = {"pred": 4096 + 4, "pred_cout20": 4096 + 4, "head": 8192 + 8}


# (the pred and head packers take no sigma: every case of theirs runs without one)
PACKER_CASES = [(p, c) for p in PACKERS for c in CASES if not (p.startswith(("pred", "head")) and c == "sigma_null")]


@pytest.mark.parametrize("packer,case", PACKER_CASES, ids=[f"{p}-{c}" for p, c in PACKER_CASES])
def test_packer(packer, case):
    no_sigma = packer.startswith(("pred", "head"))
    w = edge_weights(case, PACKER_SHAPES[packer], seed=len(packer) * 31 + CASES.index(case))
    sigma = None if no_sigma else sigma_for(case)
    a, b = run_packer(packer, w, sigma, POISON[0]), run_packer(packer, w, sigma, POISON[1])
    wr = written(a, b)
    doc = DOC_BYTES.get(packer, a.size)
    assert wr[:doc].all(), f"{packer}/{case}: {int((~wr[:doc]).sum())} documented bytes not written (first {int(np.argmin(wr))})"
    assert not wr[doc:].any(), f"{packer}/{case}: padding bytes written"
    name = f"{packer}/{case}"
    if packer.startswith("plain"):
        check_plain(packer, a, w, sigma)
    elif packer == "up":
        check_up(packer, a, w, 32, sigma)
    elif packer == "wt":
        check_wt(packer, a, w, 0, w.shape[1], sigma)
    elif packer == "wt_slice":
        check_wt(packer, a, w, 16, 32, sigma)
    elif packer.startswith("pred"):
        check_pred(packer, a, w, w.shape[0])
    else:
        check_head(packer, a, w)
    if case == "same_sign" and packer == "up":
        tail = R.tail_of(a, 4 * w.size, 2)
        q = np.abs(R.quot32(w, sigma)).max()
        assert tail[0] > 3.5 * q, f"{name}: the folded sums must raise the bound to ~4 max |w / sigma| ({tail[0]} vs {q})"
    print(f"{name}: {dict((k, v) for k, v in PACK_STATS.items() if k.split('/')[0] == packer)}")


# ---------------------------------------------------------------------------------------------------------------------
# 4. rejections
# ---------------------------------------------------------------------------------------------------------------------
def _rej_layers(specs):
    """Device buffers for a rejected call: every destination sized for any layout so that nothing could go out of bounds."""
    bufs, arr = [], (hip_layer() * len(specs))()
    rng = np.random.RandomState(3)
    for e, sp in zip(arr, specs):
        rows, cin, k3 = sp["rows"], sp["cin"], sp["k3"]
        cols = cin * k3
        big = max(plain_bytes(rows, cin, k3), wt_bytes(rows, cin), up_bytes(rows, 16, max(cin - 16, 16)))
        t = dict(w=f32dev(rng.randn(rows, cols) * 0.05), u=f32dev(rng.randn(rows)), v=f32dev(rng.randn(cols)),
                 pk=torch.randint(0, 255, (big,), dtype=torch.uint8, device="cuda"),
                 sk=torch.randint(0, 255, (big,), dtype=torch.uint8, device="cuda"),
                 sc=f32dev(rng.randn(rows)), iv=f32dev([7.0]), bn=f32dev(np.ones(rows)), ss=f32dev([0.5]))
        bufs.append(t)
        e.w_bar, e.u, e.v, e.packed = t["w"].data_ptr(), t["u"].data_ptr(), t["v"].data_ptr(), t["pk"].data_ptr()
        e.rows, e.cols, e.k3, e.up_c0, e.wt, e.flags = rows, cols, k3, sp.get("up", 0), sp.get("wt", 0), sp.get("flags", 0)
        e.packed_skip = t["sk"].data_ptr() if sp.get("skip") else None
        e.bn_scale = None if sp.get("no_bn") else t["bn"].data_ptr()
        e.scale_out = t["sc"].data_ptr() if sp.get("scale") else None
        e.inv_sigma_out = t["iv"].data_ptr()
        e.sigma_src = t["ss"].data_ptr() if e.flags & NO_ITERATE else None
        e.wmax = 1.0
    return arr, bufs


OKL = dict(rows=32, cin=16, k3=27)
REJECT = {
    "n0": ([OKL], 0, BAD_ARG, 0),
    "n17": ([OKL] * 17, 17, BAD_ARG, 0),
    "flags3": ([OKL, dict(OKL, flags=3)], 2, BAD_ARG, 0),
    "rows48": ([OKL, dict(OKL, rows=48)], 2, UNSUPPORTED, 0),
    "no_iterate_up": ([dict(OKL, flags=NO_ITERATE), dict(rows=32, cin=32, k3=27, up=16, flags=NO_ITERATE)], 2, BAD_ARG, 0),
    "scale_without_bn": ([OKL, dict(OKL, scale=True, no_bn=True)], 2, BAD_ARG, 0),
    "skip_without_up": ([OKL, dict(OKL, skip=True)], 2, BAD_ARG, 0),
    "wt_k1": ([OKL, dict(rows=32, cin=16, k3=1, wt=1)], 2, BAD_ARG, 0),
    "nine_up": ([dict(rows=32, cin=32, k3=27, up=16)] * 9, 9, UNSUPPORTED, 0),
    "mixed_iterate": ([OKL, dict(OKL, flags=NO_ITERATE)], 2, UNSUPPORTED, 0),
    "workspace_short": ([OKL, OKL], 2, WORKSPACE, -1),
}


@pytest.mark.parametrize("case", list(REJECT))
def test_batch_rejections(case):
    specs, n, want, ws_delta = REJECT[case]
    arr, bufs = _rej_layers(specs)
    need = int(L().v2ce_sn_batch_workspace_bytes(arr, min(n, 16))) if n else 0
    if n > 16:
        need = 2 * int(L().v2ce_sn_batch_workspace_bytes(arr, 16))
    ws = torch.randint(0, 255, (max(need, 16) + 64,), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    before = [{k: t.clone() for k, t in b.items()} for b in bufs]
    rc = L().v2ce_sn_update_batch(arr, n, ws.data_ptr(), max(need + ws_delta, 0), stream())
    torch.cuda.synchronize()
    assert rc == want, (case, rc, L().v2ce_last_error().decode())
    assert L().v2ce_last_error().decode()
    for i, (b0, b1) in enumerate(zip(before, bufs)):
        for k in b0:
            assert torch.equal(b0[k], b1[k]), f"{case}: layer {i}: {k} changed by a refused call"


# ---------------------------------------------------------------------------------------------------------------------
# 5. the model's layers and a long run
# ---------------------------------------------------------------------------------------------------------------------
SN_PREFIXES = [f"UNet.{g}.{i}.{c}.module" for g, n in (("resblocks", 2), ("decoders", 4)) for i in range(n) for c in ("conv1", "conv2")]


def model(repack, monkeypatch):
    from v2ce_toolbox_amd.v2ce_3d import V2ce3d
    monkeypatch.setenv("V2CE_SN_REPACK", repack)
    m = V2ce3d(precision="f16x2")
    m.load_state_dict(synth.make_state_dict(0), strict=True)
    m = m.eval().to("cuda")
    m._prepare()
    monkeypatch.delenv("V2CE_SN_REPACK")
    return m


def model_entries(m):
    P = m._prep
    ents = []
    arr, n, _ = P["sn_batch"]
    ents += [arr[i] for i in range(n)]
    once = P.get("sn_once")
    if once is not None and once["tails"]:
        tarr, tn, _ = once["tail_batch"]
        ents += [tarr[i] for i in range(tn)]
    return ents


@pytest.mark.parametrize("repack", ["0", "1"])
def test_model_layers_have_a_row(repack, monkeypatch):
    m = model(repack, monkeypatch)
    keys = table_keys()
    ents = model_entries(m)
    assert len(ents) >= 12
    for e in ents:
        k = key_of(e.flags, e.k3, e.up_c0 > 0, e.wt, bool(e.packed_skip), bool(e.scale_out))
        assert k in keys, f"V2CE_SN_REPACK={repack}: the model's layer {k} (flags, k3, up, wt, skip, scale_out) has no TABLE row"


def test_model_64_calls_vs_f64_and_oracle(monkeypatch):
    m = model("0", monkeypatch)
    xn = OG.preprocess(synth.synthetic_frames(5, 32, 48, seed=11))[None]
    x = torch.from_numpy(xn).cuda()
    sd0 = synth.make_state_dict(0)
    params = dict(m.named_parameters())
    Ws = [sd0[p + ".weight_bar"].reshape(sd0[p + ".weight_bar"].shape[0], -1).numpy() for p in SN_PREFIXES]
    trajs = [R.trajectory(W, sd0[p + ".weight_u"].numpy(), 64) for W, p in zip(Ws, SN_PREFIXES)]
    inv = m._prep["sn_once"]["inv_sigma"]
    assert inv.numel() == len(SN_PREFIXES)
    worst_traj = worst_step = 0.0
    y = None
    for call in range(64):
        u_prev = [params[p + ".weight_u"].detach().cpu().numpy() for p in SN_PREFIXES]
        y = m(x)
        torch.cuda.synchronize()
        sig = 1.0 / inv.cpu().numpy().astype(np.float64)            # inv = fl32(1 / sigma): sigma within 2^-23 relative
        for k, p in enumerate(SN_PREFIXES):
            s64 = trajs[k][call][2]
            worst_traj = max(worst_traj, abs(sig[k] - s64) / s64 / R.U32)
            assert abs(sig[k] - s64) <= (SIGMA_BAR + 2 * R.U32) * s64, (call, p, sig[k], s64)
            ex, uv, uu, _ = R.check_step(Ws[k], u_prev[k], params[p + ".weight_v"].detach().cpu().numpy(),
                                         params[p + ".weight_u"].detach().cpu().numpy(), sig[k], sigma_slack=2 * R.U32)
            worst_step = max(worst_step, uv, uu)
            assert ex <= 0, (call, p, ex)
    assert m.guard_reruns == 0
    drift = max(float(np.abs(params[p + ".weight_u"].detach().cpu().numpy() - trajs[k][63][0]).max()) for k, p in enumerate(SN_PREFIXES))
    sd = U.clone_state(sd0)
    for _ in range(63):
        for p in SN_PREFIXES:
            U.sn_step(sd, p)
    want = U.forward(sd, torch.from_numpy(xn)).numpy()
    got = y.cpu().numpy()
    err = np.abs(got - want) - 1e-5 * np.abs(want)
    print(f"model 64 calls: sigma vs f64 trajectory worst {worst_traj:.2f} x 2^-24 rel, one-step worst {worst_step:.2f} ulps, u drift after 64 {drift:.2e}, "
          f"call-64 voxels max |d| {np.abs(got - want).max():.2e}")
    assert float(err.max()) <= 1e-5, float(np.abs(got - want).max())
