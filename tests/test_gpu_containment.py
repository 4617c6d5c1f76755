"""Every non-conv entry of include/v2ce_hip.h stays inside the buffers its header documents.

One TABLE row per C-ABI entry or call sequence, called through hip.lib() with raw pointers into guarded, poisoned allocations
(tests/guarded.py): every output exactly the byte size the header gives, every workspace exactly what its size query returned.
Each row runs on identical inputs with the outputs and workspaces poisoned with POISON[0], with POISON[1], with POISON[0] and a
zeroed workspace, and once more with every buffer whose alignment the header leaves open starting one element past a 256-byte
boundary.  Checked per row:

* containment: every guard byte in front of and behind every output, workspace and input still holds its poison;
* written extent: the bytes equal in the two poisoned runs are the bytes the call wrote -- all of an output the header
  documents as written, exactly the documented part of one written partially;
* independence from prior contents: the zero-workspace run and the misaligned run give the bytes of the first run;
* the product path's answer: the written bytes equal, bit for bit, what the Python wrapper of the entry returns (float-atomic
  v2ce_voxelize_events: at the tolerance of tests/test_gpu_voxelize.py);
* inputs hold the same bytes after the call as before.

A workspace 4 bytes short is refused with V2CE_ERR_WORKSPACE and nothing is written.  test_containment_table_covers_the_abi
(no GPU) requires every export of v2ce_toolbox_amd/hip.py to be exercised by a row, a host-only query, or listed in
COVERED_ELSEWHERE with the test that guards it (the conv entries: tests/test_gpu_conv_containment.py, the same scheme on
pitched rows)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from guarded import POISON, Guarded, written
from v2ce_toolbox_amd import hip, synth

OK, BAD_ARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -4
HOST_ONLY = ("_bytes", "_variant", "_variant_fused", "v2ce_ldati_plan_info", "v2ce_version", "v2ce_last_error",
             "v2ce_ldati_rank_mode", "v2ce_ldati_selfcheck")
_WP = "tests/test_gpu_weight_prep.py"
_CONV = "tests/test_gpu_conv_containment.py::test_conv_containment"     # (guarded, poisoned, pitched buffers: its ROWS)
COVERED_ELSEWHERE = {
    "v2ce_conv3d_fwd": _CONV, "v2ce_conv3d_fwd_pred": _CONV, "v2ce_conv3d_fwd_sc": _CONV, "v2ce_conv3d_fwd_tail": _CONV,
    "v2ce_conv3d_fwd_up2": _CONV, "v2ce_conv3d_fwd_up2_part": _CONV, "v2ce_conv3d_fwd_wt": _CONV,
    "v2ce_conv3d_fwd_wt_tail": _CONV, "v2ce_conv3d_head_f16x2": _CONV,
    "v2ce_pack_weights": _WP, "v2ce_pack_weights_f16x2": _WP, "v2ce_pack_weights_f16x2_up": _WP,
    "v2ce_pack_weights_f16x2_wt": _WP, "v2ce_pack_weights_f16x2_wt_slice": _WP, "v2ce_pack_pred_weights_f16x2": _WP,
    "v2ce_pack_head_weights_f16x2": _WP, "v2ce_pack_head_weights_f16x2_c3": _WP, "v2ce_sn_power_iter": _WP,
    "v2ce_sn_update_batch": _WP,
}


def L():
    return hip.lib()


def stream():
    return hip.stream_ptr()


class Refused(Exception):
    pass


class Run:
    """One execution of a row: hands out the guarded buffers, checks them afterwards."""

    def __init__(self, poison, ws_fill, misalign=False, short=None):
        self.poison, self.ws_fill, self.misalign, self.short = poison, ws_fill, misalign, short
        self.bufs = {}                                   # name -> (kind, Guarded, original bytes or None)
        self.n_ws, self.shortened, self.snapshot = 0, None, {}

    def _offset(self, itemsize, align):
        if not self.misalign:
            return 0
        return itemsize if align is None else (align % 256)

    def inp(self, name, arr, align=None):
        """A const device input: the bytes of `arr`; `align` = the alignment the header demands (None: the element's)."""
        arr = np.ascontiguousarray(arr)
        g = Guarded(arr.nbytes, self.poison, self._offset(arr.dtype.itemsize, align))
        g.fill(arr)
        self.bufs[name] = ("in", g, arr.view(np.uint8).ravel().copy() if arr.size else np.zeros(0, np.uint8))
        return g.ptr

    def out(self, name, nbytes, itemsize, init=None, align=None):
        """An output of exactly `nbytes`; init(poison) -> bytes the caller has to provide (zeroed slots), else all poison."""
        g = Guarded(nbytes, self.poison, self._offset(itemsize, align))
        if init is not None:
            g.fill(init(self.poison))
        self.bufs[name] = ("out", g, None)
        return g.ptr

    def ws(self, name, nbytes, align=256):
        """A workspace of exactly the queried size (4 bytes less when this run shortens it), filled with ws_fill."""
        assert nbytes > 0, f"{name}: the size query returned 0"
        if self.short is not None and self.n_ws == self.short:
            nbytes, self.shortened = nbytes - 4, name
        self.n_ws += 1
        g = Guarded(nbytes, self.ws_fill, self._offset(align, align))
        self.bufs[name] = ("ws", g, None)
        return g.ptr, nbytes

    def peek(self, name, dtype):
        torch.cuda.synchronize()
        _, g, _ = self.bufs[name]
        return g.t[g.front:g.front + g.n].cpu().numpy().view(dtype).copy()

    def peek_at(self, ptr, dtype):
        """The word at a device address inside one of the buffers (the LDATI status word of a workspace)."""
        torch.cuda.synchronize()
        for _, g, _ in self.bufs.values():
            if g.ptr <= ptr < g.ptr + g.n:
                o = g.front + ptr - g.ptr
                return g.t[o:o + np.dtype(dtype).itemsize].cpu().numpy().view(dtype)[0]
        raise AssertionError("address outside the call's buffers")

    def ok(self, rc, what):
        """A library call of the sequence returned rc."""
        if self.shortened is not None and rc == WORKSPACE:
            raise Refused(what)
        assert rc == OK, f"{what}: rc {rc}: {L().v2ce_last_error().decode()}"
        if self.short is not None:                       # remember what the calls before the refused one legitimately wrote
            self.snapshot = self.bodies()

    def bodies(self, kinds=("out", "ws")):
        torch.cuda.synchronize()
        res = {}
        for name, (kind, g, _) in self.bufs.items():
            if kind in kinds:
                intact, res[name] = g.read()
                assert intact, f"{name}: write outside the buffer ({g.n} bytes)"
        return res

    def finish(self):
        torch.cuda.synchronize()
        outs = {}
        for name, (kind, g, orig) in self.bufs.items():
            intact, body = g.read()
            assert intact, f"{name}: write outside the buffer ({g.n} bytes, {kind})"
            if kind == "in":
                assert np.array_equal(body, orig), f"{name}: a const input changed"
            elif kind == "out":
                outs[name] = body
        return outs

    def ws_sizes(self):
        return {name: g.n for name, (kind, g, _) in self.bufs.items() if kind == "ws"}


class Row:
    """name; entries: the exports the row exercises; call(run) -> {output: documented written mask or slice} for partial
    outputs; want() -> {output: bytes of the product path, or None where the wrapper does not expose it}; approx: outputs
    compared as f32 at close()."""

    def __init__(self, name, entries, call, want, approx=()):
        self.name, self.entries, self.call, self.approx = name, tuple(entries), call, tuple(approx)
        self.want = want


def close(got, want):
    """tests/test_gpu_voxelize.py::close"""
    d = np.abs(got.astype(np.float64) - want.astype(np.float64))
    assert np.all(d <= 2e-6 * (1.0 + np.abs(want) * 8)), f"max |d| = {d.max():.3e}"


def bytes_of(t):
    if torch.is_tensor(t):
        t = t.contiguous().cpu().numpy()
    return np.ascontiguousarray(t).view(np.uint8).ravel().copy()


def extent_mask(n, ext):
    m = np.zeros(n, bool)
    if ext is None:
        m[:] = True
    elif isinstance(ext, np.ndarray):
        m[:] = ext
    else:
        for lo, hi in ext:
            m[lo:hi] = True
    return m


def execute(row, poison, ws_fill, misalign=False):
    run = Run(poison, ws_fill, misalign)
    ext = row.call(run) or {}
    return run.finish(), ext, run.ws_sizes()


def check_row(row):
    want = row.want()
    A, ext, wss = execute(row, POISON[0], POISON[0])
    B, _, _ = execute(row, POISON[1], POISON[1])
    Z, _, _ = execute(row, POISON[0], 0)
    M, _, _ = execute(row, POISON[0], POISON[0], misalign=True)
    report = []
    for name, a in A.items():
        mask = written(a, B[name])
        if name in row.approx:                            # float atomics: the two runs may differ in the last bits of a cell
            mask = mask | (a != POISON[0]) | (B[name] != POISON[1])
        doc = extent_mask(a.size, ext.get(name))
        partial = "" if doc.all() else " (partial by contract)"
        report.append(f"{name} {int(mask.sum())}/{a.size}{partial}")
        bad = np.flatnonzero(mask != doc)
        assert bad.size == 0, (f"{row.name}: {name}: {int(mask.sum())} bytes written, {int(doc.sum())} documented; first "
                               f"difference at byte {bad[0]} of {a.size} ({'written' if mask[bad[0]] else 'not written'})")
        if name in row.approx:
            for r in (a, B[name], Z[name], M[name]):
                close(r.view(np.float32), want[name].view(np.float32))
            continue
        for label, r in (("second poison", B[name]), ("zeroed workspace", Z[name]), ("misaligned buffers", M[name])):
            assert np.array_equal(r[doc], a[doc]) and (label == "second poison" or np.array_equal(r, a)), \
                f"{row.name}: {name}: the run with {label} gave other bytes"
        if want.get(name) is not None:
            w = want[name]
            assert w.size == a.size, f"{row.name}: {name}: {a.size} bytes documented, the product path returns {w.size}"
            bad = np.flatnonzero((w != a) & doc)
            assert bad.size == 0, f"{row.name}: {name}: {bad.size} bytes differ from the product path, first at {bad[0]}"
    print(f"\ncontainment {row.name}: workspace bytes asked {wss if wss else 'none'}; written {'; '.join(report)}; guards intact")


def check_short_workspace(row):
    """Every workspace of the sequence in turn 4 bytes short: V2CE_ERR_WORKSPACE, and the refused call wrote nothing."""
    k, refused = 0, []
    while True:
        run = Run(POISON[0], POISON[0], short=k)
        try:
            row.call(run)
        except Refused as e:
            now = run.bodies()
            for name, body in now.items():
                before = run.snapshot.get(name)
                if before is None:
                    kind, g, _ = run.bufs[name]
                    before = np.full(body.size, g.poison, np.uint8)
                assert np.array_equal(body, before), f"{row.name}: {name} written by the refused {e}"
            run.finish()
            refused.append(f"{run.shortened} ({e})")
            k += 1
            continue
        assert run.shortened is None, f"{row.name}: a {run.shortened} 4 bytes short was accepted"
        break
    print(f"\ncontainment {row.name}: refused with V2CE_ERR_WORKSPACE, nothing written: {', '.join(refused) if refused else 'no workspace'}")


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def event_lists(H, W, seed, case="four"):
    """(ts i64, x i16, y i16, p i8, counts): the lists back to back.  "four": 3008 random events, an empty list, a list on
    one timestamp, 9024 events on a single pixel (a bucket beyond one 4096-entry sort tile); "empty": two empty lists;
    "cell33": one list of 33 events of one polarity in one cell."""
    rng = np.random.default_rng(seed)

    def lst(n, ts, x=None, y=None, p=None):
        return (np.sort(np.asarray(ts, np.int64)), (rng.integers(0, W, n) if x is None else np.full(n, x)).astype(np.int16),
                (rng.integers(0, H, n) if y is None else np.full(n, y)).astype(np.int16),
                (rng.integers(0, 2, n) if p is None else np.full(n, p)).astype(np.int8))

    if case == "four":
        # (12544 events in all, a multiple of 64: n * 4 ends on a 256-byte boundary, so the "+ 1" entries of the workspace's
        # per-event arrays are not absorbed by the layout's rounding)
        lists = [lst(3008, rng.integers(1000, 34000, 3008)), lst(0, []), lst(512, np.full(512, 7777)),
                 lst(9024, rng.integers(0, 33333, 9024), W - 1, H - 1, 1)]   # one polarity: one bucket for the voxeliser too
    elif case == "empty":
        lists = [lst(0, []), lst(0, [])]
    else:
        lists = [lst(33, 100 + 7 * np.arange(33), 2, 3, 1)]   # one polarity: one bucket of 33 for the voxeliser as well
    cols = [np.concatenate([l[i] for l in lists]) for i in range(4)]
    return cols[0], cols[1], cols[2], cols[3], np.array([l[0].size for l in lists], np.int64)


def dev_cols(ev):
    return tuple(torch.from_numpy(c.copy()).cuda() for c in ev[:4])


def offsets_of(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def event_inputs(run, ev, prefix=""):
    ts, x, y, p, counts = ev
    return (run.inp(prefix + "ts", ts), run.inp(prefix + "x", x), run.inp(prefix + "y", y), run.inp(prefix + "p", p),
            run.inp(prefix + "offsets", offsets_of(counts)))


def frames_u8(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


ROWS = []


def row(name, entries, approx=()):
    def deco(pair):
        def lazy():                                      # the row's inputs and closures are built at its first use, not at import
            call, want = pair()
            return call, functools.lru_cache(maxsize=None)(want)
        lazy = functools.lru_cache(maxsize=None)(lazy)
        ROWS.append(Row(name, entries, lambda run: lazy()[0](run), lambda: lazy()[1](), approx))
        return pair
    return deco


# ---------------------------------------------------------------------------------------------------------------------
# voxelisers and event grids
# ---------------------------------------------------------------------------------------------------------------------
def voxelize_batch_row(case, H=5, W=6, bins=5):
    @row(f"voxelize_batch[{case},{H}x{W}]", ["v2ce_voxelize_batch"])
    def _():
        def call(run):
            ev = event_lists(H, W, 11, case)
            n, P = ev[0].size, ev[4].size
            ts, x, y, p, off = event_inputs(run, ev)
            vol = run.out("volume", P * 2 * bins * H * W * 4, 4)
            st = run.out("status", P * 4, 4)
            nb = L().v2ce_voxelize_batch_workspace_bytes(P, bins, H, W, n)
            ws, nb = run.ws("workspace", nb)
            run.ok(L().v2ce_voxelize_batch(ts, x, y, p, off, n, P, bins, H, W, None, vol, st, ws, nb, stream()), "v2ce_voxelize_batch")

        def want():
            from v2ce_toolbox_amd.voxelize import gen_discretized_event_volume_batch
            ev = event_lists(H, W, 11, case)
            vol, st = gen_discretized_event_volume_batch(dev_cols(ev), ev[4], bins, H, W)
            return {"volume": bytes_of(vol), "status": bytes_of(st.astype(np.int32))}
        return call, want


for _case in ("four", "empty", "cell33"):
    voxelize_batch_row(_case)
# 8 x 8: the cell count (P * 2 * 64, P * 64) is a multiple of 64, so (ncells + 1) * 4 needs one 256-byte step more than
# ncells * 4 does: the last entry of the count and start arrays, which the scans read and write, is not inside rounding slack
voxelize_batch_row("four", H=8, W=8)
voxelize_batch_row("cell33", H=8, W=8)


def event_grids_row(case, kinds, H=5, W=6, bins=5):
    @row(f"event_grids_batch[{case},kinds={kinds},{H}x{W}]", ["v2ce_event_grids_batch"])
    def _():
        names = [k for k, bit in (("signed", 1), ("split", 2), ("stat", 4)) if kinds & bit]

        def call(run):
            ev = event_lists(H, W, 12, case)
            n, P = ev[0].size, ev[4].size
            ts, x, y, p, off = event_inputs(run, ev)
            cells = P * bins * H * W
            o = {"signed": run.out("signed", cells * 4, 4) if kinds & 1 else None,
                 "split": run.out("split", 2 * cells * 4, 4) if kinds & 2 else None}
            for k in ("stat_count", "stat_mean", "stat_std"):
                o[k] = run.out(k, 2 * cells * 8, 8) if kinds & 4 else None
            st = run.out("status", P * 4, 4)
            nb = L().v2ce_event_grids_workspace_bytes(P, bins, H, W, n, kinds)
            ws, nb = run.ws("workspace", nb)
            run.ok(L().v2ce_event_grids_batch(ts, x, y, p, off, n, P, bins, H, W, kinds, o["signed"], o["split"], o["stat_count"],
                                              o["stat_mean"], o["stat_std"], st, ws, nb, stream()), "v2ce_event_grids_batch")

        def want():
            from v2ce_toolbox_amd.event_grids import event_grids_batch
            ev = event_lists(H, W, 12, case)
            out, st = event_grids_batch(dev_cols(ev), ev[4], bins, H, W, kinds=names)
            res = {k: bytes_of(v) for k, v in out.items()}
            res["status"] = bytes_of(st.astype(np.int32))
            return res
        return call, want


for _kinds in (1, 2, 4, 7):
    event_grids_row("four", _kinds)
event_grids_row("empty", 7)
event_grids_row("cell33", 7)
event_grids_row("four", 7, H=8, W=8)
event_grids_row("cell33", 7, H=8, W=8)


@row("voxelize_events", ["v2ce_voxelize_events"], approx=("volume",))
def _voxelize_events():
    H, W, bins = 19, 27, 5

    def events():
        ev = event_lists(H, W, 13, "four")
        return tuple(c[:3008] for c in ev[:4])            # the random list: n > 0 and t_max > t_min are required

    def call(run):
        ts, x, y, p = events()
        n = ts.size
        vol = run.out("volume", 2 * bins * H * W * 4, 4)
        rng = run.out("t_range", 16, 8)
        run.ok(L().v2ce_voxelize_events(run.inp("ts", ts), run.inp("x", x), run.inp("y", y), run.inp("p", p), n, bins, H, W,
                                        vol, rng, stream()), "v2ce_voxelize_events")

    def want():
        from v2ce_toolbox_amd.voxelize import gen_discretized_event_volume
        ts, x, y, p = events()
        vol = gen_discretized_event_volume(tuple(torch.from_numpy(c.copy()).cuda() for c in (ts, x, y, p)), (2 * bins, H, W))
        return {"volume": bytes_of(vol), "t_range": bytes_of(np.array([ts.min(), ts.max()], np.int64))}
    return call, want


# ---------------------------------------------------------------------------------------------------------------------
# ts_diff
# ---------------------------------------------------------------------------------------------------------------------
def tsdiff_row(case, refuse=False, H=5, W=6):
    @row(f"tsdiff[{case}{',refused' if refuse else ''},{H}x{W}]", ["v2ce_tsdiff"])
    def _():
        def inputs():
            pred = event_lists(H, W, 14, case)
            gt = event_lists(H, W, 15, case)
            gp = gt[3].copy()
            if refuse:
                gp[5] = 2                                  # a GT polarity outside {-1, 0, 1}: V2CE_TSDIFF_BAD_GT_POLARITY
            return (gt[0] + 3, gt[1], gt[2], gp, gt[4]), pred

        def call(run):
            gt, pred = inputs()
            pairs, n_gt, n_pred = gt[4].size, gt[0].size, pred[0].size
            g = event_inputs(run, gt, "gt_")
            p = event_inputs(run, pred, "pred_")
            fps = run.inp("fps", np.full(pairs, 30.0))
            d = run.out("per_event_d", n_gt * 8, 8)
            stats = run.out("pair_stats", pairs * 3 * 8, 8)
            st = run.out("status", 4, 4)
            nb = L().v2ce_tsdiff_workspace_bytes(pairs, H, W, n_pred)
            ws, nb = run.ws("workspace", nb)
            run.ok(L().v2ce_tsdiff(g[0], g[1], g[2], g[3], g[4], n_gt, p[0], p[1], p[2], p[3], p[4], n_pred, fps, pairs, H, W, 1,
                                   d, stats, st, ws, nb, stream()), "v2ce_tsdiff")
            if refuse:                                     # a status bit: nothing was written to pair_stats / per_event_d
                return {"per_event_d": [], "pair_stats": []}

        def want():
            from v2ce_toolbox_amd.stage2_metrics import ts_diff_metric_batch
            gt, pred = inputs()
            if refuse:
                return {"status": bytes_of(np.array([8], np.int32)), "per_event_d": None, "pair_stats": None}
            r = ts_diff_metric_batch(dev_cols(gt), gt[4], dev_cols(pred), pred[4], 30.0, 1, height=H, width=W, per_event=True)
            return {"per_event_d": bytes_of(r.per_event_d), "status": bytes_of(np.zeros(1, np.int32)),
                    "pair_stats": bytes_of(np.stack([r.S, r.overflow, r.n_gt], 1).astype(np.int64))}
        return call, want


tsdiff_row("four")
tsdiff_row("four", refuse=True)
tsdiff_row("empty")
tsdiff_row("cell33")
tsdiff_row("four", H=8, W=8)                              # 2 * 64 cells per pair: see the 8 x 8 voxeliser rows


# ---------------------------------------------------------------------------------------------------------------------
# physical attention, log residual
# ---------------------------------------------------------------------------------------------------------------------
def physatt_row(mode, pool, H, W, K=0, case="four"):
    @row(f"physatt_batch[{mode},pool={pool},{H}x{W},K={K},{case}]", ["v2ce_physatt_batch"])
    def _():
        from v2ce_toolbox_amd import physical_att as PA

        def inputs():
            ev = event_lists(H, W, 16, case)
            return ev, frames_u8((ev[4].size + 1, H, W), 17)

        def call(run):
            ev, fr = inputs()
            n, P = ev[0].size, ev[4].size
            Hp, Wp = -(-H // pool), -(-W // pool)
            gw = PA.gauss_weights()
            maps = run.out("out_map", P * Hp * Wp * 4, 4)
            mask = run.out("out_mask", P * Hp * Wp, 1) if K else None
            st = run.out("status", P * 4, 4)
            nb = L().v2ce_physatt_workspace_bytes(P, H, W, pool, n)
            ws, nb = run.ws("workspace", nb)
            run.ok(L().v2ce_physatt_batch(run.inp("frames", fr), 1, P, H, W, run.inp("x", ev[1]), run.inp("y", ev[2]),
                                          run.inp("offsets", offsets_of(ev[4])), n, pool, PA.MODES[mode], 5.0,
                                          float(np.float32(0.6)), K, run.inp("lut", PA.lin_log_lut(1e-6)),
                                          gw.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), maps, mask, st, ws, nb, stream()),
                   "v2ce_physatt_batch")

        def want():
            ev, fr = inputs()
            res = PA.physical_attention_batch(fr, dev_cols(ev), ev[4], pool_size=pool, mode=mode, ceiling=5, threshold=0.6, K=K)
            out = {"out_map": bytes_of(res[0]), "status": bytes_of(res[-1].astype(np.int32))}
            if K:
                out["out_mask"] = bytes_of(res[1].to(torch.uint8))
            return out
        return call, want


for _mode in ("plain", "advanced"):
    for _pool in (4, 8):
        physatt_row(_mode, _pool, 19, 27)
physatt_row("ratio", 4, 19, 27, K=5)
physatt_row("ratio", 8, 19, 27)
physatt_row("advanced", 2, 5, 6)
physatt_row("advanced", 4, 19, 27, case="empty")
physatt_row("ratio", 2, 5, 6, K=3, case="cell33")


def log_residual_row(N, H, W):
    @row(f"log_residual_batch[N={N},{H}x{W}]", ["v2ce_log_residual_batch"])
    def _():
        from v2ce_toolbox_amd import physical_att as PA

        def call(run):
            out = run.out("out", (N - 1) * H * W * 4, 4)
            run.ok(L().v2ce_log_residual_batch(run.inp("frames", frames_u8((N, H, W), 18)), N, H, W,
                                               run.inp("lut", PA.lin_log_lut(0.0)), out, stream()), "v2ce_log_residual_batch")

        def want():
            return {"out": bytes_of(PA.gen_log_frame_residual_batch(frames_u8((N, H, W), 18)))}
        return call, want


log_residual_row(3, 19, 27)
log_residual_row(3, 12, 16)                              # H * W % 4 == 0: the kernel's vector path, when the pointers allow it


# ---------------------------------------------------------------------------------------------------------------------
# image gradient, frame ingest
# ---------------------------------------------------------------------------------------------------------------------
def image_grad_row(ksize, S=2, Lp=3, H=12, W=13):
    from v2ce_toolbox_amd import image_derivative as ID

    @row(f"image_grad_batch[k={ksize}]", ["v2ce_image_grad_batch"])
    def _grad():
        def call(run):
            taps = ID.gaussian_taps(ksize, 3)
            blur = run.out("blur", S * Lp * H * W * 4, 4)
            gmax = run.out("gmax_bits", S * 4, 4)
            run.ok(L().v2ce_image_grad_batch(run.inp("frames", frames_u8((S, Lp + 1, H, W), 19)), S, Lp, H, W, ID._fp(taps), ksize,
                                             blur, gmax, stream()), "v2ce_image_grad_batch")

        def want():
            blur, gmax = ID._grad_batch(torch.from_numpy(frames_u8((S, Lp + 1, H, W), 19)).cuda(), ID.gaussian_taps(ksize, 3))
            return {"blur": bytes_of(blur), "gmax_bits": bytes_of(gmax)}
        return call, want

    @row(f"image_units_grad[k={ksize}]", ["v2ce_image_units_grad"])
    def _units():
        def call(run):
            taps = ID.gaussian_taps(ksize, 3)
            units = run.out("units", S * Lp * 3 * H * W * 4, 4)
            gmax = run.out("gmax_bits", S * 4, 4)
            nb = L().v2ce_image_grad_workspace_bytes(S, Lp, H, W)
            ws, nb = run.ws("workspace", nb, align=4)     # "4-byte aligned"
            run.ok(L().v2ce_image_units_grad(run.inp("frames", frames_u8((S, Lp + 1, H, W), 19)), S, Lp, H, W, ID._fp(taps), ksize,
                                             float(np.float32(0.153)), float(np.float32(0.165)), units, gmax, ws, nb, stream()),
                   "v2ce_image_units_grad")

        def want():
            units, gmax = ID.image_units_batch(torch.from_numpy(frames_u8((S, Lp + 1, H, W), 19)).cuda(), kernel_size=ksize)
            return {"units": bytes_of(units), "gmax_bits": bytes_of(gmax)}
        return call, want


image_grad_row(11)
image_grad_row(5)


def preprocess_row(N, H, W, height):
    from v2ce_toolbox_amd import glue
    oh = H if height is None else height
    ow = int(W / H * oh)
    resize = (oh, ow) != (H, W)
    entry = "v2ce_preprocess_pairs_resize" if resize else "v2ce_preprocess_pairs"

    @row(f"{entry[5:]}[{N}x{H}x{W}->{oh}x{ow}]", [entry])
    def _():
        def call(run):
            fr = run.inp("frames", frames_u8((N, H, W), 20))
            units = run.out("units", (N - 1) * 2 * oh * ow * 4, 4)
            if resize:
                run.ok(L().v2ce_preprocess_pairs_resize(fr, N, H, W, oh, ow, float(glue.MEAN), float(glue.STD), units, stream()), entry)
            else:
                run.ok(L().v2ce_preprocess_pairs(fr, N, H, W, float(glue.MEAN), float(glue.STD), units, stream()), entry)

        def want():
            return {"units": bytes_of(glue.image_pre_processing_device(torch.from_numpy(frames_u8((N, H, W), 20)).cuda(), height))}
        return call, want


preprocess_row(3, 7, 9, None)
preprocess_row(3, 100, 37, 64)
preprocess_row(3, 16, 10, 8)                             # the exact 2 x 2 decimation


# ---------------------------------------------------------------------------------------------------------------------
# event records, range slots
# ---------------------------------------------------------------------------------------------------------------------
def events_pack_row(n):
    from v2ce_toolbox_amd.LDATI import DeviceEvents

    def cols():
        rng = np.random.default_rng(21 + n)
        return (rng.integers(-2 ** 62, 2 ** 62, n).astype(np.int64), rng.integers(-2 ** 15, 2 ** 15, n).astype(np.int16),
                rng.integers(-2 ** 15, 2 ** 15, n).astype(np.int16), rng.integers(-128, 128, n).astype(np.int8))

    def packed_want():
        c = tuple(torch.from_numpy(a).cuda() for a in cols())
        return bytes_of(DeviceEvents(None, np.array([[n]]), 0, soa=c).packed())

    @row(f"events_pack[n={n}]", ["v2ce_events_pack"])
    def _pack():
        def call(run):
            ts, x, y, p = cols()
            out = run.out("packed", n * 13, 13, align=4)   # "4-byte aligned, total*13 bytes"
            run.ok(L().v2ce_events_pack(run.inp("ts", ts), run.inp("x", x), run.inp("y", y), run.inp("p", p), n, out, stream()),
                   "v2ce_events_pack")

        def want():
            return {"packed": packed_want()}
        return call, want

    @row(f"events_unpack[n={n}]", ["v2ce_events_unpack"])
    def _unpack():
        def call(run):
            pk = run.inp("packed", packed_want(), align=4)
            o = [run.out(k, n * s, s) for k, s in (("ts", 8), ("x", 2), ("y", 2), ("p", 1))]
            run.ok(L().v2ce_events_unpack(pk, n, o[0], o[1], o[2], o[3], stream()), "v2ce_events_unpack")

        def want():
            ev = DeviceEvents(torch.from_numpy(packed_want()).cuda(), np.array([[n]]), 0)
            return dict(zip(("ts", "x", "y", "p"), (bytes_of(t) for t in ev._unpacked())))
        return call, want


for _n in (1, 255, 257):
    events_pack_row(_n)


def absmax_row(n, B=3, stride=2):
    @row(f"absmax_batch[B={B},n={n},stride={stride}]", ["v2ce_absmax_batch"])
    def _():
        def data():
            return (np.random.default_rng(22 + n).standard_normal((B, n)) * 3).astype(np.float32)

        def slots_init(poison):                            # "slots zeroed by the caller": the B slots, not what lies between
            s = np.full(B * stride * 4, poison, np.uint8)
            for b in range(B):
                s[b * stride * 4:b * stride * 4 + 4] = 0
            return s

        def call(run):
            slots = run.out("slots", B * stride * 4, 4, init=slots_init)
            run.ok(L().v2ce_absmax_batch(run.inp("x", data()), B, n, slots, stride, stream()), "v2ce_absmax_batch")
            return {"slots": [(b * stride * 4, b * stride * 4 + 4) for b in range(B)]}

        def want():                                        # the maximum of exact magnitudes has one value
            w = np.zeros((B, stride), np.float32)
            w[:, 0] = np.abs(data()).max(axis=1)
            return {"slots": bytes_of(w)}
        return call, want


absmax_row(1000)
absmax_row(1)


# ---------------------------------------------------------------------------------------------------------------------
# stage-1 metrics and losses
# ---------------------------------------------------------------------------------------------------------------------
def vox_pair(shape, seed):
    rng = np.random.default_rng(seed)
    g = np.maximum(rng.standard_normal(shape), 0).astype(np.float32)
    p = np.maximum(g + 0.3 * rng.standard_normal(shape), 0).astype(np.float32)
    return p, g


@row("voxmetrics[B=3,L=2,7x9,pools=(2,3,4)]", ["v2ce_voxmetrics"])
def _voxmetrics():
    B, Lq, C, H, W, pools = 3, 2, 20, 7, 9, (2, 3, 4)
    size = ctypes.sizeof(hip.VoxMetricsStats)

    def call(run):
        p, g = vox_pair((B, Lq, C, H, W), 23)
        karr = (ctypes.c_int * len(pools))(*pools)
        stats = run.out("stats", B * size, 8)
        nb = L().v2ce_voxmetrics_workspace_bytes(B, Lq, C, H, W, karr, len(pools))
        ws, nb = run.ws("workspace", nb)
        run.ok(L().v2ce_voxmetrics(run.inp("pred", p), run.inp("gt", g), B, Lq, C, H, W, 0.01, karr, len(pools), stats, size, ws, nb,
                                   stream()), "v2ce_voxmetrics")

    def want():
        from v2ce_toolbox_amd.stage1_metrics import voxel_metrics_batch
        p, g = vox_pair((B, Lq, C, H, W), 23)
        return {"stats": bytes_of(voxel_metrics_batch(torch.from_numpy(p).cuda(), torch.from_numpy(g).cuda(), pool_sizes=pools).raw)}
    return call, want


def voxlosses_row(volume, dims):
    entry = "v2ce_volume_losses" if volume else "v2ce_voxlosses"

    @row(f"{entry[5:]}{list(dims)}", [entry])
    def _():
        from v2ce_toolbox_amd import losses as LS
        terms = LS.VOLUME_TERMS if volume else LS.ALL
        size = ctypes.sizeof(hip.VoxLossesStats)

        def call(run):
            p, g = vox_pair(dims, 24)
            mask = LS.term_mask(terms)
            stats = run.out("stats", dims[0] * size, 8)
            nb = getattr(L(), entry + "_workspace_bytes")(*dims, mask)
            ws, nb = run.ws("workspace", nb)
            run.ok(getattr(L(), entry)(run.inp("pred", p), run.inp("gt", g), *dims, mask, stats, size, ws, nb, stream()), entry)

        def want():
            p, g = vox_pair(dims, 24)
            fn = LS.volume_losses_batch if volume else LS.voxel_losses_batch
            return {"stats": bytes_of(fn(torch.from_numpy(p).cuda(), torch.from_numpy(g).cuda(), terms=terms).raw)}
        return call, want


voxlosses_row(False, (2, 3, 20, 9, 15))
voxlosses_row(True, (2, 8, 8, 8))                        # the pyramid's minimum: min(D, H, W) = 8


# ---------------------------------------------------------------------------------------------------------------------
# event frames: sums -> refine (levels 1, 2) -> render
# ---------------------------------------------------------------------------------------------------------------------
def event_frames_row(mode, P=3, H=11, W=13):
    @row(f"event_frames[{'polarity' if mode == 0 else 'grey'},{H}x{W}]",
         ["v2ce_event_frames_sums", "v2ce_event_frames_refine", "v2ce_event_frames_render"])
    def _():
        vox = synth.synthetic_voxels(P, H, W, seed=25, regime="sparse")
        zero = lambda poison, n: np.zeros(n, np.uint8)       # "the caller zeroes it once per clip (and per level)"

        def call(run):
            w = want()
            pa, pb, qa, qb, upper = w["_plan"]
            hb0, hb1 = L().v2ce_event_frames_hist_bytes(0), L().v2ce_event_frames_hist_bytes(1)
            assert hb0 == 8 * hip.EVENT_FRAMES_LEVEL0_BINS and hb1 == 8 * 2 * hip.EVENT_FRAMES_REFINE_BINS
            assert L().v2ce_event_frames_hist_bytes(2) == hb1
            sums = run.out("sums", P * 3 * H * W * 4, 4)
            h0 = run.out("hist0", hb0, 8, init=lambda poison: zero(poison, hb0))
            run.ok(L().v2ce_event_frames_sums(run.inp("vox", vox), P, H, W, mode, sums, h0, stream()), "v2ce_event_frames_sums")
            h1 = run.out("hist1", hb1, 8, init=lambda poison: zero(poison, hb1))
            run.ok(L().v2ce_event_frames_refine(sums, P, H, W, mode, 1, pa, pb, h1, stream()), "v2ce_event_frames_refine")
            h2 = run.out("hist2", hb1, 8, init=lambda poison: zero(poison, hb1))
            run.ok(L().v2ce_event_frames_refine(sums, P, H, W, mode, 2, qa, qb, h2, stream()), "v2ce_event_frames_refine")
            frames = run.out("frames", (P + 2) * H * W * 3, 1, align=4)      # pairs [1, 1 + P) of a clip of P + 2
            run.ok(L().v2ce_event_frames_render(sums, P, H, W, mode, upper, 1, P + 2, frames, stream()), "v2ce_event_frames_render")
            return {"frames": [(H * W * 3, (1 + P) * H * W * 3)]}

        def want():
            from v2ce_toolbox_amd.event_frames import EventFrameRenderer
            r = EventFrameRenderer(keep_polarity=mode == 0, height=H, width=W)
            sums = r.add(0, torch.from_numpy(vox).cuda())
            h0 = r.level0_histogram()
            ne = np.flatnonzero(h0)
            pa, pb = int(ne[0]), int(ne[-1])
            h1 = r.refine_histogram(1, pa, pb)
            qa, qb = (pa << 10) | int(np.flatnonzero(h1[0])[0]), (pb << 10) | int(np.flatnonzero(h1[1])[-1])
            h2 = r.refine_histogram(2, qa, qb)
            res = {"sums": bytes_of(sums), "hist0": bytes_of(h0), "hist1": bytes_of(h1), "hist2": bytes_of(h2)}
            frames, upper = r.finish()
            pad = np.zeros(H * W * 3, np.uint8)
            res["frames"] = np.concatenate([pad, bytes_of(frames), pad])
            res["_plan"] = (pa, pb, qa, qb, float(upper))
            return res
        want = functools.lru_cache(maxsize=None)(want)     # call() consults it: once per row
        return call, want


event_frames_row(hip.EVENT_FRAMES_POLARITY)
event_frames_row(hip.EVENT_FRAMES_GREY)
event_frames_row(hip.EVENT_FRAMES_POLARITY, H=12, W=16)  # H * W % 4 == 0: the vector paths
event_frames_row(hip.EVENT_FRAMES_GREY, H=12, W=16)


# ---------------------------------------------------------------------------------------------------------------------
# ablation samplers: (pool ->) count -> emit
# ---------------------------------------------------------------------------------------------------------------------
def sampler_row(mode, pooling="none", zero=False, B=2, H=13, W=37):
    entries = ["v2ce_sampler_count", "v2ce_sampler_emit"] + (["v2ce_sampler_pool"] if pooling != "none" else [])
    label = {hip.SAMPLER_RANDOM: "random", hip.SAMPLER_EVEN: "even", hip.SAMPLER_PURE_SLOPE: "slope"}[mode]

    @row(f"sampler[{label},pool={pooling}{',zero' if zero else ''}]", entries)
    def _():
        vox = synth.synthetic_voxels(B, H, W, seed=26, regime="sparse")
        if zero:
            vox = np.zeros_like(vox)

        def call(run):
            w = want()
            v = run.inp("vox", vox)
            o = hip.SamplerOptions(mode=mode, rng_mode=hip.RNG_PHILOX, fps=30.0, t0=0.0, seed=77, frame_base=3, replay_M=0,
                                   u_int=None, u_dec=None, u_bern=None, pooled=None)
            if pooling != "none":
                o.pooled = run.out("pooled", vox.nbytes, 4)
                run.ok(L().v2ce_sampler_pool(v, B, H, W, hip.POOL_WEIGHTED, 3, o.pooled, stream()), "v2ce_sampler_pool")
            counts = run.out("frame_counts", B * 8, 8)
            max_int = run.out("max_int", 4, 4)
            run.ok(L().v2ce_sampler_count(v, B, H, W, ctypes.byref(o), counts, max_int, stream()), "v2ce_sampler_count")
            total = int(run.peek("frame_counts", np.int64).sum())
            assert total == w["ts"].size // 8
            out = [run.out(k, total * s, s) for k, s in (("ts", 8), ("x", 2), ("y", 2), ("p", 1))]
            st = run.out("status", 4, 4)
            nb = L().v2ce_sampler_workspace_bytes(total)
            ws, nb = run.ws("workspace", nb)
            run.ok(L().v2ce_sampler_emit(v, B, H, W, ctypes.byref(o), total, out[0], out[1], out[2], out[3], ws, nb, st, stream()),
                   "v2ce_sampler_emit")

        def want():
            from v2ce_toolbox_amd.sample_methods import sampler_device
            ev = sampler_device(torch.from_numpy(vox).cuda(), mode, 0, 30, seed=77, frame_base=3, pooling_type=pooling)
            res = dict(zip(("ts", "x", "y", "p"), (bytes_of(t) for t in ev._soa)))
            res.update(frame_counts=bytes_of(ev.seg_counts.astype(np.int64)), max_int=bytes_of(np.array([ev.max_n], np.int32)),
                       status=bytes_of(ev._status), pooled=None)
            return res
        want = functools.lru_cache(maxsize=None)(want)     # call() consults it: once per row
        return call, want


for _mode in (hip.SAMPLER_RANDOM, hip.SAMPLER_EVEN, hip.SAMPLER_PURE_SLOPE):
    sampler_row(_mode)
sampler_row(hip.SAMPLER_PURE_SLOPE, pooling="weighted")
sampler_row(hip.SAMPLER_RANDOM, zero=True)


# ---------------------------------------------------------------------------------------------------------------------
# LDATI: count -> workspace_bytes -> emit, fused_ws_bytes -> count_fused -> workspace_bytes -> emit_fused, the sweep
# ---------------------------------------------------------------------------------------------------------------------
LDATI_OPTIONS = {"default": dict(strategy="slope"), "none": dict(strategy="none"), "bidirectional": dict(bidirectional=True),
                 "weighted": dict(pooling_type="weighted")}


def ldati_row(regime, fps, opt, layout, seq, B=3, H=37, W=53):
    fused = seq == "fused"
    entries = {"two_pass": ["v2ce_ldati_count", "v2ce_ldati_emit"], "sweep": ["v2ce_ldati_count", "v2ce_ldati_emit"],
               "fused": ["v2ce_ldati_count_fused", "v2ce_ldati_emit_fused"]}[seq] + ["v2ce_ldati_status"]

    @row(f"ldati[{regime},fps={fps},{opt},{layout},{seq},B={B},{H}x{W}]", entries)
    def _():
        kw = LDATI_OPTIONS[opt]
        vox = np.zeros((B, 2, 10, H, W), np.float32) if regime == "zero" else synth.synthetic_voxels(B, H, W, seed=27, regime=regime)
        o = hip.LdatiOptions({"slope": hip.STRATEGY_SLOPE, "none": hip.STRATEGY_NONE}[kw.get("strategy", "slope")],
                             int(kw.get("bidirectional", False)),
                             {"none": hip.POOL_NONE, "weighted": hip.POOL_WEIGHTED}[kw.get("pooling_type", "none")], 3)
        seed, base, f = 4242, 5, float(fps)

        def call(run):
            w = want()
            lib, op = L(), ctypes.byref(o)
            v = run.inp("vox", vox)
            tws, tn = run.ws("tile_ws", lib.v2ce_ldati_tile_ws_bytes(B, H, W))
            seg = run.out("seg_offsets", (B * 9 + 1) * 8, 8)
            fws, fn, tile_all = None, 0, 0
            if fused:
                fws, fn = run.ws("fused_ws", lib.v2ce_ldati_fused_ws_bytes(B, H, W, f, 0.0, op, 0, 0))
                stats = run.out("stats", 8 * 8, 8)
                run.ok(lib.v2ce_ldati_count_fused(v, B, H, W, f, 0.0, op, hip.RNG_PHILOX, None, 0, seed, base, 0, 0, tws, tn, fws, fn,
                                                  seg, stats, stream()), "v2ce_ldati_count_fused")
            else:
                stats = run.out("stats", 4 * 8, 8)
                run.ok(lib.v2ce_ldati_count(v, B, H, W, op, tws, tn, seg, stats, stream()), "v2ce_ldati_count")
            s = run.peek("stats", np.int64)
            max_n, max_tile, max_seg, total = (int(x) for x in s[:4])
            if fused:
                tile_all = int(s[4])
            assert (max_n, total) == w["_stats"], ((max_n, total), w["_stats"])
            ptrs = [None] * 5
            if layout == "packed":
                ptrs[4] = run.out("packed", total * 13, 13, align=4)
            else:
                ptrs[:4] = [run.out(k, total * n, n) for k, n in (("ts", 8), ("x", 2), ("y", 2), ("p", 1))]
            if total == 0:                                # the product path makes no emit call either
                return
            ws, nb = None, 0
            if seq != "sweep":
                ws, nb = run.ws("workspace", lib.v2ce_ldati_workspace_bytes(B, H, W, f, 0.0, op, total, max_seg, max_tile,
                                                                            int(layout == "packed")))
            args = (v, B, H, W, f, 0.0, op, hip.RNG_PHILOX, None, 0, seed, base, seg, None, *ptrs, total, max_seg, max_tile, tws, ws, nb)
            if fused:
                run.ok(lib.v2ce_ldati_emit_fused(*args, fws, fn, tile_all, 0, 0, stream()), "v2ce_ldati_emit_fused")
            else:
                run.ok(lib.v2ce_ldati_emit(*args, stream()), "v2ce_ldati_emit")
            if ws is not None:
                sp = ctypes.c_void_p()
                assert lib.v2ce_ldati_status(ws, B, H, W, f, 0.0, op, total, max_seg, max_tile, ctypes.byref(sp)) == OK
                assert run.peek_at(sp.value, np.int32) == 0, "LDATI status word"

        def want():
            from v2ce_toolbox_amd.LDATI import ldati_device
            ev = ldati_device(torch.from_numpy(vox).cuda(), 0, fps, seed=seed, frame_base=base, layout=layout,
                              path="sweep" if seq == "sweep" else "bucket", **kw)
            ev.check()
            res = {"seg_offsets": bytes_of(offsets_of(ev.seg_counts.ravel())), "stats": None,
                   "_stats": (int(ev.max_n), int(ev.num_events))}
            if layout == "packed":
                res["packed"] = bytes_of(ev.packed())
            else:
                res.update(zip(("ts", "x", "y", "p"), (bytes_of(t) for t in ev._soa)))
            return res
        want = functools.lru_cache(maxsize=None)(want)     # call() consults it: once per row
        return call, want


for _regime in ("stress", "sparse"):
    for _fps in (30, 5):
        ldati_row(_regime, _fps, "default", "packed", "two_pass")
        ldati_row(_regime, _fps, "default", "soa", "fused")
        ldati_row(_regime, _fps, "bidirectional", "packed", "fused")
        ldati_row(_regime, _fps, "weighted", "soa", "two_pass")
    ldati_row(_regime, 30, "none", "soa", "two_pass")
    ldati_row(_regime, 30, "none", "packed", "fused")
    ldati_row(_regime, 30, "bidirectional", "soa", "two_pass")
    ldati_row(_regime, 30, "weighted", "packed", "two_pass")
    ldati_row(_regime, 30, "default", "packed", "sweep")
    ldati_row(_regime, 30, "default", "soa", "sweep")
# H * W % 4 == 0: the count and emit kernels read the voxel planes as float4 there (the product's 260 x 346 does); in the
# element-offset run vox then starts 4 bytes past a 16-byte boundary
for _seq, _layout in (("two_pass", "packed"), ("fused", "soa"), ("sweep", "packed")):
    ldati_row("sparse", 30, "default", _layout, _seq, B=2, H=36, W=52)
ldati_row("stress", 5, "bidirectional", "soa", "two_pass", B=2, H=36, W=52)
ldati_row("zero", 30, "default", "packed", "two_pass", B=1)
ldati_row("zero", 30, "default", "soa", "fused", B=1)


# ---------------------------------------------------------------------------------------------------------------------
# the tests
# ---------------------------------------------------------------------------------------------------------------------
def test_containment_table_covers_the_abi():
    rows = {e for r in ROWS for e in r.entries}
    assert rows <= set(hip.EXPORTS), rows - set(hip.EXPORTS)
    uncovered = [n for n in hip.EXPORTS
                 if n not in rows and n not in COVERED_ELSEWHERE and not any(n.endswith(h) or n == h for h in HOST_ONLY)]
    assert not uncovered, (f"exports without a containment row, a host-only exemption or a COVERED_ELSEWHERE entry: {uncovered}")
    assert not set(COVERED_ELSEWHERE) & rows
    assert len({r.name for r in ROWS}) == len(ROWS)


@pytest.mark.gpu
@pytest.mark.parametrize("r", ROWS, ids=[r.name for r in ROWS])
def test_containment(r):
    check_row(r)


def untouched(run):
    """Every output and workspace of a refused call still holds its poison, guards included."""
    for name, body in run.bodies().items():
        assert np.all(body == run.bufs[name][1].poison), f"{name} written by a refused call"
    run.finish()


@pytest.mark.gpu
def test_stated_alignments_are_enforced():
    """The alignments the header states beyond an element's own -- fused_ws 16 bytes; the workspaces of v2ce_physatt_batch and
    v2ce_image_units_grad, the packed record buffers of v2ce_events_pack / _unpack and v2ce_ldati_emit / _emit_fused and the
    clip buffer of v2ce_event_frames_render 4 bytes -- are refused with V2CE_ERR_BAD_ARG and the alignment's own message,
    before any launch."""
    lib, B, H, W = L(), 1, 37, 53

    def aligned_msg():
        return b"aligned" in lib.v2ce_last_error()
    o = hip.LdatiOptions(hip.STRATEGY_SLOPE, 0, hip.POOL_NONE, 3)
    run = Run(POISON[0], POISON[0])
    v = run.inp("vox", synth.synthetic_voxels(B, H, W, seed=28, regime="sparse"))
    tws, tn = run.ws("tile_ws", lib.v2ce_ldati_tile_ws_bytes(B, H, W))
    fn = lib.v2ce_ldati_fused_ws_bytes(B, H, W, 30.0, 0.0, ctypes.byref(o), 0, 0)
    fws, _ = run.ws("fused_ws", fn + 8)
    seg, stats = run.out("seg_offsets", (B * 9 + 1) * 8, 8), run.out("stats", 64, 8)
    assert lib.v2ce_ldati_count_fused(v, B, H, W, 30.0, 0.0, ctypes.byref(o), hip.RNG_PHILOX, None, 0, 1, 0, 0, 0, tws, tn, fws + 8, fn,
                                      seg, stats, stream()) == BAD_ARG
    assert b"16-byte" in lib.v2ce_last_error()
    untouched(run)
    # the packed output of both emits (refused before the segment table or the workspace is looked at)
    packed = run.out("packed", 13 * 8 + 2, 1)
    ws, nb = run.ws("workspace", 4096)
    args = (v, B, H, W, 30.0, 0.0, ctypes.byref(o), hip.RNG_PHILOX, None, 0, 1, 0, seg, None, None, None, None, None, packed + 2, 8, 8, 8,
            tws, ws, nb)
    assert lib.v2ce_ldati_emit(*args, stream()) == BAD_ARG and aligned_msg(), lib.v2ce_last_error()
    assert lib.v2ce_ldati_emit_fused(*args, fws, fn, 8, 0, 0, stream()) == BAD_ARG and aligned_msg(), lib.v2ce_last_error()
    untouched(run)

    from v2ce_toolbox_amd import physical_att as PA
    run = Run(POISON[0], POISON[0])
    P, H, W = 2, 19, 27
    gw = PA.gauss_weights()
    nb = lib.v2ce_physatt_workspace_bytes(P, H, W, 4, 0)
    ws, _ = run.ws("workspace", nb + 2)
    maps, st = run.out("out_map", P * 5 * 7 * 4, 4), run.out("status", P * 4, 4)
    assert lib.v2ce_physatt_batch(run.inp("frames", frames_u8((P + 1, H, W), 29)), 1, P, H, W, None, None,
                                  run.inp("offsets", np.zeros(P + 1, np.int64)), 0, 4, hip.PHYSATT_PLAIN, 5.0, 0.6, 0,
                                  run.inp("lut", PA.lin_log_lut(1e-6)), gw.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), maps, None,
                                  st, ws + 2, nb, stream()) == BAD_ARG
    assert aligned_msg(), lib.v2ce_last_error()
    untouched(run)

    from v2ce_toolbox_amd import image_derivative as ID
    run = Run(POISON[0], POISON[0])
    S, Lp, H, W = 1, 2, 12, 13
    taps = ID.gaussian_taps(5, 3)
    nb = lib.v2ce_image_grad_workspace_bytes(S, Lp, H, W)
    ws, _ = run.ws("workspace", nb + 2)
    units, gmax = run.out("units", S * Lp * 3 * H * W * 4, 4), run.out("gmax_bits", S * 4, 4)
    assert lib.v2ce_image_units_grad(run.inp("frames", frames_u8((S, Lp + 1, H, W), 30)), S, Lp, H, W, ID._fp(taps), 5, 0.153, 0.165,
                                     units, gmax, ws + 2, nb, stream()) == BAD_ARG
    assert aligned_msg(), lib.v2ce_last_error()
    untouched(run)

    run = Run(POISON[0], POISON[0])
    n = 5
    out = run.out("packed", n * 13 + 2, 1)
    cols = [run.inp(k, np.arange(n).astype(dt)) for k, dt in (("ts", np.int64), ("x", np.int16), ("y", np.int16), ("p", np.int8))]
    assert lib.v2ce_events_pack(*cols, n, out + 2, stream()) == BAD_ARG and aligned_msg(), lib.v2ce_last_error()
    o4 = [run.out(k, n * s, s) for k, s in (("ts_o", 8), ("x_o", 2), ("y_o", 2), ("p_o", 1))]
    assert lib.v2ce_events_unpack(out + 2, n, *o4, stream()) == BAD_ARG and aligned_msg(), lib.v2ce_last_error()
    untouched(run)

    run = Run(POISON[0], POISON[0])
    P, H, W = 1, 5, 7
    frames = run.out("frames", P * H * W * 3 + 2, 1)
    sums = run.inp("sums", np.ones((P, 3, H, W), np.float32))
    assert lib.v2ce_event_frames_render(sums, P, H, W, hip.EVENT_FRAMES_GREY, 1.0, 0, P, frames + 2, stream()) == BAD_ARG
    assert aligned_msg(), lib.v2ce_last_error()
    untouched(run)


SHORT_ROWS = list({r.entries: r for r in reversed(ROWS)}.values())[::-1]        # the first row of every call sequence


@pytest.mark.gpu
@pytest.mark.parametrize("r", SHORT_ROWS, ids=[r.name for r in SHORT_ROWS])
def test_short_workspace_is_refused(r):
    check_short_workspace(r)
