"""The entries of include/v2ce_hip_convngrad.h stay inside the buffers the header documents: the scheme of
tests/test_gpu_convupdgrad_containment.py (guarded, poisoned allocations of exactly the documented sizes, tests/guarded.py)
for v2ce_convn_wgrad and v2ce_convn_dgrad on tensors whose rows are padded (W = 70 at pitch 96, the padding of the inputs
holding NaN), at 64 -> 64 and at the two asymmetric channel pairs: with the kernel's own grid, with the grid capped at one
share (each workgroup walks all 16 tiles), without y, and with each output alone.  Per row: every guard intact with the
outputs and the workspace poisoned with POISON[0], with POISON[1], with a zeroed workspace and with every buffer one step
past a 256-byte boundary (16 bytes for the channels-last-16 tensors, 8 for the workspace, 4 for the weights); every byte of
the requested outputs written, the padding columns of d_x and d_res included; the same bytes in all four runs; the bytes of
dec2_conv.convn_wgrad / convn_dgrad; inputs unchanged; a workspace 4 bytes short is V2CE_ERR_WORKSPACE and nothing is
written."""
import numpy as np
import pytest
import torch

from test_gpu_containment import L, Row, bytes_of, check_row, check_short_workspace, stream
from tests import convn_ref as R
from v2ce_toolbox_amd import dec2_conv, hip

HOST_ONLY = ("_bytes",)


def case(dims, cin, cout, seed):
    B, Lq, H, W, pitch = dims
    rng = np.random.default_rng(seed)
    x = np.maximum(rng.standard_normal((B, cin, Lq, H, W)), 0).astype(np.float32)
    y = np.maximum(rng.standard_normal((B, cout, Lq, H, W)), 0).astype(np.float32)
    up = rng.standard_normal((B, cout, Lq, H, W)).astype(np.float32)
    w = (rng.standard_normal((cout, cin, 3, 3, 3)) * 0.1).astype(np.float32)
    return tuple(R.to_c16_np(a, pitch) for a in (x, y, up)) + (w,)


def device_case(dims, cin, cout, seed):
    x, y, up, w = (torch.from_numpy(a).cuda() for a in case(dims, cin, cout, seed))
    for t in (x, y, up):
        t.lw, t.c16 = dims[3], True
    return x, y, up, w


def wgrad_row(dims, cin, cout, cap, seed, with_y=True, outs=("d_weight", "d_shift")):
    entry = "v2ce_convn_wgrad"

    def call(run):
        x, y, up, _ = case(dims, cin, cout, seed)
        dw = run.out("d_weight", cout * cin * 27 * 4, 4) if "d_weight" in outs else None
        ds = run.out("d_shift", cout * 4, 4) if "d_shift" in outs else None
        nb = L().v2ce_convn_wgrad_workspace_bytes(cin, cout, *dims, cap)
        ws, nb = run.ws("workspace", nb, align=8)
        run.ok(L().v2ce_convn_wgrad(run.inp("x", x, align=16), run.inp("y", y, align=16) if with_y else None,
                                    run.inp("upstream", up, align=16), cin, cout, *dims, dw, ds, ws, nb, cap, stream()), entry)

    def want():
        x, y, up, _ = device_case(dims, cin, cout, seed)
        g = dec2_conv.convn_wgrad(x, y if with_y else None, up, want=tuple(n[2:] for n in outs), max_workgroups=cap)
        return {n: bytes_of(g[n[2:]]) for n in outs}
    tag = f"{cin}to{cout}{list(dims)}cap{cap}{'' if with_y else 'plain'}{'' if len(outs) == 2 else outs[0]}"
    return Row("convn_wgrad" + tag, [entry], call, want)


def dgrad_row(dims, cin, cout, cap, seed, with_y=True, outs=("d_x", "d_res")):
    entry = "v2ce_convn_dgrad"
    B, Lq, H, W, pitch = dims
    n_x, n_res = (B * Lq * (c // 16) * H * pitch * 64 for c in (cin, cout))

    def call(run):
        _, y, up, w = case(dims, cin, cout, seed)
        dx = run.out("d_x", n_x, 4, align=16) if "d_x" in outs else None
        dr = run.out("d_res", n_res, 4, align=16) if "d_res" in outs else None
        nb = L().v2ce_convn_dgrad_workspace_bytes(cin, cout, *dims, cap)
        ws, nb = run.ws("workspace", nb, align=8)
        run.ok(L().v2ce_convn_dgrad(run.inp("weight", w), run.inp("y", y, align=16) if with_y else None,
                                    run.inp("upstream", up, align=16), cin, cout, *dims, dx, dr, ws, nb, cap, stream()), entry)

    def want():
        _, y, up, w = device_case(dims, cin, cout, seed)
        g = dec2_conv.convn_dgrad(w, y if with_y else None, up, want=tuple(n[2:] for n in outs), max_workgroups=cap)
        return {n: bytes_of(g[n[2:]]) for n in outs}
    tag = f"{cin}to{cout}{list(dims)}cap{cap}{'' if with_y else 'plain'}{'' if len(outs) == 2 else outs[0]}"
    return Row("convn_dgrad" + tag, [entry], call, want)


# B, L, H, W, pitch: 8 tiles (two of them ragged in W, H = 3 leaves a one-row tile) on the kernel's own grid; 16 tiles on one
# share (a cap of 4 workgroups is one share of four pairs, or of two ci groups with two workgroups to spare)
SMALL, TWICE = (1, 2, 3, 70, 96), (2, 2, 3, 70, 96)
ROWS = [wgrad_row(SMALL, 64, 64, 0, 81), wgrad_row(TWICE, 64, 64, 4, 82), wgrad_row(SMALL, 64, 32, 0, 83),
        wgrad_row(SMALL, 32, 64, 3, 84, with_y=False), wgrad_row(SMALL, 64, 64, 0, 85, outs=("d_weight",)),
        wgrad_row(SMALL, 64, 64, 0, 86, outs=("d_shift",)),
        dgrad_row(SMALL, 64, 64, 0, 91), dgrad_row(TWICE, 64, 64, 2, 92), dgrad_row(SMALL, 64, 32, 0, 93),
        dgrad_row(SMALL, 32, 64, 3, 94, with_y=False), dgrad_row(SMALL, 64, 64, 0, 95, outs=("d_x",)),
        dgrad_row(SMALL, 64, 64, 0, 96, outs=("d_res",))]
SHORT = [ROWS[0], ROWS[1], ROWS[6], ROWS[7]]


def test_rows_cover_the_convngrad_abi():
    rows = {e for r in ROWS for e in r.entries}
    assert rows <= set(hip.CONVNGRAD_EXPORTS), rows - set(hip.CONVNGRAD_EXPORTS)
    uncovered = [n for n in hip.CONVNGRAD_EXPORTS if n not in rows and not any(n.endswith(h) for h in HOST_ONLY)]
    assert not uncovered, f"exports of include/v2ce_hip_convngrad.h without a containment row: {uncovered}"
    assert len({r.name for r in ROWS}) == len(ROWS)


@pytest.mark.gpu
@pytest.mark.parametrize("r", ROWS, ids=[r.name for r in ROWS])
def test_containment(r):
    check_row(r)


@pytest.mark.gpu
@pytest.mark.parametrize("r", SHORT, ids=[r.name for r in SHORT])
def test_short_workspace_is_refused(r):
    check_short_workspace(r)
