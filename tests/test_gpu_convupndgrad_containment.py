"""The entries of include/v2ce_hip_convupndgrad.h stay inside the buffers the header documents: the scheme of
tests/test_gpu_convupdgrad_containment.py (guarded, poisoned allocations of exactly the documented sizes, tests/guarded.py)
for v2ce_convupn_dgrad at 128 + 64 -> 64 on tensors whose rows are padded (W = 70 at pitch 96, W0 = 35 at pitch0 40, the
padding of the inputs holding NaN): with the kernel's own grid, with the grid capped at 3 workgroups (one share: fewer
workgroups than the six channel groups would like, each walking all 16 tiles), with only the shortcut's share requested
(g1 and weight NULL) and with each output alone.  Per row: every guard intact with the outputs and the workspace poisoned
with POISON[0], with POISON[1], with a zeroed workspace and with every buffer one step past a 256-byte boundary (16 bytes
for the channels-last-16 tensors, 8 for the workspace, 4 for the weights); every byte of the requested outputs written, the
padding columns included; the same bytes in all four runs; the bytes of dec2_block.convupn_dgrad; inputs unchanged; a
workspace 4 bytes short is V2CE_ERR_WORKSPACE and nothing is written."""
import numpy as np
import pytest
import torch

from test_gpu_containment import L, Row, bytes_of, check_row, check_short_workspace, stream
from tests import convupn_dgrad_ref as R
from v2ce_toolbox_amd import dec2_block, hip

HOST_ONLY = ("_bytes",)
C0, C1, COUT = R.DEC2


def case(dims, seed):
    B, Lq, H, W, pitch, pitch0 = dims
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((COUT, C0 + C1, 3, 3, 3)) * 0.1).astype(np.float32)
    s = (rng.standard_normal((COUT, C0 + C1)) * 0.1).astype(np.float32)
    g1, gd = (rng.standard_normal((B, COUT, Lq, H, W)).astype(np.float32) for _ in range(2))
    return w, s, R.to_c16(g1, pitch), R.to_c16(gd, pitch)


def dgrad_row(dims, cap, seed, short_only=False, outs=("d_x0", "d_x1")):
    entry = "v2ce_convupn_dgrad"
    B, Lq, H, W, pitch, pitch0 = dims
    H0, W0 = (H + 1) // 2, (W + 1) // 2
    n0, n1 = B * Lq * (C0 // 16) * H0 * pitch0 * 64, B * Lq * (C1 // 16) * H * pitch * 64

    def call(run):
        w, s, g1, gd = case(dims, seed)
        d0 = run.out("d_x0", n0, 4, align=16) if "d_x0" in outs else None
        d1 = run.out("d_x1", n1, 4, align=16) if "d_x1" in outs else None
        nb = L().v2ce_convupn_dgrad_workspace_bytes(C0, C1, COUT, *dims, cap)
        ws, nb = run.ws("workspace", nb, align=8)
        run.ok(L().v2ce_convupn_dgrad(None if short_only else run.inp("weight", w), run.inp("short_weight", s),
                                      None if short_only else run.inp("g1", g1, align=16), run.inp("gd", gd, align=16), C0, C1,
                                      COUT, *dims, d0, d1, ws, nb, cap, stream()), entry)

    def want():
        w, s, g1, gd = (torch.from_numpy(a).cuda() for a in case(dims, seed))
        for t in (g1, gd):
            t.lw, t.c16 = W, True
        # (out['x0'] carries pitch0; without it the call is told c0: 192 input channels say it anyway)
        out = {"x0": torch.full((B, Lq, C0 // 16, H0, pitch0, 16), float("nan"), device="cuda")} if "d_x0" in outs else None
        g = dec2_block.convupn_dgrad(None if short_only else w, s, None if short_only else g1, gd, want=tuple(n[2:] for n in outs),
                                     out=out, max_workgroups=cap)
        return {n: bytes_of(g[n[2:]]) for n in outs}
    return Row(f"convupn_dgrad{list(dims)}cap{cap}{'short' if short_only else ''}{'' if len(outs) == 2 else outs[0]}", [entry], call, want)


# B, L, H, W, pitch, pitch0: 8 tiles (two of them ragged in W, H = 3 leaves a one-row tile) on 48 workgroups; 16 tiles on one
# share of 6 workgroups under a cap of 3; the shortcut alone; one output alone
ROWS = [dgrad_row((1, 2, 3, 70, 96, 40), 0, 81), dgrad_row((2, 2, 3, 70, 96, 40), 3, 82),
        dgrad_row((1, 2, 3, 70, 96, 40), 6, 83, short_only=True), dgrad_row((1, 2, 3, 70, 96, 40), 0, 84, outs=("d_x0",)),
        dgrad_row((1, 2, 3, 70, 96, 40), 0, 85, outs=("d_x1",))]


def test_rows_cover_the_convupndgrad_abi():
    rows = {e for r in ROWS for e in r.entries}
    assert rows <= set(hip.CONVUPNDGRAD_EXPORTS), rows - set(hip.CONVUPNDGRAD_EXPORTS)
    uncovered = [n for n in hip.CONVUPNDGRAD_EXPORTS if n not in rows and not any(n.endswith(h) for h in HOST_ONLY)]
    assert not uncovered, f"exports of include/v2ce_hip_convupndgrad.h without a containment row: {uncovered}"
    assert len({r.name for r in ROWS}) == len(ROWS)


@pytest.mark.gpu
@pytest.mark.parametrize("r", ROWS, ids=[r.name for r in ROWS])
def test_containment(r):
    check_row(r)


@pytest.mark.gpu
@pytest.mark.parametrize("r", ROWS[:2], ids=[r.name for r in ROWS[:2]])
def test_short_workspace_is_refused(r):
    check_short_workspace(r)
