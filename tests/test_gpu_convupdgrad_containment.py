"""The entries of include/v2ce_hip_convupdgrad.h stay inside the buffers the header documents: the scheme of
tests/test_gpu_convupgrad_containment.py (guarded, poisoned allocations of exactly the documented sizes, tests/guarded.py)
for v2ce_convup_dgrad on tensors whose rows are padded (W = 70 at pitch 96, W0 = 35 at pitch0 40, the padding of the inputs
holding NaN): with the kernel's own grid, with the grid capped at 3 workgroups (one share: each workgroup walks all 16
tiles), with only the shortcut's share requested (g1 and weight NULL) and with each output alone.  Per row: every guard
intact with the outputs and the workspace poisoned with POISON[0], with POISON[1], with a zeroed workspace and with every
buffer one step past a 256-byte boundary (16 bytes for the channels-last-16 tensors, 8 for the workspace, 4 for the weights);
every byte of the requested outputs written, the padding columns included; the same bytes in all four runs; the bytes of
last_block.convup_dgrad; inputs unchanged; a workspace 4 bytes short is V2CE_ERR_WORKSPACE and nothing is written."""
import numpy as np
import pytest
import torch

from test_gpu_containment import L, Row, bytes_of, check_row, check_short_workspace, stream
from tests import last_block_dgrad_ref as D
from v2ce_toolbox_amd import hip, last_block

HOST_ONLY = ("_bytes",)


def case(dims, seed):
    B, Lq, H, W, pitch, pitch0 = dims
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((32, 96, 3, 3, 3)) * 0.1).astype(np.float32)
    s = (rng.standard_normal((32, 96)) * 0.1).astype(np.float32)
    g1, gd = (rng.standard_normal((B, 32, Lq, H, W)).astype(np.float32) for _ in range(2))
    return w, s, D.to_c16(g1, pitch), D.to_c16(gd, pitch)


def dgrad_row(dims, cap, seed, short_only=False, outs=("d_x0", "d_x1")):
    entry = "v2ce_convup_dgrad"
    B, Lq, H, W, pitch, pitch0 = dims
    H0, W0 = (H + 1) // 2, (W + 1) // 2
    n0, n1 = B * Lq * 4 * H0 * pitch0 * 64, B * Lq * 2 * H * pitch * 64

    def call(run):
        w, s, g1, gd = case(dims, seed)
        d0 = run.out("d_x0", n0, 4, align=16) if "d_x0" in outs else None
        d1 = run.out("d_x1", n1, 4, align=16) if "d_x1" in outs else None
        nb = L().v2ce_convup_dgrad_workspace_bytes(*dims, cap)
        ws, nb = run.ws("workspace", nb, align=8)
        run.ok(L().v2ce_convup_dgrad(None if short_only else run.inp("weight", w), run.inp("short_weight", s),
                                     None if short_only else run.inp("g1", g1, align=16), run.inp("gd", gd, align=16), *dims,
                                     d0, d1, ws, nb, cap, stream()), entry)

    def want():
        w, s, g1, gd = (torch.from_numpy(a).cuda() for a in case(dims, seed))
        for t in (g1, gd):
            t.lw, t.c16 = W, True
        out = {"x0": torch.full((B, Lq, 4, H0, pitch0, 16), float("nan"), device="cuda")} if "d_x0" in outs else None
        g = last_block.convup_dgrad(None if short_only else w, s, None if short_only else g1, gd, want=tuple(n[2:] for n in outs),
                                    out=out, max_workgroups=cap)
        return {n: bytes_of(g[n[2:]]) for n in outs}
    return Row(f"convup_dgrad{list(dims)}cap{cap}{'short' if short_only else ''}{'' if len(outs) == 2 else outs[0]}", [entry], call, want)


# B, L, H, W, pitch, pitch0: 8 tiles (two of them ragged in W, H = 3 leaves a one-row tile) on 24 workgroups; 16 tiles on one
# share of 3 workgroups; the shortcut alone; one output alone
ROWS = [dgrad_row((1, 2, 3, 70, 96, 40), 0, 71), dgrad_row((2, 2, 3, 70, 96, 40), 3, 72),
        dgrad_row((1, 2, 3, 70, 96, 40), 6, 73, short_only=True), dgrad_row((1, 2, 3, 70, 96, 40), 0, 74, outs=("d_x0",)),
        dgrad_row((1, 2, 3, 70, 96, 40), 0, 75, outs=("d_x1",))]


def test_rows_cover_the_convupdgrad_abi():
    rows = {e for r in ROWS for e in r.entries}
    assert rows <= set(hip.CONVUPDGRAD_EXPORTS), rows - set(hip.CONVUPDGRAD_EXPORTS)
    uncovered = [n for n in hip.CONVUPDGRAD_EXPORTS if n not in rows and not any(n.endswith(h) for h in HOST_ONLY)]
    assert not uncovered, f"exports of include/v2ce_hip_convupdgrad.h without a containment row: {uncovered}"
    assert len({r.name for r in ROWS}) == len(ROWS)


@pytest.mark.gpu
@pytest.mark.parametrize("r", ROWS, ids=[r.name for r in ROWS])
def test_containment(r):
    check_row(r)


@pytest.mark.gpu
@pytest.mark.parametrize("r", ROWS[:2], ids=[r.name for r in ROWS[:2]])
def test_short_workspace_is_refused(r):
    check_short_workspace(r)
