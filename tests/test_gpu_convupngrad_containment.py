"""The entries of include/v2ce_hip_convupngrad.h stay inside the buffers the header documents: the scheme of
tests/test_gpu_convupgrad_containment.py (guarded, poisoned allocations of exactly the documented sizes, tests/guarded.py)
for v2ce_convupn_wgrad at dec2's channel counts (128, 64, 64) on tensors whose rows are padded ([1, 2, 4, 70]: W = 70 at pitch
96, W0 = 35 at pitch0 40, the padding holding NaN): with the kernel's own grid (8 tiles on 96 workgroups), with the grid
capped at the 12 workgroups of one share (each workgroup walks all 8 tiles; the workspace is that of 12), and with only
d_short and d_short_bias requested (g1 NULL).  Per row: every guard intact with the outputs and the workspace poisoned with
POISON[0], with POISON[1], with a zeroed workspace and with every buffer one step past a 256-byte boundary (16 bytes for the
channels-last-16 tensors, 8 for the workspace, 4 for the outputs); every byte of the requested outputs written; the same
bytes in all four runs; the bytes of dec2_block.convupn_wgrad; inputs unchanged; a workspace 4 bytes short is
V2CE_ERR_WORKSPACE and nothing is written."""
import numpy as np
import pytest
import torch

from test_gpu_containment import L, Row, bytes_of, check_row, check_short_workspace, stream
from tests import convn_ref as N
from v2ce_toolbox_amd import dec2_block, hip

HOST_ONLY = ("_bytes",)
TRIPLE = (128, 64, 64)
PAIRS = 12


def case(dims, seed):
    B, Lq, H, W, pitch, pitch0 = dims
    c0, c1, cout = TRIPLE
    rng = np.random.default_rng(seed)
    x0 = rng.standard_normal((B, c0, Lq, (H + 1) // 2, (W + 1) // 2)).astype(np.float32)
    x1 = rng.standard_normal((B, c1, Lq, H, W)).astype(np.float32)
    g1, gd = (rng.standard_normal((B, cout, Lq, H, W)).astype(np.float32) for _ in range(2))
    return (N.to_c16_np(x0, pitch0),) + tuple(N.to_c16_np(a, pitch) for a in (x1, g1, gd))


def wgrad_row(dims, cap, seed, short_only=False):
    entry = "v2ce_convupn_wgrad"
    c0, c1, cout = TRIPLE

    def call(run):
        x0, x1, g1, gd = case(dims, seed)
        dw = None if short_only else run.out("d_weight", cout * (c0 + c1) * 27 * 4, 4)
        ds, db = run.out("d_short", cout * (c0 + c1) * 4, 4), run.out("d_short_bias", cout * 4, 4)
        nb = L().v2ce_convupn_wgrad_workspace_bytes(*TRIPLE, *dims, cap)
        ws, nb = run.ws("workspace", nb, align=8)
        run.ok(L().v2ce_convupn_wgrad(run.inp("x0", x0, align=16), run.inp("x1", x1, align=16),
                                      None if short_only else run.inp("g1", g1, align=16), run.inp("gd", gd, align=16), *TRIPLE,
                                      *dims, dw, ds, db, ws, nb, cap, stream()), entry)

    def want():
        x0, x1, g1, gd = (torch.from_numpy(a).cuda() for a in case(dims, seed))
        x0.lw = (dims[3] + 1) // 2
        for t in (x1, g1, gd):
            t.lw, t.c16 = dims[3], True
        names = ("short", "short_bias") if short_only else ("weight", "short", "short_bias")
        g = dec2_block.convupn_wgrad(x0, x1, None if short_only else g1, gd, want=names, max_workgroups=cap)
        return {"d_" + n: bytes_of(g[n]) for n in names}
    return Row(f"convupn_wgrad{list(dims)}cap{cap}{'short' if short_only else ''}", [entry], call, want)


# B, L, H, W, pitch, pitch0: 8 tiles (half of them ragged in W) on 96 workgroups; on one share of 12 workgroups
ROWS = [wgrad_row((1, 2, 4, 70, 96, 40), 0, 81), wgrad_row((1, 2, 4, 70, 96, 40), PAIRS, 82),
        wgrad_row((1, 2, 4, 70, 96, 40), 2 * PAIRS, 83, short_only=True)]


def test_rows_cover_the_convupngrad_abi():
    rows = {e for r in ROWS for e in r.entries}
    assert rows <= set(hip.CONVUPNGRAD_EXPORTS), rows - set(hip.CONVUPNGRAD_EXPORTS)
    uncovered = [n for n in hip.CONVUPNGRAD_EXPORTS if n not in rows and not any(n.endswith(h) for h in HOST_ONLY)]
    assert not uncovered, f"exports of include/v2ce_hip_convupngrad.h without a containment row: {uncovered}"
    assert len({r.name for r in ROWS}) == len(ROWS)
    q = hip.lib().v2ce_convupn_wgrad_workspace_bytes
    per_wg = (28 * 32 * 32 + 32) * 8
    assert q(*TRIPLE, 1, 2, 4, 70, 96, 40, 0) == 8 * PAIRS * per_wg and q(*TRIPLE, 1, 2, 4, 70, 96, 40, PAIRS) == PAIRS * per_wg


@pytest.mark.gpu
@pytest.mark.parametrize("r", ROWS, ids=[r.name for r in ROWS])
def test_containment(r):
    check_row(r)


@pytest.mark.gpu
@pytest.mark.parametrize("r", ROWS[:2], ids=[r.name for r in ROWS[:2]])
def test_short_workspace_is_refused(r):
    check_short_workspace(r)
