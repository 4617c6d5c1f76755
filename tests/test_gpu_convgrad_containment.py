"""The entries of include/v2ce_hip_convgrad.h stay inside the buffers the header documents: the scheme of
tests/test_gpu_pred_head_containment.py (guarded, poisoned allocations of exactly the documented sizes, tests/guarded.py)
for v2ce_conv32_wgrad on tensors whose rows are padded (W = 70 at pitch 96, the padding holding NaN): with the kernel's own
grid, and with the grid capped at 3 workgroups (each walks several tiles; the workspace is that of 3).  Per row: every guard
intact with the outputs and the workspace poisoned with POISON[0], with POISON[1], with a zeroed workspace and with every
buffer one step past a 256-byte boundary (16 bytes for the channels-last-16 tensors, 8 for the workspace, 4 for the
outputs); every byte of d_weight and d_shift written; the same bytes in all four runs; the bytes of
last_conv.conv32_wgrad; inputs unchanged; a workspace 4 bytes short is V2CE_ERR_WORKSPACE and nothing is written."""
import numpy as np
import pytest
import torch

from test_gpu_containment import L, Row, bytes_of, check_row, check_short_workspace, stream
from tests import last_conv_ref as R
from v2ce_toolbox_amd import hip, last_conv

HOST_ONLY = ("_bytes",)


def case(dims, seed):
    B, Lq, H, W, pitch = dims
    rng = np.random.default_rng(seed)
    x = np.maximum(rng.standard_normal((B, 32, Lq, H, W)), 0).astype(np.float32)
    y = np.maximum(rng.standard_normal((B, 32, Lq, H, W)), 0).astype(np.float32)
    up = rng.standard_normal((B, 32, Lq, H, W)).astype(np.float32)
    return tuple(R.to_c16(a, pitch) for a in (x, y, up))


def wgrad_row(dims, cap, seed, with_y=True):
    entry = "v2ce_conv32_wgrad"

    def call(run):
        x, y, up = case(dims, seed)
        dw, ds = run.out("d_weight", 32 * 32 * 27 * 4, 4), run.out("d_shift", 32 * 4, 4)
        nb = L().v2ce_conv32_wgrad_workspace_bytes(*dims, cap)
        ws, nb = run.ws("workspace", nb, align=8)
        run.ok(L().v2ce_conv32_wgrad(run.inp("x", x, align=16), run.inp("y", y, align=16) if with_y else None,
                                     run.inp("upstream", up, align=16), *dims, dw, ds, ws, nb, cap, stream()), entry)

    def want():
        x, y, up = (torch.from_numpy(a).cuda() for a in case(dims, seed))
        for t in (x, y, up):
            t.lw, t.c16 = dims[3], True
        g = last_conv.conv32_wgrad(x, y if with_y else None, up, max_workgroups=cap)
        return {"d_weight": bytes_of(g["weight"]), "d_shift": bytes_of(g["shift"])}
    return Row(f"conv32_wgrad{list(dims)}cap{cap}{'' if with_y else 'plain'}", [entry], call, want)


# B, L, H, W, pitch: 8 tiles (two of them ragged in W, H = 3 leaves a one-row tile); 16 tiles on 3 workgroups
ROWS = [wgrad_row((1, 2, 3, 70, 96), 0, 61), wgrad_row((2, 2, 3, 70, 96), 3, 62), wgrad_row((1, 2, 3, 70, 96), 2, 63, with_y=False)]


def test_rows_cover_the_convgrad_abi():
    rows = {e for r in ROWS for e in r.entries}
    assert rows <= set(hip.CONVGRAD_EXPORTS), rows - set(hip.CONVGRAD_EXPORTS)
    uncovered = [n for n in hip.CONVGRAD_EXPORTS if n not in rows and not any(n.endswith(h) for h in HOST_ONLY)]
    assert not uncovered, f"exports of include/v2ce_hip_convgrad.h without a containment row: {uncovered}"
    assert len({r.name for r in ROWS}) == len(ROWS)


@pytest.mark.gpu
@pytest.mark.parametrize("r", ROWS, ids=[r.name for r in ROWS])
def test_containment(r):
    check_row(r)


@pytest.mark.gpu
@pytest.mark.parametrize("r", ROWS[:2], ids=[r.name for r in ROWS[:2]])
def test_short_workspace_is_refused(r):
    check_short_workspace(r)
