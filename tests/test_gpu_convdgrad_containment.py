"""The entries of include/v2ce_hip_convdgrad.h stay inside the buffers the header documents: the scheme of
tests/test_gpu_convgrad_containment.py (guarded, poisoned allocations of exactly the documented sizes, tests/guarded.py) for
v2ce_conv32_dgrad on tensors whose rows are padded (W = 70 at pitch 96, the padding of the inputs holding NaN): with the
kernel's own grid, and with the grid capped at 3 workgroups (each walks several tiles).  Per row: every guard intact with the
outputs and the workspace poisoned with POISON[0], with POISON[1], with a zeroed workspace and with every buffer one step past
a 256-byte boundary (16 bytes for the channels-last-16 tensors, 8 for the workspace, 4 for the weight); every byte of d_x and
d_res written, the padding columns included; the same bytes in all four runs; the bytes of last_conv.conv32_dgrad; inputs
unchanged; a workspace 4 bytes short is V2CE_ERR_WORKSPACE and nothing is written."""
import numpy as np
import pytest
import torch

from test_gpu_containment import L, Row, bytes_of, check_row, check_short_workspace, stream
from tests import last_conv_dgrad_ref as D
from v2ce_toolbox_amd import hip, last_conv

HOST_ONLY = ("_bytes",)


def case(dims, seed):
    B, Lq, H, W, pitch = dims
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((32, 32, 3, 3, 3)) * 0.1).astype(np.float32)
    y = np.maximum(rng.standard_normal((B, 32, Lq, H, W)), 0).astype(np.float32)
    up = rng.standard_normal((B, 32, Lq, H, W)).astype(np.float32)
    return w, D.to_c16(y, pitch), D.to_c16(up, pitch)


def dgrad_row(dims, cap, seed, with_y=True, outs=("d_x", "d_res")):
    entry = "v2ce_conv32_dgrad"
    B, Lq, H, W, pitch = dims
    nbytes = B * Lq * 2 * H * pitch * 64

    def call(run):
        w, y, up = case(dims, seed)
        dx = run.out("d_x", nbytes, 4, align=16) if "d_x" in outs else None
        dr = run.out("d_res", nbytes, 4, align=16) if "d_res" in outs else None
        nb = L().v2ce_conv32_dgrad_workspace_bytes(*dims, cap)
        ws, nb = run.ws("workspace", nb, align=8)
        run.ok(L().v2ce_conv32_dgrad(run.inp("weight", w), run.inp("y", y, align=16) if with_y else None,
                                     run.inp("upstream", up, align=16), *dims, dx, dr, ws, nb, cap, stream()), entry)

    def want():
        w, y, up = (torch.from_numpy(a).cuda() for a in case(dims, seed))
        for t in (y, up):
            t.lw, t.c16 = W, True
        g = last_conv.conv32_dgrad(w, y if with_y else None, up, want=tuple(n[2:] for n in outs), max_workgroups=cap)
        return {n: bytes_of(g[n[2:]]) for n in outs}
    return Row(f"conv32_dgrad{list(dims)}cap{cap}{'' if with_y else 'plain'}{'' if len(outs) == 2 else outs[0]}", [entry], call, want)


# B, L, H, W, pitch: 8 tiles (two of them ragged in W, H = 3 leaves a one-row tile); 16 tiles on 3 workgroups; one output alone
ROWS = [dgrad_row((1, 2, 3, 70, 96), 0, 71), dgrad_row((2, 2, 3, 70, 96), 3, 72), dgrad_row((1, 2, 3, 70, 96), 2, 73, with_y=False),
        dgrad_row((1, 2, 3, 70, 96), 0, 74, outs=("d_x",)), dgrad_row((1, 2, 3, 70, 96), 0, 75, outs=("d_res",))]


def test_rows_cover_the_convdgrad_abi():
    rows = {e for r in ROWS for e in r.entries}
    assert rows <= set(hip.CONVDGRAD_EXPORTS), rows - set(hip.CONVDGRAD_EXPORTS)
    uncovered = [n for n in hip.CONVDGRAD_EXPORTS if n not in rows and not any(n.endswith(h) for h in HOST_ONLY)]
    assert not uncovered, f"exports of include/v2ce_hip_convdgrad.h without a containment row: {uncovered}"
    assert len({r.name for r in ROWS}) == len(ROWS)


@pytest.mark.gpu
@pytest.mark.parametrize("r", ROWS, ids=[r.name for r in ROWS])
def test_containment(r):
    check_row(r)


@pytest.mark.gpu
@pytest.mark.parametrize("r", ROWS[:2], ids=[r.name for r in ROWS[:2]])
def test_short_workspace_is_refused(r):
    check_short_workspace(r)
