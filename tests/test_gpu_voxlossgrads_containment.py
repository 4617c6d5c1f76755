"""The entries of include/v2ce_hip_grad.h stay inside the buffers the header documents: the scheme of
tests/test_gpu_containment.py (guarded, poisoned allocations of exactly the documented sizes, tests/guarded.py) for
v2ce_voxloss_grads and v2ce_volume_loss_grads.  Per row: every guard intact with the outputs and the workspace poisoned
with POISON[0], with POISON[1], with a zeroed workspace and with pred, gt and grad one element past a 256-byte boundary;
every byte of grad written; the same bytes in all four runs; the bytes of losses.voxel_loss_grads_batch /
volume_loss_grads_batch; inputs unchanged; a workspace 4 bytes short is V2CE_ERR_WORKSPACE and nothing is written."""
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_containment import L, Row, bytes_of, check_row, check_short_workspace, stream, vox_pair
from v2ce_toolbox_amd import hip
from v2ce_toolbox_amd import losses as LS

ALL_LOSS = ("pyramid", "pt", "ef", "ef_splitp", "match", "compensation", "norml1", "norml2")
HOST_ONLY = ("_bytes",)


def grads_row(volume, dims, seed):
    entry = "v2ce_volume_loss_grads" if volume else "v2ce_voxloss_grads"
    size = ctypes.sizeof(hip.VoxLossGradCoeffs)

    def coef():
        if volume:
            return LS.grad_coeffs(dims, ("pyramid", "pt"), add_base_loss=True)
        p, _ = vox_pair(dims, seed)
        return LS.grad_coeffs(dims, ALL_LOSS, add_base_loss=True, pred_sq_sum=float((p.astype(np.float64) ** 2).sum()))

    def call(run):
        p, g = vox_pair(dims, seed)
        c = coef()
        up = run.inp("upstream", np.array([1.5], np.float32))
        grad = run.out("grad", p.size * 4, 4)
        nb = getattr(L(), entry + "_workspace_bytes")(*dims, ctypes.byref(c), size)
        ws, nb = run.ws("workspace", nb)
        run.ok(getattr(L(), entry)(run.inp("pred", p), run.inp("gt", g), *dims, ctypes.byref(c), size, up, grad, ws, nb, stream()),
               entry)

    def want():
        p, g = vox_pair(dims, seed)
        fn = LS.volume_loss_grads_batch if volume else LS.voxel_loss_grads_batch
        up = torch.full((1,), 1.5, device="cuda")
        return {"grad": bytes_of(fn(torch.from_numpy(p).cuda(), torch.from_numpy(g).cuda(), coef=coef(), upstream=up))}
    return Row(f"{entry[5:]}{list(dims)}", [entry], call, want)


ROWS = [grads_row(False, (2, 3, 20, 9, 11), 41), grads_row(True, (2, 25, 9, 10), 42)]


def test_rows_cover_the_grad_abi():
    rows = {e for r in ROWS for e in r.entries}
    assert rows <= set(hip.GRAD_EXPORTS), rows - set(hip.GRAD_EXPORTS)
    uncovered = [n for n in hip.GRAD_EXPORTS if n not in rows and not any(n.endswith(h) for h in HOST_ONLY)]
    assert not uncovered, f"exports of include/v2ce_hip_grad.h without a containment row: {uncovered}"
    assert len({r.name for r in ROWS}) == len(ROWS)


@pytest.mark.gpu
@pytest.mark.parametrize("r", ROWS, ids=[r.name for r in ROWS])
def test_containment(r):
    check_row(r)


@pytest.mark.gpu
@pytest.mark.parametrize("r", ROWS, ids=[r.name for r in ROWS])
def test_short_workspace_is_refused(r):
    check_short_workspace(r)
