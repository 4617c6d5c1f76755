"""The entries of include/v2ce_hip_train.h stay inside the buffers the header documents: the scheme of
tests/test_gpu_voxlossgrads_containment.py (guarded, poisoned allocations of exactly the documented sizes,
tests/guarded.py) for v2ce_pred_head_fwd and v2ce_pred_head_grads, on features whose rows are padded (W = 70 at pitch
96, the padding holding NaN).  Per row: every guard intact with the outputs and the workspace poisoned with POISON[0],
with POISON[1], with a zeroed workspace and with every buffer one step past a 256-byte boundary (16 bytes for the
channels-last-16 tensors, 8 for the workspace, 4 for the dense ones); every byte of y, d_weight and d_bias written, of
d_feat exactly the columns below W; the same bytes in all four runs; the bytes of pred_head.pred_head_forward /
pred_head_grads; inputs unchanged; a workspace 4 bytes short is V2CE_ERR_WORKSPACE and nothing is written."""
import numpy as np
import pytest
import torch

from test_gpu_containment import L, Row, bytes_of, check_row, check_short_workspace, stream
from tests import pred_head_ref as R
from v2ce_toolbox_amd import hip, pred_head

HOST_ONLY = ("_bytes",)
DIMS = (2, 2, 20, 3, 70, 96)                 # B, L, Cout, H, W, pitch: 840 positions, 7 tiles, the last with 72 positions


def case(seed):
    B, Lq, cout, H, W, pitch = DIMS
    rng = np.random.default_rng(seed)
    feat = rng.standard_normal((B, 32, Lq, H, W)).astype(np.float32)
    weight = (rng.standard_normal((cout, 32)) * 0.2).astype(np.float32)
    bias = (rng.standard_normal(cout) * 0.1).astype(np.float32)
    up = rng.standard_normal((B, Lq, cout, H, W)).astype(np.float32)
    return R.to_c16(feat, pitch), weight, bias, up


def device_case(seed):
    f, w, b, u = (torch.from_numpy(a).cuda() for a in case(seed))
    f.lw, f.c16 = DIMS[4], True
    return f, w, b, u


def fwd_row(seed):
    entry = "v2ce_pred_head_fwd"
    B, Lq, cout, H, W, pitch = DIMS

    def call(run):
        f, w, b, _ = case(seed)
        y = run.out("y", B * Lq * cout * H * W * 4, 4)
        nb = L().v2ce_pred_head_fwd_workspace_bytes(*DIMS)
        ws, nb = run.ws("workspace", nb, align=8)
        run.ok(L().v2ce_pred_head_fwd(run.inp("feat", f, align=16), run.inp("weight", w), run.inp("bias", b), *DIMS, y, ws, nb,
                                      stream()), entry)

    def want():
        f, w, b, _ = device_case(seed)
        return {"y": bytes_of(pred_head.pred_head_forward(f, w, b))}
    return Row(f"pred_head_fwd{list(DIMS)}", [entry], call, want)


def grads_row(seed):
    entry = "v2ce_pred_head_grads"
    B, Lq, cout, H, W, pitch = DIMS

    def forward_y():
        f, w, b, _ = device_case(seed)
        return pred_head.pred_head_forward(f, w, b)

    def call(run):
        f, w, _, u = case(seed)
        y = forward_y().cpu().numpy()
        dw, db = run.out("d_weight", cout * 32 * 4, 4), run.out("d_bias", cout * 4, 4)
        df = run.out("d_feat", f.nbytes, 4, align=16)
        nb = L().v2ce_pred_head_grads_workspace_bytes(*DIMS)
        ws, nb = run.ws("workspace", nb, align=8)
        run.ok(L().v2ce_pred_head_grads(run.inp("feat", f, align=16), run.inp("y", y), run.inp("upstream", u),
                                        run.inp("weight", w), *DIMS, dw, db, df, ws, nb, stream()), entry)
        cols = np.zeros(f.shape, bool)
        cols[:, :, :, :, :W, :] = True                             # the padding columns are not written
        return {"d_feat": np.repeat(cols.ravel(), 4)}

    def want():
        f, w, _, u = device_case(seed)
        g = pred_head.pred_head_grads(f, forward_y(), u, w, want=("weight", "bias", "feat"))
        return {"d_weight": bytes_of(g["weight"]), "d_bias": bytes_of(g["bias"]), "d_feat": bytes_of(g["feat"])}
    return Row(f"pred_head_grads{list(DIMS)}", [entry], call, want)


ROWS = [fwd_row(51), grads_row(52)]


def test_rows_cover_the_train_abi():
    rows = {e for r in ROWS for e in r.entries}
    assert rows <= set(hip.TRAIN_EXPORTS), rows - set(hip.TRAIN_EXPORTS)
    uncovered = [n for n in hip.TRAIN_EXPORTS if n not in rows and not any(n.endswith(h) for h in HOST_ONLY)]
    assert not uncovered, f"exports of include/v2ce_hip_train.h without a containment row: {uncovered}"
    assert len({r.name for r in ROWS}) == len(ROWS)


@pytest.mark.gpu
@pytest.mark.parametrize("r", ROWS, ids=[r.name for r in ROWS])
def test_containment(r):
    check_row(r)


@pytest.mark.gpu
@pytest.mark.parametrize("r", ROWS, ids=[r.name for r in ROWS])
def test_short_workspace_is_refused(r):
    check_short_workspace(r)
