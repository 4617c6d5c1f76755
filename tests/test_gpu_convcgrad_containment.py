"""The entries of include/v2ce_hip_convcgrad.h stay inside the buffers the header documents: the scheme of
tests/test_gpu_convngrad_containment.py (guarded, poisoned allocations of exactly the documented sizes, tests/guarded.py)
for v2ce_convc_wgrad and v2ce_convc_dgrad on tensors whose rows are padded (W = 70 at pitch 96, the padding of the inputs
holding NaN), at 128 -> 128 (four groups on either side: the input gradient fetches its weights again per tile) and at
256 -> 32 (eight ci groups against one co group): shapes [1,2,3,70] (8 tiles, the kernel's own grid) and [2,2,3,70]
(16 tiles, capped at one share), without y, with each output alone and with both.  Per row: every guard intact with the
outputs and the workspace poisoned with POISON[0], with POISON[1], with a zeroed workspace and with every buffer one step
past a 256-byte boundary; every byte of the requested outputs written, the padding columns of d_x and d_res included, and
none of them NaN; the same bytes in all four runs; the bytes of conv_grads.convc_wgrad / convc_dgrad; inputs unchanged; a
workspace 4 bytes short is V2CE_ERR_WORKSPACE and nothing is written."""
import pytest
import torch

from test_gpu_containment import L, Row, bytes_of, check_row, check_short_workspace, stream
from test_gpu_convngrad_containment import case, device_case
from v2ce_toolbox_amd import conv_grads, hip

HOST_ONLY = ("_bytes",)


def wgrad_row(dims, cin, cout, cap, seed, with_y=True, outs=("d_weight", "d_shift")):
    entry = "v2ce_convc_wgrad"

    def call(run):
        x, y, up, _ = case(dims, cin, cout, seed)
        dw = run.out("d_weight", cout * cin * 27 * 4, 4) if "d_weight" in outs else None
        ds = run.out("d_shift", cout * 4, 4) if "d_shift" in outs else None
        nb = L().v2ce_convc_wgrad_workspace_bytes(cin, cout, *dims, cap)
        ws, nb = run.ws("workspace", nb, align=8)
        run.ok(L().v2ce_convc_wgrad(run.inp("x", x, align=16), run.inp("y", y, align=16) if with_y else None,
                                    run.inp("upstream", up, align=16), cin, cout, *dims, dw, ds, ws, nb, cap, stream()), entry)

    def want():
        x, y, up, _ = device_case(dims, cin, cout, seed)
        g = conv_grads.convc_wgrad(x, y if with_y else None, up, want=tuple(n[2:] for n in outs), max_workgroups=cap)
        assert not any(torch.isnan(t).any() for t in g.values()), "NaN reached an output"
        return {n: bytes_of(g[n[2:]]) for n in outs}
    tag = f"{cin}to{cout}{list(dims)}cap{cap}{'' if with_y else 'plain'}{'' if len(outs) == 2 else outs[0]}"
    return Row("convc_wgrad" + tag, [entry], call, want)


def dgrad_row(dims, cin, cout, cap, seed, with_y=True, outs=("d_x", "d_res")):
    entry = "v2ce_convc_dgrad"
    B, Lq, H, W, pitch = dims
    n_x, n_res = (B * Lq * (c // 16) * H * pitch * 64 for c in (cin, cout))

    def call(run):
        _, y, up, w = case(dims, cin, cout, seed)
        dx = run.out("d_x", n_x, 4, align=16) if "d_x" in outs else None
        dr = run.out("d_res", n_res, 4, align=16) if "d_res" in outs else None
        nb = L().v2ce_convc_dgrad_workspace_bytes(cin, cout, *dims, cap)
        ws, nb = run.ws("workspace", nb, align=8)
        run.ok(L().v2ce_convc_dgrad(run.inp("weight", w), run.inp("y", y, align=16) if with_y else None,
                                    run.inp("upstream", up, align=16), cin, cout, *dims, dx, dr, ws, nb, cap, stream()), entry)

    def want():
        _, y, up, w = device_case(dims, cin, cout, seed)
        g = conv_grads.convc_dgrad(w, y if with_y else None, up, want=tuple(n[2:] for n in outs), max_workgroups=cap)
        assert not any(torch.isnan(t).any() for t in g.values()), "NaN reached an output"
        return {n: bytes_of(g[n[2:]]) for n in outs}
    tag = f"{cin}to{cout}{list(dims)}cap{cap}{'' if with_y else 'plain'}{'' if len(outs) == 2 else outs[0]}"
    return Row("convc_dgrad" + tag, [entry], call, want)


# B, L, H, W, pitch: 8 tiles (two of them ragged in W, H = 3 leaves a one-row tile) on the kernel's own grid; 16 tiles on one
# share (a cap of the pair count, or of the ci groups)
SMALL, TWICE = (1, 2, 3, 70, 96), (2, 2, 3, 70, 96)
ROWS = [wgrad_row(SMALL, 128, 128, 0, 181), wgrad_row(TWICE, 128, 128, 16, 182), wgrad_row(SMALL, 256, 32, 0, 183),
        wgrad_row(TWICE, 256, 32, 8, 184, with_y=False),
        dgrad_row(SMALL, 128, 128, 0, 191), dgrad_row(TWICE, 128, 128, 4, 192), dgrad_row(SMALL, 256, 32, 0, 193),
        dgrad_row(TWICE, 256, 32, 8, 194, with_y=False)]
SHORT = [ROWS[0], ROWS[1], ROWS[4], ROWS[5]]
for _i, (_cin, _cout) in enumerate(((128, 128), (256, 32))):            # each output alone
    ROWS += [wgrad_row(SMALL, _cin, _cout, 0, 185 + _i, outs=("d_weight",)), wgrad_row(TWICE, _cin, _cout, 0, 187 + _i, outs=("d_shift",)),
             dgrad_row(SMALL, _cin, _cout, 0, 195 + _i, outs=("d_x",)), dgrad_row(TWICE, _cin, _cout, 0, 197 + _i, outs=("d_res",))]


def test_rows_cover_the_convcgrad_abi():
    rows = {e for r in ROWS for e in r.entries}
    assert rows <= set(hip.CONVCGRAD_EXPORTS), rows - set(hip.CONVCGRAD_EXPORTS)
    uncovered = [n for n in hip.CONVCGRAD_EXPORTS if n not in rows and not any(n.endswith(h) for h in HOST_ONLY)]
    assert not uncovered, f"exports of include/v2ce_hip_convcgrad.h without a containment row: {uncovered}"
    assert len({r.name for r in ROWS}) == len(ROWS)


@pytest.mark.gpu
@pytest.mark.parametrize("r", ROWS, ids=[r.name for r in ROWS])
def test_containment(r):
    check_row(r)


@pytest.mark.gpu
@pytest.mark.parametrize("r", SHORT, ids=[r.name for r in SHORT])
def test_short_workspace_is_refused(r):
    check_short_workspace(r)
