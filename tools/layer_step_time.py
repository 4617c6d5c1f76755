"""Host overhead of the trainable decoder layers: the wall time of one ``fit_dec2_block`` step -- Dec2Block -> LastBlock ->
PredHead -> calculate_loss -> backward -> Adam step on cached trunk tensors -- at a shape small enough that Python between
the launches shows.  Prints one JSON line: the median of 15 steps after 3 warm-up steps, ms.

    python tools/layer_step_time.py [--layers-from DIR] [--out FILE.json]

``--layers-from DIR`` takes last_conv.py, last_block.py, dec2_conv.py, dec2_block.py (and whatever else DIR holds) from DIR
in place of the package's own: another commit's layers on this commit's library, for an A/B of the Python side alone
(one process each in the order parent, folded, parent, folded)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPE = (1, 8, 2, 128, 176)
WARMUP, STEPS = 3, 15


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--layers-from", default=None)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    import v2ce_toolbox_amd
    if args.layers_from:
        v2ce_toolbox_amd.__path__.insert(0, os.path.abspath(args.layers_from))
    import torch
    from v2ce_toolbox_amd import dec2_block, losses, synth
    from v2ce_toolbox_amd.dec2_block import Dec2Block
    from v2ce_toolbox_amd.last_block import LastBlock
    from v2ce_toolbox_amd.pred_head import PredHead
    from v2ce_toolbox_amd.v2ce_3d import V2ce3d
    m = V2ce3d(precision="f16x2")
    m.load_state_dict(synth.make_state_dict(0))
    m = m.eval().to("cuda:0")
    B, L, _, H, W = SHAPE
    x = torch.randn(SHAPE, generator=torch.Generator().manual_seed(1)).cuda()
    gt = torch.randn((B, L, 20, H, W), generator=torch.Generator().manual_seed(2)).abs().cuda()
    snap = m.sn_snapshot()
    h1, s2, x1 = m.forward_dec2_sources(x)
    m.sn_restore(snap)
    dec2, block, head = Dec2Block.from_model(m), LastBlock.from_model(m), PredHead.from_model(m)
    opt = torch.optim.Adam([q for mod in (dec2, block, head) for q in mod.parameters()], lr=1e-4)
    ts = []
    for _ in range(WARMUP + STEPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        opt.zero_grad(set_to_none=True)
        total, _ = losses.calculate_loss(head(block(dec2(h1, s2), x1)), gt)
        total.backward()
        opt.step()
        loss = float(total.detach())
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts = sorted(ts[WARMUP:])
    res = {"layers": os.path.dirname(dec2_block.__file__), "shape": list(SHAPE), "median_ms": ts[len(ts) // 2], "min_ms": ts[0],
           "max_ms": ts[-1], "last_loss": loss}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f)


if __name__ == "__main__":
    main()
