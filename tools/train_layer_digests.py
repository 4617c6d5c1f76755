"""Record what the trainable decoder layers compute, as digests, so that two trees can be compared value for value.

    python tools/train_layer_digests.py OUT.json

Public names only (last_conv / last_block / dec2_conv / dec2_block / pred_head / finetune / losses), a seeded ``synth``
model in both precisions, seeded inputs at the shapes of the golden cases ``b2_l3_5x7`` and ``b1_l2_3x70`` (odd extents, a
ragged last tile, pitch 96 against a logical width of 70).  OUT.json holds two records (``read`` loads them):

  values  {key: sha256 of the contiguous f32 bytes}.  A tensor whose padding columns are specified (zeros: the norms'
          outputs, every gradient) is digested whole; the output of a convolution launch is allocated uninitialised and only
          its logical columns ``[..., :lw, :]`` are written, so only those are digested (keys ending in ``:lw``).
            A  the chain Dec2Block -> LastBlock (x1 requires grad) -> PredHead -> calculate_loss -> backward: every tensor
               between the six layers, its ``.lw``, presence and bytes of ``.absmax``, every parameter's ``.grad``,
               ``x1.grad``, every ``guard``, ``weight_u`` / ``weight_v`` after the forward
            B  TailConvs(input_grads=False); LastConv with and without inputs that require grad; convup_dgrad on the golden
               cases of tests/golden/.lastblock_dgrad at max_workgroups 0 and 3, both wants, g1=None and gd=None
            C  two steps each of the five fits with all groups: the history and the state_dict after write_back (one
               digest of all its keys' digests, and the names of the tensors the fit changed)
          The loss terms are those without the pyramid's 8-voxel minimum (the cases are 5 and 3 rows high).
  errors  {label: [exception type, message]} of a fixed list of bad calls ("none" where a call is accepted).

The digests are a property of this code on one machine with one torch (the layers use torch reductions): run both trees
in the same place.  One process, one short run."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import last_block_dgrad_ref as D  # noqa: E402
from v2ce_toolbox_amd import dec2_block, dec2_conv, finetune, last_block, last_conv, losses, synth  # noqa: E402
from v2ce_toolbox_amd.dec2_block import Dec2Block, Dec2Convs, Dec2Norms  # noqa: E402
from v2ce_toolbox_amd.dec2_conv import Dec2Conv  # noqa: E402
from v2ce_toolbox_amd.last_block import LastBlock, TailConvs  # noqa: E402
from v2ce_toolbox_amd.last_conv import LastConv, TailNorms  # noqa: E402
from v2ce_toolbox_amd.pred_head import PredHead  # noqa: E402
from v2ce_toolbox_amd.v2ce_3d import V2ce3d  # noqa: E402

CASES = {"b2_l3_5x7": (2, 3, 5, 7), "b1_l2_3x70": (1, 2, 3, 70)}
LOSS = ("ef", "ef_splitp", "compensation")
DEV = "cuda:0"


def sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy(), np.float32).tobytes()).hexdigest()


_STATE = []


def make_model(precision):
    if not _STATE:
        _STATE.append(synth.make_state_dict(0))
    m = V2ce3d(precision=precision)
    m.load_state_dict(_STATE[0])
    return m.eval().to(DEV)


def randn(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(DEV)


def image(case):
    B, L, H, W = CASES[case]
    return randn((B, L, 2, H, W), 11)


def voxels(case):
    B, L, H, W = CASES[case]
    return randn((B, L, 20, H, W), 12).abs().contiguous()


def frozen(model, accessor, x):
    """The accessor's tensors with the model's spectral-norm state put back."""
    snap = model.sn_snapshot()
    out = getattr(model, accessor)(x)
    model.sn_restore(snap)
    return out


def leaf(t):
    """A copy of a trunk tensor that requires grad and carries the original's attributes."""
    g = t.clone().requires_grad_(True)
    g.lw, g.c16 = t.lw, True
    if hasattr(t, "absmax"):
        g.absmax = t.absmax
    return g


def put(rec, key, t, padded):
    """padded: the padding columns are specified -> the whole tensor; else the logical columns only."""
    if t is None:
        rec[key] = None
        return
    lw = getattr(t, "lw", None)
    if padded or lw is None:
        rec[key] = sha(t)
    else:
        rec[key + ":lw"] = sha(t[..., :lw, :])
    if lw is not None:
        rec[key + ".lw"] = int(lw)
        rec[key + ".shape"] = list(t.shape)
    rec[key + ".absmax"] = sha(t.absmax) if hasattr(t, "absmax") else None


def put_layer(rec, key, layer):
    for n, p in layer.named_parameters():
        rec[f"{key}.{n}.grad"] = None if p.grad is None else sha(p.grad)
    for n, b in layer.named_buffers():
        if n.endswith(("weight_u", "weight_v", "guard")):
            rec[f"{key}.{n}"] = sha(b)


def group_a(rec, tag, model, case):
    x = image(case)
    h1, s2, x1 = frozen(model, "forward_dec2_sources", x)
    x1g = leaf(x1)
    dec2, block, head = Dec2Block.from_model(model), LastBlock.from_model(model), PredHead.from_model(model)
    z1, zd = dec2.convs(h1, s2)
    t2, r2 = dec2.norms(z1, zd)
    x0 = dec2.conv(t2, r2)
    y1, yd = block.convs(x0, x1g)
    t, r = block.norms(y1, yd)
    feat = block.conv(t, r)
    pred = head(feat)
    for k, a, padded in (("h1", h1, False), ("s2", s2, False), ("x1", x1, False), ("dec2.z1", z1, False), ("dec2.zd", zd, False),
                         ("dec2.t", t2, True), ("dec2.res", r2, True), ("x0", x0, False), ("last.z1", y1, False),
                         ("last.zd", yd, False), ("last.t", t, True), ("last.res", r, True), ("feat", feat, False),
                         ("pred", pred, True)):
        put(rec, f"A.{tag}.{k}", a, padded)
    for k, layer in (("dec2", dec2), ("last", block)):      # u, v, guard after the forward
        put_layer(rec, f"A.{tag}.fwd.{k}", layer)
    total, parts = losses.calculate_loss(pred, voxels(case), loss=LOSS)
    total.backward()
    rec[f"A.{tag}.loss"] = repr(float(total.detach()))
    rec[f"A.{tag}.loss_dict"] = {n: repr(float(v)) for n, v in parts.items()}
    for k, layer in (("dec2", dec2), ("last", block), ("head", head)):
        put_layer(rec, f"A.{tag}.{k}", layer)
    rec[f"A.{tag}.x1.grad"] = sha(x1g.grad)


def group_b(rec, tag, model, case):
    x = image(case)
    B, L, H, W = CASES[case]
    # TailConvs without input gradients
    x0, x1 = frozen(model, "forward_tail_sources", x)
    convs = TailConvs.from_model(model)
    z1, zd = convs(x0, x1)
    put(rec, f"B.{tag}.convs.z1", z1, False)
    put(rec, f"B.{tag}.convs.zd", zd, False)
    torch.autograd.backward([z1, zd], [randn(z1.shape, 21), randn(zd.shape, 22)])
    put_layer(rec, f"B.{tag}.convs", convs)
    # LastConv with and without inputs that require grad
    t, res = frozen(model, "forward_tail_inputs", x)
    up = randn(t.shape, 23)
    for k, (a, b) in (("grad", (leaf(t), leaf(res))), ("nograd", (t, res))):
        conv = LastConv.from_model(model)
        feat = conv(a, b)
        put(rec, f"B.{tag}.conv.{k}.feat", feat, False)
        feat.backward(up)
        put_layer(rec, f"B.{tag}.conv.{k}", conv)
        rec[f"B.{tag}.conv.{k}.t.grad"] = None if a.grad is None else sha(a.grad)
        rec[f"B.{tag}.conv.{k}.res.grad"] = None if b.grad is None else sha(b.grad)


def group_b_dgrad(rec, case):
    z = D.load_case(case)
    W = z["g1"].shape[-1]

    def dev(a):
        t = torch.from_numpy(np.ascontiguousarray(D.to_c16(a, W + 3), np.float32)).to(DEV)
        t.lw, t.c16 = W, True
        return t
    w, s, g1, gd = torch.from_numpy(z["kw"]).to(DEV), torch.from_numpy(z["ks"]).to(DEV), dev(z["g1"]), dev(z["gd"])
    for cap in (0, 3):
        for want in (("x0", "x1"), ("x0",), ("x1",)):
            for k, args in (("both", (w, s, g1, gd)), ("g1none", (None, s, None, gd)), ("gdnone", (w, None, g1, None))):
                g = last_block.convup_dgrad(*args, want=want, max_workgroups=cap)
                for n, t in g.items():
                    put(rec, f"B.dgrad.{case}.cap{cap}.{'+'.join(want)}.{k}.{n}", t, True)


FITS = (("fit_tail", finetune.TAIL_GROUPS), ("fit_tail_norms", finetune.TAIL_NORM_GROUPS),
        ("fit_last_block", finetune.LAST_BLOCK_GROUPS), ("fit_dec2_conv", finetune.DEC2_CONV_GROUPS),
        ("fit_dec2_block", finetune.DEC2_BLOCK_GROUPS))


def group_c(rec, precision, case):
    x, gt = image(case), voxels(case)
    for name, groups in FITS:
        model = make_model(precision)
        before = {k: sha(v.float()) for k, v in model.state_dict().items()}
        hist = getattr(finetune, name)(model, [x], [gt], train=groups, loss=LOSS, steps=2, lr=1e-3)
        key = f"C.{precision}.{case}.{name}"
        rec[key + ".history"] = [{"loss": repr(h["loss"]), "loss_dict": {n: repr(v) for n, v in h["loss_dict"].items()}}
                                 for h in hist]
        after = {k: sha(v.float()) for k, v in model.state_dict().items()}
        # the whole state_dict as one digest of its keys' digests, and which tensors the fit changed
        rec[key + ".state"] = hashlib.sha256("\n".join(f"{k} {after[k]}" for k in sorted(after)).encode()).hexdigest()
        rec[key + ".changed"] = sorted(k for k in after if after[k] != before[k])


def c16(G, H=4, W=6, B=1, L=2, lw=None, pitch=None):
    t = torch.zeros(B, L, G, H, pitch or W, 16, device=DEV)
    t.lw, t.c16 = (lw or W), True
    return t


def bad_calls(model):
    """[(label, call)]: every call is made on tensors that pass the device check, so the check named is the one met."""
    a2, a3, a4 = c16(2), c16(3), c16(4)
    narrow = c16(2, lw=5)
    s4, s3, s8 = c16(4, H=2, W=3), c16(3, H=2, W=3), c16(8, H=2, W=3)          # sources of a [.., 4, 6] skip tensor
    w32, w64x32, w96 = (torch.zeros(s, device=DEV) for s in ((32, 32, 3, 3, 3), (64, 32, 3, 3, 3), (32, 96, 3, 3, 3)))
    sw = torch.zeros(32, 96, device=DEV)
    w64 = torch.zeros(64, 64, 3, 3, 3, device=DEV)
    lc, lb, dc, db = last_conv, last_block, dec2_conv, dec2_block

    def req(t):
        g = t.clone().requires_grad_(True)
        g.lw, g.c16 = t.lw, True
        return g
    calls = [
        # wrong plane count, entries
        ("planes.conv32_wgrad.x", lambda: lc.conv32_wgrad(a3, a3, a3)),
        ("planes.conv32_wgrad.upstream", lambda: lc.conv32_wgrad(a2, a2, a3)),
        ("planes.conv32_dgrad.upstream", lambda: lc.conv32_dgrad(w32, None, a3)),
        ("planes.conv32_dgrad.y", lambda: lc.conv32_dgrad(w32, a3, a2)),
        ("planes.convup_wgrad.x0", lambda: lb.convup_wgrad(s3, a2, a2, a2)),
        ("planes.convup_wgrad.x1", lambda: lb.convup_wgrad(s4, a3, a2, a2)),
        ("planes.convup_wgrad.g1", lambda: lb.convup_wgrad(s4, a2, a3, a2)),
        ("planes.convup_dgrad.g1", lambda: lb.convup_dgrad(w96, sw, a3, a2)),
        ("planes.convup_dgrad.gd", lambda: lb.convup_dgrad(w96, sw, a2, a3)),
        ("planes.convn_wgrad.x", lambda: dc.convn_wgrad(a3, a2, a2)),
        ("planes.convn_wgrad.upstream", lambda: dc.convn_wgrad(a2, None, a3)),
        ("planes.convn_dgrad.upstream", lambda: dc.convn_dgrad(w32, None, a3)),
        ("planes.convupn_wgrad.x0", lambda: db.convupn_wgrad(s3, a2, a2, a2)),
        ("planes.convupn_wgrad.x1", lambda: db.convupn_wgrad(s4, a3, a2, a2)),
        ("planes.convupn_wgrad.gd", lambda: db.convupn_wgrad(s4, a2, a2, a3)),
        # wrong plane count, layers
        ("planes.LastConv.t", lambda: LastConv.from_model(model)(a3, a3)),
        ("planes.LastConv.res", lambda: LastConv.from_model(model)(a2, a4)),
        ("planes.TailNorms.z1", lambda: TailNorms.from_model(model)(a3, a3)),
        ("planes.TailNorms.zd", lambda: TailNorms.from_model(model)(a2, a4)),
        ("planes.TailConvs.x0", lambda: TailConvs.from_model(model)(s3, a2)),
        ("planes.TailConvs.x0.128", lambda: TailConvs.from_model(model)(s8, a2)),
        ("planes.TailConvs.x1", lambda: TailConvs.from_model(model)(s4, a4)),
        ("planes.LastBlock.x1", lambda: LastBlock.from_model(model)(s4, a3)),
        ("planes.Dec2Conv.t", lambda: Dec2Conv.from_model(model)(a2, a2)),
        ("planes.Dec2Conv.t.48", lambda: Dec2Conv.from_model(model)(a3, a3)),
        ("planes.Dec2Conv.res", lambda: Dec2Conv.from_model(model)(a4, a2)),
        ("planes.Dec2Norms.z1", lambda: Dec2Norms.from_model(model)(a2, a2)),
        ("planes.Dec2Norms.zd", lambda: Dec2Norms.from_model(model)(a4, a2)),
        ("planes.Dec2Convs.x0", lambda: Dec2Convs.from_model(model)(s4, a4)),
        ("planes.Dec2Convs.x1", lambda: Dec2Convs.from_model(model)(s8, a2)),
        ("planes.Dec2Convs.x0.48", lambda: Dec2Convs.from_model(model)(s3, a4)),
        ("planes.Dec2Block.x1", lambda: Dec2Block.from_model(model)(s8, a3)),
        # mismatched .lw
        ("lw.conv32_wgrad.y", lambda: lc.conv32_wgrad(a2, narrow, a2)),
        ("lw.conv32_wgrad.upstream", lambda: lc.conv32_wgrad(a2, a2, narrow)),
        ("lw.conv32_dgrad.y", lambda: lc.conv32_dgrad(w32, narrow, a2)),
        ("lw.convup_wgrad.x0", lambda: lb.convup_wgrad(c16(4, H=2, W=3, lw=2), a2, a2, a2)),
        ("lw.convup_wgrad.g1", lambda: lb.convup_wgrad(s4, a2, narrow, a2)),
        ("lw.convup_dgrad.gd", lambda: lb.convup_dgrad(w96, sw, a2, narrow)),
        ("lw.convn_wgrad.y", lambda: dc.convn_wgrad(a4, narrow, a2)),
        ("lw.convn_wgrad.upstream", lambda: dc.convn_wgrad(a4, None, narrow)),
        ("lw.convn_dgrad.y", lambda: dc.convn_dgrad(w32, narrow, a2)),
        ("lw.convupn_wgrad.x0", lambda: db.convupn_wgrad(c16(8, H=2, W=3, lw=2), a4, a4, a4)),
        ("lw.convupn_wgrad.gd", lambda: db.convupn_wgrad(s8, a4, a4, c16(4, lw=5))),
        ("lw.LastConv.res", lambda: LastConv.from_model(model)(a2, narrow)),
        ("lw.TailNorms.zd", lambda: TailNorms.from_model(model)(a2, narrow)),
        ("lw.TailConvs.x0", lambda: TailConvs.from_model(model)(c16(4, H=2, W=3, lw=2), a2)),
        ("lw.Dec2Conv.res", lambda: Dec2Conv.from_model(model)(a4, c16(4, lw=5))),
        ("lw.Dec2Norms.zd", lambda: Dec2Norms.from_model(model)(a4, c16(4, lw=5))),
        ("lw.Dec2Convs.x0", lambda: Dec2Convs.from_model(model)(c16(8, H=2, W=3, lw=2), a4)),
        ("lw.outside", lambda: lc.conv32_wgrad(c16(2, lw=7), a2, a2)),
        # a 64-channel tensor into the 32-channel names
        ("c64.conv32_wgrad.x", lambda: lc.conv32_wgrad(a4, a2, a2)),
        ("c64.conv32_wgrad.all", lambda: lc.conv32_wgrad(a4, a4, a4)),
        ("c64.conv32_dgrad.weight", lambda: lc.conv32_dgrad(w64x32, None, a2)),
        ("c64.conv32_dgrad.weight64", lambda: lc.conv32_dgrad(w64, None, a4)),
        ("c64.conv32_dgrad.upstream", lambda: lc.conv32_dgrad(w32, None, a4)),
        ("c64.convup_wgrad.x1", lambda: lb.convup_wgrad(s8, a4, a4, a4)),
        ("c64.convup_wgrad.g1", lambda: lb.convup_wgrad(s4, a2, a4, a2)),
        ("c64.convup_dgrad.g1", lambda: lb.convup_dgrad(w96, sw, a4, a4)),
        ("c64.convup_dgrad.weight", lambda: lb.convup_dgrad(torch.zeros(64, 192, 3, 3, 3, device=DEV), sw, a2, a2)),
        # sources that require grad
        ("grad.Dec2Convs.x0", lambda: Dec2Convs.from_model(model)(req(s8), a4)),
        ("grad.Dec2Convs.x1", lambda: Dec2Convs.from_model(model)(s8, req(a4))),
        ("grad.Dec2Block.x0", lambda: Dec2Block.from_model(model)(req(s8), a4)),
        ("grad.TailConvs.x0", lambda: TailConvs.from_model(model)(req(s4), a2)),
        ("grad.TailConvs.x1", lambda: TailConvs.from_model(model)(s4, req(a2))),
        # a layer built without a model
        ("nomodel.LastConv", lambda: LastConv().to(DEV)(a2, a2)),
        ("nomodel.TailConvs", lambda: TailConvs().to(DEV)(s4, a2)),
        ("nomodel.Dec2Conv", lambda: Dec2Conv().to(DEV)(a4, a4)),
        ("nomodel.Dec2Convs", lambda: Dec2Convs().to(DEV)(s8, a4)),
        # out holds a key that is not wanted; other argument checks of the shared prologue
        ("out.conv32_wgrad", lambda: lc.conv32_wgrad(a2, a2, a2, want=("shift",), out={"weight": w32})),
        ("out.conv32_dgrad", lambda: lc.conv32_dgrad(w32, a2, a2, want=("x",), out={"res": c16(2)})),
        ("out.convup_wgrad", lambda: lb.convup_wgrad(s4, a2, a2, a2, want=("weight",), out={"short": sw})),
        ("out.convup_dgrad", lambda: lb.convup_dgrad(w96, sw, a2, a2, want=("x1",), out={"x0": c16(4, H=2, W=3)})),
        ("out.convn_wgrad", lambda: dc.convn_wgrad(a4, a2, a2, want=("shift",), out={"weight": w32})),
        ("out.convn_dgrad", lambda: dc.convn_dgrad(w32, a2, a2, want=("x",), out={"res": c16(2)})),
        ("out.convupn_wgrad", lambda: db.convupn_wgrad(s8, a4, a4, a4, want=("weight",), out={"short": sw})),
        ("elements.conv32_wgrad", lambda: lc.conv32_wgrad(a2, a2, a2, out={"shift": torch.zeros(31, device=DEV)})),
        ("elements.convup_wgrad", lambda: lb.convup_wgrad(s4, a2, a2, a2, out={"short": torch.zeros(32, 95, device=DEV)})),
        ("shape.conv32_dgrad.out", lambda: lc.conv32_dgrad(w32, a2, a2, out={"x": c16(2, W=7)})),
        ("shape.convn_dgrad.out", lambda: dc.convn_dgrad(w64x32, a4, a4, out={"x": c16(4)})),
        ("shape.convup_dgrad.x0", lambda: lb.convup_dgrad(w96, sw, a2, a2, out={"x0": c16(4, H=2, W=2)})),
        ("overlap.conv32_dgrad", lambda: lc.conv32_dgrad(w32, a2, a2, want=("res",), out={"res": a2})),
        ("want.conv32_wgrad", lambda: lc.conv32_wgrad(a2, a2, a2, want=("weight", "bias"))),
        ("want.convup_dgrad", lambda: lb.convup_dgrad(w96, sw, a2, a2, want=())),
        ("cap.convn_dgrad", lambda: dc.convn_dgrad(w32, a2, a2, max_workgroups=-1)),
        ("needs.convup_wgrad.g1", lambda: lb.convup_wgrad(s4, a2, None, a2)),
        ("needs.convupn_wgrad.gd", lambda: db.convupn_wgrad(s8, a4, a4, None)),
        ("weight.convn_dgrad", lambda: dc.convn_dgrad(torch.zeros(32, 48, 3, 3, 3, device=DEV), None, a2)),
        ("weight.convup_dgrad.short", lambda: lb.convup_dgrad(w96, torch.zeros(32, 95, device=DEV), a2, a2)),
        ("upsample.convup_wgrad", lambda: lb.convup_wgrad(c16(4, H=3, W=3), a2, a2, a2)),
        ("upsample.Dec2Convs", lambda: Dec2Convs.from_model(model)(c16(8, H=3, W=3), a4)),
    ]
    return calls


def write(out_path, values, errors):
    """One line per group of values (``A.f32.b2_l3_5x7`` ...: the key's first three parts) and per error label."""
    groups = {}
    for k in sorted(values):
        *head, rest = k.split(".", 3)
        head = ".".join(head)
        groups.setdefault(head, {})[rest] = values[k]
    rows = lambda d: ",\n".join(f"  {json.dumps(k)}: {json.dumps(d[k], sort_keys=True)}" for k in sorted(d))
    with open(out_path, "w") as f:
        f.write(f'{{"torch": {json.dumps(torch.__version__)},\n "values": {{\n{rows(groups)}\n }},\n'
                f' "errors": {{\n{rows(errors)}\n }}}}\n')


def read(path):
    """-> (torch version, {key: value} with the groups' keys joined again, {label: [type, message]})."""
    with open(path) as f:
        d = json.load(f)
    return d["torch"], {f"{g}.{k}": v for g, rows in d["values"].items() for k, v in rows.items()}, d["errors"]


def main(out_path):
    values, errors = {}, {}
    for precision in ("f32", "f16x2"):
        for case in CASES:
            tag = f"{precision}.{case}"
            group_a(values, tag, make_model(precision), case)
            group_b(values, tag, make_model(precision), case)
            group_c(values, precision, case)
            print(f"{tag}: {len(values)} values", flush=True)
    for case in CASES:
        group_b_dgrad(values, case)
    for label, call in bad_calls(make_model("f32")):
        try:
            call()
            errors[label] = ["none", ""]
        except Exception as e:  # noqa: BLE001 -- the record is of whatever the call raises
            errors[label] = [type(e).__name__, str(e)]
    torch.cuda.synchronize()
    write(out_path, values, errors)
    print(f"{len(values)} values, {len(errors)} error records -> {out_path}")


if __name__ == "__main__":
    main(sys.argv[1])
