"""The fold of the last_* and dec2_* training layers into one decoder block (conv_grads.py, decoder_block.py; DESIGN.md
4.8q), without a GPU.

Values.  ``tools/train_layer_digests.py`` ran on the parent commit and on the folded tree, on one MI355X with one torch;
``profiles/r23_a_layers_parent.json`` and ``profiles/r23_b_layers_folded.json`` are its two outputs.  Every value digest is
equal key for key.  The error records name the same exception type for every bad call, and the same message except for the
labels of ``REWORDED``, each of which must carry the documented form of DESIGN.md 4.8q.

Compatibility.  The eight classes, built without a model, have the parameter names, the ``state_dict`` keys and the shapes
written down from the parent, and the four modules keep the names their users import."""
import json
import os

import pytest

from v2ce_toolbox_amd import dec2_block, dec2_conv, last_block, last_conv

PROFILES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles")

SHARED = "channels-last-16 [b, l, c / 16, h, pitch, 16] with c in "
# label of the error record -> a fragment of the documented new message ("Reworded messages")
REWORDED = {
    # (a) the shape checks [b, l, 2, ...], [b, l, 4, h0, pitch0, 16] and [b, l, 2 or 4, ...] are the shared one
    **{k: SHARED + "(32,)" for k in (
        "c64.conv32_dgrad.upstream", "c64.conv32_dgrad.weight64", "c64.conv32_wgrad.all", "c64.conv32_wgrad.x",
        "c64.convup_dgrad.g1", "c64.convup_wgrad.g1", "c64.convup_wgrad.x1", "planes.TailNorms.z1", "planes.TailNorms.zd",
        "planes.conv32_dgrad.upstream", "planes.conv32_dgrad.y", "planes.conv32_wgrad.upstream", "planes.conv32_wgrad.x",
        "planes.convup_dgrad.g1", "planes.convup_dgrad.gd", "planes.convup_wgrad.g1", "planes.convup_wgrad.x1")},
    "planes.convup_wgrad.x0": SHARED + "(64,)",
    "planes.TailConvs.x0": SHARED + "(64, 128)",
    **{k: SHARED + "(32, 64)" for k in (
        "planes.LastBlock.x1", "planes.LastConv.t", "planes.Dec2Conv.t.48", "planes.convn_dgrad.upstream",
        "planes.convn_wgrad.upstream", "planes.convn_wgrad.x")},
    # (b) the 32-channel layers check the channel counts as the 64-channel layers do
    "planes.LastConv.res": "must match t",
    "planes.TailConvs.x0.128": "x0 must have 64 channels and x1 32",
    "planes.TailConvs.x1": "x0 must have 64 channels and x1 32",
    "lw.TailConvs.x0": "h0 = (h + 1) // 2 = 2 and lw = 3",
    # (c) the 32-channel entries speak the N-channel bodies' words
    "lw.conv32_wgrad.y": "must match upstream",
    "lw.conv32_wgrad.upstream": "must match upstream",
    "lw.convup_wgrad.g1": "must match x1 (1, 2, 2, 4, 6, 16) (lw 6) but for the planes",
    "c64.conv32_dgrad.weight": "weight must be [32, 32, 3, 3, 3] (upstream has 32 channels)",
}


def load(name):
    """The tool's file with its one-line groups of values flattened again: {group: {rest: v}} -> {group.rest: v}."""
    with open(os.path.join(PROFILES, name)) as f:
        d = json.load(f)
    d["values"] = {f"{g}.{k}": v for g, rows in d["values"].items() for k, v in rows.items()}
    return d


@pytest.fixture(scope="module")
def records():
    return load("r23_a_layers_parent.json"), load("r23_b_layers_folded.json")


def test_every_value_digest_of_the_folded_tree_is_the_parents(records):
    parent, folded = records
    assert parent["torch"] == folded["torch"]                    # the digests belong to one machine and one torch
    a, b = parent["values"], folded["values"]
    assert set(a) == set(b) and len(a) == 896
    assert [k for k in a if a[k] != b[k]] == []
    # what the record covers: both precisions, both cases, the three groups, range slots, gradients of the inputs
    for precision in ("f32", "f16x2"):
        for case in ("b2_l3_5x7", "b1_l2_3x70"):
            tag = f"{precision}.{case}"
            assert a[f"A.{tag}.x1.grad"] and a[f"A.{tag}.dec2.convs.weight_bar.grad"] and a[f"A.{tag}.fwd.last.conv.weight_u"]
            assert a[f"B.{tag}.conv.grad.t.grad"] and a[f"B.{tag}.conv.nograd.t.grad"] is None
            assert (a[f"A.{tag}.x0.absmax"] is not None) == (precision == "f16x2")
            assert (a[f"A.{tag}.feat.absmax"] is not None) == (precision == "f16x2")     # LastConv's output carries one too
            for fit in ("fit_tail", "fit_tail_norms", "fit_last_block", "fit_dec2_conv", "fit_dec2_block"):
                assert len(a[f"C.{tag}.{fit}.history"]) == 2 and len(a[f"C.{tag}.{fit}.state"]) == 64
            assert len(a[f"C.{tag}.fit_dec2_block.changed"]) == 30 and len(a[f"C.{tag}.fit_tail.changed"]) == 7
    assert a["B.dgrad.b1_l2_3x70.cap3.x0.g1none.x0"] and a["B.dgrad.b2_l3_5x7.cap0.x0+x1.both.x1"]


def test_the_error_records_differ_in_the_documented_messages_only(records):
    parent, folded = records
    a, b = parent["errors"], folded["errors"]
    assert set(a) == set(b) and len(a) >= 90
    assert all(v[0] != "none" for v in a.values())                # every bad call of the list is refused
    assert {k for k in a if a[k][0] != b[k][0]} == set()          # exception types stay
    assert {k for k in a if a[k][1] != b[k][1]} == set(REWORDED)
    for k, form in REWORDED.items():
        assert form in b[k][1] and form not in a[k][1], k
    # a message changed only where a 32-channel check (or the N-channel '2 or 4' plane check) became the shared one
    assert all("Dec2" not in k and "convn" not in k and "convupn" not in k or "2 or 4" in a[k][1] for k in REWORDED)


PARAMS2, BUFS2 = ["weight_bar", "bn_weight", "bn_bias"], ["weight_u", "weight_v", "running_mean", "running_var", "eps", "guard"]
PARAMS1 = ["weight_bar", "short_weight", "short_bias"]
BUFS1 = ["weight_u", "weight_v", "bn1_mean", "bn1_var", "bnd_mean", "bnd_var", "eps", "guard"]
NORMS = ["bn1_weight", "bn1_bias", "bnd_weight", "bnd_bias"]


def conv2_shapes(c):
    return [(c, c, 3, 3, 3), (c,), (c,), (c,), (c * 27,), (c,), (c,), (), (1,)]


def conv1_shapes(c, cin):
    return [(c, cin, 3, 3, 3), (c, cin, 1, 1, 1), (c,), (c,), (cin * 27,), (c,), (c,), (c,), (c,), (), (1,)]


LAYERS = [
    (last_conv.LastConv, PARAMS2, PARAMS2 + BUFS2, conv2_shapes(32)),
    (dec2_conv.Dec2Conv, PARAMS2, PARAMS2 + BUFS2, conv2_shapes(64)),
    (last_block.TailConvs, PARAMS1, PARAMS1 + BUFS1, conv1_shapes(32, 96)),
    (dec2_block.Dec2Convs, PARAMS1, PARAMS1 + BUFS1, conv1_shapes(64, 192)),
    (last_conv.TailNorms, NORMS, NORMS, [(32,)] * 4),
    (dec2_block.Dec2Norms, NORMS, NORMS, [(64,)] * 4),
]


@pytest.mark.parametrize("cls,params,keys,shapes", LAYERS, ids=[c[0].__name__ for c in LAYERS])
def test_state_dict_and_parameter_names_are_the_parents(cls, params, keys, shapes):
    layer = cls()
    assert [n for n, _ in layer.named_parameters()] == params
    sd = layer.state_dict()
    assert list(sd) == keys and [tuple(v.shape) for v in sd.values()] == shapes
    assert all(p.requires_grad for p in layer.parameters())


def test_blocks_and_module_level_names():
    for cls, convs, norms, conv in ((last_block.LastBlock, last_block.TailConvs, last_conv.TailNorms, last_conv.LastConv),
                                    (dec2_block.Dec2Block, dec2_block.Dec2Convs, dec2_block.Dec2Norms, dec2_conv.Dec2Conv)):
        block = cls(convs(), norms(), conv())
        want = [f"convs.{k}" for k in PARAMS1 + BUFS1] + [f"norms.{k}" for k in NORMS] + [f"conv.{k}" for k in PARAMS2 + BUFS2]
        assert list(block.state_dict()) == want and len(list(block.parameters())) == 10
    assert [n for n, _ in last_block.TailConvs(bias=False).named_parameters()] == ["weight_bar", "short_weight"]
    assert last_block.TailConvs(input_grads=True).input_grads and not last_block.TailConvs().input_grads
    with pytest.raises(ValueError, match="no gradient with respect to x0 and x1"):
        dec2_block.Dec2Convs(input_grads=True)
    for mod, names in ((last_conv, ("conv32_wgrad", "conv32_dgrad", "LastConv", "TailNorms", "WANT", "DGRAD_WANT", "_planar_pitched")),
                       (last_block, ("convup_wgrad", "convup_dgrad", "TailConvs", "LastBlock", "WANT", "DGRAD_WANT", "_SHAPES")),
                       (dec2_conv, ("convn_wgrad", "convn_dgrad", "Dec2Conv", "WANT", "DGRAD_WANT")),
                       (dec2_block, ("convupn_wgrad", "Dec2Convs", "Dec2Norms", "Dec2Block", "WANT"))):
        assert all(hasattr(mod, n) for n in names), mod.__name__
    assert last_conv.WANT == dec2_conv.WANT == ("weight", "shift") and last_conv.DGRAD_WANT == dec2_conv.DGRAD_WANT == ("x", "res")
    assert last_block.WANT == dec2_block.WANT == ("weight", "short", "short_bias") and last_block.DGRAD_WANT == ("x0", "x1")
    assert last_block._SHAPES == {"weight": (32, 96, 3, 3, 3), "short": (32, 96), "short_bias": (32,)}
    assert (last_conv.C, last_block.C, last_block.C0, last_block.C1, last_block.CIN) == (32, 32, 64, 32, 96)
    assert (dec2_conv.C, dec2_block.C, dec2_block.C0, dec2_block.C1, dec2_block.CIN) == (64, 64, 128, 64, 192)


def test_the_32_channel_names_keep_their_own_c_entries():
    from v2ce_toolbox_amd import conv_grads as G
    assert (G._CONV32_WGRAD.symbol, G._CONV32_DGRAD.symbol, G._CONVUP_WGRAD.symbol) == \
        ("v2ce_conv32_wgrad", "v2ce_conv32_dgrad", "v2ce_convup_wgrad")
    assert not (G._CONV32_WGRAD.pass_channels or G._CONV32_DGRAD.pass_channels or G._CONVUP_WGRAD.pass_channels)
    assert G._CONV32_WGRAD.channels == G._CONV32_DGRAD.channels == ((32,), (32,)) and G._CONVUP_WGRAD.channels == ((64,), (32,), (32,))
    assert last_conv.conv32_wgrad is G.conv32_wgrad and last_block.convup_wgrad is G.convup_wgrad
    assert dec2_conv.convn_wgrad is G.convn_wgrad and dec2_block.convupn_wgrad is G.convupn_wgrad
