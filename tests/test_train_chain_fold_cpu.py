"""The fold of the seven ``finetune.fit_*`` into one stage table and one loop, and of ``V2ce3d``'s stop ladder into one stop
table, without a GPU.

Values.  ``tools/train_chain_digests.py`` ran on the parent commit and on the folded tree, on one MI355X with one torch, in
one session; ``profiles/r26_a_chain_parent.json`` and ``profiles/r26_b_chain_folded.json`` are its two outputs.  Every value
and every error record (type and message) is equal, key for key: nothing is reworded.

Compatibility.  The ``*_GROUPS`` tuples, the signatures of the seven fits and the eight accessors and the ``--train``
choices are the literals written down from the parent."""
import hashlib
import inspect
import json
import os

import pytest

from v2ce_toolbox_amd import finetune
from v2ce_toolbox_amd.v2ce_3d import V2ce3d

PROFILES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles")
PRECISIONS, CASES = ("f32", "f16x2"), ("b2_l3_5x7", "b1_l2_3x70")
FITS = ("fit_head", "fit_tail", "fit_tail_norms", "fit_last_block", "fit_dec2_conv", "fit_dec2_block", "fit_dec1_conv")
STAGE_NAMES = ("head", "tail", "tail_norms", "last_block", "dec2_conv", "dec2_block", "dec1_conv")
ACCESSORS = ("forward_features", "forward_tail_inputs", "forward_tail_normed", "forward_tail_sources", "forward_dec2_inputs",
             "forward_dec2_normed", "forward_dec2_sources", "forward_dec1_inputs")
# written down from the parent
TAIL = ("pred", "conv2", "bn2")
TAIL_NORM = TAIL + ("bn1", "bnd")
LAST_BLOCK = TAIL_NORM + ("conv1", "convd")
DEC2_CONV = LAST_BLOCK + ("dec2_conv2", "dec2_bn2")
DEC2_BLOCK = DEC2_CONV + ("dec2_conv1", "dec2_convd", "dec2_bn1", "dec2_bnd")
DEC1_CONV = DEC2_BLOCK + ("dec1_conv2", "dec1_bn2")
GROUPS = {"fit_tail": TAIL, "fit_tail_norms": TAIL_NORM, "fit_last_block": LAST_BLOCK, "fit_dec2_conv": DEC2_CONV,
          "fit_dec2_block": DEC2_BLOCK, "fit_dec1_conv": DEC1_CONV}
ADDED = (("pred",), ("conv2", "bn2"), ("bn1", "bnd"), ("conv1", "convd"), ("dec2_conv2", "dec2_bn2"),
         ("dec2_conv1", "dec2_convd", "dec2_bn1", "dec2_bnd"), ("dec1_conv2", "dec1_bn2"))
REST = ("loss: 'Sequence[str]' = ('pyramid', 'ef', 'ef_splitp', 'compensation'), steps: 'int', lr: 'float', optimizer: 'str' = 'adam', "
        "cache_bytes: 'int' = 8589934592, **loss_options) -> 'List[dict]'")


def text_digest(value):
    """The tool's digest of a history or of a list of names, as it writes digests: the first 128 bits."""
    return hashlib.sha256(json.dumps(value, sort_keys=True).encode()).hexdigest()[:32]


def load(name):
    """The tool's file with its one-line groups of values flattened again: {group: {rest: v}} -> {group.rest: v}."""
    with open(os.path.join(PROFILES, name)) as f:
        d = json.load(f)
    d["values"] = {f"{g}.{k}": v for g, rows in d["values"].items() for k, v in rows.items()}
    return d


@pytest.fixture(scope="module")
def records():
    return load("r26_a_chain_parent.json"), load("r26_b_chain_folded.json")


def test_every_value_and_every_error_record_of_the_folded_tree_is_the_parents(records):
    parent, folded = records
    assert parent["torch"] == folded["torch"]                    # the digests belong to one machine and one torch
    a, b = parent["values"], folded["values"]
    assert set(a) == set(b) and len(a) == 900
    assert [k for k in a if a[k] != b[k]] == []
    ea, eb = parent["errors"], folded["errors"]
    assert set(ea) == set(eb) and len(ea) == 63
    assert [k for k in ea if ea[k] != eb[k]] == []                # type and message: nothing is reworded
    assert all(v[0] != "none" for v in ea.values())              # every bad call of the list is refused


def test_the_record_covers_what_it_claims(records):
    a, errors = records[0]["values"], records[0]["errors"]
    for precision in PRECISIONS:
        for case in CASES:
            tag = f"{precision}.{case}"
            for fit in FITS:
                assert len(a[f"F.{tag}.{fit}.history"]) == 2 and len(a[f"F.{tag}.{fit}.state"]) == 32
                assert a[f"F.{tag}.{fit}.lengths"] == [2, len(a[f"F.{tag}.{fit}.changed"])]
                assert a[f"F.{tag}.{fit}.calls"] == [0, 0]
            assert a[f"F.{tag}.fit_head.changed"] == ["UNet.pred.conv3d.bias", "UNet.pred.conv3d.weight"]
            deep, shallow = set(a[f"F.{tag}.fit_dec1_conv.changed"]), set(a[f"F.{tag}.fit_dec2_block.changed"])
            assert deep > shallow and (len(deep), len(shallow)) == (35, 30)
            for fit in FITS[1:]:                                  # depth selection: the shallower tuple trains no deeper layer
                assert a[f"G.{tag}.{fit}.own.lengths"][0] == 2 and 0 < a[f"G.{tag}.{fit}.own.lengths"][1] <= len(a[f"F.{tag}.{fit}.changed"])
                below = FITS[FITS.index(fit) - 1]
                assert a[f"G.{tag}.{fit}.shallower.state"] == a[f"F.{tag}.{below}.state"]
                assert a[f"G.{tag}.{fit}.shallower.history"] == text_digest(a[f"F.{tag}.{below}.history"])
                assert a[f"G.{tag}.{fit}.shallower.changed"] == text_digest(a[f"F.{tag}.{below}.changed"])
            for fit in ("fit_dec1_conv", "fit_tail"):
                assert a[f"H.{tag}.{fit}.lengths"] == [3, len(a[f"F.{tag}.{fit}.changed"])]
            for acc in ACCESSORS:
                key = f"I.{tag}.{acc}"
                assert a[f"{key}.calls_delta"] == 1 and a[f"{key}.model_before"] == a[f"{key}.model_after"]
                assert (a[f"{key}.out0.absmax"] is not None) == (precision == "f16x2")
                if precision == "f32":
                    assert all(a[f"{key}.out{j}.absmax"] is None for j in range(a[f"{key}.count"]))
            assert [a[f"I.{tag}.{acc}.count"] for acc in ACCESSORS] == [1, 2, 2, 2, 3, 3, 3, 4]
    assert not any(k.endswith(".error") for k in a)               # the parent refuses none of the cases at any depth
    assert errors["fit_tail.train_and_loss"][1].startswith("train must be")          # train is checked in front of loss
    assert errors["fit_dec1_conv.train_name"][1] == f"train must be a non-empty subset of {DEC1_CONV}, got ('pred', 'nope')"
    assert errors["fit_head.train_name"] == ["TypeError", "calculate_loss() got an unexpected keyword argument 'train'"]


def test_groups_signatures_and_choices_are_the_parents():
    assert (finetune.TAIL_GROUPS, finetune.TAIL_NORM_GROUPS, finetune.LAST_BLOCK_GROUPS) == (TAIL, TAIL_NORM, LAST_BLOCK)
    assert (finetune.DEC2_CONV_GROUPS, finetune.DEC2_BLOCK_GROUPS, finetune.DEC1_CONV_GROUPS) == (DEC2_CONV, DEC2_BLOCK, DEC1_CONV)
    assert str(inspect.signature(finetune.fit_head)) == "(model, image_units, gt_voxels, *, " + REST
    for fit, groups in GROUPS.items():
        assert str(inspect.signature(getattr(finetune, fit))) == \
            f"(model, image_units, gt_voxels, *, train: 'Sequence[str]' = {groups}, " + REST, fit
    assert str(inspect.signature(V2ce3d.forward_features)) == "(self, x: 'torch.Tensor') -> 'torch.Tensor'"
    for acc in ACCESSORS[1:]:
        assert str(inspect.signature(getattr(V2ce3d, acc))) == "(self, x: 'torch.Tensor')", acc
    train = [action for action in finetune.build_parser()._actions if action.dest == "train"][0]
    assert tuple(train.choices) == ("head", "tail", "tail_norms", "last_block", "dec2_conv2", "dec2_block", "dec1_conv2")
    assert train.default == "head" and all(f"({fit})" in train.help for fit in FITS)


def test_the_stage_table_and_the_depth_of_a_train_tuple():
    assert tuple(stage.name for stage in finetune.STAGES) == STAGE_NAMES
    assert tuple(tuple(stage.groups) for stage in finetune.STAGES) == ADDED
    assert all(callable(getattr(finetune, "fit_" + stage.name)) and hasattr(V2ce3d, stage.accessor) for stage in finetune.STAGES)
    # the layer classes per depth: separate layers up to the last block, then LastBlock; Dec2Block, and Dec2BlockThrough under dec1
    assert [tuple(path for _, path in stage.layers) for stage in finetune.STAGES] == [
        (), ("last_conv.LastConv",), ("last_conv.LastConv", "last_conv.TailNorms"),
        ("last_conv.LastConv", "last_conv.TailNorms", "last_block.TailConvs"), ("last_block.LastBlock", "dec2_conv.Dec2Conv"),
        ("last_block.LastBlock", "dec2_block.Dec2Block"), ("last_block.LastBlock", "dec2_block.Dec2BlockThrough", "dec1_conv.Dec1Conv")]
    depth = lambda train, allowed=DEC1_CONV: finetune.STAGES[finetune._depth(train, allowed)].name
    for name, added in zip(STAGE_NAMES, ADDED):
        assert all(depth((g,)) == name for g in added)
    assert [depth(groups, groups) for groups in GROUPS.values()] == list(STAGE_NAMES[1:])
    assert depth(("pred",)) == "head" and depth(("pred", "dec1_bn2")) == "dec1_conv" and depth(("bn1", "pred"), TAIL_NORM) == "tail_norms"
    for bad in (("dec2_bn2",), ("pred", "pred"), ()):
        with pytest.raises(ValueError) as e:
            finetune._depth(bad, LAST_BLOCK)
        assert str(e.value) == f"train must be a non-empty subset of {LAST_BLOCK}, got {bad}"


def test_one_block_inputs_and_the_stop_table():
    assert not hasattr(V2ce3d, "_block_inputs_unfused") and hasattr(V2ce3d, "_block_inputs")
    assert V2ce3d.STOPS == {"tail": (1, "inputs"), "normed": (1, "normed"), "sources": (1, "sources"), "dec2": (2, "inputs"),
                            "dec2_normed": (2, "normed"), "dec2_sources": (2, "sources"), "dec1": (3, "inputs")}
