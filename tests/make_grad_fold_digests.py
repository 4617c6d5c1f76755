"""Recipe of tests/golden/.gradfold/digests.json: sha256 digests of the bytes that the 32-channel gradient entries
(last_conv.conv32_wgrad / conv32_dgrad, last_block.convup_wgrad) gave while they still had kernels of their own, next to the
N-channel entries (dec2_conv.convn_wgrad / convn_dgrad at 32 -> 32, dec2_block.convupn_wgrad at 64 + 32 -> 32).  Since the
32-channel entries forward to the N-channel kernels, a comparison of the two would compare a kernel with itself; the digests
keep tests/test_gpu_convngrad.py::test_32_to_32_gives_the_bytes_of_the_32_channel_entries and
tests/test_gpu_convupngrad.py::test_64_32_32_gives_the_bytes_of_the_older_entry tied to the bytes of the separate kernels.

The kernels have no atomics and a fixed order of summation, so the digests are a property of the code, not of the GPU that
ran it.  Each entry is the sha256 of the contiguous f32 bytes of one output (the channels-last-16 outputs with their padding
columns):

  conv32/NAME/capK/{weight,shift,x,res}   the inputs t, y, upstream of tests/golden/.lastconv/NAME.npz and the seeded weight
                                          of conv32_weight(), max_workgroups = K in CONV32_CAPS.  Cap 1 puts all 60 tiles
                                          of b1_l3_20x70 into one workgroup: the f32 chain (32 tiles) flushes in mid-walk
  conv32/NAME/plain/{weight,shift}        y = None at the default grid
  convup/NAME/capK/{weight,short,short_bias}   the inputs x0, x1, g1, gd of tests/golden/.lastblock/NAME*.npz, K in CONVUP_CAPS
  convup/NAME/short_only/{short,short_bias}    want = ("short", "short_bias"), g1 = None

The maker asserts that the N-channel entries give the same digests before it writes.  It needs the GPU and was run once, at
the last commit at which the 32-channel entries had kernel files of their own; not collected by pytest.

    python tests/make_grad_fold_digests.py [out_file]   (default tests/golden/.gradfold/digests.json)
"""
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import last_block_ref as LR  # noqa: E402
from tests import last_conv_ref as CR  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", ".gradfold", "digests.json")
CASES = ("b2_l3_5x7", "b1_l2_3x70", "b1_l3_20x70")
CONV32_CAPS = (0, 3, 1)
CONVUP_CAPS = (0, 3, 7)
CONVUP_KEYS = ("weight", "short", "short_bias")
DEV = "cuda"


def digest(t):
    a = t.detach().contiguous().cpu().numpy()
    assert a.dtype.name == "float32", a.dtype
    return hashlib.sha256(a.tobytes()).hexdigest()


def conv32_inputs(name):
    """-> x, y, upstream as channels-last-16 at the activation pitch, and the seeded weight [32, 32, 3, 3, 3]."""
    c = CR.load_case(name)
    W = c["t"].shape[4]
    x, y, up = (torch.from_numpy(CR.to_c16(c[k], CR.pitch_of(W))).to(DEV) for k in ("t", "y", "upstream"))
    for a in (x, y, up):
        a.lw, a.c16 = W, True
    gen = torch.Generator().manual_seed(5)
    w = (torch.randn((32, 32, 3, 3, 3), generator=gen) * 0.1).to(DEV)
    return x, y, up, w


def convup_inputs(name):
    """-> x0 at the source pitch and x1, g1, gd at the activation pitch, channels-last-16."""
    z = LR.load_case(name)
    W = z["x1"].shape[-1]
    x0 = torch.from_numpy(LR.src_to_c16(z["x0"], LR.pitch_of((W + 1) // 2))).to(DEV)
    x0.lw, x0.c16 = (W + 1) // 2, True
    rest = []
    for k in ("x1", "g1", "gd"):
        a = torch.from_numpy(LR.to_c16(z[k], LR.pitch_of(W))).to(DEV)
        a.lw, a.c16 = W, True
        rest.append(a)
    return (x0, *rest)


def conv32_outputs(name, wgrad, dgrad):
    """Every recorded output of one case through the entries `wgrad`, `dgrad` -> {key: tensor}."""
    x, y, up, w = conv32_inputs(name)
    out = {}
    for cap in CONV32_CAPS:
        g = dict(wgrad(x, y, up, max_workgroups=cap))
        g.update(dgrad(w, y, up, max_workgroups=cap))
        assert set(g) == {"weight", "shift", "x", "res"}, sorted(g)
        out.update({f"conv32/{name}/cap{cap}/{k}": v for k, v in g.items()})
    plain = wgrad(x, None, up)
    out.update({f"conv32/{name}/plain/{k}": plain[k] for k in ("weight", "shift")})
    torch.cuda.synchronize()
    return out


def convup_outputs(name, wgrad):
    x0, x1, g1, gd = convup_inputs(name)
    out = {}
    for cap in CONVUP_CAPS:
        g = wgrad(x0, x1, g1, gd, max_workgroups=cap)
        assert set(g) == set(CONVUP_KEYS), sorted(g)
        out.update({f"convup/{name}/cap{cap}/{k}": v for k, v in g.items()})
    short = wgrad(x0, x1, None, gd, want=("short", "short_bias"))
    out.update({f"convup/{name}/short_only/{k}": short[k] for k in ("short", "short_bias")})
    torch.cuda.synchronize()
    return out


def load():
    with open(PATH) as f:
        return json.load(f)


def main(path):
    from v2ce_toolbox_amd import dec2_block, dec2_conv, last_block, last_conv
    digests = {}
    for name in CASES:
        old = conv32_outputs(name, last_conv.conv32_wgrad, last_conv.conv32_dgrad)
        old.update(convup_outputs(name, last_block.convup_wgrad))
        new = conv32_outputs(name, dec2_conv.convn_wgrad, dec2_conv.convn_dgrad)
        new.update(convup_outputs(name, dec2_block.convupn_wgrad))
        assert sorted(old) == sorted(new)
        for key in old:
            digests[key] = digest(old[key])
            assert digest(new[key]) == digests[key], f"{key}: the N-channel entry gives other bytes"
    n = len(CASES) * (len(CONV32_CAPS) * 4 + 2 + len(CONVUP_CAPS) * len(CONVUP_KEYS) + 2)
    assert len(digests) == n, (len(digests), n)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(digests, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(digests)} digests -> {path}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else PATH)
