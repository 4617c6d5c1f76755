"""NumPy f64 restatement of the stage-1 loss statistics (include/v2ce_hip.h, v2ce_voxlosses_stats) and of the values
``ModelInterface.calculate_loss`` makes of them.  Written from the definitions, independent of the package: the GPU
tests compare the records against ``seq_stats`` / ``volume_stats`` and the CPU tests compare ``loss_values`` against
the reference's own results stored in tests/golden/.voxlosses/."""
import numpy as np

F = np.float64
THRESHOLD = np.float32(0.01)
SUM_KEYS = ("n", "sq_sum", "abs_diff_sum", "pred_abs_sum", "pred_sq_sum", "pyr_n", "pyr_sq_sum", "temporal_n",
            "temporal_sq_sum", "ef_n", "ef_sq_sum", "comp_n", "comp_sq_sum", "match_n", "match_sum", "match_low")


def to_volumes(v):
    """'b l (p c) h w -> (b p) (l c) h w' with p = 2."""
    B, L, C, H, W = v.shape
    return v.reshape(B, L, 2, C // 2, H, W).transpose(0, 2, 1, 3, 4, 5).reshape(B * 2, L * (C // 2), H, W)


def volume_stats(p32, g32, pyramid=True, temporal=True):
    """One volume [D, H, W]: elementwise, pyramid (k = 2, 4, 8) and temporal (pool 3 padded, pool 5) sums."""
    p, g = p32.astype(F), g32.astype(F)
    D, H, W = p.shape
    d = p - g
    s = {"n": D * H * W, "sq_sum": (d * d).sum(), "abs_diff_sum": np.abs(d).sum(), "pred_abs_sum": np.abs(p).sum(),
         "pred_sq_sum": (p * p).sum(), "pyr_n": np.zeros(3, np.int64), "pyr_sq_sum": np.zeros(3),
         "temporal_n": np.zeros(2, np.int64), "temporal_sq_sum": np.zeros(2)}
    if pyramid:
        for q, k in enumerate((2, 4, 8)):
            Dk, Hk, Wk = D // k, H // k, W // k
            pool = lambda a: a[:Dk * k, :Hk * k, :Wk * k].reshape(Dk, k, Hk, k, Wk, k).sum(axis=(1, 3, 5)) / F(k ** 3)
            e = pool(p) - pool(g)
            s["pyr_n"][q] = e.size
            s["pyr_sq_sum"][q] = (e * e).sum()
    if temporal:
        J = (D - 1) // 3 + 1                                       # AvgPool1d(3, stride 3, padding 1): divisor always 3
        pad = lambda a: np.concatenate([np.zeros((1, H, W)), a, np.zeros((3, H, W))])[:3 * J]
        pool3 = lambda a: pad(a).reshape(J, 3, H, W).sum(axis=1) / F(3)
        e = pool3(p) - pool3(g)
        s["temporal_n"][0] = e.size
        s["temporal_sq_sum"][0] = (e * e).sum()
        J = D // 5
        pool5 = lambda a: a[:5 * J].reshape(J, 5, H, W).sum(axis=1) / F(5)
        e = pool5(p) - pool5(g)
        s["temporal_n"][1] = e.size
        s["temporal_sq_sum"][1] = (e * e).sum()
    return s


def seq_stats(p32, g32, terms=("pyramid", "temporal", "ef", "compensation", "match")):
    """One sequence [L, 20, H, W]: every field of the record."""
    L, C, H, W = p32.shape
    assert C == 20
    pv, gv = to_volumes(p32[None]), to_volumes(g32[None])
    vols = [volume_stats(pv[q], gv[q], "pyramid" in terms, "temporal" in terms) for q in range(2)]
    s = {k: vols[0][k] + vols[1][k] for k in vols[0]}
    p, g = p32.astype(F), g32.astype(F)
    s.update(ef_n=np.zeros(4, np.int64), ef_sq_sum=np.zeros(4), comp_n=0, comp_sq_sum=0.0, match_n=0, match_sum=0.0,
             match_low=0)
    if "ef" in terms:
        ap, ag = np.abs(p), np.abs(g)
        sp = lambda a: a.reshape(L, 2, 10, H, W).sum(axis=2)
        frames = [(ap.sum(axis=1), ag.sum(axis=1)), (ap.sum(axis=(0, 1)), ag.sum(axis=(0, 1))),
                  (sp(ap), sp(ag)), (sp(ap).sum(axis=0), sp(ag).sum(axis=0))]
        for q, (a, b) in enumerate(frames):
            e = a - b
            s["ef_n"][q] = e.size
            s["ef_sq_sum"][q] = (e * e).sum()
    if "compensation" in terms:
        def mean(v32, v):
            m = v32 > THRESHOLD
            return (v * m).sum(axis=(1, 2)) / np.maximum(m.sum(axis=(1, 2)), 1)      # [L, W]
        e = mean(p32, p) - mean(g32, g)
        s["comp_n"] = e.size
        s["comp_sq_sum"] = (e * e).sum()
    if "match" in terms:
        t = np.argmax(g32, axis=0)[None]                           # the first maximum; a NaN counts as the maximum
        m = p.max(axis=0)
        with np.errstate(invalid="ignore"):
            lse = np.log(np.exp(p - m[None]).sum(axis=0))
        gap = m - np.take_along_axis(p, t, axis=0)[0]
        s["match_n"] = gap.size
        s["match_sum"] = (gap + lse).sum()
        s["match_low"] = int((-gap < -80).sum())
    return s


def batch_stats(p32, g32, terms=("pyramid", "temporal", "ef", "compensation", "match")):
    """[B, L, 20, H, W] -> list of per-b records."""
    return [seq_stats(p32[b], g32[b], terms) for b in range(p32.shape[0])]


def total(records):
    return {k: sum(r[k] for r in records) for k in records[0]}


def term_values(s, ef_type="c+cl", add_base_loss=False, alpha_efc=5, kinds=("ef", "ef_splitp")):
    """The f64 value of every term from one (summed) record; terms whose statistics are absent are left out."""
    v = {}
    mse = s["sq_sum"] / s["n"]
    v["l1"], v["l2"] = s["abs_diff_sum"] / s["n"], mse
    v["norml1"], v["norml2"] = s["pred_abs_sum"], np.sqrt(s["pred_sq_sum"])
    if s["pyr_n"][0]:
        v["pyramid_loss"] = ((mse if add_base_loss else 0.0) + (s["pyr_sq_sum"] / s["pyr_n"]).sum()) / 3
    if s["temporal_n"][0]:
        v["pt_loss"] = (mse + (s["temporal_sq_sum"] / s["temporal_n"]).sum()) / 2
    if s["ef_n"][0] and kinds:
        m = s["ef_sq_sum"] / s["ef_n"]
        acc = 0.0
        for kind in kinds:
            c, cl = (m[2], m[3]) if kind == "ef_splitp" else (m[0], m[1])
            e = {"only_c": c, "cl": cl, "c+cl": alpha_efc * c + cl}[ef_type]
            acc += 2 * e if kind == "ef_splitp" else e
        v["ef_loss"] = acc / len(kinds)
    if s["comp_n"]:
        v["compensation"] = s["comp_sq_sum"] / s["comp_n"]
    if s["match_n"]:
        v["match"] = s["match_sum"] / s["match_n"]
    return v


DEFAULT_LOSS = ("pyramid", "ef", "ef_splitp", "compensation")
KEY_OF = {"pyramid": "pyramid_loss", "pt": "pt_loss", "match": "match", "compensation": "compensation",
          "norml1": "norml1", "norml2": "norml2"}


def loss_values(stage_records, loss=DEFAULT_LOSS, ef_type="c+cl", add_base_loss=False, alpha_pyramid=1000, alpha_ef=0.5,
                alpha_efc=5, alpha_match=0.5, alpha_compensation=1, alpha_norm=1e-5):
    """calculate_loss in f64 on one summed record per refinement stage: (loss, loss_dict)."""
    kinds = tuple(k for k in ("ef", "ef_splitp") if k in loss)
    vals = [term_values(s, ef_type, add_base_loss, alpha_efc, kinds) for s in stage_records]
    mean = lambda key: float(np.mean([v[key] for v in vals]))
    weights = {"pyramid": alpha_pyramid, "pt": alpha_pyramid, "match": alpha_match, "compensation": alpha_compensation,
               "norml1": alpha_norm, "norml2": alpha_norm}
    out, d = 0.0, {}
    if kinds:
        d["ef_loss"] = mean("ef_loss")
        out += alpha_ef * d["ef_loss"]
    for name in ("pyramid", "pt", "match", "compensation", "norml1", "norml2"):
        if name in loss:
            d[KEY_OF[name]] = mean(KEY_OF[name])
            out += weights[name] * d[KEY_OF[name]]
    return out, d
