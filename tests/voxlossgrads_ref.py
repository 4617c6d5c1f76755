"""NumPy f64 restatement of the gradient of the stage-1 voxel losses with respect to pred (include/v2ce_hip_grad.h),
written from the closed forms, independent of the package: ``coeffs`` is the twin of ``losses.grad_coeffs`` and
``term_grads`` evaluates every term of the gradient on [B, L, 20, H, W] inputs.  The CPU tests compare it against the
reference's own autograd results stored in tests/golden/.voxlossgrads/, the GPU tests compare the kernels against it."""
import numpy as np

from tests.voxlosses_ref import THRESHOLD, to_volumes

F = np.float64
FIELDS = ("a_sq", "a_pyr", "a_t3", "a_t5", "a_ef", "a_comp", "a_match", "a_l1", "a_l2")
TERMS = ("sq", "pyr2", "pyr4", "pyr8", "t3", "t5", "ef", "comp", "match", "l1", "l2")
DEFAULT_LOSS = ("pyramid", "ef", "ef_splitp", "compensation")
ALL_LOSS = ("pyramid", "pt", "ef", "ef_splitp", "match", "compensation", "norml1", "norml2")


def from_volumes(v, B):
    """'(b p) (l c) h w -> b l (p c) h w' with p = 2, c = 10."""
    N, D, H, W = v.shape
    return v.reshape(B, 2, D // 10, 10, H, W).transpose(0, 2, 1, 3, 4, 5).reshape(B, D // 10, 20, H, W)


def coeffs(shape, loss=DEFAULT_LOSS, ef_type="c+cl", add_base_loss=False, alpha_pyramid=1000, alpha_ef=0.5, alpha_efc=5,
           alpha_match=0.5, alpha_compensation=1, alpha_pt=1, alpha_norm=1e-5, stages=1, pred_sq_sum=None):
    """The factor of every linear piece of the gradient: alpha, 2 / count, 1 / k^3, / 3, / 2, / len(kinds), / stages."""
    if len(shape) == 5:
        B, L, _, H, W = shape
        N, D = 2 * B, 10 * L
    else:
        N, D, H, W = shape
        B = L = 0
    c = {"a_sq": 0.0, "a_pyr": [0.0, 0.0, 0.0], "a_t3": 0.0, "a_t5": 0.0, "a_ef": [0.0, 0.0, 0.0, 0.0], "a_comp": 0.0,
         "a_match": 0.0, "a_l1": 0.0, "a_l2": 0.0}
    s = 1.0 / stages
    HW = H * W
    n = N * D * HW
    if "pyramid" in loss:
        for q, k in enumerate((2, 4, 8)):
            n_k = N * (D // k) * (H // k) * (W // k)
            c["a_pyr"][q] = alpha_pyramid * 2.0 / (3.0 * k ** 3 * n_k) * s
        if add_base_loss:
            c["a_sq"] += alpha_pyramid * 2.0 / (3.0 * n) * s
    if "pt" in loss:
        n3, n5 = N * HW * ((D - 1) // 3 + 1), N * HW * (D // 5)
        c["a_t3"] = alpha_pyramid * 2.0 / (2.0 * 3.0 * n3) * s
        c["a_t5"] = alpha_pyramid * 2.0 / (2.0 * 5.0 * n5) * s
        c["a_sq"] += alpha_pyramid * 2.0 / (2.0 * n) * s
    kinds = [k for k in ("ef", "ef_splitp") if k in loss]
    if kinds:
        w_c = {"only_c": 1.0, "cl": 0.0, "c+cl": float(alpha_efc)}[ef_type]
        w_cl = {"only_c": 0.0, "cl": 1.0, "c+cl": 1.0}[ef_type]
        base = alpha_ef / len(kinds) * s
        ef_n = (B * L * HW, B * HW, B * L * 2 * HW, B * 2 * HW)
        if "ef" in kinds:
            c["a_ef"][0] = base * w_c * 2.0 / ef_n[0]
            c["a_ef"][1] = base * w_cl * 2.0 / ef_n[1]
        if "ef_splitp" in kinds:
            c["a_ef"][2] = base * 2.0 * w_c * 2.0 / ef_n[2]
            c["a_ef"][3] = base * 2.0 * w_cl * 2.0 / ef_n[3]
    if "compensation" in loss:
        c["a_comp"] = alpha_compensation * 2.0 / (B * L * W) * s
    if "match" in loss:
        c["a_match"] = alpha_match * 1.0 / (B * 20 * HW) * s
    if "norml1" in loss:
        c["a_l1"] = alpha_norm * s
    if "norml2" in loss:
        norm = float(np.sqrt(F(pred_sq_sum)))
        c["a_l2"] = alpha_norm / norm * s if norm > 0 else 0.0
    return c


def volume_term_grads(p32, g32, c):
    """[N, D, H, W]: the elementwise, pyramid and temporal terms -> {term: [N, D, H, W] f64}; absent terms are left out."""
    p, g = p32.astype(F), g32.astype(F)
    N, D, H, W = p.shape
    out = {}
    if c["a_sq"]:
        out["sq"] = c["a_sq"] * (p - g)
    for q, k in enumerate((2, 4, 8)):
        if not c["a_pyr"][q]:
            continue
        Dk, Hk, Wk = D // k, H // k, W // k
        pool = lambda a: a[:, :Dk * k, :Hk * k, :Wk * k].reshape(N, Dk, k, Hk, k, Wk, k).sum(axis=(2, 4, 6)) / F(k ** 3)
        e = pool(p) - pool(g)
        t = np.zeros_like(p)
        t[:, :Dk * k, :Hk * k, :Wk * k] = c["a_pyr"][q] * e.repeat(k, axis=1).repeat(k, axis=2).repeat(k, axis=3)
        out[f"pyr{k}"] = t
    d = np.arange(D)
    if c["a_t3"]:
        J = (D - 1) // 3 + 1                                       # AvgPool1d(3, stride 3, padding 1): divisor always 3
        pad = lambda a: np.concatenate([np.zeros((N, 1, H, W)), a, np.zeros((N, 3, H, W))], axis=1)[:, :3 * J]
        pool3 = lambda a: pad(a).reshape(N, J, 3, H, W).sum(axis=2) / F(3)
        e = pool3(p) - pool3(g)
        j = (d + 1) // 3
        out["t3"] = c["a_t3"] * e[:, np.minimum(j, J - 1)] * (j < J)[None, :, None, None]
    if c["a_t5"]:
        J = D // 5
        pool5 = lambda a: a[:, :5 * J].reshape(N, J, 5, H, W).sum(axis=2) / F(5)
        e = pool5(p) - pool5(g)
        j = d // 5
        out["t5"] = c["a_t5"] * e[:, np.minimum(j, J - 1)] * (j < J)[None, :, None, None]
    return out


def term_grads(p32, g32, c):
    """[B, L, 20, H, W]: every term of the gradient -> {term: [B, L, 20, H, W] f64}; absent terms are left out."""
    B, L, C, H, W = p32.shape
    assert C == 20
    out = {k: from_volumes(v, B) for k, v in volume_term_grads(to_volumes(p32), to_volumes(g32), c).items()}
    p, g = p32.astype(F), g32.astype(F)
    sign = np.sign(p)                                              # sign(0) = 0, as in the backward of torch.abs
    if any(c["a_ef"]):
        ap, ag = np.abs(p), np.abs(g)
        sp = lambda a: a.reshape(B, L, 2, 10, H, W).sum(axis=3)    # [B, L, 2, H, W]
        E0 = ap.sum(axis=2) - ag.sum(axis=2)                       # [B, L, H, W]
        E1 = ap.sum(axis=(1, 2)) - ag.sum(axis=(1, 2))             # [B, H, W]
        E2 = sp(ap) - sp(ag)
        E3 = sp(ap).sum(axis=1) - sp(ag).sum(axis=1)               # [B, 2, H, W]
        a = c["a_ef"]
        per = (a[0] * E0[:, :, None] + a[1] * E1[:, None, None] + a[2] * E2 + a[3] * E3[:, None])   # [B, L, 2, H, W]
        out["ef"] = sign * per.repeat(10, axis=2)
    if c["a_comp"]:
        mp, mg = p32 > THRESHOLD, g32 > THRESHOLD
        cp, cg = np.maximum(mp.sum(axis=(2, 3)), 1), np.maximum(mg.sum(axis=(2, 3)), 1)             # [B, L, W]
        e = (p * mp).sum(axis=(2, 3)) / cp - (g * mg).sum(axis=(2, 3)) / cg
        out["comp"] = c["a_comp"] * (e / cp)[:, :, None, None, :] * mp
    if c["a_match"]:
        m = p.max(axis=1, keepdims=True)
        lse = m + np.log(np.exp(p - m).sum(axis=1, keepdims=True))
        t = np.argmax(g32, axis=1)                                 # the first maximum
        hot = np.arange(L)[None, :, None, None, None] == t[:, None]
        out["match"] = c["a_match"] * (np.exp(p - lse) - hot)
    if c["a_l1"]:
        out["l1"] = c["a_l1"] * sign
    if c["a_l2"]:
        out["l2"] = c["a_l2"] * p
    return out


def total(terms, shape):
    """(the gradient, the elementwise sum of the absolute contributions) of a dict of terms."""
    g, m = np.zeros(shape), np.zeros(shape)
    for k in TERMS:
        if k in terms:
            g = g + terms[k]
            m = m + np.abs(terms[k])
    return g, m


def grad(p32, g32, loss=DEFAULT_LOSS, stages=1, **opts):
    """(gradient, M) of calculate_loss(p32, g32, loss=loss, **opts)[0] for one of `stages` stages."""
    sq = (p32.astype(F) ** 2).sum() if "norml2" in loss else None
    c = coeffs(p32.shape, loss, stages=stages, pred_sq_sum=sq, **opts)
    return total(term_grads(p32, g32, c), p32.shape)


def volume_grad(p32, g32, loss=("pyramid", "pt"), stages=1, **opts):
    c = coeffs(p32.shape, loss, stages=stages, **opts)
    return total(volume_term_grads(p32, g32, c), p32.shape)
