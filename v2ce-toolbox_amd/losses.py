"""The voxel-only terms of the reference's stage-1 loss -- ``ModelInterface.calculate_loss``
(``train/scripts/model/model_interface.py``) and the classes of ``train/scripts/model/losses.py`` -- from one device
pass over ``pred`` and ``gt``:

* ``voxel_losses_batch(pred, gt, terms=ALL)``   per-sequence sufficient statistics of ``[B, L, 20, H, W]`` f32 device
  tensors (``csrc/voxlosses.hip`` through ``v2ce_voxlosses``) and one host synchronisation; ``VoxLosses`` turns them
  into the reference's values
* ``volume_losses_batch(pred, gt, terms)``   the same for ``[N, D, H, W]`` (pyramid and temporal terms only)
* drop-ins ``Pyramid3dLoss(add_base_loss)``, ``PyramidTemporalLoss()`` on ``[N, D, H, W]`` and ``CompensationLoss()``,
  ``MatchLoss()`` on ``[B, L, 20, H, W]``: the reference's constructor arguments and ``forward``, 0-d f32 device tensors
* ``calculate_loss(pred_voxels, gt_voxels, loss=...)``   the reference's weighted total and ``loss_dict``
* ``voxel_loss_grads_batch(pred, gt, loss=..., ...)`` / ``volume_loss_grads_batch``   the gradient of that total with
  respect to ``pred`` (``csrc/voxlossgrads.hip`` through ``v2ce_voxloss_grads`` / ``v2ce_volume_loss_grads``), f32, shaped
  like ``pred``; ``grad_coeffs`` turns a loss list, its options and the shape into the kernel's f64 factors

Every value is the f64 quotient of the f64 statistics, rounded to f32 once; the reference computes in f32 throughout
(its ``torch.norm`` is off by up to 5e-4 relative at full size).  Every gradient element is the f64 closed form of the
reference's autograd result, rounded to f32 once.  When a prediction requires grad, ``calculate_loss`` and the drop-in
modules return a value with a ``grad_fn`` (one ``torch.autograd.Function`` per refinement stage: the statistics call
forward, one gradient call backward, no host synchronisation in the backward); otherwise, and under
``torch.no_grad()``, they do exactly the statistics call.  ``gt`` gets no gradient and there is no double backward.
The match gradient is the f64 softmax, so it stays finite where the reference's f32 ``log(softmax)`` has underflowed
(``match_low > 0``).  There is no CPU path.
"""
from __future__ import annotations

import ctypes
import math
from typing import Dict, Optional, Sequence

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import hip

CHANNELS = 20
TERMS = {"pyramid": hip.VOXLOSSES_PYRAMID, "temporal": hip.VOXLOSSES_TEMPORAL, "ef": hip.VOXLOSSES_EF,
         "compensation": hip.VOXLOSSES_COMPENSATION, "match": hip.VOXLOSSES_MATCH}
ALL = tuple(TERMS)
VOLUME_TERMS = ("pyramid", "temporal")
STATS_DTYPE = np.dtype([("struct_size", "<i8"), ("term_mask", "<i8"), ("n", "<i8"), ("sq_sum", "<f8"),
                        ("abs_diff_sum", "<f8"), ("pred_abs_sum", "<f8"), ("pred_sq_sum", "<f8"), ("pyr_n", "<i8", 3),
                        ("pyr_sq_sum", "<f8", 3), ("temporal_n", "<i8", 2), ("temporal_sq_sum", "<f8", 2),
                        ("ef_n", "<i8", 4), ("ef_sq_sum", "<f8", 4), ("comp_n", "<i8"), ("comp_sq_sum", "<f8"),
                        ("match_n", "<i8"), ("match_sum", "<f8"), ("match_low", "<i8")])
assert STATS_DTYPE.itemsize == ctypes.sizeof(hip.VoxLossesStats)
_SUMMED = tuple(n for n in STATS_DTYPE.names if n not in ("struct_size", "term_mask"))
EF_TYPES = ("only_c", "cl", "c+cl")
# what calculate_loss accepts: the terms it computes, the ones the reference configures without using them there, and
# the ones this package cannot compute
LOSS_NAMES = ("ef", "ef_splitp", "pyramid", "pt", "match", "compensation", "norml1", "norml2")
_IGNORED = ("l1", "l2", "physical")
_NEEDS_MODEL = {"gan": "it needs the discriminator network, which this package does not have",
                "encoder": "it needs the VoxelEncoder network and its weights, which this package does not have",
                "imu": "it needs the model's IMU output, which this package does not have"}
PYRAMID_MIN = 8
TEMPORAL_MIN = 5


def term_mask(terms) -> int:
    mask = 0
    for t in terms:
        if t not in TERMS:
            raise ValueError(f"unknown term {t!r}: choose from {ALL}")
        mask |= TERMS[t]
    return mask


class VoxLosses:
    """Per-sequence (or per-volume) statistics of ``voxel_losses_batch`` / ``volume_losses_batch`` as host numpy arrays,
    one row per b: every field of ``v2ce_voxlosses_stats`` is an attribute (``n``, ``sq_sum``, ``pyr_sq_sum`` [B, 3],
    ...).  ``raw`` holds the records as returned.  The accessors return the reference's value per row, f32."""

    def __init__(self, terms, fields: Dict[str, np.ndarray], raw: Optional[np.ndarray] = None):
        self.terms = tuple(terms)
        self.fields = fields
        self.raw = raw

    def __getattr__(self, name):
        f = self.__dict__.get("fields")
        if f is not None and name in f:
            return f[name]
        raise AttributeError(name)

    def __len__(self):
        return int(self.fields["n"].shape[0])

    def select(self, rows) -> "VoxLosses":
        """The statistics of some rows (an index or slice of b)."""
        r = np.atleast_1d(np.arange(len(self))[rows])
        return VoxLosses(self.terms, {k: v[r] for k, v in self.fields.items()},
                         None if self.raw is None else self.raw[r])

    def total(self) -> "VoxLosses":
        """All rows as one batch: what the reference returns for the whole input."""
        return VoxLosses(self.terms, {k: v.sum(axis=0, keepdims=True) for k, v in self.fields.items()})

    def _need(self, term):
        if term not in self.terms:
            raise ValueError(f"the {term!r} statistics were not requested (terms={self.terms})")

    @staticmethod
    def _f32(v):
        return np.asarray(v, np.float64).astype(np.float32)

    def _mse(self):
        return self.sq_sum / self.n

    def _pyramid(self, add_base_loss):
        self._need("pyramid")
        s = (self.pyr_sq_sum / self.pyr_n).sum(axis=1)
        return ((self._mse() + s) if add_base_loss else s) / 3.0

    def _pt(self):
        self._need("temporal")
        return (self._mse() + (self.temporal_sq_sum / self.temporal_n).sum(axis=1)) / 2.0

    def _ef(self, ef_type, alpha_efc, kinds):
        self._need("ef")
        if ef_type not in EF_TYPES:
            raise ValueError(f"Invalid ef_type {ef_type}!")
        kinds = tuple(kinds)
        if not kinds or any(k not in ("ef", "ef_splitp") for k in kinds):
            raise ValueError(f"kinds must name 'ef' and / or 'ef_splitp', got {kinds}")
        m = self.ef_sq_sum / self.ef_n                       # [B, 4]: ef c, ef cl, ef_splitp c, ef_splitp cl
        out = 0.0
        for kind in kinds:
            c, cl = (m[:, 2], m[:, 3]) if kind == "ef_splitp" else (m[:, 0], m[:, 1])
            v = c if ef_type == "only_c" else (cl if ef_type == "cl" else alpha_efc * c + cl)
            out = out + (2.0 * v if kind == "ef_splitp" else v)
        return out / len(kinds)

    def _compensation(self):
        self._need("compensation")
        return self.comp_sq_sum / self.comp_n

    def _match(self):
        self._need("match")
        return self.match_sum / self.match_n

    def pyramid(self, add_base_loss=False) -> np.ndarray:
        """Pyramid3dLoss: ((MSE if add_base_loss) + MSE of the 2-, 4- and 8-pooled volumes) / 3."""
        return self._f32(self._pyramid(add_base_loss))

    def pt(self) -> np.ndarray:
        """PyramidTemporalLoss: (MSE + MSE of the two temporal pools) / 2 -- the reference divides by its two pools."""
        return self._f32(self._pt())

    def ef(self, ef_type="c+cl", alpha_efc=5, kinds=("ef", "ef_splitp")) -> np.ndarray:
        """The event-frame term of calculate_loss over the requested kinds: (ef + 2 ef_splitp) / 2 for both."""
        return self._f32(self._ef(ef_type, alpha_efc, kinds))

    def compensation(self) -> np.ndarray:
        return self._f32(self._compensation())

    def match(self) -> np.ndarray:
        return self._f32(self._match())

    def norml1(self) -> np.ndarray:
        return self._f32(self.pred_abs_sum)

    def norml2(self) -> np.ndarray:
        return self._f32(np.sqrt(self.pred_sq_sum))

    def l1(self) -> np.ndarray:
        return self._f32(self.abs_diff_sum / self.n)

    def l2(self) -> np.ndarray:
        return self._f32(self._mse())


def _check(t, name, dims, what):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch tensor")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32 (got {t.dtype})")
    if t.dim() != dims or (dims == 5 and t.shape[2] != CHANNELS):
        raise ValueError(f"{name} must be {what}, got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if not t.is_cuda:
        raise hip.V2ceHipError(f"{name} must live on a HIP device (got {t.device}); there is no CPU path")


def _check_pair(pred, gt, dims, what):
    _check(pred, "pred", dims, what)
    _check(gt, "gt", dims, what)
    if pred.shape != gt.shape:
        raise ValueError(f"pred {tuple(pred.shape)} and gt {tuple(gt.shape)} differ in shape")
    if pred.device != gt.device:
        raise ValueError("pred and gt live on different devices")


def _check_sizes(terms, D, H, W):
    if "pyramid" in terms and min(D, H, W) < PYRAMID_MIN:
        raise ValueError(f"input image (T: {D} H: {H} W: {W}) smaller than kernel size (kT: 8 kH: 8 kW: 8): the "
                         f"pyramid's AvgPool3d(8) needs min(D, H, W) >= 8")
    if "temporal" in terms and D < TEMPORAL_MIN:
        raise ValueError(f"Given input size: (1x{D}). Calculated output size: (1x0). Output size is too small: the "
                         f"temporal term's AvgPool1d(5) needs D >= 5")


def _run(entry, ws_entry, name, pred, gt, dims, terms):
    mask = term_mask(terms)
    L = hip.lib()
    ws_bytes = getattr(L, ws_entry)(*dims, mask)
    if ws_bytes == 0:
        raise hip.V2ceHipError(f"{name}: unsupported shape {tuple(pred.shape)} with terms {tuple(terms)}")
    n = dims[0]
    dev = pred.device
    with torch.cuda.device(dev):
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        out = torch.empty(n * STATS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        hip.check(getattr(L, entry)(pred.data_ptr(), gt.data_ptr(), *dims, mask, out.data_ptr(),
                                    ctypes.sizeof(hip.VoxLossesStats), ws.data_ptr(), ws_bytes, hip.stream_ptr(dev)),
                  name)
        rec = out.cpu().numpy().view(STATS_DTYPE)                         # the one synchronisation
    if (rec["struct_size"] != STATS_DTYPE.itemsize).any():
        raise hip.V2ceHipError(f"{name} wrote records of another layout")
    return VoxLosses(terms, {k: rec[k].copy() for k in _SUMMED}, rec)


def voxel_losses_batch(pred: torch.Tensor, gt: torch.Tensor, *, terms: Sequence[str] = ALL) -> VoxLosses:
    """Sufficient statistics of the stage-1 loss terms per sequence b of ``pred``, ``gt`` [B, L, 20, H, W] (f32,
    contiguous, on one device), in one pass and one host synchronisation.  ``terms``: any of ``ALL``; the elementwise
    sums (l1, l2, norml1, norml2) always come along."""
    terms = tuple(terms)
    term_mask(terms)
    _check_pair(pred, gt, 5, "[b, l, 20, h, w] (channels (p c): 2 polarities x 10 bins)")
    B, Lq, C, H, W = (int(v) for v in pred.shape)
    _check_sizes(terms, 10 * Lq, H, W)
    return _run("v2ce_voxlosses", "v2ce_voxlosses_workspace_bytes", "v2ce_voxlosses", pred, gt, (B, Lq, C, H, W), terms)


def volume_losses_batch(pred: torch.Tensor, gt: torch.Tensor, *, terms: Sequence[str] = VOLUME_TERMS) -> VoxLosses:
    """The elementwise, pyramid and temporal statistics per volume n of ``pred``, ``gt`` [N, D, H, W]."""
    terms = tuple(terms)
    term_mask(terms)
    if any(t not in VOLUME_TERMS for t in terms):
        raise ValueError(f"[n, d, h, w] volumes have the terms {VOLUME_TERMS} only, got {terms}")
    _check_pair(pred, gt, 4, "[n, d, h, w]")
    N, D, H, W = (int(v) for v in pred.shape)
    _check_sizes(terms, D, H, W)
    return _run("v2ce_volume_losses", "v2ce_volume_losses_workspace_bytes", "v2ce_volume_losses", pred, gt,
                (N, D, H, W), terms)


def _scalar(v, device):
    return torch.tensor(float(v), dtype=torch.float32, device=device)


class Pyramid3dLoss(torch.nn.Module):
    """losses.py Pyramid3dLoss on [N, D, H, W]: MSE of AvgPool3d(k, stride k) for k = 2, 4, 8, summed, / 3."""

    def __init__(self, add_base_loss=False):
        super().__init__()
        self.add_base_loss = add_base_loss

    def forward(self, pred, target):
        if _wants_grad(pred):
            return _StageLoss.apply(pred, target, _Stage(("pyramid",), dict(add_base_loss=self.add_base_loss,
                                                                            alpha_pyramid=1), volume=True))
        s = volume_losses_batch(pred, target, terms=("pyramid",)).total()
        return _scalar(s.pyramid(self.add_base_loss)[0], pred.device)


class PyramidTemporalLoss(torch.nn.Module):
    """losses.py PyramidTemporalLoss on [N, D, H, W]: MSE plus the MSE of two average pools along D, / 2."""

    def forward(self, pred, target):
        if _wants_grad(pred):
            return _StageLoss.apply(pred, target, _Stage(("pt",), dict(alpha_pyramid=1), volume=True))
        s = volume_losses_batch(pred, target, terms=("temporal",)).total()
        return _scalar(s.pt()[0], pred.device)


class CompensationLoss(torch.nn.Module):
    """losses.py CompensationLoss on [B, L, 20, H, W]: its dim = (2, 3) reduces channels and rows."""

    def forward(self, pred, target):
        if _wants_grad(pred):
            return _StageLoss.apply(pred, target, _Stage(("compensation",), dict(alpha_compensation=1)))
        s = voxel_losses_batch(pred, target, terms=("compensation",)).total()
        return _scalar(s.compensation()[0], pred.device)


class MatchLoss(torch.nn.Module):
    """losses.py MatchLoss on [B, L, 20, H, W]: NLL of softmax over l at the first argmax over l of the target."""

    def forward(self, pred, target):
        if _wants_grad(pred):
            return _StageLoss.apply(pred, target, _Stage(("match",), dict(alpha_match=1)))
        s = voxel_losses_batch(pred, target, terms=("match",)).total()
        return _scalar(s.match()[0], pred.device)


def check_loss_names(loss) -> tuple:
    loss = tuple(loss)
    for name in loss:
        if name in _NEEDS_MODEL:
            raise ValueError(f"loss {name!r} cannot be computed here: {_NEEDS_MODEL[name]}")
        if name not in LOSS_NAMES and name not in _IGNORED:
            raise ValueError(f"unknown loss {name!r}: choose from {LOSS_NAMES}")
    return loss


def terms_for(loss) -> tuple:
    """The statistics that the names of a loss list need."""
    t = []
    if "pyramid" in loss:
        t.append("pyramid")
    if "pt" in loss:
        t.append("temporal")
    if "ef" in loss or "ef_splitp" in loss:
        t.append("ef")
    if "compensation" in loss:
        t.append("compensation")
    if "match" in loss:
        t.append("match")
    return tuple(t)


def loss_values(stats: Sequence[VoxLosses], loss, *, ef_type="c+cl", add_base_loss=False, alpha_pyramid=1000,
                alpha_ef=0.5, alpha_efc=5, alpha_match=0.5, alpha_compensation=1, alpha_pt=1, alpha_norm=1e-5):
    """calculate_loss on the one-row statistics of each refinement stage: (loss, loss_dict) as f64 / f32 numpy
    scalars, the terms in the reference's order.  ``alpha_pt`` is accepted and, as in the reference
    (model_interface.py:281), not used: the pt term is weighted by ``alpha_pyramid``."""
    mean = lambda f: float(np.mean([float(f(s)[0]) for s in stats]))
    total, d = 0.0, {}
    kinds = tuple(k for k in ("ef", "ef_splitp") if k in loss)
    if kinds:
        v = mean(lambda s: s._ef(ef_type, alpha_efc, kinds))
        total += alpha_ef * v
        d["ef_loss"] = np.float32(v)
    if "pyramid" in loss:
        v = mean(lambda s: s._pyramid(add_base_loss))
        total += alpha_pyramid * v
        d["pyramid_loss"] = np.float32(v)
    if "pt" in loss:
        v = mean(lambda s: s._pt())
        total += alpha_pyramid * v
        d["pt_loss"] = np.float32(v)
    if "match" in loss:
        v = mean(lambda s: s._match())
        total += alpha_match * v
        d["match"] = np.float32(v)
    if "compensation" in loss:
        v = mean(lambda s: s._compensation())
        total += alpha_compensation * v
        d["compensation"] = np.float32(v)
    if "norml1" in loss:
        v = mean(lambda s: s.pred_abs_sum)
        total += alpha_norm * v
        d["norml1"] = np.float32(v)
    if "norml2" in loss:
        v = mean(lambda s: np.sqrt(s.pred_sq_sum))
        total += alpha_norm * v
        d["norml2"] = np.float32(v)
    return np.float32(total), d


def calculate_loss(pred_voxels, gt_voxels, *, loss=("pyramid", "ef", "ef_splitp", "compensation"), ef_type="c+cl",
                   add_base_loss=False, alpha_pyramid=1000, alpha_ef=0.5, alpha_efc=5, alpha_match=0.5,
                   alpha_compensation=1, alpha_pt=1, alpha_norm=1e-5):
    """The voxel-related part of ModelInterface.calculate_loss.  ``pred_voxels``: [B, L, 20, H, W] or a list of
    refinement stages, each term averaged over the stages.  Returns ``(loss, loss_dict)``: a 0-d f32 device tensor and
    0-d f32 host tensors under the reference's keys.  'gan', 'encoder' and 'imu' raise ValueError; 'physical' is
    skipped, as the reference skips it when the prediction carries no attention maps."""
    loss = check_loss_names(loss)
    if ef_type not in EF_TYPES:
        raise ValueError(f"Invalid ef_type {ef_type}!")
    stages = list(pred_voxels) if isinstance(pred_voxels, (list, tuple)) else [pred_voxels]
    if not stages:
        raise ValueError("pred_voxels is an empty list")
    terms = terms_for(loss)
    opts = dict(ef_type=ef_type, add_base_loss=add_base_loss, alpha_pyramid=alpha_pyramid, alpha_ef=alpha_ef,
                alpha_efc=alpha_efc, alpha_match=alpha_match, alpha_compensation=alpha_compensation, alpha_pt=alpha_pt,
                alpha_norm=alpha_norm)
    if not any(_wants_grad(p) for p in stages):
        stats = [voxel_losses_batch(p, gt_voxels, terms=terms).total() for p in stages]
        total, d = loss_values(stats, loss, **opts)
        return _scalar(total, gt_voxels.device), {k: torch.tensor(float(v), dtype=torch.float32) for k, v in d.items()}
    # one autograd node per stage: its value is the stage's share of the total, its backward one gradient call
    plans = [_Stage(loss, opts, stages=len(stages)) for _ in stages]
    shares = [_StageLoss.apply(p, gt_voxels, plan) for p, plan in zip(stages, plans)]
    total, d = loss_values([plan.stats.total() for plan in plans], loss, **opts)
    if len(shares) == 1:
        out = shares[0]                                   # its value is the total itself
    else:
        # the total as the no-grad call rounds it (f64 over all stages, one rounding), carried by the stages' nodes:
        # the bracket is exactly zero and passes the incoming gradient to every stage unchanged
        s = torch.stack(shares).sum()
        out = _scalar(total, gt_voxels.device) + (s - s.detach())
    return out, {k: torch.tensor(float(v), dtype=torch.float32) for k, v in d.items()}


# ---------------------------------------------------------------------------------------------------------------------
# gradients

_OPTION_DEFAULTS = dict(ef_type="c+cl", add_base_loss=False, alpha_pyramid=1000, alpha_ef=0.5, alpha_efc=5,
                        alpha_match=0.5, alpha_compensation=1, alpha_pt=1, alpha_norm=1e-5)
DEFAULT_LOSS = ("pyramid", "ef", "ef_splitp", "compensation")
VOLUME_LOSS_NAMES = ("pyramid", "pt")
COEFF_FIELDS = tuple(n for n, _ in hip.VoxLossGradCoeffs._fields_ if n != "struct_size")


def _wants_grad(t) -> bool:
    return torch.is_grad_enabled() and isinstance(t, torch.Tensor) and t.requires_grad


def grad_coeffs(shape, loss=DEFAULT_LOSS, *, ef_type="c+cl", add_base_loss=False, alpha_pyramid=1000, alpha_ef=0.5,
                alpha_efc=5, alpha_match=0.5, alpha_compensation=1, alpha_pt=1, alpha_norm=1e-5, stages=1,
                pred_sq_sum=None) -> hip.VoxLossGradCoeffs:
    """The factors of ``v2ce_voxloss_grad_coeffs`` for the gradient of ``calculate_loss(..., loss=loss, <options>)`` on a
    ``shape`` [B, L, 20, H, W] prediction (or [N, D, H, W]: 'pyramid' and 'pt' only): per linear piece of the loss its
    alpha, 2 / (the batch-total count of the forward record), 1 / k^3, the / 3 and / 2 of the pyramid and temporal
    classes, / len(kinds) of the event-frame term and 1 / ``stages`` in one f64.  ``pred_sq_sum``: the batch total of
    the forward record's field, needed by 'norml2' (whose gradient is zero where the norm is).  As in ``loss_values``,
    ``alpha_pt`` is accepted and not used."""
    loss = check_loss_names(loss)
    if ef_type not in EF_TYPES:
        raise ValueError(f"Invalid ef_type {ef_type}!")
    if int(stages) < 1:
        raise ValueError(f"stages must be >= 1, got {stages}")
    shape = tuple(int(v) for v in shape)
    if len(shape) == 5:
        B, L, C, H, W = shape
        if C != CHANNELS:
            raise ValueError(f"shape must be [b, l, 20, h, w], got {shape}")
        N, D = 2 * B, 10 * L
    elif len(shape) == 4:
        N, D, H, W = shape
        B = L = 0
        bad = [n for n in loss if n in LOSS_NAMES and n not in VOLUME_LOSS_NAMES]
        if bad:
            raise ValueError(f"[n, d, h, w] volumes have the losses {VOLUME_LOSS_NAMES} only, got {bad}")
    else:
        raise ValueError(f"shape must be [b, l, 20, h, w] or [n, d, h, w], got {shape}")
    _check_sizes(terms_for(loss), D, H, W)
    c = hip.VoxLossGradCoeffs(struct_size=ctypes.sizeof(hip.VoxLossGradCoeffs))
    s = 1.0 / int(stages)
    HW = H * W
    n = N * D * HW
    a_sq = 0.0
    if "pyramid" in loss:
        for q, k in enumerate((2, 4, 8)):
            c.a_pyr[q] = alpha_pyramid * 2.0 / (3.0 * k ** 3 * (N * (D // k) * (H // k) * (W // k))) * s
        if add_base_loss:
            a_sq += alpha_pyramid * 2.0 / (3.0 * n) * s
    if "pt" in loss:
        c.a_t3 = alpha_pyramid * 2.0 / (2.0 * 3.0 * (N * HW * ((D - 1) // 3 + 1))) * s
        c.a_t5 = alpha_pyramid * 2.0 / (2.0 * 5.0 * (N * HW * (D // 5))) * s
        a_sq += alpha_pyramid * 2.0 / (2.0 * n) * s
    c.a_sq = a_sq
    kinds = tuple(k for k in ("ef", "ef_splitp") if k in loss)
    if kinds:
        w_c = {"only_c": 1.0, "cl": 0.0, "c+cl": float(alpha_efc)}[ef_type]
        w_cl = {"only_c": 0.0, "cl": 1.0, "c+cl": 1.0}[ef_type]
        base = alpha_ef / len(kinds) * s
        ef_n = (B * L * HW, B * HW, B * L * 2 * HW, B * 2 * HW)
        if "ef" in kinds:
            c.a_ef[0] = base * w_c * 2.0 / ef_n[0]
            c.a_ef[1] = base * w_cl * 2.0 / ef_n[1]
        if "ef_splitp" in kinds:
            c.a_ef[2] = base * 2.0 * w_c * 2.0 / ef_n[2]
            c.a_ef[3] = base * 2.0 * w_cl * 2.0 / ef_n[3]
    if "compensation" in loss:
        c.a_comp = alpha_compensation * 2.0 / (B * L * W) * s
    if "match" in loss:
        c.a_match = alpha_match * 1.0 / (B * CHANNELS * HW) * s
    if "norml1" in loss:
        c.a_l1 = alpha_norm * s
    if "norml2" in loss:
        if pred_sq_sum is None:
            raise ValueError("'norml2' needs pred_sq_sum, the batch total of the forward statistics")
        norm = math.sqrt(float(pred_sq_sum))
        c.a_l2 = alpha_norm / norm * s if norm > 0 else 0.0
    return c


def _check_f32_device(t, name, device):
    """ValueError for what a gradient call refuses in an argument of its own."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
        raise ValueError(f"{name} must be a float32 tensor (got {getattr(t, 'dtype', type(t))})")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if t.device != device:
        raise ValueError(f"{name} lives on {t.device}, pred on {device}")


def _overlaps(a, b) -> bool:
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * 4 and b0 < a0 + a.numel() * 4


_WHAT = {5: "[b, l, 20, h, w] (channels (p c): 2 polarities x 10 bins)", 4: "[n, d, h, w]"}


def _check_grad_pair(pred, gt, ndim):
    for t, nm in ((pred, "pred"), (gt, "gt")):
        if isinstance(t, torch.Tensor) and t.dtype != torch.float32:
            raise ValueError(f"{nm} must be float32 (got {t.dtype})")
    _check_pair(pred, gt, ndim, _WHAT[ndim])
    return tuple(int(v) for v in pred.shape)


def _run_grads(entry, pred, gt, dims, coef, upstream, grad):
    dev = pred.device
    if grad is not None:
        _check_f32_device(grad, "grad", dev)
        if grad.shape != pred.shape:
            raise ValueError(f"grad {tuple(grad.shape)} and pred {tuple(pred.shape)} differ in shape")
        if _overlaps(grad, pred) or _overlaps(grad, gt):
            raise ValueError("grad overlaps pred or gt")
    if upstream is not None:
        _check_f32_device(upstream, "upstream", dev)
        if upstream.numel() != 1:
            raise ValueError(f"upstream must hold one element, got {tuple(upstream.shape)}")
        if _overlaps(upstream, pred) or _overlaps(upstream, gt) or (grad is not None and _overlaps(upstream, grad)):
            raise ValueError("upstream overlaps pred, gt or grad")
    L = hip.lib()
    size = ctypes.sizeof(hip.VoxLossGradCoeffs)
    ws_bytes = getattr(L, entry + "_workspace_bytes")(*dims, ctypes.byref(coef), size)
    if ws_bytes == 0:
        raise hip.V2ceHipError(f"{entry}: unsupported shape {tuple(pred.shape)} for these coefficients")
    with torch.cuda.device(dev):
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        if grad is None:
            grad = torch.empty_like(pred)
        hip.check(getattr(L, entry)(pred.data_ptr(), gt.data_ptr(), *dims, ctypes.byref(coef), size, hip.ptr(upstream),
                                    grad.data_ptr(), ws.data_ptr(), ws_bytes, hip.stream_ptr(dev)), entry)
    return grad


def voxel_loss_grads_batch(pred: torch.Tensor, gt: torch.Tensor, *, loss: Sequence[str] = DEFAULT_LOSS, ef_type="c+cl",
                           add_base_loss=False, alpha_pyramid=1000, alpha_ef=0.5, alpha_efc=5, alpha_match=0.5,
                           alpha_compensation=1, alpha_pt=1, alpha_norm=1e-5, stages=1,
                           upstream: Optional[torch.Tensor] = None, stats: Optional[VoxLosses] = None,
                           grad: Optional[torch.Tensor] = None, coef: Optional[hip.VoxLossGradCoeffs] = None) -> torch.Tensor:
    """d calculate_loss(pred, gt, loss=loss, <options>)[0] / d pred for ``pred``, ``gt`` [B, L, 20, H, W] (f32, contiguous,
    one device): an f32 tensor shaped like ``pred``, every element written.  ``stages``: the number of refinement stages
    the total averages over (this call is one of them).  ``upstream``: one f32 on the device that multiplies the
    gradient (an incoming ``grad_output``); nothing is copied to the host.  ``stats``: the forward statistics of this
    pair, if at hand -- only 'norml2' needs them, and they are computed here (one synchronisation) when it does and
    they were not passed.  ``grad``: write here instead of allocating; it must not overlap ``pred`` or ``gt``.
    ``coef``: the factors themselves, instead of ``loss`` and its options (``grad_coeffs``)."""
    dims = _check_grad_pair(pred, gt, 5)
    if coef is None:
        loss = check_loss_names(loss)
        sq = None
        if "norml2" in loss:
            if stats is None:
                stats = voxel_losses_batch(pred, gt, terms=())
            sq = float(np.sum(stats.pred_sq_sum))
        coef = grad_coeffs(dims, loss, ef_type=ef_type, add_base_loss=add_base_loss, alpha_pyramid=alpha_pyramid,
                           alpha_ef=alpha_ef, alpha_efc=alpha_efc, alpha_match=alpha_match,
                           alpha_compensation=alpha_compensation, alpha_pt=alpha_pt, alpha_norm=alpha_norm, stages=stages,
                           pred_sq_sum=sq)
    return _run_grads("v2ce_voxloss_grads", pred, gt, dims, coef, upstream, grad)


def volume_loss_grads_batch(pred: torch.Tensor, gt: torch.Tensor, *, loss: Sequence[str] = VOLUME_LOSS_NAMES,
                            add_base_loss=False, alpha_pyramid=1000, stages=1, upstream: Optional[torch.Tensor] = None,
                            grad: Optional[torch.Tensor] = None,
                            coef: Optional[hip.VoxLossGradCoeffs] = None) -> torch.Tensor:
    """The [N, D, H, W] counterpart of ``voxel_loss_grads_batch``: the 'pyramid' and 'pt' terms of the volumes that
    'b l (p c) h w -> (b p) (l c) h w' makes, weighted as ``calculate_loss`` weights them."""
    dims = _check_grad_pair(pred, gt, 4)
    if coef is None:
        coef = grad_coeffs(dims, loss, add_base_loss=add_base_loss, alpha_pyramid=alpha_pyramid, stages=stages)
    return _run_grads("v2ce_volume_loss_grads", pred, gt, dims, coef, upstream, grad)


class _Stage:
    """What one refinement stage's autograd node computes: the loss list and options of its share of the total, and
    after the forward its statistics (per row)."""

    def __init__(self, loss, opts, stages=1, volume=False):
        self.loss, self.opts, self.stages, self.volume = tuple(loss), {**_OPTION_DEFAULTS, **opts}, stages, volume
        self.stats = None


class _StageLoss(torch.autograd.Function):
    """forward: the statistics call of today and this stage's share of the weighted total (its terms / stages) as a
    0-d f32 device tensor; backward: one gradient call that reads grad_output on the device."""

    @staticmethod
    def forward(ctx, pred, gt, plan):
        terms = terms_for(plan.loss)
        plan.stats = (volume_losses_batch if plan.volume else voxel_losses_batch)(pred, gt, terms=terms)
        total, _ = loss_values([plan.stats.total()], plan.loss, **plan.opts)
        ctx.save_for_backward(pred, gt)
        ctx.plan = plan
        ctx.set_materialize_grads(False)
        return _scalar(np.float32(np.float64(total) / plan.stages) if plan.stages != 1 else total, pred.device)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        if grad_output is None or not ctx.needs_input_grad[0]:
            return None, None, None
        pred, gt = ctx.saved_tensors
        plan = ctx.plan
        up = grad_output.detach().to(device=pred.device, dtype=torch.float32).reshape(1).contiguous()
        o = plan.opts
        if plan.volume:
            g = volume_loss_grads_batch(pred, gt, loss=plan.loss, add_base_loss=o["add_base_loss"],
                                        alpha_pyramid=o["alpha_pyramid"], stages=plan.stages, upstream=up)
        else:
            g = voxel_loss_grads_batch(pred, gt, loss=plan.loss, stages=plan.stages, upstream=up, stats=plan.stats, **o)
        return g, None, None
