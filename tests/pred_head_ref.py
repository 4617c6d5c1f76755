"""numpy f64 restatement of the prediction head (include/v2ce_hip_train.h) in the reference's layouts:
feat [B, 32, L, H, W], y / upstream [B, Cout, L, H, W], weight [Cout, 32], bias [Cout].  Every product and sum is f64;
nothing is rounded here.  Helpers convert to and from the layouts of the kernels."""
import numpy as np

CIN = 32


def forward(feat, weight, bias):
    """relu(conv1x1x1(feat) + bias) in f64 -> [B, Cout, L, H, W]."""
    f, w = np.asarray(feat, np.float64), np.asarray(weight, np.float64).reshape(-1, CIN)
    pre = np.einsum("bclhw,oc->bolhw", f, w) + np.asarray(bias, np.float64)[None, :, None, None, None]
    return np.maximum(pre, 0.0)


def masked(y, upstream):
    """torch's relu backward on the result: upstream where y > 0, else 0 (a NaN in y gives 0)."""
    with np.errstate(invalid="ignore"):
        return np.where(np.asarray(y) > 0, np.asarray(upstream, np.float64), 0.0)


def grads(feat, y, upstream, weight):
    """-> dict d_weight [Cout, 32], d_bias [Cout], d_feat [B, 32, L, H, W], and abs_weight / abs_bias = the sums of the
    absolute values of the terms of d_weight / d_bias, all f64."""
    f, w = np.asarray(feat, np.float64), np.asarray(weight, np.float64).reshape(-1, CIN)
    m = masked(y, upstream)
    return {"d_weight": np.einsum("bolhw,bclhw->oc", m, f), "d_bias": m.sum(axis=(0, 2, 3, 4)),
            "d_feat": np.einsum("bolhw,oc->bclhw", m, w),
            "abs_weight": np.einsum("bolhw,bclhw->oc", np.abs(m), np.abs(f)), "abs_bias": np.abs(m).sum(axis=(0, 2, 3, 4))}


def positions(feat):
    B, _, L, H, W = np.asarray(feat).shape
    return B * L * H * W


def pitch_of(w):
    """V2ce3d._pitch: rows of at least 64 floats are padded to a multiple of 32."""
    return w if w < 64 else (w + 31) // 32 * 32


def to_c16(feat, pitch=None, fill=np.nan):
    """[B, 32, L, H, W] -> channels-last-16 [B, L, 2, H, pitch, 16] f32, padding columns filled with `fill`."""
    f = np.asarray(feat, np.float32)
    B, C, L, H, W = f.shape
    pitch = W if pitch is None else pitch
    out = np.full((B, L, 2, H, pitch, 16), fill, np.float32)
    out[:, :, :, :, :W, :] = f.reshape(B, 2, 16, L, H, W).transpose(0, 3, 1, 4, 5, 2)
    return out


def from_c16(c16, W):
    """channels-last-16 [B, L, 2, H, pitch, 16] -> [B, 32, L, H, W]."""
    c = np.asarray(c16)
    B, L, _, H, _, _ = c.shape
    return np.ascontiguousarray(c[:, :, :, :, :W, :].transpose(0, 2, 5, 1, 3, 4).reshape(B, 32, L, H, W))


def to_dense(y):
    """[B, Cout, L, H, W] -> the kernels' [B, L, Cout, H, W]."""
    return np.ascontiguousarray(np.asarray(y).transpose(0, 2, 1, 3, 4))


def from_dense(y):
    """[B, L, Cout, H, W] -> [B, Cout, L, H, W]."""
    return np.ascontiguousarray(np.asarray(y).transpose(0, 2, 1, 3, 4))


def ulp32(x):
    """The spacing of f32 at |x| (of the smallest normal below it)."""
    a = np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** -126).astype(np.float32)
    return np.spacing(a).astype(np.float64)
