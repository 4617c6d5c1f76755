"""float64 restatement, from the uint8 integers, of the formula behind v2ce_image_grad_batch / v2ce_image_units_grad
(csrc/imgrad.hip): the reference's get_batch_double_blurred_image_gradient (train/scripts/utils/image_derivative.py:38-75)
and the three-channel image units of train/scripts/data/event_pack_dataset.py:66-73.  It shares no code with either.

The reference's channel 2 comes out of two float32 convolutions, so its bytes are no contract: THIS is the truth the
kernel and the reference are both measured against (the goldens under tests/golden/.imgrad record the reference's own
error, recipe tests/make_imgrad_goldens.py).  The constants of the formula are the float32 blur taps (torchvision's
_get_gaussian_kernel1d in torch float32), taken here as exact numbers; everything else is float64.  Channels 0 / 1 are
float32 by definition -- three separately rounded operations -- and are restated in float32."""
import numpy as np

GOLDEN_NAMES = ("min_6x6", "ragged_7x70", "tile_edges", "r37x50", "ramp_12x13", "one_hot_9x9", "k5_s1p5_21x40",
                "two_packets", "flat_8x8")
TILE_H, TILE_W = 16, 64                           # the output tile of grad_blur_kernel (csrc/imgrad.hip: kTH, kTW)
MEAN, STD = 0.153, 0.165


def sobel_squares(frames):
    """int64 [..., H, W]: Gx^2 + Gy^2 of the zero-padded uint8 frames (F.conv2d(padding=1) is a cross-correlation)."""
    f = np.asarray(frames)
    assert f.dtype == np.uint8
    p = np.pad(f.astype(np.int64), [(0, 0)] * (f.ndim - 2) + [(1, 1), (1, 1)])
    H, W = f.shape[-2:]
    at = lambda dy, dx: p[..., 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    gx = (at(-1, 1) + 2 * at(0, 1) + at(1, 1)) - (at(-1, -1) + 2 * at(0, -1) + at(1, -1))
    gy = (at(1, -1) + 2 * at(1, 0) + at(1, 1)) - (at(-1, -1) + 2 * at(-1, 0) + at(-1, 1))
    return gx * gx + gy * gy


def gradient(frames):
    """float64 [S, L, H, W] from uint8 [S, L+1, H, W]: the larger Sobel magnitude of a pair's two frames, of the / 255 frames."""
    sq = sobel_squares(frames)
    return np.sqrt(np.maximum(sq[:, :-1], sq[:, 1:]).astype(np.float64)) / 255.0


def blur(g, taps):
    """float64: the 2-D blur with the outer product of ``taps``, the map reflected without repeating its edge."""
    w = np.asarray(taps, dtype=np.float64)
    r = w.size // 2
    H, W = g.shape[-2:]
    p = np.pad(g, [(0, 0)] * (g.ndim - 2) + [(r, r), (r, r)], mode="reflect")
    rows = sum(w[k] * p[..., :, k:k + W] for k in range(w.size))
    return sum(w[k] * rows[..., k:k + H, :] for k in range(w.size))


def blurred_gradient(frames, taps):
    """float64 [S, L, H, W] from uint8 [S, L+1, H, W]."""
    return blur(gradient(frames), taps)


def normalised_frames(frames, mean=MEAN, std=STD):
    """float32 [S, L, 2, H, W]: (u8 / 255 - mean) / std, three float32 operations (frame_normalize of the / 255 frames)."""
    x = np.asarray(frames).astype(np.float32) / np.float32(255)
    x = (x - np.float32(mean)) / np.float32(std)
    return np.stack([x[:, :-1], x[:, 1:]], axis=2)


def units_channel2(frames, taps):
    """float64 [S, L, H, W]: the blurred gradient over its packet's maximum (NaN for a packet of black frames) and the
    maxima float64 [S]."""
    b = blurred_gradient(frames, taps)
    m = b.reshape(b.shape[0], -1).max(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return b / m[:, None, None, None], m


def ulp32(x):
    """One float32 unit in the last place at |x|."""
    return float(np.spacing(np.float32(abs(x))))
