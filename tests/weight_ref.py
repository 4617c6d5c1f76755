"""f64 and bit-exact numpy references of the weight preparation stage (a plain module, not a conftest): the spectral-norm power
iteration of csrc/sn.hip and the split-half packers of conv3d.hip, conv3d_up.hip, conv3d_wt.hip and conv3d_head.hip.

Layouts (include/v2ce_hip.h and the comments at the pack kernels):
  plain   [plane][tap][Cin / 16][Cout][16] fp16, then {max |w / sigma|, pre-scale} (f32)
  up      the plain buffer with a 16-byte tail {max, pre-scale, 0, 0}, then the folded region of the first C0 channels,
          [plane][slot = 12 list + (4 dt + 2 a + b)][C0 / 16][Cout][16] for the nine lists documented in conv3d_up.hip
  wt      [plane][9 slot + 3 dh + dw][Cin / 16][Cout][16] with slot = the row of the F(2, 3) matrix G, then {bound, pre-scale, 0, 0}
  pred    [k][plane][o][16]: entry 8 half + j = channel (j & 3) + 8 (j >> 2) + 16 k + 4 half, then {pre-scale}
  head    [s][plane][co][8 h + j]: input channel h, tap 8 s + j (taps >= 27 zero), then {max |w|, pre-scale}
"""
import math

import numpy as np

U32 = 2.0 ** -24          # unit roundoff of f32
F16_MAX = 65504.0


def pow2_prescale(amax):
    """common.h pow2_prescale: the power of two that puts amax in [2^14, 2^15) (1 for amax <= 0 or NaN)."""
    amax = float(amax)
    if not amax > 0.0:
        return np.float32(1.0)
    _, e = math.frexp(amax)
    return np.float32(2.0 ** min(100, max(-100, 15 - e)))


def split(v32):
    """hi = f16(v), lo = f16(v - hi): both round to nearest even; v - hi is exact in f32."""
    v32 = np.asarray(v32, np.float32)
    hi = v32.astype(np.float16)
    lo = (v32 - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def split_err(lo):
    """Upper bound of |v - (hi + lo)|: the rounding of the residual to fp16 (2^-11 relative, 2^-25 absolute once subnormal)."""
    return np.abs(lo.astype(np.float64)) * 2.0 ** -11 * (1 + 2.0 ** -10) + 2.0 ** -25


# ---------------------------------------------------------------------------------------------------------------------
# spectral norm
# ---------------------------------------------------------------------------------------------------------------------
def half_step(A, x):
    """One half of the power iteration in f64: t = A x, y = t / |t|.  Returns (t, y, |t|, bar) where bar[i] bounds the distance
    of the kernel's f32 y[i] (csrc/sn.hip: f64 sums, then f32 roundings of t, of the norm, of norm + 1e-12 and of the quotient)
    from y[i]: five roundings of 2^-24 relative, the f64 sum's own error and the 1e-12 of the denominator."""
    A = np.asarray(A, np.float64)
    x = np.asarray(x, np.float64)
    t = A @ x
    mag = np.abs(A) @ np.abs(x)
    nt = float(np.sqrt(t @ t))
    y = t / nt if nt > 0 else np.zeros_like(t)
    bar = 5.0 * U32 * np.abs(y) * (1 + 1e-6) + (2.0 ** -48 * mag + 1e-12) / max(nt, 1e-300)
    return t, y, nt, bar


def ulps(got, want):
    """|got - want| in f32 ulps of want (at least the ulp of the smallest normal)."""
    want = np.asarray(want, np.float64)
    ulp = np.spacing(np.maximum(np.abs(want), 2.0 ** -126).astype(np.float32)).astype(np.float64)
    return np.abs(np.asarray(got, np.float64) - want) / ulp


def check_step(W, u_prev, v, u, sigma, sigma_slack=0.0):
    """The kernel's (v, u, sigma) of one power iteration from its own previous f32 u.  v is compared with the f64 half-step
    from u_prev, u and sigma with the f64 half-step from the kernel's v (so that every bar is a few ulps).  Returns the worst
    excess over the bars (<= 0 passes) and the worst ulps of v, u and sigma."""
    W = np.asarray(W, np.float64)
    _, v64, _, bv = half_step(W.T, u_prev)
    s64, u64, ns, bu = half_step(W, v)
    # sigma = sum u_i s_i with u = fl(s / den): |s| (1 + 2 x rounding of s_i, norm, den, quotient, result) + the f64 sums
    bs = (7.0 * U32 + sigma_slack) * ns + 2.0 ** -48 * float(np.abs(W) @ np.abs(np.asarray(v, np.float64)) @ np.abs(u64))
    ex = max(float((np.abs(np.asarray(v, np.float64) - v64) - bv).max()),
             float((np.abs(np.asarray(u, np.float64) - u64) - bu).max()),
             abs(float(sigma) - ns) - bs)
    return ex, float(ulps(v, v64).max()), float(ulps(u, u64).max()), float(ulps(sigma, ns))


def trajectory(W, u0, steps):
    """f64 power iteration from u0: [(u, v, sigma)] after every step (sigma = u . W v)."""
    W = np.asarray(W, np.float64)
    u = np.asarray(u0, np.float64)
    out = []
    for _ in range(steps):
        t = W.T @ u
        v = t / (np.linalg.norm(t) + 1e-12)
        s = W @ v
        u = s / (np.linalg.norm(s) + 1e-12)
        out.append((u, v, float(u @ s)))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# packers
# ---------------------------------------------------------------------------------------------------------------------
def quot32(w, sigma):
    """fl32(w / sigma) (sigma None: w)."""
    w = np.asarray(w, np.float32)
    return w if sigma is None else (w / np.float32(sigma)).astype(np.float32)


def decode(buf_u8, n_halves_per_plane):
    """(hi, lo) planes of a packed buffer (bytes) as fp16 arrays, and the f32 words behind them."""
    h = np.frombuffer(buf_u8.tobytes(), np.uint8)
    hi = h[:2 * n_halves_per_plane].view(np.float16)
    lo = h[2 * n_halves_per_plane:4 * n_halves_per_plane].view(np.float16)
    return hi, lo


def tail_of(buf_u8, off, count):
    return np.frombuffer(buf_u8.tobytes()[off:off + 4 * count], np.float32)


def up_offsets(parity):
    """Nearest 2x upsample, output row h = 2 i + parity: tap d in {-1, 0, +1} reads upsampled row h + d, i.e. source row
    i + ((parity + d) >> 1).  Returns, per folded tap a (the distinct source offsets in order), the taps d that land there."""
    src = {d: (parity + d) >> 1 for d in (-1, 0, 1)}
    offs = sorted(set(src.values()))
    return [[d for d in (-1, 0, 1) if src[d] == o] for o in offs]


def up_lists():
    """The nine tap lists of the folded region, each a [2][2] (a, b) table of signed (dh, dw) term lists.
    0..3: phase p = 2 ph + pw, the folded taps.  At an odd output size the last row (column) is even and its +1 neighbour is
    the zero padding, not the source pixel again: 4 + pw removes the phantom dh = +1 term of phase (0, pw) (folded along W as
    the phase is), 6 + ph the phantom dw = +1 term of phase (ph, 0), 8 adds back the corner's dh = dw = +1 term removed twice."""
    lists = []
    for ph in (0, 1):
        for pw in (0, 1):
            fh, fw = up_offsets(ph), up_offsets(pw)
            lists.append([[[(+1, dh, dw) for dh in fh[a] for dw in fw[b]] for b in (0, 1)] for a in (0, 1)])
    e = up_offsets(0)
    for pw in (0, 1):
        fw = up_offsets(pw)
        lists.append([[[(-1, dh, dw) for dh in e[a] if dh == 1 for dw in fw[b]] for b in (0, 1)] for a in (0, 1)])
    for ph in (0, 1):
        fh = up_offsets(ph)
        lists.append([[[(-1, dh, dw) for dh in fh[a] for dw in e[b] if dw == 1] for b in (0, 1)] for a in (0, 1)])
    lists.append([[[(+1, dh, dw) for dh in e[a] if dh == 1 for dw in e[b] if dw == 1] for b in (0, 1)] for a in (0, 1)])
    return lists


def up_fold_f64(w, sigma, C0):
    """f64 values (w / sigma, unscaled) of the folded region [108][C0/16][Cout][16], the sums of |terms| and term counts."""
    Cout = w.shape[0]
    g = np.asarray(w, np.float64)[:, :C0].reshape(Cout, C0, 3, 3, 3) / (1.0 if sigma is None else float(sigma))
    val = np.zeros((108, Cout, C0))
    mag = np.zeros_like(val)
    cnt = np.zeros(108)
    for li, tab in enumerate(up_lists()):
        for dt in range(3):
            for a in (0, 1):
                for b in (0, 1):
                    slot = li * 12 + dt * 4 + a * 2 + b
                    for sg, dh, dw in tab[a][b]:
                        val[slot] += sg * g[:, :, dt, dh + 1, dw + 1]
                        mag[slot] += np.abs(g[:, :, dt, dh + 1, dw + 1])
                    cnt[slot] = len(tab[a][b])
    lay = lambda x: x.reshape(108, Cout, C0 // 16, 16).transpose(0, 2, 1, 3)
    return lay(val), lay(mag), cnt


G_F23 = np.array([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]])   # Winograd F(2, 3): g -> G g


def wt_f64(w, sigma, ci0, cin):
    """f64 G-transformed w / sigma of input channels [ci0, ci0 + cin) along T: [4 * 9][cin/16][Cout][16], |G| g sums, counts."""
    Cout = w.shape[0]
    g = np.asarray(w, np.float64)[:, ci0:ci0 + cin].reshape(Cout, cin, 3, 9) / (1.0 if sigma is None else float(sigma))
    val = np.einsum("sk,ockt->sotc", G_F23, g)                 # [4][Cout][9][cin]
    mag = np.einsum("sk,ockt->sotc", np.abs(G_F23), np.abs(g))
    cnt = (G_F23 != 0).sum(1)
    lay = lambda x: x.transpose(0, 2, 3, 1).reshape(36, cin // 16, 16, Cout).transpose(0, 1, 3, 2)
    return lay(val), lay(mag), np.repeat(cnt, 9)


def pred_planes(w, cout):
    """v2ce_pack_pred_weights_f16x2 restated: [2][2][32][16] (hi, lo) and the pre-scale."""
    w = np.asarray(w, np.float32).reshape(cout, 32)
    s = pow2_prescale(np.abs(w).max())
    hi = np.zeros((2, 32, 16), np.float16)
    lo = np.zeros_like(hi)
    for k in range(2):
        for half in range(2):
            for j in range(8):
                c = (j & 3) + 8 * (j >> 2) + 16 * k + 4 * half
                h, l = split((w[:, c] * s).astype(np.float32))
                hi[k, :cout, 8 * half + j], lo[k, :cout, 8 * half + j] = h, l
    return hi, lo, s


def head_planes(w):
    """v2ce_pack_head_weights_f16x2 restated: w [32][2][27] -> [4][32][16] (hi, lo), {max |w|, pre-scale}."""
    w = np.asarray(w, np.float32).reshape(32, 2, 27)
    m = np.float32(np.abs(w).max())
    s = pow2_prescale(m)
    v = np.zeros((4, 32, 2, 8), np.float32)
    for s_ in range(4):
        for j in range(8):
            if 8 * s_ + j < 27:
                v[s_, :, :, j] = w[:, :, 8 * s_ + j] * s
    hi, lo = split(v.reshape(4, 32, 16))
    return hi, lo, np.array([m, s], np.float32)
