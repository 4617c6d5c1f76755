"""f64 convolution reference at a position set (shared by the f64 tests of the conv kernels; a plain module, not a conftest).

positions() picks the output positions a large launch is checked at: all positions of a few time steps, all positions on
the first two and last two rows and columns (the ragged boxes), and a seeded uniform fraction of the rest.  conv_at()
evaluates an f64 conv3d there (input patches gathered, one f64 matmul per chunk of positions)."""
import numpy as np
import torch
import torch.nn.functional as F


def time_steps(T):
    """First, last, and both members of a Winograd pair (all of them when T <= 4)."""
    j = 2 * ((T // 2) // 2)
    return sorted({0, T - 1, j, min(j + 1, T - 1)})


def positions(B, T, Ho, Wo, seed, frac=0.12):
    """Output positions (b, t, h, w): the time steps of time_steps(T), the first and last two rows and columns, and a seeded
    fraction `frac` of the rest, for every sequence b."""
    sel = np.zeros((T, Ho, Wo), bool)
    sel[time_steps(T)] = True
    sel[:, :2] = sel[:, -2:] = True
    sel[:, :, :2] = sel[:, :, -2:] = True
    rng = np.random.RandomState(seed)
    out = []
    for b in range(B):
        m = sel | (rng.random_sample(sel.shape) < frac)
        t, h, w = np.nonzero(m)
        out.append((np.full_like(t, b), t, h, w))
    return tuple(torch.from_numpy(np.concatenate(v)) for v in zip(*out))


def conv_at(x, w, stride, pos, chunk=4096):
    """f64 conv3d (padding k // 2, stride (1, s, s)) of x [B, C, T, H, W] with w [Cout, C, k, k, k] at the output
    positions pos = (b, t, h, w): [N, Cout]."""
    k = w.shape[2]
    p = k // 2
    xp = F.pad(x.double(), (p, p, p, p, p, p))
    wm = w.double().reshape(w.shape[0], -1).t()
    b, t, h, ww = pos
    out = []
    for i in range(0, b.numel(), chunk):
        bi, ti, hi, wi = b[i:i + chunk], t[i:i + chunk], h[i:i + chunk] * stride, ww[i:i + chunk] * stride
        cols = torch.stack([xp[bi, :, ti + dt, hi + dh, wi + dw] for dt in range(k) for dh in range(k) for dw in range(k)], dim=2)
        out.append(cols.reshape(cols.shape[0], -1) @ wm)
    return torch.cat(out)


def at(y, pos):
    """[B, C, T, H, W] at the positions: [N, C]."""
    b, t, h, w = pos
    return y[b, :, t, h, w]
