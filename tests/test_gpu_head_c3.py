"""GPU: the head convolution with THREE input channels in split-half arithmetic (v2ce_conv3d_head_f16x2 with C0 = 3 and the
table of v2ce_pack_head_weights_f16x2_c3; csrc/conv3d_head.hip) -- the first layer of a model built with
--apply_image_grad (train/main.py:203-204) -- against the float64 convolution at the tolerance of the two-channel head
tests (tests/test_gpu_upfold.py: 1e-5 abs + 1e-5 rel), and a whole three-channel V2ce3d against the oracle."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
TOL = 1e-5


def assert_close(a, b, what="", tol=TOL):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = np.abs(a - b) - tol * np.abs(b)
    i = np.unravel_index(np.argmax(err), err.shape)
    assert err[i] <= tol, f"{what}: max excess at {i}: got {a[i]!r} want {b[i]!r} (|d|={abs(a[i]-b[i]):.3e})"


def to_btchw(x_ncdhw):
    return x_ncdhw.permute(0, 2, 1, 3, 4).contiguous()


def _model(B):
    from v2ce_toolbox_amd.v2ce_3d import V2ce3d
    m = V2ce3d.__new__(V2ce3d)
    torch.nn.Module.__init__(m)
    m._maps, m.precision, m._slot = {}, "f16x2", 0
    m._prep = {"absmax": torch.zeros((8, B, 2), device="cuda")}
    return m


def _table(w):
    from v2ce_toolbox_amd import hip
    L = hip.lib()
    assert L.v2ce_pack_head_weights_f16x2_c3_bytes() == 6 * 2 * 32 * 16 * 2 + 16
    tab = torch.empty(L.v2ce_pack_head_weights_f16x2_c3_bytes() // 2, dtype=torch.float16, device="cuda")
    hip.check(L.v2ce_pack_head_weights_f16x2_c3(w.cuda().contiguous().data_ptr(), tab.data_ptr(), hip.stream_ptr("cuda")), "pack")
    return tab


def _head(x_ncdhw, tab, bias):
    """x [B, 3, T, H, W] on the host -> (y [B, 32, T, H, W] host, the range slots [8, B, 2])."""
    from v2ce_toolbox_amd.v2ce_3d import V2ce3d
    m = _model(x_ncdhw.shape[0])
    y = V2ce3d._head_split(m, to_btchw(x_ncdhw).cuda(), tab, bias.cuda())
    torch.cuda.synchronize()
    return V2ce3d.to_planar(y).permute(0, 2, 1, 3, 4).cpu().numpy(), m._prep["absmax"].cpu().numpy()


# (B, T, H, W, scale): below the (4, 4, 64) output box, one past it in T and W, three boxes along W; then the inputs 1000x down
# and up, which moves the pre-scale and the range-guard value of their slots.
#
# The tolerance of the two-channel head tests, 1e-5 abs + 1e-5 rel, is a statement about activations of unit scale: the test
# inputs there span -0.93 .. 5.1.  The layer is homogeneous -- conv, bias and LeakyReLU of (s x, s bias) are s times those of
# (x, bias) -- and every float32 result carries rounding error in proportion to s (at s = 1e3 one float32 rounding of a single
# product already exceeds 1e-5), so the scaled cases scale the bias with the input and state the same tolerance in the scaled
# unit: |got - want| / s <= 1e-5 + 1e-5 |want| / s.  For s = 1e-3 that is a thousand times tighter than the unscaled form.
CASES = [(1, 2, 5, 7, 1.0), (2, 5, 6, 66, 1.0), (1, 3, 9, 130, 1.0), (2, 5, 6, 66, 1e-3), (2, 5, 6, 66, 1e3)]


@pytest.mark.parametrize("case", CASES)
def test_head_c3_split_half_vs_f64(case):
    B, T, H, W, scale = case
    g = torch.Generator().manual_seed(11 + H + W)
    x = torch.rand(B, 3, T, H, W, generator=g) * 6.0 - 0.93          # the range of normalised frames
    x[:, 2] = torch.rand(B, T, H, W, generator=g)                    # the gradient channel lies in [0, 1]
    x[0] *= 0.01                                                      # sequence 0 lives 100x lower: its own pre-scale
    x *= scale
    w = torch.randn(32, 3, 3, 3, 3, generator=g) * (2.0 / 81) ** 0.5
    bias = 0.3 * scale * torch.randn(32, generator=g)
    got, slots = _head(x, _table(w), bias)
    want = F.leaky_relu(F.conv3d(x.double(), w.double(), bias.double(), 1, 1), 0.01).numpy()
    excess = np.abs(got / scale - want / scale) - TOL * np.abs(want / scale)
    print(f"head c3 {case}: max |d| / s = {np.abs(got - want).max() / scale:.3e}, max excess over the relative part {excess.max():.3e}")
    assert_close(got / scale, want / scale, f"head c3 {case}")
    # the table's tail: { max |w|, a power-of-two pre-scale that puts it in [2^14, 2^15) }
    tail = _table(w)[6 * 2 * 32 * 16:][:4].view(torch.float32).cpu().numpy()
    assert tail[0] == float(w.abs().max()) and 16384 <= tail[0] * tail[1] < 32768
    for b in range(B):
        xmax, ymax = float(x[b].abs().max()), float(np.abs(want[b]).max())
        assert abs(slots[0, b, 0] - xmax) <= 1e-6 * xmax                          # max |x| over the three planes
        assert abs(slots[1, b, 0] - ymax) <= 2e-5 * max(1.0, ymax)                # max |y|
        # the guard value, as for two channels (81 products instead of 54): 81 * 2^-25 * (max|w| / xs + max|x| / ws)
        xs, ws = 2.0 ** (15 - np.frexp(np.float32(xmax))[1]), float(tail[1])
        guard = 81 * 2.0 ** -25 * (float(tail[0]) / xs + xmax / ws)
        assert abs(slots[1, b, 1] - guard) <= 1e-5 * guard, (b, slots[1, b, 1], guard)


def test_head_c3_sequence_alone_and_in_a_batch():
    g = torch.Generator().manual_seed(5)
    x = torch.rand(3, 3, 5, 6, 66, generator=g) * 6.0 - 0.93
    x[0] *= 30
    x[2] *= 0.02
    w = torch.randn(32, 3, 3, 3, 3, generator=g) * (2.0 / 81) ** 0.5
    bias = 0.3 * torch.randn(32, generator=g)
    tab = _table(w)
    batch, slots = _head(x, tab, bias)
    for b in range(3):
        alone, s1 = _head(x[b:b + 1], tab, bias)
        assert alone.tobytes() == batch[b:b + 1].tobytes(), b
        assert s1[:2, 0].tobytes() == slots[:2, b].tobytes(), b


def test_head_rejects_other_channel_counts():
    import ctypes
    from v2ce_toolbox_amd import hip
    L = hip.lib()
    one = ctypes.c_void_p(16)
    for c0, want in ((1, -2), (4, -2)):
        d = hip.ConvDesc(B=1, T=2, C0=c0, H0=5, W0=7, C1=0, Hin=5, Win=7, Cout=32, Hout=5, Wout=7, ksize=3, stride_hw=1,
                         act=hip.ACT_LEAKY, tile_t=0, tile_h=0, tile_w=0, precision=hip.PRECISION_F16X2, W0_pitch=7,
                         Win_pitch=7, Wout_pitch=8, layout=hip.LAYOUT_C16, absmax_batch_stride=0)
        assert L.v2ce_conv3d_head_f16x2(ctypes.byref(d), one, one, one, one, None, None, None) == want
    assert L.v2ce_pack_head_weights_f16x2_c3(None, one, None) == -1


@pytest.fixture(scope="module")
def three_channel_case():
    """The state dict of synth.make_state_dict with a seeded (32, 3, 3, 3, 3) head of the same standard deviation, one
    [1, 2, 3, 32, 40] input from image_units_batch, and the oracle's voxels."""
    from oracle import unet as U
    from v2ce_toolbox_amd import image_derivative as ID
    from v2ce_toolbox_amd import synth
    sd = synth.make_state_dict(0)
    w2 = sd["UNet.head.conv3d.weight"]
    assert tuple(w2.shape) == (32, 2, 3, 3, 3)
    g = torch.Generator().manual_seed(2024)
    sd["UNet.head.conv3d.weight"] = torch.randn(32, 3, 3, 3, 3, generator=g) * float(w2.std())
    units, gmax = ID.image_units_batch(synth.synthetic_frames(3, 32, 40, seed=3))
    assert units.shape == (1, 2, 3, 32, 40) and float(gmax[0]) > 0
    x = units.cpu()
    assert float(x[:, :, 2].max()) == 1.0 and float(x[:, :, 2].min()) >= 0
    want = U.forward(U.clone_state(sd), x).numpy()
    return sd, x, want


@pytest.mark.parametrize("precision", ["f16x2", "f32"])
def test_three_channel_model_equals_oracle(three_channel_case, precision):
    from v2ce_toolbox_amd.v2ce_3d import V2ce3d
    sd, x, want = three_channel_case
    m = V2ce3d(in_channels=3, precision=precision)
    m.load_state_dict(sd, strict=True)
    m = m.eval().to("cuda")
    y = m(x.cuda()).cpu().numpy()
    assert (m._prep["head_split"] is not None) == (precision == "f16x2")             # the default path took the split head
    assert y.shape == want.shape
    err = np.abs(y - want)
    assert np.all(err <= 1e-5 + 1e-5 * np.abs(want)), (precision, err.max())
