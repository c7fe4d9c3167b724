"""The unpool / Gram-backward epilogue (stx_conv_params.unpool_out, conv16.hip) at the chunk
counts and block forms its schedule branches on, which test_unpool_gram_epilogue (cin = 2c:
8 or 16 chunks) does not reach: the window pass runs inside the conv's K loop, four
accumulator elements per 16-channel chunk, with a remainder after short loops, and in the
two-group (K2) block each group takes half of the elements and group 1 hands its window
bits to group 0 with its sums.

Same references and bound as test_unpool_gram_epilogue: the unfused pair (the data gradient,
then the streaming Gram backward with up_dp) and fp64 of the same math, rel < 2e-6, on a z
quantised to eighths so that many windows hold ties.  Also the engine's guard: a feature
map that is not exactly twice its pooled size takes the streaming path."""
import pytest
import torch

from styletransfer_amd import _native as N
from styletransfer_amd import network, ops
from styletransfer_amd import weights as W

pytestmark = pytest.mark.gpu
TOL64 = 2e-6


def rel(a, b):
    a = a.double().cpu()
    b = b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def rnd(*shape, dev, seed=0, scale=1.0, shift=0.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.rand(*shape, generator=g) * scale + shift).to(dev)


def _operands(dev, b, cin, c, h, w, with_aux):
    """d = conv^T (cin -> c) is h x w; z is 2h x 2w with c channels."""
    z = rnd(b, c, 2 * h, 2 * w, dev=dev, seed=301, scale=2, shift=-1)
    z = (z * 8).round() / 8               # quantised: equal values inside many windows
    dz = rnd(b, cin, h, w, dev=dev, seed=302, scale=2e-3, shift=-1e-3)
    wgt = rnd(cin, c, 3, 3, dev=dev, seed=303, scale=0.2, shift=-0.1)
    t = rnd(b, c, c, dev=dev, seed=304, scale=1e-2)
    aux = rnd(b, c, 2 * h, 2 * w, dev=dev, seed=305) if with_aux else None
    ws = torch.empty(N.lib().stx_gram_ws(b, c, 4 * h * w), device=dev, dtype=torch.uint8)
    fin = ops.FinalizeBatch()
    _, coef = ops.style_loss(z, t[0], weight=2.0, defer_ws=ws, fin=fin)
    ca = torch.zeros(N.STX_AMAX_SLOTS, device=dev)
    fin.jobs[0].coef_amax = ca.data_ptr()
    fin.flush()
    wtT = ops.conv_weight_prep(wgt, transpose=True)
    w16 = ops.conv_weight_prep16(wgt, transpose=True)
    return z, dz, wtT, w16, coef, ca, aux


def _fused_and_pair(dev, z, dz, wtT, w16, coef, ca, aux, asc, s2, zam, cin, c):
    am = torch.zeros(N.STX_AMAX_SLOTS, device=dev)
    y = ops.conv2d(dz, wtT, cin, c, 3, wt16=w16, out_amax=am, aux=aux, aux_scale=asc,
                   unpool_out=(z, coef, ca, zam, s2))
    d = ops.conv2d(dz, wtT, cin, c, 3, wt16=w16)
    ref = ops.gram_bwd_fused(coef, z, up_dp=d, acc_scale=s2, z_amax=zam, aux=aux,
                             aux_scale=asc)
    torch.cuda.synchronize()
    return y, d, ref, am


CASES = {
    # b, cin, c, h, w, aux
    "1chunk": (1, 16, 64, 4, 32, False),       # the whole window pass in the remainder
    "3chunks": (1, 48, 64, 4, 32, False),      # odd count (not K2): loop part + remainder
    "k2-1chunk-aux": (1, 32, 128, 4, 32, True),  # K2, one chunk per group, grid.y = 2
    "k2-5chunks": (2, 160, 64, 8, 64, False),  # K2, five chunks per group, tiles and images
    "ragged-chunk": (1, 40, 64, 4, 32, False),  # 3 chunks, the last of 8 channels
}


@pytest.mark.parametrize("case", list(CASES), ids=list(CASES))
def test_unpool_schedule_shapes(dev, case):
    b, cin, c, h, w, with_aux = CASES[case]
    z, dz, wtT, w16, coef, ca, aux = _operands(dev, b, cin, c, h, w, with_aux)
    asc = -0.37 if with_aux else 0.0
    s2 = torch.tensor(0.75, device=dev)
    zam = ops.amax(z)
    y, d, ref, am = _fused_and_pair(dev, z, dz, wtT, w16, coef, ca, aux, asc, s2, zam, cin, c)
    assert y.shape == z.shape
    e = rel(y, ref)
    print(f"{case}: vs the unfused pair {e:.2e}")
    assert e < TOL64, e
    assert float(am.max()) == float(y.abs().max())
    # fp64 of the same math
    z64, d64 = z.double().cpu(), d.double().cpu()
    rz = z64.clamp_min(0)
    win = rz.reshape(b, c, h, 2, w, 2).permute(0, 1, 2, 4, 3, 5).reshape(b, c, h, w, 4)
    first = torch.nn.functional.one_hot(win.argmax(-1), 4).double()  # first max
    routed = (first * d64.unsqueeze(-1)).reshape(b, c, h, w, 2, 2)
    up = routed.permute(0, 1, 2, 4, 3, 5).reshape(b, c, 2 * h, 2 * w) * (z64 > 0)
    A = coef.double().cpu()[:, :c, :c]
    gz = float(s2) * torch.einsum("bcd,bchw->bdhw", A, z64)
    if with_aux:
        gz = gz + asc * aux.double().cpu()
    e64 = rel(y, up + gz)
    print(f"{case}: vs fp64 {e64:.2e}")
    assert e64 < TOL64, e64


def test_unpool_window_comparison_sequence(dev):
    """NaNs, signed-zero ties and all-negative windows: the fused epilogue routes d exactly
    where the unfused pair does (relu on the bits, strict > in slot order, the mask from the
    selected raw z).  A NaN of z reaches every channel of its pixel through A.z in both, so
    the NaN patterns must coincide; every other element agrees to 1e-5 of max|ref| -- two
    fp32 evaluations of the same sums differ by about 1e-6 of it, and a window routed to
    another slot differs by a whole |d|, asserted below to be far above that."""
    b, cin, c, h, w = 1, 32, 64, 4, 32
    z, dz, wtT, w16, coef, ca, aux = _operands(dev, b, cin, c, h, w, False)
    zam = ops.amax(z)                      # of the finite z: the bound both launches take
    # the A.z term brought to the size of d, so that the bound below resolves a routing error
    d0 = ops.conv2d(dz, wtT, cin, c, 3, wt16=w16)
    az = torch.einsum("bcd,bchw->bdhw", coef[:, :c, :c], z)
    s2 = (d0.abs().median() / az.abs().max()).reshape(())
    nan = float("nan")
    # (channel, window row, window column) <- the four slots [top-left, top-right, bottom-..]
    special = {
        (0, 0, 0): [0.5, nan, 0.75, 0.25],     # NaN loses every comparison: slot 2
        (1, 1, 3): [nan, 0.5, 0.75, 0.25],     # NaN first: nothing beats it, no routing
        (2, 0, 5): [-0.0, 0.0, -1.0, -2.0],    # zeros tie: slot 0, masked (z = -0 is not > 0)
        (3, 2, 7): [0.0, -0.0, 0.0, -0.0],
        (40, 3, 0): [0.5, 0.5, 0.5, 0.5],      # a four-way tie: slot 0
        (41, 1, 30): [-0.125, -1.0, -0.5, -2.0],  # all negative: nothing routed
        (33, 2, 16): [-1.0, -1.0, -1.0, -1.0],
    }
    for (k, wy, wx), v in special.items():
        z[0, k, 2 * wy, 2 * wx], z[0, k, 2 * wy, 2 * wx + 1] = v[0], v[1]
        z[0, k, 2 * wy + 1, 2 * wx], z[0, k, 2 * wy + 1, 2 * wx + 1] = v[2], v[3]
    y, d, ref, am = _fused_and_pair(dev, z, dz, wtT, w16, coef, ca, None, 0.0, s2, zam, cin, c)
    yn, rn = torch.isnan(y), torch.isnan(ref)
    assert torch.equal(yn, rn), (int(yn.sum()), int(rn.sum()))
    assert 0 < int(yn.sum()) < y.numel() // 8     # the NaN pixels only
    fin = ~rn
    bound = 1e-5 * float(ref[fin].abs().max())
    worst = float((y[fin] - ref[fin]).abs().max())
    print(f"worst element {worst:.3e}, bound {bound:.3e}, median |d| {float(d.abs().median()):.3e}")
    assert float(d.abs().median()) > 20 * bound   # a misrouted window would show
    assert worst <= bound, (worst, bound)
    assert torch.isnan(am.max())                  # out_amax: a NaN wins


def test_odd_feature_map_takes_streaming_path(dev):
    """A 9 x 65 image: Z2 is 65 wide and its floored pooled size 4 x 32 fits the unpool
    launch's tiles, but Z2 is not twice it -- the engine must take the streaming Gram
    backward there (the unpool launch refuses the shapes).  The fused engine's gradient
    against the generic per-piece autograd path, to the parity tests' tolerance."""
    shape = (1, 3, 9, 65)
    style = torch.from_numpy(W.synthetic_image(1000, shape)).to(dev)
    content = torch.from_numpy(W.synthetic_image(2000, shape)).to(dev)
    x0 = torch.from_numpy(W.synthetic_image(3000, shape)).to(dev)
    net = network.StyleNetwork(style, content)
    grads = []
    for generic in (False, True):
        x = x0.clone().requires_grad_()
        if generic:
            net._forward_generic(x, content, None)
        else:
            net(x, content)
        (net.get_total_current_style_loss(100_000) + net.get_total_current_content_loss()).backward()
        grads.append(x.grad.clone())
    torch.cuda.synchronize()
    e = rel(grads[0], grads[1])
    print(f"engine vs generic: {e:.2e}")
    assert e < 1e-4, e
