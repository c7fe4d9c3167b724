"""fp16 hi/lo split-MFMA conv (conv16.hip) vs an fp64 reference of the same op.

The split path must be as accurate as fp32 arithmetic: every case checks
rel = ||y - y64|| / ||y64|| against fp64 at 2e-6 (fp32 summation alone is ~1e-7
here; bf16-level arithmetic would be ~1e-3), and the fp32 MFMA kernel on the same
inputs for scale.  Also covers the fused epilogue (mask, Gram-backward phase 2,
ReLU+MaxPool backward, out_amax), tiny/huge input scales, and padding channels."""
import pytest
import torch
import torch.nn.functional as F

from styletransfer_amd import _native as N
from styletransfer_amd import ops

pytestmark = pytest.mark.gpu
TOL64 = 2e-6


def rel(a, b):
    a = a.double().cpu()
    b = b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def rnd(*shape, dev, seed=0, scale=1.0, shift=0.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.rand(*shape, generator=g) * scale + shift).to(dev)


def vinput(x, mode):
    if mode == N.STX_IN_RELU:
        return F.relu(x)
    if mode == N.STX_IN_RELU_POOL2:
        return F.max_pool2d(F.relu(x), 2, 2)
    if mode == N.STX_IN_UPSAMPLE2:
        return F.interpolate(x, scale_factor=2, mode="nearest")
    return x


CASES = [
    # n, cin, cout, h, w, mode
    (1, 64, 64, 70, 130, N.STX_IN_RELU),
    (2, 64, 128, 34, 36, N.STX_IN_RELU_POOL2),
    (1, 128, 256, 40, 40, N.STX_IN_RELU_POOL2),
    (2, 128, 64, 12, 10, N.STX_IN_UPSAMPLE2),
    (2, 128, 128, 16, 16, N.STX_IN_RAW),
    (1, 20, 70, 33, 17, N.STX_IN_RAW),       # cin, cout not tile multiples
    (1, 16, 5, 9, 67, N.STX_IN_RELU),        # smallest eligible cout, ragged width
    # small grids with cout % 128 == 0: 128 x 128 blocks (WM = 2), ragged and exact
    (2, 128, 128, 18, 70, N.STX_IN_RAW),
    (2, 64, 256, 32, 64, N.STX_IN_RAW),
    (2, 128, 128, 64, 64, N.STX_IN_RAW),     # ITN residual conv shape
    # full-chip grids (many tiles per CU), every loader mode
    (2, 64, 64, 256, 256, N.STX_IN_RELU),
    (4, 64, 128, 128, 128, N.STX_IN_RAW),
    (4, 64, 128, 256, 256, N.STX_IN_RELU_POOL2),
    (8, 128, 64, 64, 64, N.STX_IN_UPSAMPLE2),
    (3, 48, 70, 150, 170, N.STX_IN_RELU),    # ragged tiles, 3 chunks, cout % 64 != 0
]


@pytest.mark.parametrize("case", CASES)
def test_split_conv_fwd(dev, case):
    n, cin, cout, h, w, mode = case
    x = rnd(n, cin, h, w, dev=dev, seed=1, scale=2, shift=-1)
    wgt = rnd(cout, cin, 3, 3, dev=dev, seed=2, scale=0.2, shift=-0.1)
    b = rnd(cout, dev=dev, seed=3)
    wt = ops.conv_weight_prep(wgt)
    w16 = ops.conv_weight_prep16(wgt)
    amax = torch.zeros(N.STX_AMAX_SLOTS, device=dev)
    y = ops.conv2d(x, wt, cin, cout, 3, in_mode=mode, bias=b, wt16=w16, out_amax=amax)
    y32 = ops.conv2d(x, wt, cin, cout, 3, in_mode=mode, bias=b)
    ref = F.conv2d(vinput(x.double().cpu(), mode), wgt.double().cpu(), b.double().cpu(),
                   padding=1)
    torch.cuda.synchronize()
    assert y.shape == ref.shape
    e16, e32 = rel(y, ref), rel(y32, ref)
    assert e16 < TOL64, (e16, e32)
    assert float(amax.max()) == float(y.abs().max())


@pytest.mark.parametrize("case", [(2, 32, 64, 64, 64), (1, 64, 128, 34, 70), (3, 16, 24, 9, 13),
                                  (8, 32, 64, 256, 256)])
def test_split_conv_stride2(dev, case):
    """3x3 stride-2 pad-1 forward (ITN downsampling convs, loader mode LM_S2) vs fp64,
    ragged output tiles included; out_amax is the exact max|y|."""
    n, cin, cout, h, w = case
    x = rnd(n, cin, h, w, dev=dev, seed=7, scale=2, shift=-1)
    wgt = rnd(cout, cin, 3, 3, dev=dev, seed=8, scale=0.2, shift=-0.1)
    b = rnd(cout, dev=dev, seed=9)
    assert ops.split_eligible(cin, cout, 3, 2)
    wt = ops.conv_weight_prep(wgt)
    w16 = ops.conv_weight_prep16(wgt)
    amax = torch.zeros(N.STX_AMAX_SLOTS, device=dev)
    y = ops.conv2d(x, wt, cin, cout, 3, stride=2, bias=b, wt16=w16, out_amax=amax)
    y32 = ops.conv2d(x, wt, cin, cout, 3, stride=2, bias=b)
    if n * h * w > 100_000:  # the ITN shape: against the fp32 MFMA kernel (no fp64 conv)
        assert rel(y, y32) < 1e-5
    else:
        ref = F.conv2d(x.double().cpu(), wgt.double().cpu(), b.double().cpu(), stride=2,
                       padding=1)
        assert y.shape == ref.shape
        assert rel(y, ref) < TOL64, (rel(y, ref), rel(y32, ref))
    torch.cuda.synchronize()
    assert float(amax.max()) == float(y.abs().max())


@pytest.mark.parametrize("case", [(8, 128, 64, 64, 64, False),    # ITN up-conv 1 (B = 8)
                                  (8, 64, 32, 128, 128, False),   # ITN up-conv 2
                                  (2, 32, 48, 20, 45, True),      # ragged tiles, relu_out
                                  (1, 16, 20, 17, 33, False),     # wo = 66, odd bands
                                  (2, 20, 40, 9, 40, True),       # ragged chunk, cout 40
                                  (1, 40, 72, 12, 24, False),     # cout > 64: two blocks
                                  (1, 128, 64, 270, 480, False)])  # video 1080p / 4
def test_split_conv_upsample_parity(dev, case):
    """The upsampled-input conv as four output-parity 2x2 convs over the input
    (stx_conv_params.wt16_up, summed weights W'[a][b][ry][rx]) vs fp64 of
    conv(nearest_x2(x)) (UpsampleConvLayer, stransfer/network.py:578-600), and the
    upsampled-halo kernel on the same inputs; out_amax is the exact max|y|."""
    n, cin, cout, h, w, relu = case
    x = rnd(n, cin, h, w, dev=dev, seed=17, scale=2, shift=-1)
    wgt = rnd(cout, cin, 3, 3, dev=dev, seed=18, scale=0.2, shift=-0.1)
    b = rnd(cout, dev=dev, seed=19)
    wt, w16 = ops.conv_weight_prep(wgt), ops.conv_weight_prep16(wgt)
    up = ops.conv_weight_prep16_up(wgt)
    amax = torch.zeros(N.STX_AMAX_SLOTS, device=dev)
    mode = N.STX_IN_UPSAMPLE2
    y = ops.conv2d(x, wt, cin, cout, 3, in_mode=mode, bias=b, wt16=w16, wt16_up=up,
                   relu_out=relu, out_amax=amax)
    y2 = ops.conv2d(x, wt, cin, cout, 3, in_mode=mode, bias=b, wt16=w16, relu_out=relu)
    torch.cuda.synchronize()
    assert float(amax.max()) == float(y.abs().max())
    if n * h * w * cin > 3_000_000:  # (no fp64 conv at the full sizes: the other kernel)
        assert rel(y, y2) < 1e-5, rel(y, y2)
        return
    ref = F.conv2d(vinput(x.double().cpu(), mode), wgt.double().cpu(), b.double().cpu(),
                   padding=1)
    if relu:
        ref = ref.relu()
    assert y.shape == ref.shape
    assert rel(y, ref) < TOL64, (rel(y, ref), rel(y2, ref))


@pytest.mark.parametrize("scale", [1e-9, 1.0, 3e4])
def test_split_conv_scales(dev, scale):
    """Per-tensor power-of-two scaling: tiny and large inputs keep fp32 accuracy."""
    n, cin, cout, h, w = 1, 32, 64, 24, 40
    x = rnd(n, cin, h, w, dev=dev, seed=4, scale=2 * scale, shift=-scale)
    wgt = rnd(cout, cin, 3, 3, dev=dev, seed=5, scale=0.2, shift=-0.1)
    wt = ops.conv_weight_prep(wgt)
    y = ops.conv2d(x, wt, cin, cout, 3, wt16=ops.conv_weight_prep16(wgt))
    ref = F.conv2d(x.double().cpu(), wgt.double().cpu(), padding=1)
    assert rel(y, ref) < TOL64


@pytest.mark.parametrize("case", [(2, 64, 64, 20, 36), (1, 128, 256, 16, 16),
                                  (1, 256, 128, 8, 8)])
def test_split_conv_dgrad(dev, case):
    n, cin, cout, h, w = case
    x = rnd(n, cin, h, w, dev=dev, seed=11, scale=2, shift=-1).double().cpu().requires_grad_()
    wgt = rnd(cout, cin, 3, 3, dev=dev, seed=12, scale=0.2, shift=-0.1)
    y = F.conv2d(x, wgt.double().cpu(), padding=1)
    dy = rnd(*y.shape, dev=dev, seed=13, scale=2e-3, shift=-1e-3)
    (ref,) = torch.autograd.grad(y, x, dy.double().cpu())
    wtT = ops.conv_weight_prep(wgt, transpose=True)
    dx = ops.conv2d(dy, wtT, cout, cin, 3, wt16=ops.conv_weight_prep16(wgt, transpose=True))
    assert rel(dx, ref) < TOL64


@pytest.mark.parametrize("case", [(2, 32, 64, 33, 30), (8, 32, 64, 128, 128), (2, 32, 64, 50, 98),
                                  (8, 32, 64, 256, 256), (4, 64, 128, 128, 128),
                                  (1, 32, 64, 34, 65), (2, 32, 64, 37, 99)])
def test_split_conv_dilate(dev, case):
    """stride-2 data gradient as a stride-1 conv over the zero-dilated input: widths > 32
    on the 64 x 4 parity-class tiles (only the taps that meet non-zero dilated positions
    run), incl. ragged tiles and the ImageTransformNet's two shapes at B = 8; narrow
    widths on the generic tiles.  Odd widths > 32 (65, 99): rows whose start is only 4-B
    aligned, so the epilogue's paired 8-B stores and its 4-B right-edge fallback both run
    (ADVICE r5)."""
    n, cin, cout, h, w = case
    x = rnd(n, cin, h, w, dev=dev, seed=14).double().cpu().requires_grad_()
    wgt = rnd(cout, cin, 3, 3, dev=dev, seed=15, scale=0.2, shift=-0.1)
    y = F.conv2d(x, wgt.double().cpu(), stride=2, padding=1)
    dy = rnd(*y.shape, dev=dev, seed=16, scale=2, shift=-1)
    (ref,) = torch.autograd.grad(y, x, dy.double().cpu())
    wtT = ops.conv_weight_prep(wgt, transpose=True)
    dx = ops.conv2d(dy, wtT, cout, cin, 3, in_mode=N.STX_IN_DILATE2, hv=h, wv=w,
                    wt16=ops.conv_weight_prep16(wgt, transpose=True))
    assert dx.shape == ref.shape
    assert rel(dx, ref) < TOL64


def test_split_conv_fused_epilogue(dev):
    """Data-gradient conv with ReLU mask + Gram-backward phase 2, and accumulate/aux."""
    n, c, h, w = 2, 64, 20, 36
    z = rnd(n, c, h, w, dev=dev, seed=91, scale=2, shift=-1)
    dy = rnd(n, c, h, w, dev=dev, seed=92, scale=2, shift=-1)
    wgt = rnd(c, c, 3, 3, dev=dev, seed=93, scale=0.2, shift=-0.1)
    t = rnd(c, c, dev=dev, seed=94)
    loss, coef = ops.style_loss(z, t, weight=2.0)
    s2 = torch.tensor(0.5, device=dev)
    wtT = ops.conv_weight_prep(wgt, transpose=True)
    w16 = ops.conv_weight_prep16(wgt, transpose=True)
    out = ops.conv2d(dy, wtT, c, c, 3, mask=z, p2_z=z, p2_coef=coef, p2_scale=s2, wt16=w16)
    out32 = ops.conv2d(dy, wtT, c, c, 3, mask=z, p2_z=z, p2_coef=coef, p2_scale=s2)
    assert rel(out, out32) < 2e-6
    aux = rnd(n, c, h, w, dev=dev, seed=96)
    old = rnd(n, c, h, w, dev=dev, seed=97)
    o1 = old.clone()
    ops.conv2d(dy, wtT, c, c, 3, aux=aux, aux_scale=-0.25, accumulate=True, relu_out=True,
               out=o1, wt16=w16)
    o2 = old.clone()
    ops.conv2d(dy, wtT, c, c, 3, aux=aux, aux_scale=-0.25, accumulate=True, relu_out=True,
               out=o2)
    assert rel(o1, o2) < 2e-6


@pytest.mark.parametrize("shape", [(1, 64, 512, 512), (1, 128, 256, 256), (2, 64, 160, 300),
                                   (4, 64, 128, 128)])
@pytest.mark.parametrize("scaled", [False, True])
def test_split_conv_fused_epilogue_large(dev, shape, scaled):
    """The Gram-backward data gradient at the VGG shapes (conv1_2^T at 512^2, conv2_2^T at
    256^2 with two 64-cout blocks, ragged tiles, a batch of 4): dZ = [Z > 0] conv^T(dY) + s2 A.Z against the fp32-MFMA kernel's fused
    epilogue, and out_amax is the exact max|dZ|."""
    n, c, h, w = shape
    z = rnd(n, c, h, w, dev=dev, seed=191, scale=2, shift=-1)
    dy = rnd(n, c, h, w, dev=dev, seed=192, scale=2e-3, shift=-1e-3)
    wgt = rnd(c, c, 3, 3, dev=dev, seed=193, scale=0.2, shift=-0.1)
    t = rnd(c, c, dev=dev, seed=194)
    _, coef = ops.style_loss(z, t, weight=2.0)
    s2 = torch.tensor(0.375, device=dev) if scaled else None
    wtT = ops.conv_weight_prep(wgt, transpose=True)
    w16 = ops.conv_weight_prep16(wgt, transpose=True)
    am = torch.zeros(N.STX_AMAX_SLOTS, device=dev)
    out = ops.conv2d(dy, wtT, c, c, 3, mask=z, p2_z=z, p2_coef=coef, p2_scale=s2, wt16=w16,
                     out_amax=am)
    out32 = ops.conv2d(dy, wtT, c, c, 3, mask=z, p2_z=z, p2_coef=coef, p2_scale=s2)
    torch.cuda.synchronize()
    assert rel(out, out32) < 2e-6, rel(out, out32)
    assert float(am.max()) == float(out.abs().max())


@pytest.mark.parametrize("shape", [(1, 64, 512, 512), (1, 128, 256, 256), (2, 64, 160, 300),
                                   (4, 64, 128, 128), (1, 64, 20, 34)])
@pytest.mark.parametrize("scaled", [False, True])
def test_split_phase2_precomputed_scale(dev, shape, scaled):
    """The Gram-backward phase on the fp16 split MFMA with A's scale precomputed by the
    batched Gram finalize (stx_gram_fin_job.coef_amax -> stx_conv_params.p2_wt_amax, the
    Gatys dZ1 / dZ3 launches): the finalize's amax is max|A| exactly, and the data gradient
    matches the fp32-MFMA phase (ragged width 34: the per-pixel z2 loads)."""
    n, c, h, w = shape
    z = rnd(n, c, h, w, dev=dev, seed=291, scale=2, shift=-1)
    dy = rnd(n, c, h, w, dev=dev, seed=292, scale=2e-3, shift=-1e-3)
    wgt = rnd(c, c, 3, 3, dev=dev, seed=293, scale=0.2, shift=-0.1)
    t = rnd(n, c, c, dev=dev, seed=294)
    ws = torch.empty(N.lib().stx_gram_ws(n, c, h * w), device=dev, dtype=torch.uint8)
    fin = ops.FinalizeBatch()
    _, coef = ops.style_loss(z, t, weight=2.0, diag_alpha=1e-3, defer_ws=ws, fin=fin)
    ca = torch.zeros(N.STX_AMAX_SLOTS, device=dev)
    assert len(fin.jobs) == 1
    fin.jobs[0].coef_amax = ca.data_ptr()
    fin.flush()
    torch.cuda.synchronize()
    assert float(ca.max()) == float(coef.abs().max())
    s2 = torch.tensor(-0.375, device=dev) if scaled else None
    wtT = ops.conv_weight_prep(wgt, transpose=True)
    w16 = ops.conv_weight_prep16(wgt, transpose=True)
    am = torch.zeros(N.STX_AMAX_SLOTS, device=dev)
    out = ops.conv2d(dy, wtT, c, c, 3, mask=z, p2_z=z, p2_coef=coef, p2_scale=s2, wt16=w16,
                     out_amax=am, p2_wt_amax=ca)
    out32 = ops.conv2d(dy, wtT, c, c, 3, mask=z, p2_z=z, p2_coef=coef, p2_scale=s2)
    # repeated launches give the same bits (a staging race showed up only as run-to-run
    # differences in the last 16 couts of a tile, two blocks per CU)
    reps = [ops.conv2d(dy, wtT, c, c, 3, mask=z, p2_z=z, p2_coef=coef, p2_scale=s2, wt16=w16,
                       p2_wt_amax=ca) for _ in range(3)]
    torch.cuda.synchronize()
    assert rel(out, out32) < 2e-6, rel(out, out32)
    assert float(am.max()) == float(out.abs().max())
    for r in reps:
        assert torch.equal(r, out)


@pytest.mark.parametrize("mode", [N.STX_IN_RELU, N.STX_IN_RELU_POOL2, N.STX_IN_UPSAMPLE2])
def test_split_conv_phase2_needs_raw_input(dev, mode):
    """The fused Gram-backward phase exists only for raw-input data gradients: any
    other loader mode on the split path is rejected, not silently dropped."""
    n, c, h, w = 1, 64, 16, 36
    hv, wv = {N.STX_IN_RELU: (h, w), N.STX_IN_RELU_POOL2: (h // 2, w // 2),
              N.STX_IN_UPSAMPLE2: (2 * h, 2 * w)}[mode]
    z = rnd(n, c, hv, wv, dev=dev, seed=91, scale=2, shift=-1)
    dy = rnd(n, c, h, w, dev=dev, seed=92, scale=2, shift=-1)
    wgt = rnd(c, c, 3, 3, dev=dev, seed=93, scale=0.2, shift=-0.1)
    _, coef = ops.style_loss(z, rnd(c, c, dev=dev, seed=94))
    wtT = ops.conv_weight_prep(wgt, transpose=True)
    w16 = ops.conv_weight_prep16(wgt, transpose=True)
    with pytest.raises(N.NativeError, match="raw-input"):
        ops.conv2d(dy, wtT, c, c, 3, in_mode=mode, p2_z=z, p2_coef=coef, wt16=w16)
        torch.cuda.synchronize()


def test_amax(dev):
    x = rnd(3, 5, 7, 11, dev=dev, seed=7, scale=4, shift=-2)
    x.view(-1)[123] = -9.5
    assert float(ops.amax(x).max()) == 9.5
    assert float(ops.amax(torch.zeros(0, device=dev)).max()) == 0.0
    big = rnd(1 << 22, dev=dev, seed=8, scale=2, shift=-1)
    big[777777] = 3.25
    g = ops.amax(big)
    assert g.numel() == N.STX_AMAX_SLOTS and float(g.max()) == 3.25


@pytest.mark.parametrize("shape", [(2, 64, 64, 20, 70), (1, 128, 128, 17, 99),
                                   # full-chip grids, ragged last row pair
                                   (2, 64, 64, 255, 258), (2, 64, 128, 128, 130)])
def test_split_conv_pool_out(dev, shape):
    """Fused VGG ReLU+MaxPool2d output (floor mode, odd sizes) beside y; bit-exact
    against pooling the kernel's own y."""
    n, cin, cout, h, w = shape
    x = rnd(n, cin, h, w, dev=dev, seed=31, scale=2, shift=-1)
    wgt = rnd(cout, cin, 3, 3, dev=dev, seed=32, scale=0.2, shift=-0.1)
    b = rnd(cout, dev=dev, seed=33, scale=0.2, shift=-0.1)
    wt = ops.conv_weight_prep(wgt)
    pool = torch.full((n, cout, h // 2, w // 2), float("nan"), device=dev)
    y = ops.conv2d(x, wt, cin, cout, 3, bias=b, wt16=ops.conv_weight_prep16(wgt),
                   pool_out=pool)
    assert torch.equal(pool, F.max_pool2d(F.relu(y), 2, 2))


def test_vgg_fused_pool_matches_unfused(dev):
    """VGG forward with the fused pool outputs == the RELU_POOL2 loader path."""
    from styletransfer_amd import vgg as V
    from styletransfer_amd import weights as W
    feat = V.VGGFeatures(V.load_vgg19_weights(), dev)
    x = torch.from_numpy(W.synthetic_image(3, (1, 3, 128, 160))).to(dev)
    zs = feat.forward(x)
    ref = []
    cur = x
    for l in range(5):
        cur = feat.conv(l, cur)
        ref.append(cur)
    for a, b in zip(zs, ref):
        assert rel(a, b) < 1e-6


@pytest.mark.parametrize("shape", [(1, 64, 64, 64), (2, 128, 24, 40), (1, 256, 16, 16),
                                   (1, 96, 9, 24), (3, 64, 8, 7), (1, 64, 512, 512),
                                   # C = 256 on the whole-triangle 8-wave kernel: the Gatys
                                   # conv3_1 tap (128 splits), fast_st's B = 8 at 64^2, a
                                   # ragged last split (960 px), and hw % 32 != 0 (fallback)
                                   (1, 256, 128, 128), (8, 256, 64, 64), (2, 256, 24, 40),
                                   (1, 256, 12, 10)])
def test_split_gram(dev, shape):
    """fp16 hi/lo split Gram partials (z_amax given) vs fp64, and the style loss /
    backward coefficients they feed vs the fp32 MFMA path."""
    b, c, h, w = shape
    z = rnd(b, c, h, w, dev=dev, seed=41, scale=2, shift=-1)
    am = ops.amax(z)
    g16 = ops.gram(z, z_amax=am)
    f = z.double().cpu().reshape(b, c, h * w)
    ref = torch.bmm(f, f.transpose(1, 2)) / (c * h * w)
    assert rel(g16, ref) < TOL64
    t = rnd(c, c, dev=dev, seed=42, scale=0.02)
    l16, a16 = ops.style_loss(z, t, weight=3.0, z_amax=am)
    l32, a32 = ops.style_loss(z, t, weight=3.0)
    assert rel(l16, l32) < 1e-5
    assert rel(a16, a32) < 1e-5


@pytest.mark.parametrize("case", [(1, 64, 64, 64, N.STX_IN_RELU, True),
                                  (2, 64, 38, 72, N.STX_IN_RELU, False),
                                  (1, 32, 30, 100, N.STX_IN_RAW, False),
                                  (1, 64, 256, 256, N.STX_IN_RELU, True),
                                  # Gatys conv1_2 at 512^2, and a batch of 2 at 256^2
                                  (1, 64, 512, 512, N.STX_IN_RELU, True),
                                  (2, 64, 256, 256, N.STX_IN_RELU, False),
                                  (3, 64, 200, 260, N.STX_IN_RAW, True),
                                  # 3 input channels (conv1_1, convfew.hip): 64 x 8 tiles
                                  (1, 3, 64, 128, N.STX_IN_RAW, False),
                                  (2, 3, 30, 70, N.STX_IN_RAW, False)])
def test_fused_gram_partials(dev, case):
    """Gram partials emitted by the conv epilogue (stx_conv_params.gram_part): their
    sum is the Gram of the conv output (vs fp64), the conv output and pooled output are
    unchanged, and style_loss_from_parts equals style_loss on the stored output."""
    n, cin, h, w, mode, pool = case
    cout = 64
    x = rnd(n, cin, h, w, dev=dev, seed=91, scale=2, shift=-1)
    wgt = rnd(cout, cin, 3, 3, dev=dev, seed=92, scale=0.1, shift=-0.05)
    bias = rnd(cout, dev=dev, seed=93, scale=0.2, shift=-0.1)
    wt = ops.conv_weight_prep(wgt)
    w16 = ops.conv_weight_prep16(wgt)
    nt = ops.conv_gram_tiles(cin, cout, h, w, n=n, in_mode=mode)
    tiles = -(-w // 64) * -(-h // (8 if cin == 3 else 4))
    assert nt == tiles, (nt, tiles)  # one partial per output tile
    parts = torch.full((n * nt * 4096,), float("nan"), device=dev)
    kw = {}
    if pool:
        kw["pool_out"] = torch.empty(n, cout, h // 2, w // 2, device=dev)
    y = ops.conv2d(x, wt, cin, cout, 3, in_mode=mode, bias=bias, wt16=w16, gram_part=parts,
                   **kw)
    kw2 = {}
    if pool:
        kw2["pool_out"] = torch.empty(n, cout, h // 2, w // 2, device=dev)
    y2 = ops.conv2d(x, wt, cin, cout, 3, in_mode=mode, bias=bias, wt16=w16, **kw2)
    assert torch.equal(y, y2)
    if pool:
        assert torch.equal(kw["pool_out"], kw2["pool_out"])
    assert torch.isfinite(parts).all()
    g = parts.view(n, nt, 64, 64).double().sum(1).cpu() / (cout * h * w)
    f = y.double().cpu().reshape(n, cout, h * w)
    ref = torch.bmm(f, f.transpose(1, 2)) / (cout * h * w)
    assert rel(g, ref) < TOL64, rel(g, ref)
    t = rnd(cout, cout, dev=dev, seed=94, scale=0.02)
    ws = torch.empty(N.lib().stx_gram_ws(n, cout, h * w), device=dev, dtype=torch.uint8)
    lp, a_f = ops.style_loss_from_parts(parts, nt, n, cout, h * w, t, weight=3.0, defer_ws=ws)
    lf = torch.zeros(1, device=dev)
    ops.loss_finalize([lp], lf)
    l32, a32 = ops.style_loss(y, t, weight=3.0)
    assert rel(lf[0], l32) < 1e-5
    assert rel(a_f, a32) < 1e-5


@pytest.mark.parametrize("case", [(1, 64, 256, 256, N.STX_IN_RAW, False, False),   # Gatys conv2_1
                                  (1, 128, 256, 256, N.STX_IN_RELU, True, True),   # Gatys conv2_2
                                  (2, 128, 128, 128, N.STX_IN_RELU, True, True),
                                  (4, 64, 128, 128, N.STX_IN_RAW, False, False),   # 256 blocks
                                  (2, 128, 38, 72, N.STX_IN_RELU, False, True),    # ragged
                                  (3, 64, 70, 100, N.STX_IN_RAW, True, False)])
def test_fused_gram128(dev, case):
    """The 128-channel taps' Gram out of the conv epilogue (8-wave blocks, three 64 x 64
    tiles per block, conv_gram_tile128): the partials add up to the Gram of the stored
    output (vs fp64), y and the pooled output equal the unfused launch bit for bit, and
    style_loss_from_parts equals style_loss on y.  With mse_ref (the content tap): the
    epilogue's MSE sums give the same content / feature / feature-mse values as stx_mse on
    y (stransfer/network.py:134-201)."""
    n, cin, h, w, mode, pool, with_mse = case
    cout = 128
    x = rnd(n, cin, h, w, dev=dev, seed=291, scale=2, shift=-1)
    wgt = rnd(cout, cin, 3, 3, dev=dev, seed=292, scale=0.1, shift=-0.05)
    bias = rnd(cout, dev=dev, seed=293, scale=0.2, shift=-0.1)
    wt, w16 = ops.conv_weight_prep(wgt), ops.conv_weight_prep16(wgt)
    nt = ops.conv_gram_tiles(cin, cout, h, w, n=n, in_mode=mode)
    assert nt == -(-w // 64) * -(-h // 4), nt
    assert ops.conv_gram_groups(cin, cout, h, w, n=n, in_mode=mode) == 0  # 64-channel only
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    # more than one round of 8-wave blocks: the standalone Gram (fast_st's B = 8)
    assert ops.conv_gram_tiles(cin, cout, h, w, n=cus // nt + 1, in_mode=mode) == 0
    assert ops.conv_gram_tiles(cin, cout, h, w, n=n, in_mode=N.STX_IN_UPSAMPLE2) == 0
    parts = torch.full((n * 3 * nt * 4096,), float("nan"), device=dev)
    kw = {}
    if pool:
        kw["pool_out"] = torch.empty(n, cout, h // 2, w // 2, device=dev)
    c = None
    if with_mse:
        c = rnd(n, cout, h, w, dev=dev, seed=295, scale=1.0, shift=-0.4)
        kw["mse_ref"] = c
        kw["mse_parts"] = torch.full((2 * n * nt,), float("nan"), device=dev)
    y = ops.conv2d(x, wt, cin, cout, 3, in_mode=mode, bias=bias, wt16=w16, gram_part=parts, **kw)
    kw2 = {}
    if pool:
        kw2["pool_out"] = torch.empty(n, cout, h // 2, w // 2, device=dev)
    y2 = ops.conv2d(x, wt, cin, cout, 3, in_mode=mode, bias=bias, wt16=w16, **kw2)
    assert torch.equal(y, y2)
    if pool:
        assert torch.equal(kw["pool_out"], kw2["pool_out"])
    assert torch.isfinite(parts).all()
    pt = parts.view(n, 3, nt, 64, 64).double().sum(2).cpu()
    g = torch.empty(n, cout, cout, dtype=torch.float64)
    g[:, :64, :64], g[:, :64, 64:], g[:, 64:, 64:] = pt[:, 0], pt[:, 1], pt[:, 2]
    g[:, 64:, :64] = pt[:, 1].transpose(1, 2)
    g /= cout * h * w
    f = y.double().cpu().reshape(n, cout, h * w)
    ref = torch.bmm(f, f.transpose(1, 2)) / (cout * h * w)
    assert rel(g, ref) < TOL64, rel(g, ref)
    t = rnd(cout, cout, dev=dev, seed=294, scale=0.02)
    ws = torch.empty(N.lib().stx_gram_ws(n, cout, h * w), device=dev, dtype=torch.uint8)
    mo = torch.full((3,), float("nan"), device=dev) if with_mse else None
    lp, a_f = ops.style_loss_from_parts(parts, nt, n, cout, h * w, t, weight=3.0, defer_ws=ws,
                                        mse_parts=kw.get("mse_parts"), mse_out=mo)
    lf = torch.zeros(1, device=dev)
    ops.loss_finalize([lp], lf)
    l32, a32 = ops.style_loss(y, t, weight=3.0)
    assert rel(lf[0], l32) < 1e-5
    assert rel(a_f, a32) < 1e-5
    if with_mse:
        m32 = ops.mse(y, c, mode=2)
        yd, cd = y.double(), c.double()
        m64 = [float(((yd - cd) ** 2).mean()), float(((yd.relu() - cd.relu()) ** 2).mean())]
        assert abs(float(mo[0]) - m64[0]) < 1e-5 * m64[0], (float(mo[0]), m64[0])
        assert abs(float(mo[2]) - m64[1]) < 1e-5 * m64[1], (float(mo[2]), m64[1])
        assert rel(mo, m32) < 1e-5, (mo, m32)


@pytest.mark.parametrize("case", [(1, 64, 512, 512, N.STX_IN_RELU, True),   # Gatys conv1_2
                                  (8, 64, 256, 256, N.STX_IN_RELU, True),   # fast_st B8
                                  (2, 64, 38, 72, N.STX_IN_RELU, False),    # 1 ragged group
                                  (3, 64, 200, 260, N.STX_IN_RAW, True),    # 4 + 1 of 8 tiles
                                  (1, 3, 512, 512, N.STX_IN_RAW, False),    # conv1_1 (convfew)
                                  (2, 3, 30, 70, N.STX_IN_RAW, False)])
def test_fused_gram_grouped(dev, case):
    """In-launch group sums of the fused Gram partials (stx_conv_params.gram_cnt): the
    last block of each group of STX_GRAM_GROUP tiles sums the group's partials (sc1
    hand-off, ticket counter).  The group sums add up to the Gram (vs fp64), the conv
    and pooled outputs equal the ungrouped launch bit for bit, the counters are zero
    after every call, repeated calls give the same bits, and the style loss from the sums
    equals the direct one."""
    n, cin, h, w, mode, pool = case
    cout, G = 64, N.STX_GRAM_GROUP
    x = rnd(n, cin, h, w, dev=dev, seed=191, scale=2, shift=-1)
    wgt = rnd(cout, cin, 3, 3, dev=dev, seed=192, scale=0.1, shift=-0.05)
    bias = rnd(cout, dev=dev, seed=193, scale=0.2, shift=-0.1)
    wt, w16 = ops.conv_weight_prep(wgt), ops.conv_weight_prep16(wgt)
    nt = ops.conv_gram_tiles(cin, cout, h, w, n=n, in_mode=mode)
    ng = ops.conv_gram_groups(cin, cout, h, w, n=n, in_mode=mode)
    assert nt > 0 and ng == -(-nt // G), (nt, ng)
    slab = torch.full((n * (nt + ng) * 4096,), float("nan"), device=dev)
    cnt = torch.zeros(n * ng, device=dev, dtype=torch.int32)

    def run(kw_gram):
        kw = dict(kw_gram)
        if pool:
            kw["pool_out"] = torch.empty(n, cout, h // 2, w // 2, device=dev)
        y = ops.conv2d(x, wt, cin, cout, 3, in_mode=mode, bias=bias, wt16=w16, **kw)
        return y, kw.get("pool_out")

    y, p1 = run(dict(gram_part=slab, gram_cnt=cnt))
    torch.cuda.synchronize()
    assert int(cnt.abs().sum()) == 0
    sums = slab[n * nt * 4096:].clone()
    y2, p2 = run({})
    assert torch.equal(y, y2)
    if pool:
        assert torch.equal(p1, p2)
    assert torch.isfinite(sums).all()
    g = sums.view(n, ng, 64, 64).double().sum(1).cpu() / (cout * h * w)
    f = y.double().cpu().reshape(n, cout, h * w)
    ref = torch.bmm(f, f.transpose(1, 2)) / (cout * h * w)
    assert rel(g, ref) < TOL64, rel(g, ref)
    for _ in range(3):  # the counters rearm: same bits on every call
        run(dict(gram_part=slab, gram_cnt=cnt))
    torch.cuda.synchronize()
    assert int(cnt.abs().sum()) == 0
    assert torch.equal(slab[n * nt * 4096:], sums)
    t = rnd(cout, cout, dev=dev, seed=194, scale=0.02)
    ws = torch.empty(N.lib().stx_gram_ws(n, cout, h * w), device=dev, dtype=torch.uint8)
    lp, a_f = ops.style_loss_from_parts(sums, ng, n, cout, h * w, t, weight=3.0, defer_ws=ws)
    lf = torch.zeros(1, device=dev)
    ops.loss_finalize([lp], lf)
    l32, a32 = ops.style_loss(y, t, weight=3.0)
    assert rel(lf[0], l32) < 1e-5
    assert rel(a_f, a32) < 1e-5


@pytest.mark.parametrize("shape", [(1, 128, 256, 256), (2, 128, 24, 40), (1, 64, 32, 32),
                                   (1, 256, 16, 16), (3, 128, 8, 12)])
def test_style_content_loss(dev, shape):
    """ops.style_content_loss (the content tap: the style loss with the content, feature
    and feature-mse sums in the same pass over z where the Gram kernel allows it)
    equals style_loss + mse(mode=2) run separately."""
    b, c, h, w = shape
    z = rnd(b, c, h, w, dev=dev, seed=51, scale=2, shift=-1)
    cz = rnd(b, c, h, w, dev=dev, seed=52, scale=2, shift=-1)
    t = rnd(c, c, dev=dev, seed=53, scale=0.02)
    am = ops.amax(z)
    ws = torch.empty(N.lib().stx_style_content_ws(b, c, h * w), device=dev, dtype=torch.uint8)
    m = torch.full((3,), float("nan"), device=dev)
    lp, a_f = ops.style_content_loss(z, t, cz, m, weight=3.0, diag_alpha=0.5, z_amax=am,
                                     defer_ws=ws)
    lf = torch.zeros(1, device=dev)
    ops.loss_finalize([lp], lf)
    ws2 = torch.empty(N.lib().stx_gram_ws(b, c, h * w), device=dev, dtype=torch.uint8)
    lp2, a2 = ops.style_loss(z, t, weight=3.0, diag_alpha=0.5, z_amax=am, defer_ws=ws2)
    l2 = torch.zeros(1, device=dev)
    ops.loss_finalize([lp2], l2)
    m2 = ops.mse(z, cz, mode=2)
    assert torch.equal(lf, l2) and torch.equal(a_f, a2)
    assert rel(m, m2) < 1e-6, (m, m2)
    zd, cd = z.double().cpu(), cz.double().cpu()
    ref0 = ((zd - cd) ** 2).mean()
    mr = ((zd.clamp(min=0) - cd.clamp(min=0)) ** 2).mean()
    ref = torch.stack([ref0, mr * mr / z.numel(), mr])
    assert rel(m, ref) < 1e-5, (m, ref)


# (source, shape, with z_amax) or ("parts", b, c, nparts, with mse_parts): every Gram partial
# kernel, every fin_groups value (nsplit <= 8: 4, <= 16: 2, else 1) and the padded coef
FIN_CASES = [
    ("z", (2, 64, 8, 12), True),        # fp16 split, general kernel
    ("z", (1, 64, 9, 13), False),       # hw % 4 != 0: scalar fallback
    ("z", (1, 128, 6, 10), False),      # fp32 MFMA v2
    ("z", (1, 256, 8, 16), True),       # tri256
    ("z", (1, 48, 8, 12), False),       # coef pitch 64 > c: the padding is zeroed first
    ("zc", (2, 128, 8, 16), True),      # content tap, MSE fused into the tri pass
    ("zc", (1, 64, 8, 12), False),      # content tap, separate MSE pass
    ("parts", 2, 64, 3, False),
    ("parts", 2, 64, 12, False),
    ("parts", 2, 64, 20, False),
    ("parts", 1, 128, 5, True),         # content tap from a conv epilogue's sums
]
_fin_immediate = {}


def _fin_case(dev, i, fin=None):
    """Case i of FIN_CASES through its public op, immediate (fin None) or deferred into
    fin: (coef, deferred loss part, mse_out or None, tensors to keep until the flush)."""
    case, L, seed = FIN_CASES[i], N.lib(), 700 + 10 * i
    m = torch.full((3,), float("nan"), device=dev)
    if case[0] == "parts":
        _, b, c, nparts, with_mse = case
        hw, U = 96, 3 if c == 128 else 1
        parts = rnd(b * U * nparts * 4096, dev=dev, seed=seed, scale=2, shift=-1)
        t = rnd(c, c, dev=dev, seed=seed + 1, scale=0.02)
        mp = rnd(2 * b * nparts, dev=dev, seed=seed + 2) if with_mse else None
        ws = torch.empty(L.stx_gram_ws(b, c, hw), device=dev, dtype=torch.uint8)
        lp, coef = ops.style_loss_from_parts(parts, nparts, b, c, hw, t, weight=3.0,
                                             diag_alpha=0.5, defer_ws=ws, fin=fin, mse_parts=mp,
                                             mse_out=m if with_mse else None)
        return coef, lp, (m if with_mse else None), (parts, t, mp, ws)
    kind, (b, c, h, w), with_amax = case
    z = rnd(b, c, h, w, dev=dev, seed=seed, scale=2, shift=-1)
    t = rnd(b, c, c, dev=dev, seed=seed + 1, scale=0.02)
    am = ops.amax(z) if with_amax else None
    if kind == "zc":
        cz = rnd(b, c, h, w, dev=dev, seed=seed + 2, scale=2, shift=-1)
        ws = torch.empty(L.stx_style_content_ws(b, c, h * w), device=dev, dtype=torch.uint8)
        lp, coef = ops.style_content_loss(z, t, cz, m, weight=3.0, diag_alpha=0.5, z_amax=am,
                                          defer_ws=ws, fin=fin)
        return coef, lp, m, (z, t, am, cz, ws)
    ws = torch.empty(L.stx_gram_ws(b, c, h * w), device=dev, dtype=torch.uint8)
    lp, coef = ops.style_loss(z, t, weight=3.0, diag_alpha=0.5, z_amax=am, defer_ws=ws, fin=fin)
    return coef, lp, None, (z, t, am, ws)


def _fin_results(dev, coef, lp, m):
    loss = torch.zeros(1, device=dev)
    ops.loss_finalize([lp], loss)
    torch.cuda.synchronize()
    return coef, loss, m


def _fin_reference(dev, i):
    if i not in _fin_immediate:
        coef, lp, m, _ = _fin_case(dev, i)
        _fin_immediate[i] = _fin_results(dev, coef, lp, m)
    return _fin_immediate[i]


def _fin_assert_same(got, want, i):
    for g, w in zip(got, want):
        assert (g is None) == (w is None), FIN_CASES[i]
        if g is not None:
            assert not torch.isnan(w).any() and torch.equal(g, w), FIN_CASES[i]


@pytest.mark.parametrize("i", range(len(FIN_CASES)))
def test_deferred_finalize_bit_identical(dev, i):
    """A finalize deferred into stx_gram_finalize_batch gives the bits of the immediate
    call (include/stx.h): coef, the loss and mse_out, for features and for precomputed
    partials, with and without the content companion."""
    want = _fin_reference(dev, i)
    fin = ops.FinalizeBatch()
    coef, lp, m, keep = _fin_case(dev, i, fin)
    assert len(fin.jobs) == 1
    fin.flush()
    _fin_assert_same(_fin_results(dev, coef, lp, m), want, i)


def test_deferred_finalize_batched_bit_identical(dev):
    """The same with up to STX_FIN_MAX jobs of different shapes in one flush (the batch
    kernel's block-range decode)."""
    for lo in range(0, len(FIN_CASES), N.STX_FIN_MAX):
        idx = range(lo, min(lo + N.STX_FIN_MAX, len(FIN_CASES)))
        fin = ops.FinalizeBatch()
        runs = [_fin_case(dev, i, fin) for i in idx]
        assert len(fin.jobs) == len(idx)
        fin.flush()
        for i, (coef, lp, m, keep) in zip(idx, runs):
            _fin_assert_same(_fin_results(dev, coef, lp, m), _fin_reference(dev, i), i)


@pytest.mark.parametrize("shape", [(2, 64, 20, 70), (1, 128, 34, 64), (1, 256, 16, 16),
                                   (1, 64, 9, 13), (1, 64, 128, 256), (3, 128, 32, 96),
                                   (2, 64, 2, 32), (2, 256, 32, 48)])
def test_split_gram_bwd(dev, shape):
    """Gram backward dz = s*A.z + unpool(dp)*(z>0) + aux as the split phase alone
    (1x1 mode) vs the fp32 MFMA 1x1 conv."""
    n, c, h, w = shape
    z = rnd(n, c, h, w, dev=dev, seed=51, scale=2, shift=-1)
    t = rnd(c, c, dev=dev, seed=52, scale=0.02)
    _, coef = ops.style_loss(z, t, weight=5.0)
    dp = rnd(n, c, h // 2, w // 2, dev=dev, seed=53, scale=2, shift=-1)
    aux = rnd(n, c, h, w, dev=dev, seed=54)
    s = torch.tensor(0.75, device=dev)
    a16 = ops.gram_bwd_fused(coef, z, acc_scale=s, up_dp=dp, aux=aux, aux_scale=-0.25,
                             z_amax=ops.amax(z))
    a32 = ops.gram_bwd_fused(coef, z, acc_scale=s, up_dp=dp, aux=aux, aux_scale=-0.25)
    assert rel(a16, a32) < 2e-6
    # without the unpool term (C = 256 takes the co-split streaming kernel)
    c16 = ops.gram_bwd_fused(coef, z, acc_scale=s, aux=aux, aux_scale=-0.25, z_amax=ops.amax(z))
    c32 = ops.gram_bwd_fused(coef, z, acc_scale=s, aux=aux, aux_scale=-0.25)
    assert rel(c16, c32) < 2e-6
    b16 = ops.gram_bwd_fused(coef, z, z_amax=ops.amax(z))
    f = z.double().cpu().reshape(n, c, h * w)
    A = coef.double().cpu()[:, :c, :c]
    ref = torch.bmm(A.transpose(1, 2), f).reshape(n, c, h, w)
    assert rel(b16, ref) < TOL64


@pytest.mark.parametrize("c", [64, 128])
def test_split_gram_bwd_window_ties(dev, c):
    """Quantised z: many 2x2 windows with tied maxima and exact zeros -- the pooled
    gradient must go to the first maximum in row-major order (max_pool2d backward)
    exactly as the fp32 path routes it (streaming kernel for C = 64/128)."""
    n, h, w = 2, 16, 64
    z = (rnd(n, c, h, w, dev=dev, seed=61, scale=4, shift=-2) * 2).round() / 2
    t = rnd(c, c, dev=dev, seed=62, scale=0.02)
    _, coef = ops.style_loss(z, t, weight=5.0)
    dp = rnd(n, c, h // 2, w // 2, dev=dev, seed=63, scale=2, shift=-1)
    zero = torch.zeros_like(coef)
    a16 = ops.gram_bwd_fused(zero, z, up_dp=dp, z_amax=ops.amax(z))
    a32 = ops.gram_bwd_fused(zero, z, up_dp=dp)
    assert torch.equal(a16, a32)
    # reference: autograd of max_pool2d(relu(z))
    zz = z.detach().cpu().double().requires_grad_(True)
    F.max_pool2d(F.relu(zz), 2, 2).backward(dp.cpu().double())
    assert torch.equal(a16.cpu().double(), zz.grad)
    b16 = ops.gram_bwd_fused(coef, z, up_dp=dp, z_amax=ops.amax(z))
    b32 = ops.gram_bwd_fused(coef, z, up_dp=dp)
    assert rel(b16, b32) < 2e-6


@pytest.mark.parametrize("case", [(8, 128, 128, 16, 32, N.STX_IN_RAW),
                                  (2, 64, 32, 20, 16, N.STX_IN_RELU),
                                  (2, 128, 64, 8, 16, N.STX_IN_UPSAMPLE2),
                                  (3, 40, 24, 9, 48, N.STX_IN_RAW),
                                  # cout <= 32: 32 x 64 wave tiles (two cin rows per lane)
                                  (2, 64, 32, 8, 16, N.STX_IN_UPSAMPLE2),
                                  (2, 72, 32, 12, 32, N.STX_IN_RAW),
                                  (1, 64, 16, 16, 32, N.STX_IN_RELU),
                                  # cout 64/128, cin % 64 == 0: the LDS-staged kernel
                                  (2, 64, 64, 12, 32, N.STX_IN_RELU),
                                  (1, 128, 128, 1, 16, N.STX_IN_RAW),
                                  (3, 192, 64, 10, 24, N.STX_IN_UPSAMPLE2),
                                  (1, 64, 128, 3, 16, N.STX_IN_RAW),
                                  # cout 128: two step groups per block (K2), ReLU input,
                                  # an odd step count (the second group's last step empty)
                                  (2, 128, 128, 6, 32, N.STX_IN_RELU),
                                  (3, 64, 128, 5, 48, N.STX_IN_RELU),
                                  (1, 128, 128, 3, 16, N.STX_IN_RAW),
                                  # cout 64, cin % 128 == 0: 128 cins per block
                                  (2, 256, 64, 6, 16, N.STX_IN_RAW),
                                  (1, 128, 64, 5, 32, N.STX_IN_RELU),
                                  # upsampled input as parity classes (wgrad16up_kernel):
                                  # the ITN up convs, ragged cin / cout tiles, CI2
                                  (2, 128, 64, 32, 32, N.STX_IN_UPSAMPLE2),
                                  (2, 64, 32, 48, 64, N.STX_IN_UPSAMPLE2),
                                  (1, 48, 40, 7, 16, N.STX_IN_UPSAMPLE2),
                                  (3, 24, 20, 5, 48, N.STX_IN_UPSAMPLE2)])
def test_split_wgrad(dev, case):
    """3x3 weight gradient on the split MFMA vs fp64 (and the fp32 MFMA kernel)."""
    n, cin, cout, h, w, mode = case
    x = rnd(n, cin, h, w, dev=dev, seed=61, scale=2, shift=-1)
    xv = vinput(x.double().cpu(), mode)
    wgt = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(xv, wgt, padding=1)
    dy = rnd(*y.shape, dev=dev, seed=62, scale=2e-3, shift=-1e-3)
    (ref,) = torch.autograd.grad(y, wgt, dy.double().cpu())
    assert ops.wgrad_path(n, cin, h, w, cout, 3, in_mode=mode) == N.STX_WGRAD_F16
    dw16 = ops.conv2d_wgrad(x, dy, cin, cout, 3, in_mode=mode)
    dw32 = ops.conv2d_wgrad(x, dy, cin, cout, 3, in_mode=mode, split=False)
    assert rel(dw16, ref) < TOL64, (rel(dw16, ref), rel(dw32, ref))
    acc = dw16.clone()
    ops.conv2d_wgrad(x, dy, cin, cout, 3, in_mode=mode, dw=acc, accumulate=True)
    assert rel(acc, 2 * ref) < TOL64


@pytest.mark.parametrize("case", [(2, 32, 64, 32, 64), (3, 24, 40, 18, 32), (1, 64, 128, 8, 128)])
def test_split_wgrad_stride2(dev, case):
    """3x3 stride-2 weight gradient (ITN downsampling convs, wgrad16 S2) vs fp64."""
    n, cin, cout, h, w = case
    x = rnd(n, cin, h, w, dev=dev, seed=64, scale=2, shift=-1)
    wgt = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x.double().cpu(), wgt, stride=2, padding=1)
    assert ops.wgrad_path(n, cin, h, w, cout, 3, stride=2) == N.STX_WGRAD_F16S2
    dy = rnd(*y.shape, dev=dev, seed=65, scale=2e-3, shift=-1e-3)
    (ref,) = torch.autograd.grad(y, wgt, dy.double().cpu())
    dw16 = ops.conv2d_wgrad(x, dy, cin, cout, 3, stride=2)
    assert rel(dw16, ref) < TOL64, rel(dw16, ref)
    acc = dw16.clone()
    ops.conv2d_wgrad(x, dy, cin, cout, 3, stride=2, dw=acc, accumulate=True)
    assert rel(acc, 2 * ref) < TOL64


@pytest.mark.parametrize("case", [(2, 3, 32, 64, 64), (2, 32, 3, 48, 80), (1, 1, 32, 20, 272),
                                  (3, 32, 2, 9, 16)])
def test_split_wgrad_9x9_few(dev, case):
    """ITN conv0 / conv22 weight gradient (9x9 pad 4, 3 <-> 32 channels, wgrad9.hip)
    vs fp64 autograd and the fp32 MFMA kernel; accumulate mode."""
    n, cin, cout, h, w = case
    x = rnd(n, cin, h, w, dev=dev, seed=71, scale=2, shift=-1)
    wgt = torch.zeros(cout, cin, 9, 9, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x.double().cpu(), wgt, padding=4)
    dy = rnd(*y.shape, dev=dev, seed=72, scale=2e-3, shift=-1e-3)
    (ref,) = torch.autograd.grad(y, wgt, dy.double().cpu())
    assert ops.wgrad_path(n, cin, h, w, cout, 9) == N.STX_WGRAD_FEW16
    dw16 = ops.conv2d_wgrad(x, dy, cin, cout, 9)
    dw32 = ops.conv2d_wgrad(x, dy, cin, cout, 9, split=False)
    assert rel(dw16, ref) < TOL64, (rel(dw16, ref), rel(dw32, ref))
    acc = dw16.clone()
    ops.conv2d_wgrad(x, dy, cin, cout, 9, dw=acc, accumulate=True)
    assert rel(acc, 2 * ref) < TOL64


@pytest.mark.parametrize("case", [((2, 32, 64, 32, 64), 3, 2, N.STX_WGRAD_F16S2),
                                  ((2, 3, 32, 64, 64), 9, 1, N.STX_WGRAD_FEW16),
                                  ((1, 128, 128, 3, 16), 3, 1, N.STX_WGRAD_F16),
                                  ((1, 8, 8, 6, 16), 3, 1, N.STX_WGRAD_F32)])
def test_wgrad_given_amax_bit_identical(dev, case):
    """One case per path: dW with the amax groups handed in (the trainers' arena bound)
    equals dW with them computed inside conv2d_wgrad, and a repeated call, bit for bit."""
    (n, cin, cout, h, w), ks, stride, path = case
    assert ops.wgrad_path(n, cin, h, w, cout, ks, stride=stride) == path
    x = rnd(n, cin, h, w, dev=dev, seed=66, scale=2, shift=-1)
    ho, wo = ops.conv_out_hw(h, w, ks, stride, ks // 2)
    dy = rnd(n, cout, ho, wo, dev=dev, seed=67, scale=2e-3, shift=-1e-3)
    own = ops.conv2d_wgrad(x, dy, cin, cout, ks, stride=stride)
    given = ops.conv2d_wgrad(x, dy, cin, cout, ks, stride=stride, x_amax=ops.amax(x),
                             dy_amax=ops.amax(dy))
    again = ops.conv2d_wgrad(x, dy, cin, cout, ks, stride=stride)
    assert torch.equal(own, given) and torch.equal(own, again)
    assert float(own.abs().max()) > 0


@pytest.mark.parametrize("shape", [(64, 64), (128, 32), (20, 70)])
def test_weight_prep16_pair(dev, shape):
    """Both split slabs in one call == the two single preps, bit for bit."""
    cout, cin = shape
    w = rnd(cout, cin, 3, 3, dev=dev, seed=91, scale=0.2, shift=-0.1)
    (a, am), (b, bm) = ops.conv_weight_prep16_pair(w)
    a1, am1 = ops.conv_weight_prep16(w)
    b1, bm1 = ops.conv_weight_prep16(w, transpose=True)
    assert torch.equal(a, a1) and torch.equal(b, b1)
    assert float(am.max()) == float(am1.max()) == float(w.abs().max())


@pytest.mark.parametrize("case", [(2, 64, 128, 32, 48), (1, 32, 64, 64, 64), (2, 64, 128, 17, 40),
                                  # producer/consumer kernel (the ITN up-conv at B8)
                                  (8, 32, 64, 128, 128)])
def test_split_dgrad_upsample_sum(dev, case):
    """UpsampleConvLayer backward (stransfer/network.py:583-605): the data gradient of a
    conv over the nearest-x2 upsampled input with the 2x2 sums fused into its epilogue
    (stx_conv_params.pool_sum) vs fp64 autograd of conv(upsample(x)), and against the
    unfused path (full-resolution dgrad + stx_upsample2x_bwd)."""
    n, cin, cout, h, w = case
    x = rnd(n, cin, h, w, dev=dev, seed=31, scale=2, shift=-1).double().cpu().requires_grad_()
    wgt = rnd(cout, cin, 3, 3, dev=dev, seed=32, scale=0.2, shift=-0.1)
    y = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), wgt.double().cpu(), padding=1)
    dy = rnd(*y.shape, dev=dev, seed=33, scale=2e-3, shift=-1e-3)
    (ref,) = torch.autograd.grad(y, x, dy.double().cpu())
    w16 = ops.conv_weight_prep16(wgt, transpose=True)
    dx = torch.full((n, cin, h, w), 7.0, device=dev)
    ops.conv2d(dy, None, cout, cin, 3, wt16=w16, in_amax=ops.amax(dy), pool_out=dx, pool_sum=True)
    assert rel(dx, ref) < TOL64
    dv = ops.conv2d(dy, None, cout, cin, 3, wt16=w16, in_amax=ops.amax(dy))
    assert rel(dx, ops.upsample2x_bwd(dv)) < 1e-6


@pytest.mark.parametrize("hw,scale", [(128, 1.0), (40, 1e-3), (18, 30.0)])
def test_composed_dgrad_weights(dev, hw, scale):
    """stx_conv_weight_compose16: the data gradient of conv3_1 with its Gram-backward
    operator folded into the weights, conv^T_{sAW}(z) == conv^T_W(s A z) (vgg.loss_backward's
    dP2 at B = 1, stransfer/network.py:92-123 through :264-314), against fp64 of the
    unfused form; the fused form at 2e-6 like every split kernel, plus the scale bound against the composed weights' fp64 maximum."""
    cout, cin = 256, 128
    g = torch.Generator(device="cpu").manual_seed(7)
    w = (torch.randn(cout, cin, 3, 3, generator=g) * 0.05).to(dev)
    A = (torch.randn(1, cout, cout, generator=g) * 1e-3).to(dev)
    z = (torch.randn(1, cout, hw, hw, generator=g) * 2.0).to(dev)
    s = torch.tensor([scale], device=dev)
    wT16 = ops.conv_weight_prep16(w, transpose=True)  # (slab, max|w|) of the plain weights
    bound = torch.zeros(N.STX_AMAX_SLOTS, device=dev)
    slab = ops.conv_weight_compose16(A, ops.amax(A), w, wT16[1], bound, scale=s)
    wc64 = scale * torch.einsum("ck,kx->cx", A[0].double(), w.double().reshape(cout, -1))
    # the slab's scale bound covers max|w'| (a loose power of two is as exact)
    assert float(bound.max()) >= float(wc64.abs().max())
    dz64 = scale * torch.einsum("ck,nchw->nkhw", A[0].double(), z.double())
    ref = F.conv_transpose2d(dz64, w.double(), padding=1)
    y = ops.conv2d(z, None, cout, cin, 3, wt16=(slab, bound), in_amax=ops.amax(z))
    assert rel(y, ref) < TOL64, rel(y, ref)
    # the unfused pair (1x1 split Gram backward, then the split data gradient) for scale
    dz = ops.gram_bwd_fused(A, z, acc_scale=s, z_amax=ops.amax(z))
    y2 = ops.conv2d(dz, ops.conv_weight_prep(w, transpose=True), cout, cin, 3, wt16=wT16)
    print(f"composed {rel(y, ref):.2e}, unfused {rel(y2, ref):.2e}")


@pytest.mark.parametrize("shape", [(1, 32, 32, 64, False), (2, 64, 32, 64, False),
                                   (1, 256, 256, 64, False), (1, 32, 32, 128, True),
                                   (1, 128, 128, 128, True), (2, 64, 32, 128, False)])
def test_unpool_gram_epilogue(dev, shape):
    """stx_conv_params.unpool_out: the pooled tap's ReLU+MaxPool backward and Gram backward
    in the epilogue of the data gradient that produces the pooled gradient (conv2_1^T in
    the Gatys iteration): dZ2 = unpool(d)[Z2 > 0] + s A Z2 with d never stored.  Against
    the unfused launches (conv2_1^T, then the streaming Gram backward) and fp64; ties in the
    2x2 windows (quantised z) exercise the first-maximum rule; out_amax is max|y|."""
    b, h, w, c, with_aux = shape          # d is h x w, z is 2h x 2w (c channels)
    z = rnd(b, c, 2 * h, 2 * w, dev=dev, seed=301, scale=2, shift=-1)
    z = (z * 8).round() / 8               # quantised: equal values inside many windows
    # the producing conv: conv2_1^T (128 -> 64) or conv3_1^T (256 -> 128)
    dz3 = rnd(b, 2 * c, h, w, dev=dev, seed=302, scale=2e-3, shift=-1e-3)
    wgt = rnd(2 * c, c, 3, 3, dev=dev, seed=303, scale=0.2, shift=-0.1)
    t = rnd(b, c, c, dev=dev, seed=304, scale=1e-2)
    aux = rnd(b, c, 2 * h, 2 * w, dev=dev, seed=305) if with_aux else None
    asc = -0.37 if with_aux else 0.0
    ws = torch.empty(N.lib().stx_gram_ws(b, c, 4 * h * w), device=dev, dtype=torch.uint8)
    fin = ops.FinalizeBatch()
    _, coef = ops.style_loss(z, t[0], weight=2.0, defer_ws=ws, fin=fin)
    ca = torch.zeros(N.STX_AMAX_SLOTS, device=dev)
    fin.jobs[0].coef_amax = ca.data_ptr()
    fin.flush()
    s2 = torch.tensor(0.75, device=dev)
    wtT = ops.conv_weight_prep(wgt, transpose=True)
    w16 = ops.conv_weight_prep16(wgt, transpose=True)
    zam = ops.amax(z)
    am = torch.zeros(N.STX_AMAX_SLOTS, device=dev)
    y = ops.conv2d(dz3, wtT, 2 * c, c, 3, wt16=w16, out_amax=am, aux=aux, aux_scale=asc,
                   unpool_out=(z, coef, ca, zam, s2))
    d = ops.conv2d(dz3, wtT, 2 * c, c, 3, wt16=w16)
    ref = ops.gram_bwd_fused(coef, z, up_dp=d, acc_scale=s2, z_amax=zam, aux=aux,
                             aux_scale=asc)
    torch.cuda.synchronize()
    assert y.shape == z.shape
    assert rel(y, ref) < 2e-6, rel(y, ref)
    assert float(am.max()) == float(y.abs().max())
    if b * h * w <= 4096:  # fp64 of the same math
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
        assert rel(y, up + gz) < 2e-6, rel(y, up + gz)


@pytest.mark.parametrize("case", [(1, 64, 64, 256, 256), (8, 64, 64, 64, 96)])
def test_pool_only_output(dev, case):
    """stx_conv_params.y = NULL with pool_out (the VGG content target's conv1_2): the pooled
    output equals the one the full launch writes, bit for bit, and no full-resolution
    output is written (a sentinel buffer stays untouched)."""
    n, cin, cout, h, w = case
    x = rnd(n, cin, h, w, dev=dev, seed=311, scale=2, shift=-1)
    wgt = rnd(cout, cin, 3, 3, dev=dev, seed=312, scale=0.2, shift=-0.1)
    b = rnd(cout, dev=dev, seed=313)
    wt, w16 = ops.conv_weight_prep(wgt), ops.conv_weight_prep16(wgt)
    am1 = torch.zeros(N.STX_AMAX_SLOTS, device=dev)
    am2 = torch.zeros(N.STX_AMAX_SLOTS, device=dev)
    p1 = torch.empty(n, cout, h // 2, w // 2, device=dev)
    p2 = torch.full_like(p1, 7.0)
    y = ops.conv2d(x, wt, cin, cout, 3, in_mode=N.STX_IN_RELU, bias=b, wt16=w16, pool_out=p1,
                   out_amax=am1)
    r = ops.conv2d(x, wt, cin, cout, 3, in_mode=N.STX_IN_RELU, bias=b, wt16=w16, pool_out=p2,
                   out_amax=am2, pool_only=True)
    torch.cuda.synchronize()
    assert r is p2
    assert torch.equal(p1, p2)
    assert float(am1.max()) == float(am2.max()) == float(y.abs().max())
