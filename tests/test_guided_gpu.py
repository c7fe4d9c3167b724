"""Region-guided Gatys transfer on the GPU: the guided Gram kernels against the fp64
restatement (tests/guided_ref.py), and GuidedGatysEngine under the three-way protocol of
tests/test_multistyle_gpu.py (HIP error against fp64 at most max(3 x the torch-fp32 error,
2e-5), branch decisions forced to the engine's own).

Tolerances are the project's: split-MFMA kernels 2e-6 of fp64, fp32-MFMA Gram 2e-5
(tests/test_ops_gpu.py), loss values 1e-4."""
import os
import shutil

import numpy as np
import pytest
import torch
from PIL import Image

import forced_ref as FR
import guided_ref as GR
from conftest import REPO
from styletransfer_amd import _native as N
from styletransfer_amd import constants, ops
from styletransfer_amd import vgg as V
from styletransfer_amd import weights as W

pytestmark = pytest.mark.gpu

K, FLOOR = 3.0, 2e-5  # tests/test_multistyle_gpu.py
SPLIT, FP32 = 2e-6, 2e-5
SHAPES = [(1, 64, 32, 32, 2), (2, 128, 16, 24, 3), (1, 256, 8, 8, 4), (3, 96, 7, 9, 2)]
IDS = ["x".join(map(str, s)) for s in SHAPES]


def _rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _within(name, hip, r32, r64):
    e, r = _rel(hip, r64), _rel(r32, r64)
    print(f"{name}: hip {e:.2e} fp32 {r:.2e}")
    assert e <= max(K * r, FLOOR), f"{name}: hip {e:.2e} vs fp32 {r:.2e}"


def _weights(R, hw, seed, kind="soft"):
    """[R][hw] fp64 rows normalised to sum hw.  soft: random in (0, 1), region 0 zero over
    the first third of the pixels (whole split ranges without weight); small: region 0
    covers 2 % of the pixels (w_max ~ 50); binary: 0/1 masks; ones."""
    g = torch.Generator().manual_seed(seed)
    if kind == "ones":
        return torch.ones(R, hw, dtype=torch.float64)
    w = torch.rand(R, hw, generator=g, dtype=torch.float64) * 0.95 + 0.05
    if kind == "soft":
        w[0, :hw // 3] = 0
    elif kind == "small":
        w[0] = 0
        w[0, hw // 2:hw // 2 + max(1, hw // 50)] = 1
    elif kind == "binary":
        w = (w > 0.5).to(torch.float64)
        w[:, 0] = 1
    return GR.normalise(w)


def _case(shape, seed=0, zscale=1.0, kind="soft"):
    b, c, h, w, R = shape
    g = torch.Generator().manual_seed(seed)
    z = (torch.randn(b, c, h, w, generator=g) * zscale).float()
    wts = _weights(R, h * w, seed + 1, kind).float()
    # targets of the Gram's own scale (diagonal ~ 1 / c), well away from G itself so that
    # G - T does not cancel
    T = torch.randn(R, c, c, generator=g) * (2.0 / c * zscale * zscale)
    T = (0.5 * (T + T.transpose(1, 2))).float().contiguous()
    lam = [1.0 + 0.5 * r for r in range(R)]
    return z, wts, T, lam


def _forward(z, wts, T, lam, dev, weight=3.0, split=True):
    zd, wd = z.to(dev), wts.to(dev).contiguous()
    b, c = z.shape[:2]
    R = wts.shape[0]
    G = torch.empty((b, R, c, c), device=dev, dtype=torch.float32)
    za = ops.amax(zd) if split else None
    loss_r, coef = ops.guided_style_loss(zd, wd, T.to(dev), lam, weight=weight, z_amax=za,
                                         g_out=G)
    return G, loss_r, coef


def _check_forward(z, wts, T, lam, dev, tol, weight=3.0, split=True):
    G, loss_r, coef = _forward(z, wts, T, lam, dev, weight, split)
    z64, w64, T64 = z.double(), wts.double(), T.double()
    G64 = GR.guided_gram(z64, w64)
    l64 = GR.region_losses(z64, w64, T64)
    A64 = GR.coef(z64, w64, T64, lam, weight)
    c = z.shape[1]
    eG = _rel(G, G64)
    eA = _rel(coef[:, :, :c, :c], A64)
    eL = [abs(float(loss_r[r]) - float(l64[r])) / float(l64[r]) for r in range(len(lam))]
    print(f"G {eG:.2e} coef {eA:.2e} loss {max(eL):.2e}")
    assert eG <= tol, eG
    assert eA <= tol, eA
    assert max(eL) <= 1e-4, eL
    if coef.shape[-1] != c:  # the padding is zero
        assert float(coef[:, :, c:, :].abs().max()) == 0.0 == float(coef[:, :, :, c:].abs().max())


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_guided_forward_vs_fp64(dev, shape):
    """hw % 8 == 0: the split path (2e-6); (3,96,7,9): hw = 63, the fp32 path (2e-5)."""
    hw = shape[2] * shape[3]
    _check_forward(*_case(shape), dev, SPLIT if hw % 8 == 0 else FP32)


@pytest.mark.parametrize("variant", ["z1e-3", "z1e3", "small", "binary", "noamax"])
def test_guided_forward_variants(dev, variant):
    shape = SHAPES[0]
    if variant.startswith("z"):  # the amax exponents
        _check_forward(*_case(shape, zscale=float(variant[1:])), dev, SPLIT)
    elif variant == "noamax":  # the fp32 path on a shape the split path would take
        _check_forward(*_case(shape), dev, FP32, split=False)
    else:
        z, wts, T, lam = _case(shape, kind=variant)
        if variant == "small":
            assert 45 <= float(wts.max()) <= 55
        _check_forward(z, wts, T, lam, dev, SPLIT)


@pytest.mark.parametrize("shape", [(1, 64, 32, 32, 1), (2, 128, 16, 24, 1), (1, 256, 8, 8, 1)],
                         ids=["64", "128", "256"])
def test_guided_r1_ones_is_the_style_loss(dev, shape):
    z, wts, T, _ = _case(shape, kind="ones")
    G, loss_r, coef = _forward(z, wts, T, [1.0], dev, weight=3.0)
    zd = z.to(dev)
    za = ops.amax(zd)
    assert _rel(G[:, 0], ops.gram(zd, z_amax=za)) <= SPLIT
    loss, coef0 = ops.style_loss(zd, T[0].to(dev).contiguous(), weight=3.0, z_amax=za)
    assert _rel(coef[:, 0], coef0) <= FP32
    assert abs(float(loss_r[0]) - float(loss)) <= 1e-4 * abs(float(loss))


def _check_backward(shape, dev, split=True, accumulate=False, scale=None):
    b, c, h, w, R = shape
    z, wts, T, lam = _case(shape, seed=5)
    z64, w64 = z.double(), wts.double()
    A64 = GR.coef(z64, w64, T.double(), lam, 2.0)
    cp = ops.coef_pitch(c)
    coef = torch.zeros(b, R, cp, cp)
    coef[:, :, :c, :c] = A64.float()
    zd, wd, cd = z.to(dev), wts.to(dev).contiguous(), coef.to(dev)
    ref = GR.gram_bwd(coef[:, :, :c, :c].double(), z64, w64, 1.0 if scale is None else scale)
    base = torch.randn(z.shape, generator=torch.Generator().manual_seed(9)) * float(ref.std())
    dz = base.to(dev).clone() if accumulate else None
    s = None if scale is None else torch.tensor([scale], device=dev, dtype=torch.float32)
    out = ops.guided_gram_bwd(cd, zd, wd, dz=dz, acc_scale=s, accumulate=accumulate,
                              z_amax=ops.amax(zd) if split else None,
                              coef_amax=ops.amax(cd) if split else None)
    if accumulate:
        ref = ref + base.double()
    e = _rel(out, ref)
    print(f"dz {e:.2e}")
    assert e <= FP32, e


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_guided_backward_vs_fp64(dev, shape):
    _check_backward(shape, dev)


@pytest.mark.parametrize("variant", ["accumulate", "scale", "noamax", "noamax-ragged"])
def test_guided_backward_variants(dev, variant):
    if variant == "accumulate":
        _check_backward(SHAPES[1], dev, accumulate=True)
    elif variant == "scale":
        _check_backward(SHAPES[0], dev, scale=-0.375, accumulate=True)
    elif variant == "noamax":
        _check_backward(SHAPES[0], dev, split=False)
    else:
        _check_backward(SHAPES[3], dev, split=False, accumulate=True)


def test_guided_backward_512_channels(dev):
    """c = 512 takes the 32-pixel tile (the c x 64 slab would not fit 64 KB of LDS)."""
    _check_backward((1, 512, 6, 7, 2), dev)
    _check_backward((1, 512, 6, 7, 2), dev, split=False)


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3]], ids=["split", "fp32"])
def test_guided_kernels_are_deterministic(dev, shape):
    z, wts, T, lam = _case(shape)
    a = _forward(z, wts, T, lam, dev)
    b_ = _forward(z, wts, T, lam, dev)
    for u, v in zip(a, b_):
        assert torch.equal(u, v)
    zd, wd = z.to(dev), wts.to(dev).contiguous()
    amax = dict(z_amax=ops.amax(zd), coef_amax=ops.amax(a[2]))
    for kw in (amax, {}):
        d0 = ops.guided_gram_bwd(a[2], zd, wd, **kw)
        d1 = ops.guided_gram_bwd(a[2], zd, wd, **kw)
        assert torch.equal(d0, d1)


def test_guided_style_loss_module_autograd(dev):
    """network.GuidedStyleLoss: `.loss` = sum_r lam_r loss_r and its gradient through
    autograd.GuidedStyleLossFn (the upstream gradient as the device scale)."""
    from styletransfer_amd import network
    shape = SHAPES[1]
    z, wts, T, lam = _case(shape, seed=7)
    mod = network.GuidedStyleLoss(T, wts.reshape(shape[4], shape[2], shape[3]), lam)
    zd = z.to(dev).requires_grad_()
    assert mod(zd) is zd
    (mod.loss * 2.5).backward()
    z64 = z.double().requires_grad_()
    ref = (GR.region_losses(z64, wts.double(), T.double()) * torch.tensor(lam).double()).sum()
    (ref * 2.5).backward()
    assert abs(float(mod.loss.detach()) - float(ref.detach())) <= 1e-4 * abs(float(ref.detach()))
    assert _rel(zd.grad, z64.grad) <= FP32


# ------------------------------------------------------------------------------ engine
VGG_SEED = 1234


@pytest.fixture(scope="module")
def vgg_np():
    return W.vgg19_synthetic(VGG_SEED, 5)


@pytest.fixture(scope="module")
def feat(vgg_np, dev):
    return V.VGGFeatures(vgg_np, dev)


def _img(seed, h, w):
    return torch.from_numpy(W.synthetic_image(seed, (1, 3, h, w)))


def _feathered(h, w):
    """Complementary left / right guides with a linear seam a quarter of the width wide."""
    x = torch.arange(w, dtype=torch.float32)
    left = ((0.625 * w - x) / (0.25 * w)).clamp(0, 1)[None].expand(h, w)
    return torch.stack([left, 1 - left]).contiguous()


@pytest.mark.parametrize("hw", [(64, 64), (40, 24)], ids=["64x64", "40x24-ragged"])
def test_engine_iteration_three_way(dev, feat, vgg_np, hw):
    """One eager iteration, Adam left out.  At 40 x 24 tap 5 is 10 x 6 = 60 pixels: the
    ragged (fp32) forward path."""
    h, w = hw
    content, init = _img(12, h, w), _img(14, h, w)
    styles = [_img(11, h, w), _img(13, h + 8, w)]  # a style image of another size
    guides = _feathered(h, w)
    lam = [1.0, 0.5]
    eng = V.GuidedGatysEngine(feat, styles, content, guides, region_weights=lam, init=init)
    eng.adam = False
    eng._iteration()
    torch.cuda.synchronize()
    masks = FR.vgg_branches_from_z(eng.st.z)
    r64 = GR.engine_iteration(vgg_np, init, content, styles, guides, lam, masks, torch.float64)
    r32 = GR.engine_iteration(vgg_np, init, content, styles, guides, lam, masks, torch.float32)
    hip = eng.losses()
    for l in range(5):
        _within(f"style{l + 1}", hip[l], r32[0][l], r64[0][l])
    _within("regions", eng.region_losses(), r32[1], r64[1])
    _within("content", hip[5], r32[2], r64[2])
    _within("dx", eng.grad, r32[4], r64[4])
    assert abs(float(eng.total) - float(r64[3])) <= 1e-4 * abs(float(r64[3]))


def test_engine_r1_ones_is_the_unguided_engine(dev, feat):
    h = w = 64
    content, init, style = _img(12, h, w), _img(14, h, w), _img(11, h, w)
    eng = V.GuidedGatysEngine(feat, [style], content, torch.ones(1, h, w), init=init)
    eng.adam = False
    eng._iteration()
    x = init.to(dev).contiguous()
    targets = [t.reshape(t.shape[-2:]).contiguous() for t in feat.style_targets(style.to(dev))]
    c4 = V.content_target(feat, content.to(dev)).clone()
    total = torch.zeros((), device=dev)
    st = V.loss_forward(feat, targets, x, c4, folded_weights=(100_000.0, 1.0), total=total)
    dx = V.loss_backward(feat, st, feature_grad=False)
    ref = V.loss_values(st)
    assert _rel(eng.losses()[:6], ref[:6]) <= 2e-5
    for l in range(6):
        assert abs(float(eng.losses()[l]) - float(ref[l])) <= 2e-5 * abs(float(ref[l]))
    assert abs(float(eng.total) - float(total)) <= 2e-5 * abs(float(total))
    assert _rel(eng.grad, dx) <= 2e-5


def test_guided_style_targets(dev, feat):
    """No style guide: feat.style_targets' value.  An all-ones guide: the same Gram.  A
    half-image guide: the guided Gram of the style features (fp64 of the same Z)."""
    h, w = 48, 40
    style = _img(11, h, w).to(dev)
    plain = feat.style_targets(style)
    none = V.guided_style_targets(feat, [style])
    ones = V.guided_style_targets(feat, [style], [torch.ones(h, w)])
    guide = torch.zeros(h, w)
    guide[: h // 2] = 1
    half = V.guided_style_targets(feat, [style, style], [guide, None])
    zs = feat.forward(style)
    maps = GR.tap_maps(guide[None])
    for l in range(5):
        assert torch.equal(none[l][0], plain[l][0])
        assert _rel(ones[l][0], plain[l][0]) <= FP32
        ref = GR.guided_gram(zs[l].double().cpu(), maps[l])[0, 0]
        assert _rel(half[l][0], ref) <= FP32
        assert torch.equal(half[l][1], plain[l][0])
    with pytest.raises(ValueError, match="region 0"):
        V.guided_style_targets(feat, [style], [torch.zeros(h, w)])


def test_engine_regions_are_indexed_not_averaged(dev, feat):
    h = w = 64
    content = _img(12, h, w)
    guides = torch.zeros(2, h, w)
    guides[0, :, :w // 2] = 1
    guides[1, :, w // 2:] = 1
    out = []
    for second in (13, 15):
        eng = V.GuidedGatysEngine(feat, [_img(11, h, w), _img(second, h, w)], content, guides)
        eng.adam = False
        eng._iteration()
        out.append(eng.region_losses().clone())
    assert torch.equal(out[0][:, 0], out[1][:, 0])
    assert bool((out[0][:, 1] != out[1][:, 1]).all())


def test_engine_graph_replay_is_the_eager_iteration(dev, feat):
    h = w = 64
    args = ([_img(11, h, w), _img(13, h, w)], _img(12, h, w), _feathered(h, w))
    res = []
    for graph in (True, False):
        eng = V.GuidedGatysEngine(feat, *args)
        eng.run(3, graph=graph)
        torch.cuda.synchronize()
        res.append((eng.x.clone(), eng.total.clone()))
    assert torch.equal(res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1])
    assert float((res[0][0] - args[1].to(dev)).abs().max()) > 0


@pytest.fixture
def project_root(tmp_path, monkeypatch):
    """A scratch PROJECT_ROOT with the data layout the CLI reads and the CWD there."""
    for rel_path in ("data/dancing.jpg", "data/styles/picasso.jpg"):
        dst = tmp_path / rel_path
        dst.parent.mkdir(parents=True, exist_ok=True)
        shutil.copy(os.path.join(REPO, rel_path), dst)
    monkeypatch.setattr(constants, "PROJECT_ROOT_PATH", str(tmp_path))
    monkeypatch.chdir(tmp_path)
    return tmp_path


def test_cli_gatys_guided(dev, project_root, monkeypatch):
    from click.testing import CliRunner
    from styletransfer_amd import img_utils
    from styletransfer_amd.clis import cli
    m = np.zeros((120, 160), np.uint8)
    m[:, :90] = 255
    Image.fromarray(m, mode="L").save(project_root / "m0.png")
    Image.fromarray(255 - m, mode="L").save(project_root / "m1.png")
    seen = []
    orig = img_utils.imshow

    def spy(t, *a, **k):
        seen.append(t.detach().clone())
        return orig(t, *a, **k)
    monkeypatch.setattr(img_utils, "imshow", spy)
    r = CliRunner().invoke(cli, ["gatys_guided", "data/dancing.jpg",
                                 "-r", "data/styles/picasso.jpg:m0.png",
                                 "-r", "data/dancing.jpg:m1.png", "-s", "3"])
    assert r.exit_code == 0, r.output + repr(r.exception)
    got = np.asarray(Image.open(project_root / "results" / "gatys_guided.png"))
    content = img_utils.image_loader(str(project_root / "data" / "dancing.jpg"))
    assert got.shape == (constants.IMSIZE, constants.IMSIZE, 3)
    assert bool(torch.isfinite(seen[0]).all())
    assert float((seen[0] - content).abs().max()) > 0
    assert (got != np.asarray(img_utils.to_pil(content))).any()
