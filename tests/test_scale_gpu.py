"""Scale control on the GPU: the fp32 resampler against the fp64 restatement
(tests/scale_ref.py), one style weight per tap under the three-way protocol of
tests/test_multistyle_gpu.py / test_guided_gpu.py (HIP error against fp64 at most max(3 x
the torch-fp32 error, 2e-5), branch decisions forced to the engine's own), and the drivers
of styletransfer_amd/scale.py against the sequences of calls they are defined as."""
import os
import shutil

import numpy as np
import pytest
import torch
from PIL import Image

import forced_ref as FR
import scale_ref as SR
from conftest import REPO
from styletransfer_amd import constants, ops, scale
from styletransfer_amd import vgg as V
from styletransfer_amd import weights as W

pytestmark = pytest.mark.gpu

K, FLOOR = 3.0, 2e-5  # tests/test_multistyle_gpu.py, tests/test_guided_gpu.py
EPS = 2.0 ** -24

# (n, c, hi, wi) -> (ho, wo)
SHAPES = [
    ((1, 3, 5, 7), (3, 2)),            # fewer outputs than a wave
    ((1, 3, 3, 2), (9, 11)),
    ((2, 3, 37, 53), (19, 27)),        # ragged, downscale, 4-8 taps
    ((2, 3, 37, 53), (74, 106)),
    ((1, 3, 100, 100), (141, 141)),    # non-integer ratio
    ((1, 3, 141, 141), (100, 100)),
    ((1, 64, 33, 31), (66, 62)),       # many planes, scalar path
    ((1, 3, 256, 256), (512, 512)),    # many blocks, vector path
    ((1, 3, 512, 512), (128, 128)),    # 8 / 16 taps
    ((1, 3, 64, 64), (64, 128)),       # one axis skipped
]
IDS = ["x".join(map(str, a)) + "-" + "x".join(map(str, b)) for a, b in SHAPES]


def _randn(shape, seed, offset=0.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) + offset


@pytest.mark.parametrize("filter", ["triangle", "cubic"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_resample_vs_fp64(dev, shape, filter):
    """|got - ref| <= (kx + ky + 4) 2^-24 sum|w_y| sum|w_x| |x| per element: one rounding
    per weight and one per fma."""
    (n, c, hi, wi), (ho, wo) = shape
    kx, ky = SR.taps(wi, wo, filter), SR.taps(hi, ho, filter)
    for offset in (0.0, 100.0):
        x = _randn((n, c, hi, wi), 3, offset)
        got = ops.resample2d(x.to(dev), (ho, wo), filter).cpu().double().numpy()
        ref = SR.resize(x.numpy(), ho, wo, filter)
        bound = (kx + ky + 4) * EPS * SR.abs_bound(x.numpy(), ho, wo, filter)
        ratio = float((np.abs(got - ref) / bound).max())
        print(f"{filter} +{offset}: kx {kx} ky {ky} worst |err| / bound {ratio:.3f}")
        assert got.shape == (n, c, ho, wo)
        assert ratio <= 1.0


@pytest.mark.parametrize("filter", ["triangle", "cubic"])
def test_resample_identity_and_reproducibility(dev, filter):
    x = _randn((1, 3, 96, 96), 4).to(dev)
    assert torch.equal(ops.resample2d(x, 96, filter), x)
    a = ops.resample2d(x, (72, 120), filter)
    assert torch.equal(ops.resample2d(x, (72, 120), filter), a)
    # [r, h, w] tensors, and an int size
    g = x[0]
    assert torch.equal(ops.resample2d(g, (72, 120), filter), a[0])
    assert torch.equal(ops.resample2d(g, 48, filter), ops.resample2d(x, (48, 48), filter)[0])


@pytest.mark.parametrize("size", [(19, 27), (76, 108)], ids=["scalar", "vector"])
def test_resample_plane_does_not_depend_on_its_batch(dev, size):
    x = _randn((3, 3, 37, 53), 5).to(dev)
    whole = ops.resample2d(x, size)
    for i in range(3):
        assert torch.equal(ops.resample2d(x[i:i + 1].contiguous(), size), whole[i:i + 1])


def test_resample_rejects_aliasing_and_cpu_tensors(dev):
    from styletransfer_amd import _native as N
    x = _randn((1, 3, 32, 32), 6).to(dev)
    with pytest.raises(N.NativeError, match="alias"):
        ops.resample2d(x, 32, out=x)
    with pytest.raises(N.NativeError):
        ops.resample2d(x.cpu(), 16)
    with pytest.raises(ValueError):
        ops.resample2d(x, 16, filter="lanczos")


def test_resample_graph_replay_is_the_eager_result(dev):
    x = _randn((1, 3, 64, 64), 7).to(dev)
    eager = ops.resample2d(x, 100)  # (uploads the tables, sizes the workspace)
    out = torch.empty_like(eager)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with ops.graph_capture(graph):
        ops.resample2d(x, 100, out=out)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    x.copy_(_randn((1, 3, 64, 64), 8))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ops.resample2d(x, 100))


def test_pyramid(dev):
    t = _randn((1, 3, 96, 96), 9).to(dev)
    levels = scale.pyramid(t, [48, 64, 96])
    assert levels[2] is t or levels[2].data_ptr() == t.data_ptr()
    assert torch.equal(levels[0], ops.resample2d(t, 48, "cubic"))
    assert torch.equal(levels[1], ops.resample2d(t, 64, "cubic"))
    guides = torch.rand(2, 96, 96, generator=torch.Generator().manual_seed(1)).round().to(dev)
    gl = scale.pyramid(guides, [48, 96], "triangle")
    assert gl[0].shape == (2, 48, 48) and float(gl[0].min()) >= 0.0 and float(gl[0].max()) <= 1.0
    assert torch.equal(gl[0], ops.resample2d(guides, 48, "triangle").clamp_(0, 1))


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


def _rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _within(name, hip, r32, r64):
    e, r = _rel(hip, r64), _rel(r32, r64)
    print(f"{name}: hip {e:.2e} fp32 {r:.2e}")
    assert e <= max(K * r, FLOOR), f"{name}: hip {e:.2e} vs fp32 {r:.2e}"


def _iteration(feat, dev, style, content, init, sw, cw):
    """loss_forward + loss_backward, eagerly: (state, total, dx)."""
    x = init.to(dev).contiguous()
    targets = [t.reshape(t.shape[-2:]).contiguous() for t in feat.style_targets(style.to(dev))]
    c4 = V.content_target(feat, content.to(dev).contiguous()).clone()
    total = torch.zeros((), device=dev)
    st = V.loss_forward(feat, targets, x, c4, folded_weights=(sw, cw), total=total)
    dx = V.loss_backward(feat, st, feature_grad=False)
    torch.cuda.synchronize()
    return st, total, dx


def _three_way(feat, vgg_np, dev, h, w, lw, cw, style_h=None):
    content, init = _img(12, h, w), _img(14, h, w)
    style = _img(11, h + 8 if style_h is None else style_h, w)
    st, total, dx = _iteration(feat, dev, style, content, init, [1e5 * v for v in lw], cw)
    assert bool(torch.isfinite(dx).all()), "dx (a zero max|A| must give a zero, not a NaN)"
    assert bool(torch.isfinite(V.loss_values(st)[:6]).all())
    masks = FR.vgg_branches_from_z(st.z)
    r64 = SR.engine_iteration(vgg_np, init, content, style, lw, masks, torch.float64, 1e5, cw)
    r32 = SR.engine_iteration(vgg_np, init, content, style, lw, masks, torch.float32, 1e5, cw)
    hip = V.loss_values(st)
    for l in range(5):
        _within(f"style{l + 1}", hip[l], r32[0][l], r64[0][l])
    _within("content", hip[5], r32[1], r64[1])
    _within("total", total, r32[2], r64[2])
    _within("dx", dx, r32[3], r64[3])


@pytest.mark.parametrize("hw", [(64, 64), (40, 24)], ids=["64x64", "40x24-ragged"])
@pytest.mark.parametrize("case", ["mixed", "fine-only"])
def test_tap_weights_three_way(dev, feat, vgg_np, hw, case):
    lw, cw = ([1, 0.5, 2, 0, 0.25], 1.0) if case == "mixed" else ([1, 1, 1, 0, 0], 0.0)
    _three_way(feat, vgg_np, dev, hw[0], hw[1], lw, cw)


def test_top_size_iteration_three_way(dev, feat, vgg_np):
    """The only test above 512^2: one eager iteration at scale.MAX_SIDE^2, unit per-tap
    weights, against the fp64 and fp32 restatements (about 0.7 TFLOP each on the CPU)."""
    _three_way(feat, vgg_np, dev, scale.MAX_SIDE, scale.MAX_SIDE, [1, 1, 1, 1, 1], 1.0,
               style_h=scale.MAX_SIDE)


def test_unit_tap_weights_are_the_scalar_call(dev, feat):
    content, init, style = _img(12, 64, 64), _img(14, 64, 64), _img(11, 64, 64)
    a = _iteration(feat, dev, style, content, init, 1e5, 1.0)
    b = _iteration(feat, dev, style, content, init, [1e5] * 5, 1.0)
    assert torch.equal(V.loss_values(a[0]), V.loss_values(b[0]))
    assert torch.equal(a[1], b[1])
    assert torch.equal(a[2], b[2])
    # and through the engines' own argument
    e0 = V.GatysEngine(feat, style, content, init=init)
    e1 = V.GatysEngine(feat, style, content, init=init, style_layer_weights=[1] * 5)
    assert torch.equal(e0.run(2).clone(), e1.run(2))


# ----------------------------------------------------------------------------- drivers
def test_coarse_to_fine_adam_is_its_hand_chain(dev, feat):
    content, style = _img(12, 100, 100).to(dev), _img(11, 100, 100).to(dev)
    got = scale.coarse_to_fine(feat, style, content, [64, 100], [2, 2], optimizer="adam")
    c0, s0 = ops.resample2d(content, 64), ops.resample2d(style, 64)
    x0 = V.GatysEngine(feat, s0, c0).run(2).clone()
    x1 = ops.resample2d(x0, 100)
    want = V.GatysEngine(feat, style, content, init=x1).run(2)
    torch.cuda.synchronize()
    assert got.shape == (1, 3, 100, 100)
    assert torch.equal(got, want)
    assert float((got - content).abs().max()) > 0


def test_coarse_to_fine_lbfgs_is_its_hand_chain(dev, feat):
    content, style = _img(12, 100, 100).to(dev), _img(11, 100, 100).to(dev)
    got = scale.coarse_to_fine(feat, style, content, [64, 100], [1, 1], optimizer="lbfgs")
    c0, s0 = ops.resample2d(content, 64), ops.resample2d(style, 64)
    x0 = V.GatysLBFGS(feat, s0, c0).run(1).clone()
    x1 = ops.resample2d(x0, 100)
    want = V.GatysLBFGS(feat, style, content, init=x1).run(1)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert bool(torch.isfinite(got).all())


def test_one_level_is_the_plain_engine(dev, feat):
    content, style64 = _img(12, 64, 64).to(dev), _img(11, 64, 64).to(dev)
    got = scale.coarse_to_fine(feat, style64, content, [64], 3)
    assert torch.equal(got, V.GatysEngine(feat, style64, content).run(3))
    # per-tap weights and an init reach the engine
    init = _img(14, 64, 64).to(dev)
    kw = dict(style_layer_weights=[1, 0.5, 2, 0, 0.25], content_weight=2)
    got = scale.coarse_to_fine(feat, style64, content, [64], [3], init=init, **kw)
    assert torch.equal(got, V.GatysEngine(feat, style64, content, init=init, **kw).run(3))


def _feathered(h, w):
    """tests/test_guided_gpu.py: complementary left / right guides, a linear seam."""
    x = torch.arange(w, dtype=torch.float32)
    left = ((0.625 * w - x) / (0.25 * w)).clamp(0, 1)[None].expand(h, w)
    return torch.stack([left, 1 - left]).contiguous()


def test_coarse_to_fine_guided_is_its_hand_chain(dev, feat):
    content = _img(12, 96, 96).to(dev)
    styles = [_img(11, 96, 96).to(dev), _img(13, 96, 96).to(dev)]
    guides = _feathered(96, 96)
    lam = [1.0, 0.5]
    got = scale.coarse_to_fine_guided(feat, styles, content, guides, [48, 96], [2, 2],
                                      region_weights=lam)
    g0 = ops.resample2d(guides.to(dev), 48, "triangle").clamp_(0, 1)
    e = V.GuidedGatysEngine(feat, [ops.resample2d(s, 48) for s in styles],
                            ops.resample2d(content, 48), g0, region_weights=lam)
    x1 = ops.resample2d(e.run(2).clone(), 96)
    want = V.GuidedGatysEngine(feat, styles, content, guides.to(dev), region_weights=lam,
                               init=x1).run(2)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert float((got - content).abs().max()) > 0


def test_mix_scales_is_its_engine_call(dev, feat):
    fine, coarse = _img(11, 64, 64).to(dev), _img(13, 64, 64).to(dev)
    got = scale.mix_scales(feat, fine, coarse, 3, fine_taps=3)
    want = V.GatysEngine(feat, fine, coarse, content_weight=0,
                         style_layer_weights=[1, 1, 1, 0, 0]).run(3)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert bool(torch.isfinite(got).all())
    assert float((got - coarse).abs().max()) > 0
    with pytest.raises(ValueError):
        scale.mix_scales(feat, fine, _img(13, 64, 72).to(dev), 1)
    with pytest.raises(ValueError):
        scale.mix_scales(feat, fine, coarse, 1, fine_taps=5)


def test_a_plain_capture_works_after_the_levels(dev, feat):
    """Three engines built, captured and dropped in a row, then a capture of a fourth: no
    graph of a finished level is left to be destroyed during it."""
    content, style = _img(12, 64, 64).to(dev), _img(11, 64, 64).to(dev)
    x = scale.coarse_to_fine(feat, style, content, [32, 48, 64], 2)
    assert bool(torch.isfinite(x).all())
    eng = V.GatysEngine(feat, style, content).capture()
    eng.step()
    eng.step()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(eng.x).all()) and bool(torch.isfinite(eng.total))


def test_style_network_entry_points(dev):
    from styletransfer_amd import network
    content, style = _img(12, 64, 64), _img(11, 64, 64)
    net = network.StyleNetwork(style, content)
    got = net.train_gatys_multiscale(style, content, [48, 64], [2, 2], optimizer="adam")
    want = scale.coarse_to_fine(net.features(), style, content, [48, 64], [2, 2],
                                optimizer="adam", style_weight=100_000, content_weight=1)
    assert torch.equal(got, want)
    lw = [1, 0.5, 2, 0, 0.25]
    a = net.train_gatys_adam(style, content, steps=2, style_layer_weights=lw)
    targets = [l.target for l, _ in net.style_losses]
    b = V.GatysEngine(net.features(), None, content.to(dev), targets=targets,
                      style_layer_weights=lw).run(2)
    assert torch.equal(a, b)
    assert not torch.equal(a, net.train_gatys_adam(style, content, steps=2))
    g = net.train_gatys_guided([style], content, torch.ones(1, 64, 64), steps=2, sizes=[48, 64])
    assert g.shape == (1, 3, 64, 64) and bool(torch.isfinite(g).all())


# --------------------------------------------------------------------------------- CLI
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


def _run_cli(project_root, monkeypatch, argv, out_name):
    from click.testing import CliRunner
    from styletransfer_amd import img_utils
    from styletransfer_amd.clis import cli
    seen = []
    orig = img_utils.imshow

    def spy(t, *a, **k):
        seen.append(t.detach().clone())
        return orig(t, *a, **k)
    monkeypatch.setattr(img_utils, "imshow", spy)
    r = CliRunner().invoke(cli, argv)
    assert r.exit_code == 0, r.output + repr(r.exception)
    got = np.asarray(Image.open(project_root / "results" / out_name))
    content = img_utils.image_loader(str(project_root / "data" / "dancing.jpg"), imsize=128)
    assert got.shape == (128, 128, 3)
    assert seen[0].shape == (1, 3, 128, 128)
    assert bool(torch.isfinite(seen[0]).all())
    assert float((seen[0] - content).abs().max()) > 0


def test_cli_gatys_st_scales(dev, project_root, monkeypatch):
    _run_cli(project_root, monkeypatch,
             ["gatys_st", "data/dancing.jpg", "data/styles/picasso.jpg", "--scales", "64,128",
              "-s", "2", "--optimizer", "adam"], "gatys_converted.png")


def test_cli_gatys_st_coarse_style(dev, project_root, monkeypatch):
    _run_cli(project_root, monkeypatch,
             ["gatys_st", "data/dancing.jpg", "data/styles/picasso.jpg", "--scales", "64,128",
              "--scale-steps", "2,1", "--optimizer", "adam", "--coarse-style",
              "data/dancing.jpg", "--mix-steps", "2", "--layer-weights", "1,1,1,0.5,0.5",
              "--preserve-color", "match"], "gatys_converted.png")


def test_cli_gatys_guided_scales(dev, project_root, monkeypatch):
    m = np.zeros((120, 160), np.uint8)
    m[:, :90] = 255
    Image.fromarray(m, mode="L").save(project_root / "m0.png")
    Image.fromarray(255 - m, mode="L").save(project_root / "m1.png")
    _run_cli(project_root, monkeypatch,
             ["gatys_guided", "data/dancing.jpg", "-r", "data/styles/picasso.jpg:m0.png",
              "-r", "data/dancing.jpg:m1.png", "--scales", "64,128", "-s", "2"],
             "gatys_guided.png")
