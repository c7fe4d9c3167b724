"""Colour control on the GPU: stx_color_stats / stx_color_affine against the fp64
yardstick (color_ref), color.prepare / merge_luminance, and the `--preserve-color`
switches of the Gatys commands, the feed-forward converters and the video FrameEngine."""
import json
import os
import shutil

import numpy as np
import pytest
import torch
from PIL import Image

import color_ref as CR
from conftest import REPO
from styletransfer_amd import color, constants, img_utils, network, ops, video
from styletransfer_amd import weights as W

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24


def _randn(shape, seed, offset=0.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float32) + offset


# ------------------------------------------------------------------------------- stats
STAT_SHAPES = [(1, 3, 5, 7), (2, 3, 64, 64), (3, 3, 129, 67), (1, 3, 512, 512)]


@pytest.mark.parametrize("offset", [0.0, 100.0], ids=["centred", "plus100"])
@pytest.mark.parametrize("shape", STAT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stats_vs_fp64(dev, shape, offset):
    """Fewer pixels than a wave; h w % 4 != 0 (scalar loads); several blocks; the whole
    fixed-order finalize.  An N-term fp64 sum errs by at most N 2^-53 of sum|terms|:
    3e-11 at N = 512^2, so 1e-10 of the terms' mean magnitude bounds mean and covariance."""
    x = _randn(shape, 5, offset)
    xd = x.to(dev)
    got = ops.color_stats(xd)
    assert got.dtype == torch.float64 and tuple(got.shape) == (shape[0], 9)
    again = ops.color_stats(xd)
    assert torch.equal(got, again)  # bit-reproducible
    got = got.cpu().numpy()
    x64 = x.double().numpy()
    for k in range(shape[0]):
        p = x64[k].reshape(3, -1)
        ref = CR.stats(x64[k])
        e_mean = np.abs(got[k, :3] - ref[:3])
        tol_mean = 1e-10 * np.abs(p).mean(axis=1)
        print(f"{shape} +{offset} image {k}: mean err {e_mean.max():.2e} (tol {tol_mean.min():.2e})")
        assert (e_mean <= tol_mean).all(), (e_mean, tol_mean)
        for j, (a, b) in enumerate(CR.TRI):
            tol = 1e-10 * (np.abs(p[a] * p[b]).mean() + abs(ref[a] * ref[b]))
            err = abs(got[k, 3 + j] - ref[3 + j])
            assert err <= tol, (k, a, b, err, tol)


@pytest.mark.parametrize("hw", [(64, 64), (129, 67)], ids=["vector", "scalar"])
def test_stats_do_not_depend_on_the_batch(dev, hw):
    x = _randn((3, 3, *hw), 6, 0.5).to(dev)
    batch = ops.color_stats(x)
    alone = ops.color_stats(x[1:2])
    assert torch.equal(batch[1:2], alone)
    assert not torch.equal(batch[0:1], alone)


# ------------------------------------------------------------------------------ affine
AFF_SHAPES = [(1, 3, 5, 7), (2, 3, 129, 67), (1, 3, 256, 256)]


@pytest.fixture(scope="module")
def affine_case():
    """One transform for every shape: M, b, lo, hi rounded to fp32 (what the kernel gets)."""
    rng = np.random.default_rng(11)
    M = rng.standard_normal((3, 3)).astype(np.float32)
    b = rng.standard_normal(3).astype(np.float32)
    lo = np.array([-0.5, -0.25, -1.0], np.float32)
    hi = np.array([0.75, 0.5, 1.25], np.float32)
    return M, b, lo, hi


AFF_VARIANTS = [(False, None), (False, "x"), (True, None), (True, "x"), (True, "base")]


@pytest.mark.parametrize("clamp", [False, True], ids=["noclamp", "clamp"])
@pytest.mark.parametrize("with_base,alias", AFF_VARIANTS,
                         ids=["nobase", "nobase-out-is-x", "base", "base-out-is-x",
                              "base-out-is-base"])
@pytest.mark.parametrize("shape", AFF_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_affine_vs_fp64(dev, affine_case, shape, with_base, alias, clamp):
    """|err| <= 8 2^-24 (|base_c| + sum_d |M_cd| (|x_d| + |base_d|) + |b_c|): the three
    differences, three fused multiply-adds and the final add are seven roundings, each
    relative to a partial result that scale bounds.  The clamp is 1-Lipschitz and its
    bounds are the same fp32 numbers on both sides."""
    M, b, lo, hi = affine_case
    x = _randn(shape, 21)
    base = _randn(shape, 22) if with_base else None
    ref = CR.affine(x.double().numpy(), M.astype(np.float64), b.astype(np.float64),
                    None if base is None else base.double().numpy(),
                    lo if clamp else None, hi if clamp else None)
    ax = np.abs(x.double().numpy())
    ab = np.abs(base.double().numpy()) if with_base else np.zeros_like(ax)
    scale = ab + np.einsum("cd,ndhw->nchw", np.abs(M).astype(np.float64), ax + ab) \
        + np.abs(b).astype(np.float64).reshape(1, 3, 1, 1)
    xd = x.to(dev)
    bd = None if base is None else base.to(dev)
    out = {None: None, "x": xd, "base": bd}[alias]
    kw = dict(base=bd, lo=lo if clamp else None, hi=hi if clamp else None)
    first = ops.color_affine(x.to(dev), M, b, base=None if bd is None else bd.clone(),
                             lo=kw["lo"], hi=kw["hi"])
    got = ops.color_affine(xd, M, b, out=out, **kw)
    if alias is not None:
        assert got.data_ptr() == out.data_ptr()
    assert torch.equal(first, got)  # bit-identical again, aliased or not
    g = got.cpu().double().numpy()
    ratio = (np.abs(g - ref) / (EPS * scale)).max()
    print(f"{shape} base={with_base} clamp={clamp} alias={alias}: max err {ratio:.2f} x 2^-24 scale")
    assert ratio <= 8.0, ratio
    if clamp:
        g32 = got.cpu().numpy()
        for c in range(3):
            assert g32[:, c].min() >= lo[c] and g32[:, c].max() <= hi[c]
        assert (g32[:, 0] == lo[0]).any() and (g32[:, 0] == hi[0]).any()


# --------------------------------------------------------------------- prepare / finish
@pytest.fixture(scope="module")
def repo_images(dev):
    content = img_utils.image_loader(os.path.join(REPO, "data/dancing.jpg"), 64).to(dev)
    style = img_utils.image_loader(os.path.join(REPO, "data/styles/picasso.jpg"), 64).to(dev)
    return content.contiguous(), style.contiguous()  # the loader's strides are channels-last


def test_prepare_match_reaches_the_content_statistics(dev, repo_images):
    content, style = repo_images
    want = ops.color_stats(content).cpu().numpy()
    for styles in ([style], [style, content.flip(-1).contiguous()]):
        new, c2, finish = color.prepare(styles, content, "match")
        assert c2.data_ptr() == content.data_ptr() or torch.equal(c2, content)
        assert finish(style) is style
        for s in new:
            err = np.abs(ops.color_stats(s).cpu().numpy() - want).max()
            print(f"match: stats of the recoloured style vs content: {err:.2e}")
            assert err <= 1e-5, err
    # a single tensor comes back as a single tensor, and equals the yardstick
    one, _, _ = color.prepare(style, content, "match")
    ref = CR.match(style[0].double().cpu().numpy(), content[0].double().cpu().numpy())
    assert float(np.abs(one[0].double().cpu().numpy() - ref).max()) <= 1e-4


def test_prepare_luminance_and_finish_by_yiq(dev):
    """Random images in [-2, 2].  After finish(clamp=False) the output has the result's Y
    and the content's I and Q to 1e-5 in de-normalised units: 8 2^-24 x a scale of about
    6, x std, x a YIQ row sum <= 1.2."""
    g = torch.Generator().manual_seed(31)
    content, style, result = (torch.rand((1, 3, 48, 40), generator=g) * 4 - 2 for _ in range(3))
    (s2,), c2, finish = color.prepare([style.to(dev)], content.to(dev), "luminance")
    c64, s64, r64 = (t[0].double().numpy() for t in (content, style, result))
    # the transfer's inputs: luminance images, the style's moment-matched to the content's
    assert np.abs(c2[0].double().cpu().numpy() - CR.luminance(c64)).max() <= 1e-5
    a, o = CR.luma_gain(CR.stats(s64), CR.stats(c64))
    assert np.abs(s2[0].double().cpu().numpy() - CR.luminance(s64, a, o)).max() <= 1e-5
    p = CR.denorm(c2[0].double().cpu().numpy())
    assert np.abs(p[0] - p[1]).max() <= 1e-5 and np.abs(p[0] - p[2]).max() <= 1e-5
    ms, vs = CR.luma_moments(ops.color_stats(s2).cpu().numpy()[0])
    mc, vc = CR.luma_moments(CR.stats(c64))
    assert abs(ms - mc) <= 1e-5 and abs(vs - vc) <= 1e-5
    # the merge onto the ORIGINAL content
    out = finish(result.to(dev), clamp=False)[0].double().cpu().numpy()
    q, qr, qc = CR.yiq(out), CR.yiq(r64), CR.yiq(c64)
    ey, eiq = np.abs(q[0] - qr[0]).max(), np.abs(q[1:] - qc[1:]).max()
    print(f"luminance merge: Y err {ey:.2e}, IQ err {eiq:.2e}")
    assert ey <= 1e-5 and eiq <= 1e-5
    # clamped: inside the displayable gamut exactly, and equal where nothing was clamped
    lo, hi = (np.asarray(v, np.float32) for v in color.gamut_bounds())
    cl = finish(result.to(dev))[0].cpu().numpy()
    free = finish(result.to(dev), clamp=False)[0].cpu().numpy()
    for c in range(3):
        assert cl[c].min() >= lo[c] and cl[c].max() <= hi[c]
        inside = (free[c] > lo[c]) & (free[c] < hi[c])
        assert inside.any() and (~inside).any()
        assert np.array_equal(cl[c][inside], free[c][inside])
    # merge_luminance is that one launch, into a caller's buffer too
    buf = torch.empty_like(content, device=dev)
    assert color.merge_luminance(result.to(dev), content.to(dev), out=buf) is buf
    assert np.array_equal(buf[0].cpu().numpy(), cl)


# -------------------------------------------------------------------- Gatys end to end
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


def _png(path):
    return np.asarray(Image.open(path))


def test_gatys_cli_preserve_color(dev, project_root):
    """`gatys_st ... -s 5 --optimizer adam --preserve-color MODE` writes the PNG of
    finish(train_gatys_adam(...)) built by hand from color.prepare + StyleNetwork; without
    the switch, the PNG of the plain path."""
    from click.testing import CliRunner
    from styletransfer_amd.clis import cli
    content = img_utils.image_loader(str(project_root / "data/dancing.jpg"))
    style = img_utils.image_loader(str(project_root / "data/styles/picasso.jpg"))
    pngs = {}
    for mode in (None, "luminance", "match"):
        args = ["gatys_st", "data/dancing.jpg", "data/styles/picasso.jpg", "-s", "5",
                "--optimizer", "adam", "-n", f"{mode}.png"]
        r = CliRunner().invoke(cli, args + (["--preserve-color", mode] if mode else []))
        assert r.exit_code == 0, r.output + repr(r.exception)
        pngs[mode] = _png(project_root / "results" / f"{mode}.png")
        if mode is None:
            s2, c2, finish = style, content, lambda t: t
        else:
            s2, c2, finish = color.prepare(style, content, mode)
        net = network.StyleNetwork(s2, c2)
        out = finish(net.train_gatys_adam(style_image=s2, content_image=c2, steps=5,
                                          style_weight=100_000, content_weight=1))
        assert np.array_equal(pngs[mode], np.asarray(img_utils.to_pil(out))), mode
    assert (pngs[None] != pngs["match"]).any() and (pngs[None] != pngs["luminance"]).any()
    # luminance mode keeps the content's chroma: I and Q of the PNG are the photograph's
    q = CR.yiq(CR.renorm(pngs["luminance"].astype(np.float64).transpose(2, 0, 1) / 255))
    qc = CR.yiq(content[0].double().cpu().numpy())
    unclamped = (pngs["luminance"] > 0).all(axis=2) & (pngs["luminance"] < 255).all(axis=2)
    assert unclamped.mean() > 0.25
    assert np.abs(q[1:] - qc[1:])[:, unclamped].max() <= 2.0 / 255


def test_gatys_guided_cli_preserve_color(dev, project_root, monkeypatch):
    from click.testing import CliRunner
    from styletransfer_amd.clis import cli
    from styletransfer_amd.clis.gatys_guided import mask_loader
    monkeypatch.setattr(constants, "IMSIZE", 64)
    m = np.zeros((120, 160), np.uint8)
    m[:, :90] = 255
    Image.fromarray(m, mode="L").save(project_root / "m0.png")
    Image.fromarray(255 - m, mode="L").save(project_root / "m1.png")
    r = CliRunner().invoke(cli, ["gatys_guided", "data/dancing.jpg",
                                 "-r", "data/styles/picasso.jpg:m0.png",
                                 "-r", "data/dancing.jpg:m1.png", "-s", "3",
                                 "--preserve-color", "match"])
    assert r.exit_code == 0, r.output + repr(r.exception)
    got = _png(project_root / "results" / "gatys_guided.png")
    assert got.shape == (64, 64, 3)
    content = img_utils.image_loader(str(project_root / "data/dancing.jpg"))
    styles = [img_utils.image_loader(str(project_root / "data/styles/picasso.jpg")), content]
    guides = [mask_loader(str(project_root / n)) for n in ("m0.png", "m1.png")]
    s2, c2, finish = color.prepare(styles, content, "match")
    net = network.StyleNetwork(s2[0], c2)
    out = finish(net.train_gatys_guided(s2, c2, guides, style_guides=None, steps=3,
                                        style_weight=100_000, content_weight=1))
    assert np.array_equal(got, np.asarray(img_utils.to_pil(out)))
    plain = network.StyleNetwork(styles[0], content).train_gatys_guided(
        styles, content, guides, steps=3)
    assert (got != np.asarray(img_utils.to_pil(plain))).any()


# -------------------------------------------------------------------------- FrameEngine
def _video_net():
    net = network.VideoTransformNet(torch.rand([3, 64, 64]))
    net.load_state_dict({k: torch.from_numpy(v)
                         for k, v in W.itn_synthetic(777, in_channels=6)})
    return net


def _run_engines(dev, frames, raw_hw):
    """{(graph, flag): [(prev, frame, out) per frame]} of four fresh engines."""
    res = {}
    for graph in (False, True):
        for flag in (False, True):
            eng = video.FrameEngine(_video_net(), (1, 3, 64, 64), dev, graph=graph,
                                    raw_hw=raw_hw, preserve_color=flag)
            rows = []
            for f in frames:
                out = eng.step_raw(f) if raw_hw else eng.step(f.to(dev))
                rows.append((eng.prev.clone(), eng.frame.clone(), out.clone()))
            assert (eng.graph is not None) == graph
            res[graph, flag] = rows
    return res


@pytest.mark.parametrize("raw", [False, True], ids=["conditioned", "raw-resized"])
def test_frame_engine_preserve_color(dev, raw):
    """Next to a plain engine on the same three frames: prev (the recurrence) is
    bit-identical after every frame, out is merge_luminance(plain out, frame), and the
    graph replay equals the eager frames -- also through step_raw with a resize."""
    if raw:
        rng = np.random.default_rng(3)
        frames = [rng.integers(0, 256, (40, 48, 3), dtype=np.uint8) for _ in range(3)]
    else:
        frames = [torch.from_numpy(W.synthetic_image(900 + t, (1, 3, 64, 64))) for t in range(3)]
    res = _run_engines(dev, frames, (40, 48) if raw else None)
    for graph in (False, True):
        for t, (plain, flagged) in enumerate(zip(res[graph, False], res[graph, True])):
            assert torch.equal(plain[0], flagged[0]), (graph, t)  # prev: the un-merged y
            assert torch.equal(plain[1], flagged[1]), (graph, t)  # the conditioned frame
            want = color.merge_luminance(plain[2], plain[1].contiguous())
            assert torch.equal(flagged[2], want), (graph, t)
            assert not torch.equal(flagged[2], plain[2])
    for flag in (False, True):
        for t, (eager, replay) in enumerate(zip(res[False, flag], res[True, flag])):
            for a, b in zip(eager, replay):
                assert torch.equal(a, b), (flag, t)


def test_process_video_preserve_color(dev, tmp_path, monkeypatch):
    monkeypatch.setattr(constants, "IMSIZE", 64)
    arr = (np.random.default_rng(0).random((3, 40, 48, 3)) * 255).astype(np.uint8)
    src = tmp_path / "clip.npy"
    np.save(src, arr)
    net = _video_net()
    video.process_video(net, str(src), working_dir=str(tmp_path / "wd") + "/",
                        out_dir=str(tmp_path / "out") + "/", preserve_color=True)
    eng = video.FrameEngine(net, (1, 3, 64, 64), dev, graph=False)
    for i, f in enumerate(video.iterate_frames(arr, imsize=64)):
        y = eng.step(f.to(dev))
        want = np.asarray(img_utils.to_pil(color.merge_luminance(y, f.to(dev))[0]))
        assert np.array_equal(_png(tmp_path / "wd" / f"{i}.png"), want), i


# ------------------------------------------------------------- feed-forward converters
def test_convert_image_preserve_color(dev, project_root):
    from click.testing import CliRunner
    from styletransfer_amd.clis import cli
    models = project_root / "data" / "models"
    models.mkdir(parents=True)
    sd = {k: torch.from_numpy(v) for k, v in W.itn_synthetic(4321)}
    torch.save(sd, models / "fast_st_syn_epoch0.pth")
    r = CliRunner().invoke(cli, ["fast_st", "convert-image", "data/dancing.jpg", "syn",
                                 "--preserve-color"])
    assert r.exit_code == 0, r.output + repr(r.exception)
    got = _png(project_root / "results" / "converted_fast_st_syn.png")
    net = network.ImageTransformNet(torch.rand([3, 64, 64]))
    net.load_state_dict(sd)
    image = img_utils.image_loader(str(project_root / "data/dancing.jpg"))
    with torch.no_grad():
        y = net(image)
    assert np.array_equal(got, np.asarray(img_utils.to_pil(color.merge_luminance(y, image))))
    assert (got != np.asarray(img_utils.to_pil(y))).any()
    # the API argument, and its default
    net.process_image("data/dancing.jpg", "syn", out_dir="api/", preserve_color=True)
    assert np.array_equal(got, _png(project_root / "api" / "converted_fast_st_syn.png"))
    net.process_image("data/dancing.jpg", "syn", out_dir="plain/")
    assert np.array_equal(_png(project_root / "plain" / "converted_fast_st_syn.png"),
                          np.asarray(img_utils.to_pil(y)))


def test_convert_image_multi_preserve_color(dev, project_root):
    from click.testing import CliRunner
    from styletransfer_amd.clis import cli
    models = project_root / "data" / "models"
    models.mkdir(parents=True)
    names = ["a.jpg", "b.jpg"]
    net = network.MultiStyleTransformNet([torch.rand(3, 8, 8)] * 2, style_names=names)
    torch.save(net.state_dict(), models / "fast_mst_duo_epoch0.pth")
    (models / "fast_mst_duo.styles.json").write_text(json.dumps(names))
    r = CliRunner().invoke(cli, ["fast_st", "convert-image-multi", "data/dancing.jpg", "duo",
                                 "--mix", "a.jpg:0.25,b.jpg:0.75", "--preserve-color"])
    assert r.exit_code == 0, r.output + repr(r.exception)
    got = _png(project_root / "results" / "converted_fast_mst_duo.png")
    image = img_utils.image_loader(str(project_root / "data/dancing.jpg"))
    with torch.no_grad():
        y = net(image, style=torch.tensor([0.25, 0.75]))
    want = color.merge_luminance(y, image)
    assert np.array_equal(got, np.asarray(img_utils.to_pil(want)))
    out = net.process_image("data/dancing.jpg", "duo", mix=[0.25, 0.75], out_dir="api/",
                            preserve_color=True)
    assert torch.equal(out, want)
