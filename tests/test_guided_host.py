"""Region-guided Gatys transfer, the parts that need no GPU: the C ABI of the two guided
entry points, the per-tap guide maps, the fp64 oracle against autograd, and the
`gatys_guided` command line."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch
from PIL import Image

import forced_ref as FR
import guided_ref as GR
from conftest import REPO

NEW = ("stx_guided_style_loss", "stx_guided_style_ws", "stx_guided_gram_bwd")


def test_guided_symbols_and_abi_revision():
    from styletransfer_amd import _native as N
    L = N.lib()
    out = subprocess.check_output(["nm", "-D", "--defined-only", N.LIB_PATH]).decode()
    syms = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for name in NEW:
        assert name in syms, name
        assert name in N.SIGNATURES, name
    hdr = open(os.path.join(REPO, "include", "stx.h")).read()
    rev = int(re.search(r"#define STX_ABI_VERSION (\d+)", hdr).group(1))
    assert L.stx_abi_version() == 11 == rev == N.STX_ABI_VERSION
    assert int(re.search(r"#define STX_GUIDE_MAX (\d+)", hdr).group(1)) == 4 == N.STX_GUIDE_MAX


def test_guided_invalid_args_rejected():
    """R = 0, R = 5 and a null z return STX_E_INVALID before any launch (fake pointers:
    nothing is dereferenced, no GPU on this path)."""
    from styletransfer_amd import _native as N
    L = N.lib()
    lam = (C.c_float * 4)(1, 1, 1, 1)

    def fwd(z, R):
        return L.stx_guided_style_loss(z, 32, 1.0, 48, None, 64, 80, 1, 64, 1024, R, lam, 1.0,
                                       None, 96, 1 << 30, None)

    def bwd(z, R):
        return L.stx_guided_gram_bwd(16, z, 48, 64, 1, 64, 32, 32, R, None, 0, None, None, None)

    for call in (fwd, bwd):
        assert call(16, 0) == 1001
        assert b"R" in L.stx_last_error_string()
        assert call(16, 5) == 1001
        assert call(None, 2) == 1001
        assert b"required" in L.stx_last_error_string()
    assert L.stx_guided_style_ws(1, 64, 1024, 0) == 0 == L.stx_guided_style_ws(1, 64, 1024, 5)
    assert L.stx_guided_style_ws(1, 64, 1024, 2) > 0


def test_guides_for_taps_all_ones_is_exact():
    from styletransfer_amd import vgg as V
    maps = V.guides_for_taps(torch.ones(64, 64))
    assert [tuple(m.shape) for m in maps] == [(64, 64), (64, 64), (32, 32), (32, 32), (16, 16)]
    for m in maps:
        assert m.dtype == torch.float32 and bool((m == 1.0).all())


def test_guides_for_taps_floor_pooling_and_normalisation():
    from styletransfer_amd import vgg as V
    g = torch.rand(37, 41, generator=torch.Generator().manual_seed(3))
    maps = V.guides_for_taps(g)
    assert [tuple(m.shape) for m in maps] == [(37, 41), (37, 41), (18, 20), (18, 20), (9, 10)]
    for m in maps:
        assert abs(float(m.double().sum()) / m.numel() - 1.0) <= 1e-6
    # the oracle's maps are the same maps
    ref = GR.tap_maps(g[None].double())
    for m, r in zip(maps, ref):
        assert float((m.double().reshape(-1) - r[0]).abs().max()) <= 1e-6
    # R guides at once: one [R][h][w] tensor per tap
    both = V.guides_for_taps(torch.stack([g, 1 - g]))
    assert tuple(both[4].shape) == (2, 9, 10)
    assert torch.equal(both[2][0], maps[2])


def test_guides_for_taps_rejects_an_empty_region():
    from styletransfer_amd import vgg as V
    with pytest.raises(ValueError, match="region 0"):
        V.guides_for_taps(torch.zeros(64, 64))
    g = torch.ones(2, 16, 16)
    g[1] = 0
    with pytest.raises(ValueError, match="region 1"):
        V.guides_for_taps(g)


SHAPES = [(1, 64, 32, 32, 2), (2, 128, 16, 24, 3), (1, 256, 8, 8, 4), (3, 96, 7, 9, 2)]


def _case(b, c, h, w, R, seed=0):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(b, c, h, w, generator=g, dtype=torch.float64)
    wts = GR.normalise(torch.rand(R, h * w, generator=g, dtype=torch.float64) + 0.05)
    T = torch.randn(R, c, c, generator=g, dtype=torch.float64) * 0.1
    T = 0.5 * (T + T.transpose(1, 2))
    lam = [1.0 + 0.5 * r for r in range(R)]
    return z, wts, T, lam


def test_guided_ref_all_ones_is_the_plain_gram():
    z = _case(2, 64, 16, 12, 1)[0]
    G = GR.guided_gram(z, torch.ones(1, 16 * 12, dtype=torch.float64))[:, 0]
    ref = FR.gram(z)
    assert float((G - ref).abs().max() / ref.abs().max()) <= 1e-14


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_guided_ref_closed_form_gradient_is_autograd(shape):
    b, c, h, w, R = shape
    z, wts, T, lam = _case(*shape)
    zv = z.clone().requires_grad_()
    loss = (GR.region_losses(zv, wts, T) * torch.tensor(lam, dtype=torch.float64)).sum()
    loss.backward()
    dz = GR.gram_bwd(GR.coef(z, wts, T, lam), z, wts)
    err = float((dz - zv.grad).norm() / zv.grad.norm())
    assert err <= 1e-12, err


# ------------------------------------------------------------------------------- CLI
@pytest.fixture
def stubbed_cli(tmp_path, monkeypatch):
    """The `gatys_guided` command with the image loading and the training call stubbed:
    only the argument handling runs.  Returns (invoke, calls)."""
    from click.testing import CliRunner
    from styletransfer_amd import constants, img_utils, network
    from styletransfer_amd.clis import cli
    monkeypatch.setattr(constants, "PROJECT_ROOT_PATH", str(tmp_path))
    for name in ("m0.png", "m1.png", "sm.png"):
        Image.fromarray(np.full((40, 48), 255, np.uint8), mode="L").save(tmp_path / name)
    calls = []

    class FakeNet:
        def __init__(self, style, content):
            pass

        def train_gatys_guided(self, style_images, content_image, guides, **kw):
            calls.append((style_images, guides, kw))
            return torch.zeros(1, 3, 8, 8)

    monkeypatch.setattr(network, "StyleNetwork", FakeNet)
    monkeypatch.setattr(img_utils, "image_loader", lambda path, imsize=None: path)
    monkeypatch.setattr(img_utils, "imshow", lambda *a, **k: None)

    def invoke(*args):
        return CliRunner().invoke(cli, ["gatys_guided", *args])
    return invoke, calls


def test_cli_region_forms_accepted(stubbed_cli):
    from styletransfer_amd import constants
    invoke, calls = stubbed_cli
    r = invoke("c.jpg", "-r", "a.jpg:m0.png", "-r", "b.jpg:m1.png:sm.png", "-s", "7", "-sw",
               "10", "-cw", "2", "-n", "o.png")
    assert r.exit_code == 0, r.output + repr(r.exception)
    (styles, guides, kw), = calls
    assert [os.path.basename(s) for s in styles] == ["a.jpg", "b.jpg"]
    assert len(guides) == 2
    S = constants.IMSIZE
    for g in guides:  # grey / 255, centre-cropped and resized like the images
        assert tuple(g.shape) == (S, S) and float(g.min()) == 1.0 == float(g.max())
    assert kw["style_guides"][0] is None and tuple(kw["style_guides"][1].shape) == (S, S)
    assert (kw["steps"], kw["style_weight"], kw["content_weight"]) == (7, 10, 2)
    # no style mask anywhere: no style guides at all
    r = invoke("c.jpg", "-r", "a.jpg:m0.png")
    assert r.exit_code == 0 and calls[-1][2]["style_guides"] is None


def test_cli_refuses_five_regions_and_malformed_specs(stubbed_cli):
    invoke, calls = stubbed_cli
    r = invoke("c.jpg", *sum((["-r", f"s{i}.jpg:m0.png"] for i in range(5)), []))
    assert r.exit_code == 2 and "at most 4" in r.output
    r = invoke("c.jpg", "-r", "a.jpg")
    assert r.exit_code == 2 and "STYLE:MASK" in r.output
    r = invoke("c.jpg")
    assert r.exit_code == 2
    assert not calls
    r = invoke("--help")
    assert r.exit_code == 0 and "-r" in r.output and "-sw" in r.output
