"""Colour control, the parts that need no GPU: the C ABI of the two colour entry points,
the fp64 yardstick (color_ref) against itself and against an independent YIQ route, the
host matrix builders against the yardstick, and the `--preserve-color` switches."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
from PIL import Image

import color_ref as CR
from conftest import REPO

NEW = ("stx_color_stats", "stx_color_stats_ws", "stx_color_affine")


def test_color_symbols_and_abi_revision():
    from styletransfer_amd import _native as N
    L = N.lib()
    out = subprocess.check_output(["nm", "-D", "--defined-only", N.LIB_PATH]).decode()
    syms = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for name in NEW:
        assert name in syms, name
        assert name in N.SIGNATURES, name
    hdr = open(os.path.join(REPO, "include", "stx.h")).read()
    rev = int(re.search(r"#define STX_ABI_VERSION (\d+)", hdr).group(1))
    assert L.stx_abi_version() == 11 == rev == N.STX_ABI_VERSION  # additions do not bump it


def test_color_invalid_args_rejected():
    """NULL x / out / M, n <= 0, h w == 0 and a short workspace return STX_E_INVALID
    before any launch (fake pointers: nothing is dereferenced, no GPU on this path)."""
    from styletransfer_amd import _native as N
    L = N.lib()
    need = L.stx_color_stats_ws(2, 8, 8)
    assert need > 0
    assert L.stx_color_stats_ws(0, 8, 8) == 0 == L.stx_color_stats_ws(-1, 8, 8)
    assert L.stx_color_stats_ws(1, 0, 8) == 0 == L.stx_color_stats_ws(1, 8, 0)

    def stats(x=4096, out=8192, n=2, h=8, w=8, ws=16384, ws_bytes=None):
        return L.stx_color_stats(x, out, n, h, w, ws, need if ws_bytes is None else ws_bytes,
                                 None)

    for bad in (dict(x=None), dict(out=None), dict(n=0), dict(n=-3), dict(h=0), dict(w=0),
                dict(ws_bytes=need - 1), dict(ws=None)):
        assert stats(**bad) == 1001, bad
        assert b"stx_color_stats" in L.stx_last_error_string(), bad
    assert stats(ws_bytes=0) == 1001 and b"workspace" in L.stx_last_error_string()

    M = (C.c_float * 9)(*[1, 0, 0, 0, 1, 0, 0, 0, 1])
    v = (C.c_float * 3)(0, 0, 0)

    def affine(x=4096, base=None, out=8192, n=1, h=8, w=8, M=M, b=v, lo=None, hi=None):
        return L.stx_color_affine(x, base, out, n, h, w, M, b, lo, hi, None)

    for bad in (dict(x=None), dict(out=None), dict(M=None), dict(n=0), dict(n=-1), dict(h=0),
                dict(w=0), dict(lo=v), dict(hi=v)):
        assert affine(**bad) == 1001, bad
        assert b"stx_color_affine" in L.stx_last_error_string(), bad
    assert affine(x=None) == 1001 and b"required" in L.stx_last_error_string()


def test_ops_refuse_cpu_tensors():
    import torch
    from styletransfer_amd import _native as N
    from styletransfer_amd import color, ops
    x = torch.zeros(1, 3, 4, 4)
    with pytest.raises(N.NativeError):
        ops.color_stats(x)
    with pytest.raises(N.NativeError):
        ops.color_affine(x, np.eye(3))
    with pytest.raises(N.NativeError):
        color.merge_luminance(x, x)
    with pytest.raises(ValueError, match="sepia"):
        color.prepare([x], x, "sepia")


# ------------------------------------------------------------------ the yardstick itself
def _load(rel_path, size=64):
    """The repo image at size x size, ImageNet-normalised [3][size][size] fp64."""
    img = Image.open(os.path.join(REPO, rel_path)).convert("RGB")
    side = min(img.size)
    left, top = (img.size[0] - side) // 2, (img.size[1] - side) // 2
    img = img.crop((left, top, left + side, top + side)).resize((size, size), Image.BILINEAR)
    a = np.asarray(img, np.float64).transpose(2, 0, 1) / 255.0
    return CR.renorm(a)


@pytest.fixture(scope="module")
def images():
    return _load("data/dancing.jpg"), _load("data/styles/picasso.jpg")


def test_ref_match_reaches_the_content_statistics(images):
    for style, content in (images[::-1], images):
        s_style, s_content = CR.stats(style), CR.stats(content)
        got = CR.stats(CR.match(style, content))
        assert np.abs(got - s_content).max() <= 1e-9, np.abs(got - s_content).max()
        # the eigenvalue floor is a no-op for a real photograph / painting
        _, cov = CR.mu_cov(s_style)
        lam = np.linalg.eigvalsh(cov)
        print(f"smallest eigenvalue {lam.min():.2e}, floor {CR.eig_floor(cov):.2e}")
        assert lam.min() > CR.eig_floor(cov), (lam, CR.eig_floor(cov))
        A, _ = CR.match_matrix(s_style, s_content)
        exact = CR.sym_power(CR.mu_cov(s_content)[1], 0.5) @ np.linalg.inv(
            CR.sym_power(cov, 0.5))
        assert np.abs(A - exact).max() <= 1e-9


def test_ref_match_of_a_grey_style_is_finite(images):
    content = images[0]
    y = CR.luminance(images[1])  # R = G = B: a rank-one covariance
    _, cov = CR.mu_cov(CR.stats(y))
    assert np.linalg.eigvalsh(cov).min() < CR.eig_floor(cov)
    out = CR.match(y, content)
    assert np.isfinite(out).all()
    assert np.abs(CR.stats(out)[:3] - CR.stats(content)[:3]).max() <= 1e-9  # the mean still
    flat = np.zeros_like(content) + 0.25  # a constant image: zero covariance
    assert np.isfinite(CR.match(flat, content)).all()


def test_ref_merge_is_the_yiq_merge(images):
    content, stylised = images
    got = CR.merge(stylised, content)
    want = CR.merge_by_yiq(stylised, content)
    assert np.abs(got - want).max() <= 1e-12, np.abs(got - want).max()
    # and it is what it says: Y of the stylised image, I and Q of the content
    q = CR.yiq(got)
    assert np.abs(q[0] - CR.yiq(stylised)[0]).max() <= 1e-12
    assert np.abs(q[1:] - CR.yiq(content)[1:]).max() <= 1e-12
    # as one affine map with base = content
    one = CR.affine(stylised, CR.merge_matrix(), base=content)
    assert np.abs(one - got).max() <= 1e-12
    lo, hi = CR.gamut_bounds()
    cl = CR.denorm(CR.merge(stylised, content, clamp=True))
    assert cl.min() >= -1e-15 and cl.max() <= 1 + 1e-15
    assert np.abs(CR.affine(stylised, CR.merge_matrix(), base=content, lo=lo, hi=hi)
                  - CR.merge(stylised, content, clamp=True)).max() <= 1e-12


def test_ref_luminance_image_is_grey(images):
    content, style = images
    a, o = CR.luma_gain(CR.stats(style), CR.stats(content))
    for x, (ga, go) in ((content, (1.0, 0.0)), (style, (a, o))):
        lum = CR.luminance(x, ga, go)
        p = CR.denorm(lum)
        assert np.abs(p[0] - p[1]).max() <= 1e-14 and np.abs(p[0] - p[2]).max() <= 1e-14
        assert np.abs(p[0] - (ga * CR.luma_of(x) + go)).max() <= 1e-14
        assert np.abs(CR.affine(x, *CR.luma_matrix(ga, go)) - lum).max() <= 1e-12
    # the moment-matched style luminance has the content luminance's mean and variance
    ys, yc = CR.luma_of(CR.luminance(style, a, o)), CR.luma_of(content)
    assert abs(ys.mean() - yc.mean()) <= 1e-12 and abs(ys.var() - yc.var()) <= 1e-12
    # which follow from the colour stats alone
    m, v = CR.luma_moments(CR.stats(content))
    assert abs(m - yc.mean()) <= 1e-12 and abs(v - yc.var()) <= 1e-12


# -------------------------------------------------------------------------- the builders
def test_builders_equal_the_yardstick(images):
    from styletransfer_amd import color
    s_c, s_s = CR.stats(images[0]), CR.stats(images[1])

    def close(got, want):
        for g, w in zip(got, want):
            assert np.asarray(g).dtype == np.float64
            assert np.abs(np.asarray(g) - np.asarray(w)).max() <= 1e-12

    for a, b in ((s_s, s_c), (s_c, s_s)):
        close(color.match_matrix(a, b), CR.match_matrix(a, b))
        close(color.luma_gain(a, b), CR.luma_gain(a, b))
        close(color.luma_matrix(*color.luma_gain(a, b)), CR.luma_matrix(*CR.luma_gain(a, b)))
    close(color.luma_matrix(), CR.luma_matrix())
    close([color.merge_matrix()], [CR.merge_matrix()])
    close(color.gamut_bounds(), CR.gamut_bounds())
    grey = CR.stats(CR.luminance(images[1]))
    close(color.match_matrix(grey, s_c), CR.match_matrix(grey, s_c))
    assert np.isfinite(color.match_matrix(np.r_[0.25, 0.25, 0.25, np.zeros(6)], s_c)[0]).all()


# ---------------------------------------------------------------------------------- CLI
COMMANDS = (["gatys_st"], ["gatys_guided"], ["fast_st", "convert-image"],
            ["fast_st", "convert-image-multi"], ["video_st", "convert-video"])


@pytest.mark.parametrize("cmd", COMMANDS, ids=lambda c: "-".join(c))
def test_cli_help_names_the_switch(cmd):
    from click.testing import CliRunner
    from styletransfer_amd.clis import cli
    r = CliRunner().invoke(cli, [*cmd, "--help"])
    assert r.exit_code == 0 and "--preserve-color" in r.output, r.output


def test_cli_refuses_an_unknown_mode():
    from click.testing import CliRunner
    from styletransfer_amd.clis import cli
    r = CliRunner().invoke(cli, ["gatys_st", "c.jpg", "s.jpg", "--preserve-color", "sepia"])
    assert r.exit_code == 2 and "sepia" in r.output
    r = CliRunner().invoke(cli, ["gatys_guided", "c.jpg", "-r", "s.jpg:m.png",
                                 "--preserve-color", "sepia"])
    assert r.exit_code == 2 and "sepia" in r.output
