"""Colour control: colour-matched and luminance-only style transfer (Gatys et al. 2017,
"Controlling Perceptual Factors in Neural Style Transfer", section 5; the reference
project has no such feature).

Two methods, both affine per pixel in the ImageNet-normalised space the image tensors
live in, so both run on one kernel (`ops.color_affine`) fed by one reduction
(`ops.color_stats`):

  * colour matching: recolour the style image so that its RGB mean and covariance equal
    the content image's, then transfer as usual;
  * luminance-only: transfer between luminance images, then give the result the content
    image's chroma (for a feed-forward network: a post-hoc luminance merge).

The matrix builders work in fp64 numpy on 3x3 data and need no GPU; their results are
rounded to fp32 once, when they become kernel arguments.  The only host read is the 9
doubles per image at set-up (`prepare`); nothing is read per iteration or per frame.
"""
from __future__ import annotations

import numpy as np
import torch

from . import constants, ops

LUMA = np.array([0.299, 0.587, 0.114], np.float64)  # Rec.601 Y of YIQ
_MEAN = np.array(constants.IMAGENET_MEAN, np.float64)
_STD = np.array(constants.IMAGENET_STD, np.float64)

MODES = ("match", "luminance")


# --------------------------------------------------------------------- matrix builders
def unpack_stats(stats):
    """9 numbers (ops.color_stats: mean[3], cov upper triangle rr rg rb gg gb bb) ->
    (mu [3], Sigma [3][3]) in fp64."""
    s = np.asarray(stats, np.float64).reshape(9)
    cov = np.array([[s[3], s[4], s[5]],
                    [s[4], s[6], s[7]],
                    [s[5], s[7], s[8]]], np.float64)
    return s[:3].copy(), cov


def match_matrix(stats_style, stats_content):
    """(A, b) of x -> A x + b taking the style's mean and covariance to the content's:
    A = Sigma_c^1/2 Sigma_s^-1/2 (symmetric square roots by eigh; eigenvalues of Sigma_s
    floored at 1e-6 tr Sigma_s, so a grey or flat style stays finite), b = mu_c - A mu_s."""
    mu_s, cov_s = unpack_stats(stats_style)
    mu_c, cov_c = unpack_stats(stats_content)
    ls, vs = np.linalg.eigh(cov_s)
    ls = np.maximum(ls, max(1e-6 * np.trace(cov_s), 1e-12))  # 1e-12: a constant image
    lc, vc = np.linalg.eigh(cov_c)
    root_c = (vc * np.sqrt(np.maximum(lc, 0.0))) @ vc.T
    inv_root_s = (vs / np.sqrt(ls)) @ vs.T
    A = root_c @ inv_root_s
    return A, mu_c - A @ mu_s


def luma_moments(stats):
    """(mean, variance) of the de-normalised luminance of an image with these
    (normalised-space) colour stats: mu_Y = w . mu, sigma_Y^2 = w^T Sigma w."""
    mu, cov = unpack_stats(stats)
    ws = LUMA * _STD
    return float(LUMA @ (mu * _STD + _MEAN)), float(ws @ cov @ ws)


def luma_gain(stats_style, stats_content):
    """(a, o): Y -> a Y + o takes the style's luminance mean / variance to the content's
    (a flat style luminance keeps a = 1)."""
    ms, vs = luma_moments(stats_style)
    mc, vc = luma_moments(stats_content)
    a = float(np.sqrt(max(vc, 0.0) / vs)) if vs > 1e-12 else 1.0
    return a, mc - a * ms


def luma_matrix(a=1.0, o=0.0):
    """(M, b) of the luminance image (R = G = B = a Y + o after de-normalising):
    M[c][d] = a w_d std_d / std_c,  b_c = (a w . mean + o - mean_c) / std_c."""
    M = a * np.outer(1.0 / _STD, LUMA * _STD)
    b = (a * float(LUMA @ _MEAN) + o - _MEAN) / _STD
    return M, b


def merge_matrix():
    """M of the luminance merge out = base + M (x - base): M[c][d] = w_d std_d / std_c.
    YIQ^-1 maps Y to (1, 1, 1), so replacing base's luminance by x's adds the luminance
    difference to every de-normalised channel."""
    return np.outer(1.0 / _STD, LUMA * _STD)


def gamut_bounds():
    """(lo, hi): the displayable gamut, de-normalised [0, 1], per normalised channel."""
    return (0.0 - _MEAN) / _STD, (1.0 - _MEAN) / _STD


# ------------------------------------------------------------------------ device layer
def _dev(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to(constants.DEVICE, torch.float32).contiguous()


def _stats(img: torch.Tensor) -> np.ndarray:
    return ops.color_stats(img).cpu().numpy()[0]


def merge_luminance(stylised: torch.Tensor, content: torch.Tensor, out=None,
                    clamp=True) -> torch.Tensor:
    """The stylised image's luminance with the content image's chroma, one launch:
    out = content + M (stylised - content); with clamp, clamped to the displayable gamut
    (img_utils.to_pil clamps at 255, not 1: out-of-range values would wrap in .byte(),
    and the merge produces them far more often than a plain transfer)."""
    lo, hi = gamut_bounds() if clamp else (None, None)
    # img_utils.image_loader hands out channels-last strides: NCHW memory first (a no-op
    # for the tensors of the engines and the networks)
    return ops.color_affine(stylised.detach().contiguous(), merge_matrix(), None,
                            base=content.detach().contiguous(), lo=lo, hi=hi, out=out)


def prepare(style_images, content_image, mode):
    """Colour control around an ordinary transfer: returns (style_images',
    content_image', finish).  Run it BEFORE StyleNetwork(...), whose Gram targets are
    taken in __init__, and transfer with the returned images.

    mode "match": every style image recoloured to the content's mean and covariance;
      the content unchanged; finish is the identity.
    mode "luminance": the content becomes its luminance image, every style its luminance
      image moment-matched to the content's luminance; finish(result, clamp=True) merges
      the result's luminance onto the ORIGINAL content (merge_luminance).

    style_images: one [1, 3, h, w] tensor or a list of them (returned in kind)."""
    if mode not in MODES:
        raise ValueError(f"preserve-colour mode {mode!r}: expected one of {MODES}")
    single = isinstance(style_images, torch.Tensor)
    styles = [_dev(s) for s in ([style_images] if single else style_images)]
    content = _dev(content_image)
    sc = _stats(content)
    if mode == "match":
        new = [ops.color_affine(s, *match_matrix(_stats(s), sc)) for s in styles]

        def finish(result, clamp=True):
            return result
        return (new[0] if single else new), content, finish
    new = [ops.color_affine(s, *luma_matrix(*luma_gain(_stats(s), sc))) for s in styles]
    content_luma = ops.color_affine(content, *luma_matrix())

    def finish(result, clamp=True):
        return merge_luminance(_dev(result), content, clamp=clamp)
    return (new[0] if single else new), content_luma, finish
