"""Scale control: coarse-to-fine Gatys transfer and scale-mixed styles (Gatys et al. 2017,
"Controlling Perceptual Factors in Neural Style Transfer", section 6; the reference
project has no such feature).

The loss network stops at conv3_1, whose deepest tap sees a window of about 24 pixels:
at 256^2 a fair part of the image, at 1024^2 only fine texture.

  * coarse-to-fine (6.2): transfer at a low resolution, resample the result up, continue
    from it at the next resolution -- the large-scale structure is laid down where the
    network can see it.  Every level is an ordinary engine (vgg.GatysEngine, GatysLBFGS,
    GuidedGatysEngine) with its own targets and fresh optimiser state; the levels are
    joined by ops.resample2d and nothing else.
  * scale mixing (6.1): a new style image that has the fine scale of one style (the
    shallow taps' Gram losses only) and the coarse scale of another (the starting point,
    which with no content loss only the shallow taps move).

Sizes are the sides of square images.  Everything stays on the device; the resampling
tables are built on the host once per (in, out, filter) and cached (ops.resample2d)."""
from __future__ import annotations

import torch

from . import constants, ops
from . import vgg as V

# The largest side verified for every launch of a Gatys iteration.
MAX_SIDE = 1024


def check_sizes(sizes):
    """The pyramid's sides as a list of ints: strictly ascending positive multiples of 4
    (two 2x2 pools, and the 16-byte rows of the resampler's vector path), MAX_SIDE at most."""
    try:
        out = [int(s) for s in sizes]
        exact = all(float(s) == float(i) for s, i in zip(sizes, out))
    except (TypeError, ValueError):
        raise ValueError(f"sizes {sizes!r}: a list of integers expected") from None
    if not out or not exact:
        raise ValueError(f"sizes {sizes!r}: at least one integer size expected")
    for s in out:
        if s <= 0 or s % 4:
            raise ValueError(f"size {s}: a positive multiple of 4 expected")
        if s > MAX_SIDE:
            raise ValueError(f"size {s}: at most {MAX_SIDE} (scale.MAX_SIDE) supported")
    if any(b <= a for a, b in zip(out, out[1:])):
        raise ValueError(f"sizes {out}: strictly ascending expected")
    return out


def level_steps(steps, levels):
    """An int (every level) or one count per level -> a list of `levels` ints."""
    if isinstance(steps, int):
        out = [steps] * levels
    else:
        out = [int(s) for s in steps]
        if len(out) != levels:
            raise ValueError(f"{len(out)} step counts for {levels} levels")
    if min(out) < 0:
        raise ValueError(f"steps {out}: non-negative counts expected")
    return out


def _dev(t: torch.Tensor) -> torch.Tensor:
    return torch.as_tensor(t).detach().to(constants.DEVICE, torch.float32).contiguous()


def _at(t, size, filter="cubic", clamp=False):
    """t [..., h, w] at size x size: t itself where it already has that size."""
    if tuple(t.shape[-2:]) == (size, size):
        return t
    out = ops.resample2d(t, size, filter)
    return out.clamp_(0.0, 1.0) if clamp else out


def pyramid(t, sizes, filter="cubic"):
    """t (an [n, c, h, w] image batch or [r, h, w] guides, of the top size) at every size of
    `sizes`, each level resampled from t itself; the top level is t, not a copy.  Images:
    filter "cubic"; guides: "triangle", and the result clamped to [0, 1] (the rounded
    weights of a row can sum to 1 + 2^-24)."""
    sizes = check_sizes(sizes)
    t = _dev(t)
    if tuple(t.shape[-2:]) != (sizes[-1], sizes[-1]):
        raise ValueError(f"a {sizes[-1]} x {sizes[-1]} tensor expected, got {tuple(t.shape)}")
    return [_at(t, s, filter, clamp=filter == "triangle") for s in sizes]


def _release(eng):
    """Drop an engine's captured graphs and buffers now: its result has been copied out, and
    a graph left for the cyclic collector could be destroyed while a later level captures
    (ops.graph_capture)."""
    torch.cuda.current_stream().synchronize()
    for name in ("graph", "g_eval", "g_iter"):
        if getattr(eng, name, None) is not None:
            setattr(eng, name, None)
    for name in ("st", "scratch", "opt", "coef", "lws"):
        if hasattr(eng, name):
            setattr(eng, name, None)


def _finish(eng, steps):
    eng.run(steps)
    x = eng.x.detach().clone()
    _release(eng)
    return x


def coarse_to_fine(feat, style, content, sizes, steps, optimizer="adam", init=None,
                   **engine_kw):
    """Section 6.2 over vgg.GatysEngine ("adam") or vgg.GatysLBFGS ("lbfgs").  Level 0
    starts from the content at sizes[0] (or init, resampled to it if need be); level k > 0
    from level k - 1's result resampled (cubic) to sizes[k].  Every level takes the style
    and the content resampled (cubic) from the images given -- an image that already has
    the level's size is used as it is -- builds its own style targets, content target and
    engine, and runs steps[k] iterations (an int: the same count at every level; for
    "lbfgs" outer steps).  engine_kw goes to every level's engine (style_weight,
    content_weight, style_layer_weights, ...).  Returns the top-level image."""
    if optimizer not in ("adam", "lbfgs"):
        raise ValueError(f"optimizer {optimizer!r}: 'adam' or 'lbfgs' expected")
    sizes = check_sizes(sizes)
    steps = level_steps(steps, len(sizes))
    style, content = _dev(style), _dev(content)
    engine = V.GatysEngine if optimizer == "adam" else V.GatysLBFGS
    x = None if init is None else _at(_dev(init), sizes[0])
    for k, size in enumerate(sizes):
        if k > 0:
            x = ops.resample2d(x, size, "cubic")
        eng = engine(feat, _at(style, size), _at(content, size), init=x, **engine_kw)
        x = _finish(eng, steps[k])
        del eng
    return x


def coarse_to_fine_guided(feat, style_images, content, guides, sizes, steps, style_guides=None,
                          init=None, **engine_kw):
    """coarse_to_fine over vgg.GuidedGatysEngine: the guides [R, H, W] and the style guides
    (a list with None for a whole style image) are resampled per level with the triangle
    filter and clamped to [0, 1]."""
    sizes = check_sizes(sizes)
    steps = level_steps(steps, len(sizes))
    styles = [_dev(s) for s in style_images]
    content = _dev(content)
    if isinstance(guides, (list, tuple)):
        guides = torch.stack([torch.as_tensor(g).reshape(g.shape[-2:]) for g in guides])
    guides = _dev(guides)
    if guides.dim() == 2:
        guides = guides[None]
    if style_guides is not None:
        style_guides = [None if g is None else _dev(g).reshape((1,) + tuple(g.shape[-2:]))
                        for g in style_guides]
    x = None if init is None else _at(_dev(init), sizes[0])
    for k, size in enumerate(sizes):
        if k > 0:
            x = ops.resample2d(x, size, "cubic")
        sg = None if style_guides is None else \
            [None if g is None else _at(g, size, "triangle", clamp=True)[0] for g in style_guides]
        eng = V.GuidedGatysEngine(feat, [_at(s, size) for s in styles], _at(content, size),
                                  _at(guides, size, "triangle", clamp=True), style_guides=sg,
                                  init=x, **engine_kw)
        x = _finish(eng, steps[k])
        del eng
    return x


def mix_scales(feat, fine_style, coarse_style, steps, fine_taps=3, **engine_kw):
    """Section 6.1: a style image with fine_style's fine scale and coarse_style's coarse
    scale.  An Adam transfer that starts from coarse_style with no content loss and the
    style loss of the first fine_taps taps only (conv1_1 .. conv2_1 for 3), against
    fine_style.  Both images must have the same size."""
    if not 1 <= int(fine_taps) <= 4:
        raise ValueError(f"fine_taps {fine_taps}: 1 to 4 expected")
    fine_style, coarse_style = _dev(fine_style), _dev(coarse_style)
    if fine_style.shape != coarse_style.shape:
        raise ValueError(f"fine style {tuple(fine_style.shape)} and coarse style "
                         f"{tuple(coarse_style.shape)}: the same size expected")
    ft = int(fine_taps)
    eng = V.GatysEngine(feat, fine_style, coarse_style, content_weight=0,
                        style_layer_weights=[1.0] * ft + [0.0] * (5 - ft), **engine_kw)
    return _finish(eng, steps)
