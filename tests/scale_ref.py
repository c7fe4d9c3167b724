"""Test helper (not a test module): the scale control of Gatys et al. 2017, "Controlling
Perceptual Factors in Neural Style Transfer", section 6, as styletransfer_amd states it.

Resampling, in fp64 numpy: per axis scale = in / out, s = max(scale, 1), radius 1
(triangle) or 2 (cubic, Keys a = -0.5), support = radius s, and for output i the centre
c = scale (i + 0.5):

    first = max(0, int(c - support + 0.5)),  end = min(in, int(c + support + 0.5))
    w_j   = f((j - c + 0.5) / s) for j in [first, end), divided by their sum

The reference project has no such feature; this restatement is the oracle (itself checked
against torch's antialiased interpolate on the CPU in tests/test_scale_host.py).  The engine
iteration with one style weight per tap is built on tests/forced_ref.py."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

import forced_ref as FR

RADIUS = {"triangle": 1.0, "cubic": 2.0}


def _f(filter, t):
    t = np.abs(t)
    if filter == "triangle":
        return np.where(t < 1.0, 1.0 - t, 0.0)
    a = -0.5
    near = ((a + 2.0) * t - (a + 3.0)) * t * t + 1.0
    far = ((a * t - 5.0 * a) * t + 8.0 * a) * t - 4.0 * a
    return np.where(t < 1.0, near, np.where(t < 2.0, far, 0.0))


def plan(n_in, n_out, filter):
    """(first [out], count [out], w [out][k] fp64 zero padded, k = the largest count)."""
    scale = n_in / n_out
    s = max(scale, 1.0)
    support = RADIUS[filter] * s
    first = np.zeros(n_out, np.int64)
    count = np.zeros(n_out, np.int64)
    rows = []
    for i in range(n_out):
        c = scale * (i + 0.5)
        lo = max(0, int(c - support + 0.5))
        hi = min(n_in, int(c + support + 0.5))
        j = np.arange(lo, hi, dtype=np.float64)
        w = _f(filter, (j - c + 0.5) / s)
        rows.append(w / w.sum())
        first[i], count[i] = lo, hi - lo
    k = int(count.max())
    w = np.zeros((n_out, k), np.float64)
    for i, r in enumerate(rows):
        w[i, :len(r)] = r
    return first, count, w, k


def matrix(n_in, n_out, filter):
    """The axis plan as a dense [out][in] fp64 matrix (identity for an unchanged size: the
    kernel skips that axis)."""
    if n_in == n_out:
        return np.eye(n_in, dtype=np.float64)
    first, count, w, _ = plan(n_in, n_out, filter)
    m = np.zeros((n_out, n_in), np.float64)
    for i in range(n_out):
        m[i, first[i]:first[i] + count[i]] = w[i, :count[i]]
    return m


def resize(x, ho, wo, filter):
    """x [..., hi, wi] -> [..., ho, wo] in fp64: horizontal, then vertical."""
    x = np.asarray(x, np.float64)
    mx = matrix(x.shape[-1], wo, filter)
    my = matrix(x.shape[-2], ho, filter)
    return np.einsum("yh,...hx->...yx", my, np.einsum("...hw,xw->...hx", x, mx))


def abs_bound(x, ho, wo, filter):
    """sum_y |w_y| sum_x |w_x| |x| per output element, fp64: what the rounding errors of the
    two passes scale with."""
    x = np.abs(np.asarray(x, np.float64))
    mx = np.abs(matrix(x.shape[-1], wo, filter))
    my = np.abs(matrix(x.shape[-2], ho, filter))
    return np.einsum("yh,...hx->...yx", my, np.einsum("...hw,xw->...hx", x, mx))


def taps(n_in, n_out, filter):
    """The k of one axis as the error bound counts it (0 for a skipped axis)."""
    return 0 if n_in == n_out else plan(n_in, n_out, filter)[3]


def engine_iteration(vgg_np, x, content, style, layer_weights, masks, dtype,
                     style_weight=100_000.0, content_weight=1.0):
    """One Gatys iteration without the optimiser, one style weight per tap, branches forced
    to `masks` (forced_ref.vgg_branches_from_z of the engine's own Z): returns (tap losses
    [5], unweighted; content loss; total = style_weight sum_l w_l loss_l + content_weight
    content; dx)."""
    vw = [(torch.tensor(w, dtype=dtype), torch.tensor(b, dtype=dtype)) for w, b in vgg_np]
    with torch.no_grad():
        targets = [FR.gram(z) for z in FR.vgg_forward(vw, style.to(dtype))]
        c4 = FR.vgg_forward(vw, content.to(dtype))[3]
    xv = x.detach().to(dtype).clone().requires_grad_()
    zs = FR.vgg_forward(vw, xv, FR.Branches(masks))
    taps_ = torch.stack([F.mse_loss(FR.gram(z), t) for z, t in zip(zs, targets)])
    lw = torch.as_tensor(list(layer_weights), dtype=dtype)
    closs = F.mse_loss(zs[3], c4)
    total = style_weight * (taps_ * lw).sum() + content_weight * closs
    total.backward()
    return taps_.detach(), closs.detach(), total.detach(), xv.grad
