"""Test helper (not a test module): the fp64 restatement of the AdaIN contract of
include/stx.h -- channel statistics, the AdaIN transform, the mean/std loss and its analytic
gradient -- and of the encoder / decoder / training objective of styletransfer_amd/adain.py
with plain torch ops in the dtype of their inputs (ReLU masks and pool argmax forced where a
gradient crosses them, as tests/forced_ref.py does for the fast_st step).

Paper: Huang & Belongie 2017, "Arbitrary Style Transfer in Real-time with Adaptive Instance
Normalization"; the reference project has no counterpart.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

EPS32 = float(np.float32(1e-5))  # the eps the kernels receive (a C float)

# mirrors of styletransfer_amd.adain.ENCODER_PLAN / DECODER_PLAN, restated
ENCODER_PLAN = ((3, 64), "T", (64, 64), "M", (64, 128), "T", (128, 128), "M", (128, 256), "T",
                (256, 256), (256, 256), (256, 256), "M", (256, 512), "T")
DECODER_PLAN = ((512, 256, True), "U", (256, 256, True), (256, 256, True), (256, 256, True),
                (256, 128, True), "U", (128, 128, True), (128, 64, True), "U", (64, 64, True),
                (64, 3, False))
DECODER_KEYS = [f"{i}.{p}" for i in (0, 3, 5, 7, 9, 12, 14, 17, 19) for p in ("weight", "bias")]


def _planes(x):
    x = torch.as_tensor(x)
    return x.reshape(x.shape[0], x.shape[1], -1)


def chan_stats(x, eps=EPS32, relu_input=False):
    """(mean, std) [n, c] in the dtype of x: unbiased variance, eps inside the root."""
    p = _planes(x)
    if relu_input:
        p = torch.where(p <= 0, torch.zeros_like(p), p)  # keeps a NaN
    hw = p.shape[2]
    mean = p.sum(2) / hw
    var = ((p - mean[:, :, None]) ** 2).sum(2) / (hw - 1)
    return mean, torch.sqrt(var + eps)


def adain(x, smean, sstd, mix, alpha, eps=EPS32):
    """y = (1 - alpha) x + alpha (G (x - mean) / std + M), M = mix @ smean, G = mix @ sstd."""
    x = torch.as_tensor(x)
    mean, std = chan_stats(x, eps)
    M, G = mix @ smean, mix @ sstd
    p = _planes(x)
    a = (1 - alpha) + alpha * G / std
    b = alpha * (M - G * mean / std)
    return (p * a[:, :, None] + b[:, :, None]).reshape(x.shape)


def stats_loss(x, tmean, tstd, weight=1.0, eps=EPS32):
    """(L, mean part, std part), L = weight / (n c) sum [(mean-tmean)^2 + (std-tstd)^2]."""
    mean, std = chan_stats(x, eps)
    k = weight / (mean.shape[0] * mean.shape[1])
    lm, ls = k * ((mean - tmean) ** 2).sum(), k * ((std - tstd) ** 2).sum()
    return lm + ls, lm, ls


def stats_loss_grad(x, tmean, tstd, weight=1.0, eps=EPS32, g=1.0, mean=None, std=None):
    """dL/dx analytically:  g weight/(n c) [2 (mean-tmean)/hw + 2 (std-tstd)(x-mean)/((hw-1)
    std)].  mean / std: statistics to differentiate at (default: those of x)."""
    x = torch.as_tensor(x)
    p = _planes(x)
    if mean is None:
        mean, std = chan_stats(x, eps)
    n, c, hw = p.shape
    k = g * weight / (n * c)
    A = k * 2 * (mean - tmean) / hw
    B = k * 2 * (std - tstd) / ((hw - 1) * std)
    return (A[:, :, None] + B[:, :, None] * (p - mean[:, :, None])).reshape(x.shape)


# ------------------------------------------------------------------ networks, forced branches
class Branches:
    """Records (masks=None) or replays the branch decisions of one forward in execution
    order: bool masks of the ReLUs, argmax indices of the 2x2 max pools (ties -> first)."""

    def __init__(self, masks=None):
        self.replay = masks is not None
        self.it = iter(masks) if masks is not None else None
        self.rec = []

    def relu(self, v):
        m = next(self.it) if self.replay else (v > 0)
        self.rec.append(m)
        return v * m.to(v.dtype)

    def pool(self, a):
        if self.replay:
            idx = next(self.it)
        else:
            _, idx = F.max_pool2d(a, 2, 2, return_indices=True)
        self.rec.append(idx)
        b, c, h, w = a.shape
        return a.reshape(b, c, h * w).gather(2, idx.reshape(b, c, -1)).reshape(b, c, h // 2,
                                                                               w // 2)


def encoder_forward(vw, x, br: Branches | None = None):
    """The four taps relu1_1, relu2_1, relu3_1, relu4_1 of the VGG-19 prefix; vw: nine (w, b)."""
    br = br if br is not None else Branches()
    taps, k = [], 0
    for item in ENCODER_PLAN:
        if item == "M":
            x = br.pool(x)
        elif item == "T":
            taps.append(x)
        else:
            x = br.relu(F.conv2d(x, vw[k][0], vw[k][1], 1, 1))
            k += 1
    return taps


def decoder_forward(sd, t, br: Branches | None = None):
    """Decoder forward from a state dict with the module keys ('0.weight' ... '19.bias')."""
    br = br if br is not None else Branches()
    i = 0
    for item in DECODER_PLAN:
        if item == "U":
            t = F.interpolate(t, scale_factor=2, mode="nearest")
            i += 1
            continue
        t = F.conv2d(t, sd[f"{i}.weight"], sd[f"{i}.bias"], 1, 1)
        i += 1
        if item[2]:
            t = br.relu(t)
            i += 1
    return t


def training_total(sd, vw, content, style, dec_masks=None, enc_masks=None, style_weight=10.0,
                   content_weight=1.0, eps=EPS32):
    """The AdaINTrainer objective; targets and t from unforced passes (constants), the
    decoder and the loss-side encoder pass with forced branches when masks are given.
    Returns (total, decoder branches, encoder branches)."""
    with torch.no_grad():
        targets = [chan_stats(t, eps) for t in encoder_forward(vw, style)]
        fc = encoder_forward(vw, content)[3]
        eye = torch.eye(fc.shape[0], dtype=fc.dtype)
        t = adain(fc, targets[3][0], targets[3][1], eye, 1.0, eps)
    bd, be = Branches(dec_masks), Branches(enc_masks)
    out = decoder_forward(sd, t, bd)
    taps = encoder_forward(vw, out, be)
    total = content_weight * F.mse_loss(taps[3], t)
    for tap, (tm, ts) in zip(taps, targets):
        total = total + stats_loss(tap, tm, ts, style_weight, eps)[0]
    return total, bd.rec, be.rec


def forced_grads(sd_np, vw_np, content, style, dec_masks, enc_masks, dtype, **kw):
    """Decoder parameter gradients (name -> tensor) and the loss with every branch forced."""
    sd = {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True)
          for k, v in sd_np.items()}
    vw = [(torch.tensor(w, dtype=dtype), torch.tensor(b, dtype=dtype)) for w, b in vw_np]
    total, _, _ = training_total(sd, vw, torch.as_tensor(content, dtype=dtype),
                                 torch.as_tensor(style, dtype=dtype), dec_masks, enc_masks, **kw)
    total.backward()
    return {k: t.grad for k, t in sd.items()}, float(total.detach())


def natural_branches(sd_np, vw_np, content, style, dtype=torch.float64, **kw):
    sd = {k: torch.tensor(np.asarray(v), dtype=dtype) for k, v in sd_np.items()}
    vw = [(torch.tensor(w, dtype=dtype), torch.tensor(b, dtype=dtype)) for w, b in vw_np]
    with torch.no_grad():
        _, bd, be = training_total(sd, vw, torch.as_tensor(content, dtype=dtype),
                                   torch.as_tensor(style, dtype=dtype), **kw)
    return bd, be


def count_flips(a, b):
    return sum(int((u != v).sum()) for u, v in zip(a, b))
