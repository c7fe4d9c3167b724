"""Test helper (not a test module): the multi-style (conditional instance norm)
restatement of tests/forced_ref.py.

The multi-style network normalises each sample without affine and scales / shifts it
with its own rows `mix @ table` of the per-layer style tables [S][C] (Dumoulin et al., "A
Learned Representation for Artistic Style"); everything else -- the convolutions, the
forced-branch protocol, the VGG loss network and the fast_st total -- is forced_ref's.
The style loss of sample k is taken against the Grams of ITS style: per-style targets
[S][C][C] per tap, gathered by the step's style ids.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

import forced_ref as R
from styletransfer_amd import weights as W

# the InstanceNorm layers of the ImageTransformNet in forward order
IN_SITES = ["1", "4", "7"] + [f"{b}.insn{i}" for b in range(9, 14) for i in (1, 2)] + ["16", "20"]
IN_KEYS = {f"{s}.{p}" for s in IN_SITES for p in ("weight", "bias")}


def multi_sd(seeds, conv_seed=None):
    """[(key, numpy array)] of a MultiStyleTransformNet: the convolutions of
    weights.itn_synthetic(conv_seed or seeds[0]), IN tensors [S][C] with row s from
    itn_synthetic(seeds[s]) (independent styles)."""
    per = [dict(W.itn_synthetic(s)) for s in seeds]
    conv = dict(W.itn_synthetic(conv_seed if conv_seed is not None else seeds[0]))
    return [(k, np.stack([p[k] for p in per]) if k in IN_KEYS else conv[k])
            for k, _ in W.itn_synthetic(seeds[0])]


def single_sd(sd, s):
    """The single-style state_dict list of style s of a multi_sd list."""
    return [(k, v[s] if k in IN_KEYS else v) for k, v in sd]


def one_hot(ids, n_styles, dtype=torch.float64):
    return F.one_hot(torch.as_tensor(ids, dtype=torch.long), n_styles).to(dtype)


def cond_norm(v, gtab, btab, mix):
    """Conditional instance norm: IN without affine, then the sample's mixed rows."""
    g, b = mix @ gtab, mix @ btab  # [n][c]
    return F.instance_norm(v, eps=1e-5) * g[:, :, None, None] + b[:, :, None, None]


def itn_forward_cond(sd, x, mix, br: R.Branches):
    """forced_ref.itn_forward for a multi-style state_dict (IN tensors [S][C]) and the
    per-sample style weights mix [n][S]."""
    def conv(k, v, stride, pad):
        return F.conv2d(v, sd[f"{k}.weight"], sd[f"{k}.bias"], stride, pad)

    def inorm(k, v):
        return cond_norm(v, sd[f"{k}.weight"], sd[f"{k}.bias"], mix)

    h = br.relu(inorm(1, conv(0, x, 1, 4)))
    h = br.relu(inorm(4, conv(3, h, 2, 1)))
    h = br.relu(inorm(7, conv(6, h, 2, 1)))
    for b in range(9, 14):
        t = br.relu(inorm(f"{b}.insn1", conv(f"{b}.conv1", h, 1, 1)))
        h = inorm(f"{b}.insn2", conv(f"{b}.conv2", t, 1, 1) + h)
    h = F.interpolate(h, scale_factor=2, mode="nearest")
    h = br.relu(inorm(16, conv(15, h, 1, 1)))
    h = F.interpolate(h, scale_factor=2, mode="nearest")
    h = br.relu(inorm(20, conv(19, h, 1, 1)))
    return conv(22, h, 1, 4)


def style_grams(vw, styles):
    """Per tap [S][C][C]: the Grams of each style image (each its own unforced pass)."""
    per = [[R.gram(z)[0] for z in R.vgg_forward(vw, s)] for s in styles]
    return [torch.stack([p[i] for p in per]) for i in range(5)]


def _tensors(sd_np, vgg_np, styles, batch, dtype, grad):
    sd = {k: torch.tensor(v, dtype=dtype, requires_grad=grad) for k, v in sd_np}
    vw = [(torch.tensor(w, dtype=dtype), torch.tensor(b, dtype=dtype)) for w, b in vgg_np]
    st = [torch.as_tensor(s, dtype=dtype).reshape(1, *np.shape(s)[-3:]) for s in styles]
    return sd, vw, st, torch.as_tensor(batch, dtype=dtype)


def forced_grads_cond(sd_np, vgg_np, styles, batch, ids, itn_masks, vgg_masks, dtype):
    """forced_ref.forced_grads for the multi-style step: sample k on style ids[k] (one-hot
    mix), its style targets the Grams of that style.  Returns (grads by name, total)."""
    sd, vw, st, x = _tensors(sd_np, vgg_np, styles, batch, dtype, True)
    S = len(st)
    idx = torch.as_tensor(ids, dtype=torch.long)
    with torch.no_grad():
        targets = [T[idx] for T in style_grams(vw, st)]  # [B][C][C] per tap
        c4 = R.vgg_forward(vw, x)[3]
    y = itn_forward_cond(sd, x, one_hot(ids, S, dtype), R.Branches(itn_masks))
    zs = R.vgg_forward(vw, y, R.Branches(vgg_masks))
    total = R.fast_st_total(y, zs, targets, c4)
    total.backward()
    return {k: t.grad for k, t in sd.items()}, float(total.detach())


def natural_branches_cond(sd_np, vgg_np, batch, ids, n_styles, dtype=torch.float64):
    """forced_ref.natural_branches for the multi-style forward."""
    sd, vw, _, x = _tensors(sd_np, vgg_np, [], batch, dtype, False)
    with torch.no_grad():
        bi, bv = R.Branches(), R.Branches()
        y = itn_forward_cond(sd, x, one_hot(ids, n_styles, dtype), bi)
        R.vgg_forward(vw, y, bv)
    return bi.rec, bv.rec
