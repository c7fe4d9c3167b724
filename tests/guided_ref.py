"""Test helper (not a test module): the region-guided Gram losses in plain torch, in the
dtype of their inputs -- the spatial control of Gatys et al. 2017, "Controlling Perceptual
Factors in Neural Style Transfer", as styletransfer_amd states it:

    G[b][r] = 1/(c hw) sum_p wts[r][p] z[b][:,p] z[b][:,p]^T
    loss_r  = 1/(b c c) sum_{b,i,j} (G[b][r] - T[r])^2
    loss    = sum_r lam[r] loss_r
    A[b][r] = weight lam[r] 4/(b c^3 hw) (G[b][r] - T[r])
    dz[b]   = s sum_r wts[r] o (A[b][r] z[b])

The reference project has no such feature; this restatement is the oracle, built on
tests/forced_ref.py for the VGG forward with forced branch decisions."""
from __future__ import annotations

import torch
import torch.nn.functional as F

import forced_ref as FR

TAP_POOLS = (0, 0, 1, 1, 2)


def guided_gram(z, wts):
    """z [b][c][h][w], wts [R][hw] -> G [b][R][c][c]."""
    b, c, h, w = z.shape
    f = z.reshape(b, c, h * w)
    return torch.einsum("rp,bip,bjp->brij", wts.to(z.dtype), f, f) / (c * h * w)


def region_losses(z, wts, targets):
    """loss_r [R] for targets [R][c][c]."""
    d = guided_gram(z, wts) - targets.to(z.dtype)[None]
    b, c = z.shape[:2]
    return (d * d).sum(dim=(0, 2, 3)) / (b * c * c)


def coef(z, wts, targets, lam, weight=1.0):
    """A [b][R][c][c]."""
    b, c, h, w = z.shape
    d = guided_gram(z, wts) - targets.to(z.dtype)[None]
    lam = torch.as_tensor(lam, dtype=z.dtype)
    return weight * 4.0 / (b * c ** 3 * h * w) * lam[None, :, None, None] * d


def gram_bwd(A, z, wts, s=1.0):
    """The closed-form dz [b][c][h][w] = s sum_r wts[r] o (A[b][r] z[b])."""
    b, c, h, w = z.shape
    f = z.reshape(b, c, h * w)
    return (s * torch.einsum("rp,brij,bjp->bip", wts.to(z.dtype), A, f)).reshape(z.shape)


def normalise(w):
    """Rows of w [R][hw] scaled to sum hw."""
    return w * (w.shape[1] / w.sum(dim=1, keepdim=True))


def tap_maps(guides, dtype=torch.float64):
    """[R][H][W] guides -> five [R][hw_l] normalised weight rows (floor-mode 2x2 average
    pools before taps 3-4 and once more before tap 5)."""
    cur, pooled, out = guides.to(dtype), 0, []
    for k in TAP_POOLS:
        while pooled < k:
            cur = F.avg_pool2d(cur[None], 2)[0]
            pooled += 1
        out.append(normalise(cur.reshape(cur.shape[0], -1)))
    return out


def style_targets(vw, style_images, dtype):
    """T_l [R][c][c] from whole style images (no style guide)."""
    per = [[FR.gram(z)[0] for z in FR.vgg_forward(vw, s.to(dtype))] for s in style_images]
    return [torch.stack([per[r][l] for r in range(len(per))]) for l in range(5)]


def engine_iteration(vgg_np, x, content, style_images, guides, lam, masks, dtype,
                     style_weight=100_000.0, content_weight=1.0):
    """One GuidedGatysEngine iteration without Adam, branches forced to `masks`
    (forced_ref.vgg_branches_from_z of the engine's own Z): returns (tap losses [5] =
    sum_r lam_r loss_{l,r}, region losses [5][R], content loss, total, dx)."""
    vw = [(torch.tensor(w, dtype=dtype), torch.tensor(b, dtype=dtype)) for w, b in vgg_np]
    with torch.no_grad():
        targets = style_targets(vw, style_images, dtype)
        c4 = FR.vgg_forward(vw, content.to(dtype))[3]
    maps = tap_maps(guides, dtype)
    xv = x.detach().to(dtype).clone().requires_grad_()
    zs = FR.vgg_forward(vw, xv, FR.Branches(masks))
    lam_t = torch.as_tensor(lam, dtype=dtype)
    reg = torch.stack([region_losses(z, w, t) for z, w, t in zip(zs, maps, targets)])
    taps = (reg * lam_t[None]).sum(dim=1)
    closs = F.mse_loss(zs[3], c4)
    total = style_weight * taps.sum() + content_weight * closs
    total.backward()
    return taps.detach(), reg.detach(), closs.detach(), total.detach(), xv.grad
