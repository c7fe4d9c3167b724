"""Plain fp64 reference of stx_instnorm_fwd / stx_instnorm_bwd (include/stx.h), written
from the header's statement of the op and not from the kernels; numpy only.
tests/test_instnorm_ref_host.py pins it against torch fp64 autograd;
tests/test_instnorm_gpu.py compares the kernels with it element by element.

Arrays are [n][c][hw] (planes) and [c] (affine); fp32 inputs are read as float64.  Besides
each value the functions return the magnitudes its error bound scales with: a pointwise
value comes with the sum of the magnitudes of its terms, a sum with sum|terms|."""
from types import SimpleNamespace

import numpy as np


def f64(a):
    return np.asarray(a, dtype=np.float64)


def form_u(x, res=None):
    """u = x (+ res).  With res the sum is rounded once to fp32, as every kernel forms it
    (fp32 inputs); without, u is x."""
    if res is None:
        return f64(x)
    return f64(np.add(np.asarray(x, dtype=np.float32), np.asarray(res, dtype=np.float32),
                      dtype=np.float32))


def _affine(v, c, fill):
    return np.full(c, fill) if v is None else f64(v).reshape(c)


def fwd(x, gamma=None, beta=None, res=None, eps=1e-5, relu=False):
    """mean, biased var, rstd = 1 / sqrt(var + eps) per plane [n][c];
    y = (u - mean) rstd gamma + beta, then y <= 0 ? 0 : y with relu (a NaN stays).
    eps is the fp32 value the ABI takes.  Magnitudes: absmean = sum|u| / hw (the mean's
    terms) and ymag = |u gamma rstd| + |beta - mean gamma rstd| (y's two terms)."""
    u = form_u(x, res)
    n, c, hw = u.shape
    eps = float(np.float32(eps))
    g, b = _affine(gamma, c, 1.0)[None, :, None], _affine(beta, c, 0.0)[None, :, None]
    mean = u.sum(axis=2) / hw
    d = u - mean[..., None]
    var = (d * d).sum(axis=2) / hw
    rstd = 1.0 / np.sqrt(var + eps)
    gsc = g * rstd[..., None]
    sh = b - mean[..., None] * gsc
    y = d * gsc + b
    if relu:
        y = np.where(y <= 0, 0.0, y)
    return SimpleNamespace(u=u, mean=mean, var=var, rstd=rstd, y=y,
                           absmean=np.abs(u).sum(axis=2) / hw,
                           ymag=np.abs(u * gsc) + np.abs(sh))


def bwd(dy, x, gamma, mean, rstd, res=None, mask=None):
    """The backward of fwd given the forward's saved mean / rstd [n][c] (inputs, as in
    stx_instnorm_bwd) and the ReLU's 0/1 mask [n][c][hw] (None: no ReLU):
      g = dy mask;  xh = (u - mean) rstd;  sg = sum g;  sgx = sum g xh   (per plane)
      du = k (hw g - sg - xh sgx),  k = gamma rstd / hw;  sdu = sum du   (per plane)
      dgamma = sum_n sgx;  dbeta = sum_n sg;  dbias_in = sum_n sdu       (per channel)
    Magnitudes: dumag = hw|g| + |sg| + |xh sgx| per element; sgmag, sgxmag, sdumag the
    sum|terms| of the three plane sums; dgamma_mag, dbeta_mag, dbias_in_mag = sum_n |part|."""
    u = form_u(x, res)
    n, c, hw = u.shape
    mean, rstd = f64(mean).reshape(n, c, 1), f64(rstd).reshape(n, c, 1)
    g = f64(dy).reshape(n, c, hw)
    if mask is not None:
        g = np.where(f64(mask).reshape(n, c, hw) != 0, g, 0.0)
    xh = (u - mean) * rstd
    sg = g.sum(axis=2)
    sgx = (g * xh).sum(axis=2)
    k = _affine(gamma, c, 1.0)[None, :, None] * rstd / hw
    t = xh * sgx[..., None]
    du = k * (hw * g - sg[..., None] - t)
    sdu = du.sum(axis=2)
    r = SimpleNamespace(du=du, sg=sg, sgx=sgx, sdu=sdu, k=k, xh=xh, g=g,
                        dumag=hw * np.abs(g) + np.abs(sg)[..., None] + np.abs(t),
                        sgmag=np.abs(g).sum(axis=2), sgxmag=np.abs(g * xh).sum(axis=2),
                        sdumag=np.abs(du).sum(axis=2))
    for name, part in (("dgamma", sgx), ("dbeta", sg), ("dbias_in", sdu)):
        setattr(r, name, part.sum(axis=0))
        setattr(r, name + "_mag", np.abs(part).sum(axis=0))
    return r
