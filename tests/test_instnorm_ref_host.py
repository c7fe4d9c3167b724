"""Pins tests/instnorm_ref.py (the fp64 reference tests/test_instnorm_gpu.py holds the
InstanceNorm kernels to) to torch fp64 F.instance_norm and its autograd, so that a wrong
reference cannot excuse a wrong kernel.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import instnorm_ref as R

RTOL = 1e-12  # fp64 against fp64: summation-order rounding only
EPS = float(np.float32(1e-5))  # the ABI's eps is an fp32 value
N, C = 2, 3  # n * c = 6 planes


def close(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, what
    assert np.all(np.abs(a - b) <= RTOL * (1 + np.abs(b))), (what, np.abs(a - b).max())


def f32(*shape, seed, scale=1.0, shift=0.0):
    """fp32-representable values (what the kernels are given), as float64."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale + shift).double()


def torch_in(u, gamma, beta):
    if u.shape[2] > 1:
        return F.instance_norm(u, weight=gamma, bias=beta, eps=EPS)
    # F.instance_norm refuses one spatial element; the same formula by hand
    mean = u.mean(dim=2, keepdim=True)
    y = (u - mean) / torch.sqrt(u.var(dim=2, unbiased=False, keepdim=True) + EPS)
    if gamma is not None:
        y = y * gamma.view(1, -1, 1) + beta.view(1, -1, 1)
    return y


@pytest.mark.parametrize("hw", [1, 7, 63, 4100])
@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("relu", [False, True])
def test_reference_is_torch_fp64_instance_norm(hw, affine, res, relu):
    x = f32(N, C, hw, seed=1, scale=1.5, shift=0.3)
    r = f32(N, C, hw, seed=2) if res else None
    dy = f32(N, C, hw, seed=3)
    gamma = f32(C, seed=4, scale=0.5, shift=1.0) if affine else None
    beta = f32(C, seed=5) if affine else None
    # u as the kernels form it: the fp32 sum.  torch gets that u, so du is d/du
    u = torch.from_numpy(R.form_u(x.numpy(), None if r is None else r.numpy())).requires_grad_()
    if res:
        assert torch.equal(u.detach(), (x.float() + r.float()).double())
    leaves = [t.requires_grad_() for t in (gamma, beta) if t is not None]
    y = torch_in(u, gamma, beta)
    y = F.relu(y) if relu else y
    grads = torch.autograd.grad(y, [u] + leaves, dy)

    f = R.fwd(x.numpy(), None if gamma is None else gamma.detach().numpy(),
              None if beta is None else beta.detach().numpy(),
              res=None if r is None else r.numpy(), eps=1e-5, relu=relu)
    ud = u.detach()
    close(f.y, y.detach().numpy(), "y")
    close(f.mean, ud.mean(dim=2).numpy(), "mean")
    close(f.var, ud.var(dim=2, unbiased=False).numpy(), "var")
    close(f.rstd, (1 / torch.sqrt(ud.var(dim=2, unbiased=False) + EPS)).numpy(), "rstd")
    assert np.all(f.absmean >= np.abs(f.mean))
    yl = R.fwd(x.numpy(), None if gamma is None else gamma.detach().numpy(),
               None if beta is None else beta.detach().numpy(),
               res=None if r is None else r.numpy(), eps=1e-5, relu=False).y
    assert np.all(f.ymag * (1 + 1e-12) >= np.abs(yl)) and np.all(np.abs(yl) >= np.abs(f.y))

    mask = (f.y > 0).astype(np.float64) if relu else None
    b = R.bwd(dy.numpy(), x.numpy(), None if gamma is None else gamma.detach().numpy(),
              f.mean, f.rstd, res=None if r is None else r.numpy(), mask=mask)
    close(b.du, grads[0].numpy(), "du")
    close(b.sdu, grads[0].sum(dim=2).numpy(), "sum du")
    close(b.dbias_in, grads[0].sum(dim=(0, 2)).numpy(), "dbias_in")
    g = dy.numpy() * (1.0 if mask is None else mask)
    close(b.sg, g.sum(axis=2), "sg")
    close(b.sgx, (g * b.xh).sum(axis=2), "sgx")
    if affine:
        close(b.dgamma, grads[1].numpy(), "dgamma")
        close(b.dbeta, grads[2].numpy(), "dbeta")
    else:
        close(b.dgamma, b.sgx.sum(axis=0), "dgamma")
        close(b.dbeta, b.sg.sum(axis=0), "dbeta")
    # every magnitude dominates its value
    assert np.all(b.dumag * np.abs(b.k) * (1 + 1e-12) >= np.abs(b.du))
    assert np.all(b.sgmag >= np.abs(b.sg)) and np.all(b.sgxmag >= np.abs(b.sgx))
    assert np.all(b.sdumag >= np.abs(b.sdu))
    assert np.all(b.dgamma_mag >= np.abs(b.dgamma)) and np.all(b.dbeta_mag >= np.abs(b.dbeta))
    assert np.all(b.dbias_in_mag >= np.abs(b.dbias_in))


def test_mean_and_rstd_are_inputs_of_the_backward():
    """bwd uses the statistics it is given, not ones it recomputes (the GPU test hands it
    the HIP forward's saved values): with perturbed statistics it is the closed form."""
    x, dy = f32(N, C, 7, seed=6).numpy(), f32(N, C, 7, seed=7).numpy()
    f = R.fwd(x)
    m, s = f.mean + 0.25, f.rstd * 1.5
    b = R.bwd(dy, x, None, m, s)
    xh = (x - m[..., None]) * s[..., None]
    sg, sgx = dy.sum(axis=2, keepdims=True), (dy * xh).sum(axis=2, keepdims=True)
    close(b.du, s[..., None] / 7 * (7 * dy - sg - xh * sgx), "du")
