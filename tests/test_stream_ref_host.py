"""Pins tests/stream_ref.py (the fp64 references the streaming-kernel GPU tests compare
against) to torch fp64 and its autograd, so that a wrong reference cannot excuse a wrong
kernel.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import reference_cpu as O

import stream_ref as R

RTOL = 1e-12  # fp64 against fp64: summation-order rounding only


def t64(*shape, seed=0, ties=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1
    if ties:  # few distinct values: many equal neighbours and exact zeros
        x = torch.round(x * 2) / 2
    return x


def close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    assert np.all(np.abs(a - b) <= RTOL * (1 + np.abs(b))), np.abs(a - b).max()


@pytest.mark.parametrize("n", [1, 3, 1001])
def test_mse_and_grad(n):
    a, b = t64(n, seed=1), t64(n, seed=2)
    a.requires_grad_()
    loss = F.mse_loss(a, b)
    (3.5 * loss).backward()
    ga, a, loss = a.grad.numpy(), a.detach(), loss.detach()
    close(R.mse(a, b, 0), [float(loss)])
    g, mag = R.mse_grad(a, b, 3.5)
    close(g, ga)
    assert np.all(mag >= np.abs(g))
    lr = float(F.mse_loss(F.relu(a), F.relu(b)))
    close(R.mse(a, b, 0, relu_inputs=True), [lr])
    close(R.mse(a, b, 1, relu_inputs=True), [lr * lr / n, lr])
    close(R.mse(a, b, 2), [float(loss), lr * lr / n, lr])


@pytest.mark.parametrize("relu", [False, True])
def test_diff_scale_is_the_backward_of_the_mse_losses(relu):
    """d/da [s * sum (f(a) - f(b))^2 / 2] = s (f(a) - f(b)) [a > 0], with exact zeros and
    negative a against positive b (mask 0 although relu(a) - relu(b) != 0)."""
    a, b = t64(257, seed=3, ties=True), t64(257, seed=4)
    a[:4] = torch.tensor([0.0, -0.5, 0.0, -1.0], dtype=torch.float64)
    b[:4] = 0.75
    a.requires_grad_()
    f = F.relu if relu else (lambda v: v)
    (0.5 * 1.25 * -2.0 * 0.5 * ((f(a) - f(b)) ** 2).sum()).backward()
    old = t64(257, seed=5).numpy()
    v, mag = R.diff_scale(a, b, 1.25, -2.0, 0.5, relu_inputs=relu, old=old)
    close(v, a.grad.numpy() + old)
    assert np.all(mag >= np.abs(v) - 1e-15)
    if relu:
        assert np.all(v[:4] == old[:4])


def test_loss_combine_and_finalize():
    s, w = t64(7, seed=6), [0.5, -2.0, 3.0, 1.0, 1e5]
    v, mag = R.loss_combine(s, w)
    close(v, float((torch.tensor(w, dtype=torch.float64) * s[:5]).sum()))
    assert mag >= abs(v)
    parts = [t64(n, seed=10 + n) for n in (1, 65, 449)]
    inv = [0.25, 1 / 3, 2.0]
    extra = t64(2, seed=7)
    w = [1.0, -2.0, 0.5, 4.0, 8.0]
    losses, mags, tot, tmag = R.loss_finalize(parts, inv, extra, w)
    want = [iv * float(p.sum()) for p, iv in zip(parts, inv)]
    close(losses, want)
    close(tot, sum(wi * li for wi, li in zip(w, want + extra.tolist())))
    assert np.all(mags >= np.abs(losses)) and tmag >= abs(tot)
    assert R.loss_finalize(parts, inv)[2] is None


POOL_PLANES = [(3, 2, 2), (5, 7, 9), (4, 10, 14), (3, 9, 2), (2, 8, 1)]


def pool_input(nc, h, w, seed):
    """Signed, with a window of four equal values, one of all negatives (ReLU makes it a
    four-way tie at 0), pairwise ties elsewhere and a -inf window."""
    x = t64(nc, h, w, seed=seed, ties=True)
    if h >= 2 and w >= 2:
        x[0, :2, :2] = 0.5
        x[1, :2, :2] = torch.tensor([[-0.25, -1.0], [-0.5, -0.75]], dtype=torch.float64)
        x[2, :2, :2] = float("-inf")
    return x


@pytest.mark.parametrize("plane", POOL_PLANES)
@pytest.mark.parametrize("relu", [False, True])
def test_maxpool_matches_torch_cpu_exactly(plane, relu):
    nc, h, w = plane
    x = pool_input(nc, h, w, seed=20)
    y, idx = R.maxpool_fwd(x, relu_input=relu)
    if h // 2 == 0 or w // 2 == 0:
        assert y.size == 0
        return
    xt = x.clone().requires_grad_()
    ty, tidx = F.max_pool2d(F.relu(xt) if relu else xt, 2, 2, return_indices=True)
    assert np.array_equal(y, ty.detach().numpy())
    assert np.array_equal(idx, tidx.numpy())  # ties, -inf: torch CPU's choice exactly
    dy = t64(*ty.shape, seed=21)
    ty.backward(dy)
    if relu:
        close(R.relupool_bwd(dy, x), xt.grad.numpy())
        dz = R.relupool_bwd(dy, x)
        assert np.all(dz[1, :2, :2] == 0)  # the all-non-positive window: no gradient
    else:
        dx = R.maxpool_bwd(dy, idx, h, w)
        assert np.array_equal(dx, xt.grad.numpy())
        assert np.all(dx[:, 2 * (h // 2):, :] == 0) and np.all(dx[:, :, 2 * (w // 2):] == 0)


def test_maxpool_nan_wins_like_torch():
    x = t64(2, 4, 6, seed=22)
    x[0, 0, 1] = float("nan")
    x[1, 3, 4] = float("nan")
    x[1, 2, 5] = float("nan")  # two in one window: the later one (row-major) is the index
    for relu in (False, True):
        y, idx = R.maxpool_fwd(x, relu_input=relu)
        ty, tidx = F.max_pool2d(F.relu(x) if relu else x, 2, 2, return_indices=True)
        assert np.array_equal(y, ty.numpy(), equal_nan=True)
        assert np.array_equal(idx, tidx.numpy())
    assert np.isnan(R.relu(x)[0, 0, 1]) and bool(torch.isnan(F.relu(x)[0, 0, 1]))
    dz = R.relupool_bwd(np.ones((2, 2, 3)), x)
    assert dz[0, 0, 1] == 0 and dz[1, 3, 4] == 0 and dz[1, 2, 5] == 0


def test_relu():
    x = t64(300, seed=23, ties=True).requires_grad_()
    y = F.relu(x)
    dy = t64(300, seed=24)
    y.backward(dy)
    assert np.array_equal(R.relu(x), y.detach().numpy())
    assert np.array_equal(R.relu_bwd(dy, y.detach()), x.grad.numpy())
    ynan = y.detach().clone()
    ynan[5] = float("nan")
    assert R.relu_bwd(dy, ynan)[5] == 0


@pytest.mark.parametrize("plane", [(1, 1, 1), (6, 5, 7)])
def test_upsample(plane):
    x = t64(1, *plane, seed=25).requires_grad_()
    y = F.interpolate(x, scale_factor=2, mode="nearest")
    dy = t64(*y.shape, seed=26)
    y.backward(dy)
    assert np.array_equal(R.upsample_fwd(x[0]), y[0].detach().numpy())
    dx, mag = R.upsample_bwd(dy[0])
    close(dx, x.grad[0].numpy())
    assert np.all(mag >= np.abs(dx))


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (2, 3, 1, 9), (2, 3, 9, 1), (2, 3, 5, 7)])
@pytest.mark.parametrize("ties", [False, True])
def test_tv_is_the_oracle_expression(shape, ties):
    y = t64(*shape, seed=27, ties=ties).requires_grad_()
    loss = O.total_variation(y, factor=0.125)
    (2.5 * -3.0 * loss).backward()
    v, mag, g, gmag = R.tv(y, 0.125, gscale=2.5, gscale_dev=-3.0)
    close(v, float(loss))
    assert mag >= abs(v)
    close(g, y.grad.numpy())
    assert np.all(gmag >= np.abs(g))


def test_tv_constant_planes_give_zero():
    y = torch.arange(6, dtype=torch.float64).reshape(2, 3, 1, 1).expand(2, 3, 4, 5)
    v, mag, g, gmag = R.tv(y, 1.0)
    assert v == 0 and mag == 0 and not g.any() and not gmag.any()


@pytest.mark.parametrize("shape", [(2, 16, 32), (3, 7, 255)])
def test_bias_grad_is_conv2d_bias_gradient(shape):
    n, c, hw = shape
    b = torch.zeros(c, dtype=torch.float64, requires_grad=True)
    x = t64(n, 1, hw, 1, seed=28)
    wgt = t64(c, 1, 1, 1, seed=29)
    dy = t64(n, c, hw, 1, seed=30)
    F.conv2d(x, wgt, b).backward(dy)
    old = t64(c, seed=31).numpy()
    v, mag = R.bias_grad(dy[..., 0], old=old)
    close(v, b.grad.numpy() + old)
    assert np.all(mag >= np.abs(v))


def test_vec_ops():
    a, b = t64(1027, seed=32), t64(1027, seed=33)
    v, mag = R.vec_reduce(a, b, 0, mul=-0.5, add=2.0, sgn=-1.0)
    close(v, 2.0 + float(a @ b) * 0.5)
    assert mag >= abs(v)
    close(R.vec_reduce(a, None, 1)[0], float(a.abs().sum()))
    assert R.vec_reduce(a, None, 2)[0] == float(a.abs().max())
    assert R.vec_reduce(a[:0], None, 2, add=1.5)[0] == 1.5  # n = 0: out = add
    an = a.clone()
    an[-1] = float("nan")
    assert np.isnan(R.vec_reduce(an, None, 2)[0])
    y = np.full(5, np.nan)
    v, _ = R.axpby(y, a[:5], 2.0, 0.0, a_dev=0.25, a_sgn=-1.0)
    close(v, -0.5 * a[:5].numpy())  # b == 0: y's NaN does not leak
    close(R.axpby(a[:5], None, 7.0, 3.0)[0], 3.0 * a[:5].numpy())
    s = np.array([4.0, -0.5, 3.0, 0.0])
    for op, want in enumerate([-8.0, -2.0, 4.5, 3.5, 0.25, -0.5]):
        out, _ = R.scalar_op(s, op, 0, 1, 3)
        assert out[3] == want and np.array_equal(out[:3], s[:3])
    assert R.scalar_op(s, 4, 0, -1, 0)[0][0] == 0.25  # j = -1, k aliasing i


def test_grad_stats():
    g = t64(4093, seed=34)
    loss, mx, sm = R.grad_stats(g, loss=1.5)
    assert loss == 1.5 and mx == float(g.abs().max())
    close(sm, float(g.abs().sum()))
    g[17] = float("nan")
    _, mx, sm = R.grad_stats(g)
    assert np.isnan(mx) and np.isnan(sm)


def test_adam_steps_chain_to_torch_adam():
    """Three restarted single steps of R.adam equal three steps of one torch.optim.Adam."""
    p0, gs = t64(1001, seed=35), [t64(1001, seed=36 + i, ties=(i == 1)) for i in range(3)]
    pt = p0.clone().requires_grad_()
    opt = torch.optim.Adam([pt], lr=0.01, betas=(0.8, 0.99), eps=1e-6)
    p, m, v = p0.numpy(), np.zeros(1001), np.zeros(1001)
    for t, g in enumerate(gs, 1):
        pt.grad = g.clone()
        opt.step()
        p, m, v = R.adam(p, g, m, v, t, lr=0.01, b1=0.8, b2=0.99, eps=1e-6)
        close(p, pt.detach().numpy())
        close(m, opt.state[pt]["exp_avg"].numpy())
        close(v, opt.state[pt]["exp_avg_sq"].numpy())
