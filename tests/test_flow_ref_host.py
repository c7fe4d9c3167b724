"""Pins tests/flow_ref.py, the fp64 yardstick of the flow kernels, without a GPU: against
torch's grid_sample and fp64 autograd, on cases with a known answer, and on the shares of
the mask tests' flow recipe."""
import numpy as np
import pytest
import torch

import flow_ref as R

SIZES = [(64, 64), (129, 67), (96, 160)]


def _rand(shape, seed, lo=-1.0, hi=1.0):
    return np.random.default_rng(seed).uniform(lo, hi, shape)


@pytest.mark.parametrize("shape", [(1, 3, 5, 7), (2, 2, 33, 18), (1, 3, 64, 64)])
def test_warp_is_grid_sample_align_corners(shape):
    """At every valid pixel, to 1e-12 relative to max|a| (grid_sample takes normalised
    coordinates and un-normalises them: a few fp64 ulp of max(h, w) on the coordinate, times
    the Lipschitz constant 2 max|a| per axis -- below 1e-13 max|a| at these sizes)."""
    n, c, h, w = shape
    a = _rand(shape, 1)
    flow = _rand((n, 2, h, w), 2, -0.6 * max(h, w), 0.6 * max(h, w))
    out, valid, mag = R.warp(a, flow, coord_dtype=np.float64, want_mag=True)
    y, x = R.coords(flow, np.float64)
    grid = torch.from_numpy(np.stack([2 * x / (w - 1) - 1, 2 * y / (h - 1) - 1], axis=-1))
    ref = torch.nn.functional.grid_sample(torch.from_numpy(a), grid, mode="bilinear",
                                          padding_mode="zeros", align_corners=True).numpy()
    assert 0.1 < valid.mean() < 0.9
    v = np.broadcast_to(valid[:, None], shape)
    err = np.abs(out - ref)[v].max()
    print(shape, "max error", err)
    assert err <= 1e-12 * np.abs(a).max(), err
    assert (mag[v] >= np.abs(out[v])).all()
    assert (out[~v] == 0).all()


def test_warp_fill_and_no_tap_read_where_invalid():
    a = _rand((1, 3, 6, 9), 3)
    a[0, :, 0, 0] = np.nan  # the tap an invalid pixel's clamped index would hit
    flow = np.zeros((1, 2, 6, 9))
    flow[0, 0, 2, 3] = -50.0
    flow[0, 1, 4, 4] = np.nan
    fill = _rand((1, 3, 6, 9), 4)
    out, valid = R.warp(a, flow, fill=fill)
    assert not valid[0, 2, 3] and not valid[0, 4, 4] and valid.sum() == 6 * 9 - 2
    assert (out[0, :, 2, 3] == fill[0, :, 2, 3]).all() and (out[0, :, 4, 4] == fill[0, :, 4, 4]).all()
    out0, _ = R.warp(a, flow)
    assert (out0[0, :, 2, 3] == 0).all() and (out0[0, :, 4, 4] == 0).all()


@pytest.mark.parametrize("shape", [(1, 3, 5, 7), (2, 3, 16, 12)])
def test_masked_mse_gradient_is_autograd(shape):
    n, c, h, w = shape
    x, ref = _rand(shape, 5), _rand(shape, 6)
    mask = (_rand((n, h, w), 7) > 0).astype(np.float64)
    L, g, mag = R.masked_mse(x, ref, mask, 3.5)
    xt = torch.from_numpy(x).requires_grad_()
    Lt = 3.5 / xt.numel() * (torch.from_numpy(mask)[:, None] * (xt - torch.from_numpy(ref)) ** 2).sum()
    Lt.backward()
    assert abs(L - float(Lt.detach())) <= 1e-14 * mag and mag == L
    assert np.abs(g - xt.grad.numpy()).max() <= 1e-15 * np.abs(g).max()
    assert (g[np.broadcast_to(mask[:, None] == 0, shape)] == 0).all()


def test_masked_mse_selects():
    """A NaN under a zero mask reaches neither the loss nor the gradient."""
    x, ref = _rand((1, 3, 4, 4), 8), _rand((1, 3, 4, 4), 9)
    mask = np.ones((1, 4, 4))
    mask[0, 1, 2] = 0
    L0, g0, _ = R.masked_mse(x, ref, mask, 2.0)
    x[0, 1, 1, 2] = np.nan
    L1, g1, _ = R.masked_mse(x, ref, mask, 2.0)
    assert L0 == L1 and np.array_equal(g0, g1)


@pytest.mark.parametrize("hw", SIZES + [(5, 7)])
def test_zero_flow_is_identity(hw):
    h, w = hw
    a = _rand((2, 3, h, w), 10)
    z = np.zeros((2, 2, h, w), np.float32)
    out, valid = R.warp(a, z)
    assert np.array_equal(out, a) and valid.all()
    assert R.consistency(z, z)["c"].all()


def test_integer_translation():
    """(dx, dy) = (2, 1): out[i, j] = a[i + 1, j + 2]; invalid only in the last row and the
    last two columns (the entering borders); with fwd = -bwd, c = valid."""
    h, w = 12, 15
    a = _rand((1, 3, h, w), 11)
    bwd = np.zeros((1, 2, h, w), np.float32)
    bwd[:, 0], bwd[:, 1] = 2.0, 1.0
    out, valid = R.warp(a, bwd)
    want = np.zeros((h, w), bool)
    want[:h - 1, :w - 2] = True
    assert np.array_equal(valid[0], want)
    assert np.array_equal(out[0, :, :h - 1, :w - 2], a[0, :, 1:, 2:])
    assert (out[0][:, ~want] == 0).all()
    r = R.consistency(-bwd, bwd)
    assert np.array_equal(r["c"], valid) and not r["occluded"].any() and not r["boundary"].any()


def test_hand_built_occlusion_and_boundary():
    """8 x 8, zero flows but for two values.
    fwd[dx] = 1 at (2, 2): that pixel's round trip does not close, |w~ + w^|^2 = 1 >
    0.01 * 1 + 0.5: occluded; bwd is untouched there, so no gradient moves.
    bwd[dy] = 0.08 at (0, 0): a corner's differences are one-sided and unhalved on both
    axes, |grad v|^2 = 2 * 0.0064 > 0.01 * 0.0064 + 0.002: boundary.  Its neighbours (0, 1)
    and (1, 0) see the halved central difference 0.04: 0.0016 < 0.002, no boundary.  The
    corner stays valid (y = 0.08) and unoccluded (0.0064 < 0.5)."""
    fwd = np.zeros((1, 2, 8, 8), np.float32)
    bwd = np.zeros((1, 2, 8, 8), np.float32)
    fwd[0, 0, 2, 2] = 1.0
    bwd[0, 1, 0, 0] = 0.08
    r = R.consistency(fwd, bwd)
    occ = np.zeros((8, 8), bool)
    occ[2, 2] = True
    bnd = np.zeros((8, 8), bool)
    bnd[0, 0] = True
    assert r["valid"].all()
    assert np.array_equal(r["occluded"][0], occ)
    assert np.array_equal(r["boundary"][0], bnd)
    assert np.array_equal(r["c"][0], ~(occ | bnd))


def test_nan_silences_a_comparison():
    """A NaN in fwd: the occlusion test of the pixels whose taps read it is false (c follows
    valid and boundary).  A NaN in bwd: that pixel is invalid; its neighbours' boundary
    test is false."""
    fwd = np.zeros((1, 2, 8, 8), np.float32)
    bwd = np.zeros((1, 2, 8, 8), np.float32)
    fwd[0, 0, 3, 3] = np.nan
    r = R.consistency(fwd, bwd)
    assert r["c"].all()  # zero flow: the tap (3, 3) has weight 1 at (3, 3); NaN > x is false
    fwd[0, 0, 3, 3] = 0
    bwd[0, 1, 4, 4] = np.nan
    r = R.consistency(fwd, bwd)
    want = np.ones((8, 8), bool)
    want[4, 4] = False
    assert np.array_equal(r["c"][0], want) and not r["valid"][0, 4, 4]


@pytest.mark.parametrize("hw", SIZES)
def test_recipe_shares(hw):
    """Every class holds at least 1 % of the pixels; at most 0.5 % lie within a relative
    margin of 1e-4 of either threshold; the flows sit on the 1/64 grid."""
    h, w = hw
    fwd, bwd = R.recipe(h, w)
    assert fwd.dtype == bwd.dtype == np.float32 and fwd.shape == bwd.shape == (1, 2, h, w)
    for f in (fwd, bwd):
        assert np.array_equal(f * 64, np.round(f * 64))
    r = R.consistency(fwd, bwd)
    shares = dict(c=r["c"].mean(), invalid=(~r["valid"]).mean(), occluded=r["occluded"].mean(),
                  boundary=r["boundary"].mean())
    print(hw, shares)
    for k, v in shares.items():
        assert v >= 0.01, (k, v)
    near = (r["margin_occluded"] < 1e-4) | (r["margin_boundary"] < 1e-4)
    assert near.mean() <= 0.005, near.mean()
    # exact coordinates: fp32 and fp64 coordinates agree
    assert np.array_equal(R.coords(bwd, np.float32), R.coords(bwd, np.float64))
