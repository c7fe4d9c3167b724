"""The flow kernels (csrc/flow.hip), the temporal term of the Gatys engines, retarget and the
gatys_video workflow on the GPU, against the fp64 restatement tests/flow_ref.py (pinned by
tests/test_flow_ref_host.py).

Bounds come from the code, not from a run (u = 2^-24, the fp32 unit roundoff; the
conventions of tests/test_streaming_gpu.py):
  selections     bit-equal to the reference
  pointwise      |got - ref| <= (r + 1) u M, r the fp32 roundings of the expression as
                 written (counted at each use), M the magnitude sum of its terms
  reductions     |got - ref| <= (L + 16) u sum|terms|, L the longest serial chain one thread
                 adds for the shape; run twice for equal bits"""
import functools
import os

import numpy as np
import pytest
import torch

import flow_ref as R
from styletransfer_amd import constants, ops
from styletransfer_amd import vgg as V
from styletransfer_amd import weights as W

pytestmark = pytest.mark.gpu
U = 2.0 ** -24

SHAPES = [(1, 5, 7), (2, 64, 64), (1, 129, 67), (1, 96, 160)]  # (n, h, w)
IDS = ["x".join(map(str, s)) for s in SHAPES]


def _np(t):
    return t.detach().cpu().numpy()


def _rand(shape, seed, lo=-1.0, hi=1.0):
    return np.random.default_rng(seed).uniform(lo, hi, shape).astype(np.float32)


def within(got, ref, tol, what):
    got = np.asarray(got, dtype=np.float64)
    err = np.abs(got - ref)
    bad = ~(err <= tol)
    worst = float((err / np.maximum(tol, 1e-300)).max()) if err.size else 0.0
    print(f"{what}: worst error / bound {worst:.3f}")
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} outside, worst {worst:.3f}x"


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def misaligned(t, dev):
    """t's values at a base 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, device=dev, dtype=torch.float32)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


# =============================================================================== warp
WARP_R = 7  # a weight: 1 - fy, 1 - fx, their product (3); the sum: one product, three fmaf (4)


@functools.lru_cache(maxsize=None)
def grid_flows(n, h, w):
    """The recipe's bwd, and a flow of |f| up to the image size, both on the 1/64 grid:
    i + f is exact in fp32."""
    _, small = R.recipe(h, w, n=n)
    big = np.round(_rand((n, 2, h, w), 21, -max(h, w), max(h, w)) * 64) / 64
    return small, big.astype(np.float32)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
@pytest.mark.parametrize("c", [2, 3])
@pytest.mark.parametrize("which", ["recipe", "large"])
def test_warp_on_the_grid(dev, shape, c, which):
    """valid bit-equal; values within (7 + 1) u sum|w_k a_k| (WARP_R); the fill form is the
    select of the warp and the fill on valid; a batch equals its images alone."""
    n, h, w = shape
    flow = grid_flows(n, h, w)[which == "large"]
    a, fill = _rand((n, c, h, w), 22), _rand((n, c, h, w), 23)
    ref, rvalid, mag = R.warp(a, flow, want_mag=True)
    if which == "large":
        assert 0.05 < rvalid.mean() < 0.8, rvalid.mean()  # many samples leave, some stay
    ad, fd, filld = (torch.from_numpy(t).to(dev) for t in (a, flow, fill))
    out, valid = ops.flow_warp(ad, fd, want_valid=True)
    assert np.array_equal(_np(valid), rvalid.astype(np.float32))
    within(_np(out), ref, (WARP_R + 1) * U * mag, "warp")
    assert (_np(out)[~np.broadcast_to(rvalid[:, None], ref.shape)] == 0).all()
    filled = ops.flow_warp(ad, fd, fill=filld)
    assert torch.equal(bits(filled), bits(torch.where(valid[:, None] != 0, out, filld)))
    for b in range(n):
        alone = ops.flow_warp(ad[b:b + 1].contiguous(), fd[b:b + 1].contiguous())
        assert torch.equal(bits(alone), bits(out[b:b + 1]))


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_warp_unrounded_flows(dev, shape):
    """Random fp32 flows: the fp32 coordinate i + f is within delta = 2^-23 max(h, w) of the
    fp64 one.  valid is compared outside a band of 2^-20 max(h, w) around 0 and h-1 / w-1
    (at most 0.5 % of the pixels lie inside); values, where the flags agree, within the
    rounding term plus 2 M (delta_y + delta_x): bilinear sampling is Lipschitz in the
    coordinate with constant 2 M per axis, M = max|a|."""
    n, h, w = shape
    s = max(h, w)
    a = _rand((n, 3, h, w), 31)
    flow = _rand((n, 2, h, w), 32, -0.6 * s, 0.6 * s)
    ref, rvalid, mag = R.warp(a, flow, coord_dtype=np.float64, want_mag=True)
    y, x = R.coords(flow, np.float64)
    band = 2.0 ** -20 * s
    near = (np.abs(y) < band) | (np.abs(y - (h - 1)) < band) | (np.abs(x) < band) | \
        (np.abs(x - (w - 1)) < band)
    assert near.mean() <= 0.005 and 0.1 < rvalid.mean() < 0.9
    out, valid = ops.flow_warp(torch.from_numpy(a).to(dev), torch.from_numpy(flow).to(dev),
                               want_valid=True)
    gvalid = _np(valid) != 0
    assert np.array_equal(gvalid[~near], rvalid[~near])
    delta = 2.0 ** -23 * s
    tol = (WARP_R + 1) * U * mag + 2 * np.abs(a).max() * 2 * delta
    agree = np.broadcast_to((gvalid == rvalid)[:, None], ref.shape)
    within(_np(out)[agree], ref[agree], tol[agree], "warp, unrounded")


def test_warp_reads_no_tap_where_invalid(dev):
    """A NaN at every tap an invalid pixel's clamped index could hit stays out; NaN and
    infinite coordinates are invalid."""
    a = _rand((1, 3, 6, 9), 33)
    a[0, :, 0, 0] = a[0, :, 5, 8] = np.nan
    flow = np.zeros((1, 2, 6, 9), np.float32)
    flow[0, 0, 2, 3], flow[0, 1, 4, 4], flow[0, 0, 1, 1], flow[0, 1, 3, 7] = -50, np.nan, np.inf, 1e30
    ref, rvalid = R.warp(a, flow)
    out, valid = ops.flow_warp(torch.from_numpy(a).to(dev), torch.from_numpy(flow).to(dev),
                               want_valid=True)
    assert rvalid.sum() == 6 * 9 - 4 and np.array_equal(_np(valid) != 0, rvalid)
    got = _np(out)
    assert np.array_equal(got, ref.astype(np.float32), equal_nan=True)  # zero flow: exact
    assert (got[0][:, ~rvalid[0]] == 0).all()
    # a NaN tap reaches the pixels whose cell holds it, under a zero weight too: (0, 0)
    # alone, and the four pixels of the last cell
    assert np.isnan(got).sum() == 3 * 5


# ======================================================================== consistency
def sure(r, allow_nan=False):
    """The pixels whose two reference margins exceed 1e-4: an fp32 evaluation of either side
    makes fewer than 20 roundings (relative error below 1.2e-6), so the decision is the
    reference's.  allow_nan: a NaN margin is a decided comparison (false) as well."""
    mo, mb = r["margin_occluded"], r["margin_boundary"]
    with np.errstate(invalid="ignore"):
        so, sb = mo > 1e-4, mb > 1e-4
    if allow_nan:
        so, sb = so | np.isnan(mo), sb | np.isnan(mb)
    return so & sb


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_consistency_on_the_recipe(dev, shape):
    n, h, w = shape
    fwd, bwd = R.recipe(h, w, n=n)
    r = R.consistency(fwd, bwd)
    ok = sure(r)
    assert (~ok).mean() <= 0.005, (~ok).mean()
    got = _np(ops.flow_consistency(torch.from_numpy(fwd).to(dev), torch.from_numpy(bwd).to(dev)))
    assert set(np.unique(got)) <= {0.0, 1.0}
    assert np.array_equal(got[ok], r["c"][ok].astype(np.float32))
    print(shape, "c share", got.mean(), "excluded", (~ok).mean())


@pytest.mark.parametrize("where", ["fwd", "bwd"])
def test_consistency_nan(dev, where):
    """A NaN in fwd silences the occlusion test of the pixels whose taps read it; one in
    bwd makes its pixel invalid and silences its neighbours' boundary test."""
    h, w = 64, 64
    fwd, bwd = R.recipe(h, w)
    r = R.consistency(fwd, bwd)
    base = r["c"]
    if where == "fwd":  # at the source of a pixel that only the occlusion test switches off
        i, j = np.argwhere(r["occluded"][0] & ~r["boundary"][0])[0]
        y, x = R.coords(bwd)
        fwd[0, :, int(y[0, i, j]), int(x[0, i, j])] = np.nan
    else:
        bwd[0, :, 20:23, 30:33] = np.nan
    r = R.consistency(fwd, bwd)
    assert (r["c"] != base).any()
    if where == "fwd":
        assert r["c"][0, i, j] and not base[0, i, j]
    ok = sure(r, allow_nan=True)
    assert (~ok).mean() <= 0.005
    got = _np(ops.flow_consistency(torch.from_numpy(fwd).to(dev), torch.from_numpy(bwd).to(dev)))
    assert set(np.unique(got)) <= {0.0, 1.0}
    assert np.array_equal(got[ok], r["c"][ok].astype(np.float32))
    if where == "bwd":
        assert (got[0, 20:23, 30:33] == 0).all()


def test_zero_flow_and_translation(dev):
    z = torch.zeros(2, 2, 33, 18, device=dev)
    a = torch.from_numpy(_rand((2, 3, 33, 18), 41)).to(dev)
    out, valid = ops.flow_warp(a, z, want_valid=True)
    assert torch.equal(out, a) and bool((valid == 1).all())
    assert bool((ops.flow_consistency(z, z) == 1).all())
    bwd = torch.zeros(1, 2, 12, 15, device=dev)
    bwd[:, 0], bwd[:, 1] = 2.0, 1.0
    a = a[:1, :, :12, :15].contiguous()
    out, valid = ops.flow_warp(a, bwd, want_valid=True)
    assert torch.equal(out[0, :, :11, :13], a[0, :, 1:, 2:])
    assert bool((valid[0, :11, :13] == 1).all()) and float(valid.sum()) == 11 * 13
    assert torch.equal(ops.flow_consistency(-bwd, bwd), valid)


# ========================================================================= masked_mse
MSE_SHAPES = [(2, 3, 1, 3), (1, 3, 5, 7), (2, 3, 64, 64), (1, 2, 129, 67), (1, 3, 96, 160),
              (1, 3, 512, 512)]
MSE_IDS = ["x".join(map(str, s)) for s in MSE_SHAPES]
THREADS = 512 * 256  # stx_masked_mse: a fixed grid
GRAD_R = 3  # 2 weight / N rounded to fp32, x - ref, their product


def chain(shape, vec):
    """The longest serial chain of one thread's sum: 4 terms per float4 pass, or 1 per pass
    of the scalar loop."""
    total = int(np.prod(shape))
    return 4 * -(-(total // 4) // THREADS) if vec else -(-total // THREADS)


@functools.lru_cache(maxsize=None)
def mse_case(shape):
    n, c, h, w = shape
    x, ref = _rand(shape, 51, -2, 2), _rand(shape, 52, -2, 2)
    mask = (_rand((n, h, w), 53) > -0.4).astype(np.float32)
    return x, ref, mask, R.masked_mse(x, ref, mask, 37.5)


@pytest.mark.parametrize("shape", MSE_SHAPES, ids=MSE_IDS)
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "misaligned"])
def test_masked_mse(dev, shape, aligned):
    """Loss within (L + 16) u sum|terms| and the same bits twice; gradient within (3 + 1) u
    |g| (GRAD_R); accumulated onto a random gradient one rounding more, M = |g0| + |g|;
    add_to receives exactly += out[0].  A misaligned base, or hw % 4 != 0, takes the
    scalar loop: the same bounds with its own L."""
    n, c, h, w = shape
    x, ref, mask, (L_ref, g_ref, mag) = mse_case(shape)
    put = (lambda t: torch.from_numpy(t).to(dev)) if aligned else \
        (lambda t: misaligned(torch.from_numpy(t), dev))
    xd, rd, md = put(x), put(ref), put(mask)
    vec = aligned and (h * w) % 4 == 0
    L = chain(shape, vec)
    if shape[-1] == 512:
        assert L == (8 if vec else 6)  # more elements than one pass of the grid takes
    grad = put(np.zeros(shape, np.float32))
    add_to = torch.full((1,), 3.25, device=dev)
    out = ops.masked_mse(xd, rd, md, 37.5, add_to=add_to, grad=grad)
    again = ops.masked_mse(xd, rd, md, 37.5)
    assert torch.equal(bits(out), bits(again))
    within(_np(out)[0], L_ref, (L + 16) * U * mag, "masked_mse loss")
    assert torch.equal(add_to, torch.full((1,), 3.25, device=dev) + out)
    within(_np(grad), g_ref, (GRAD_R + 1) * U * np.abs(g_ref), "masked_mse grad")
    g0 = _rand(shape, 54, -3, 3)
    acc = put(g0)
    ops.masked_mse(xd, rd, md, 37.5, grad=acc, accumulate=True)
    within(_np(acc), g0.astype(np.float64) + g_ref,
           (GRAD_R + 2) * U * (np.abs(g0) + np.abs(g_ref)), "masked_mse grad, accumulated")
    off = np.broadcast_to(mask[:, None] == 0, shape)
    assert np.array_equal(_np(acc)[off], g0[off]) and (_np(grad)[off] == 0).all()


@pytest.mark.parametrize("shape", [(1, 3, 5, 7), (2, 3, 64, 64)], ids=["1x3x5x7", "2x3x64x64"])
def test_masked_mse_zero_mask_and_nan(dev, shape):
    """An all-zero mask: the loss is exactly 0 and an accumulated gradient keeps its bits (a
    -0 and a NaN included).  A NaN in x and in ref under c = 0 reaches nothing."""
    n, c, h, w = shape
    x, ref, mask, _ = mse_case(shape)
    xd, rd = torch.from_numpy(x).to(dev), torch.from_numpy(ref).to(dev)
    g0 = _rand(shape, 55)
    g0.reshape(-1)[:3] = [-0.0, np.nan, 0.0]
    acc = torch.from_numpy(g0).to(dev)
    add_to = torch.full((1,), -7.5, device=dev)
    out = ops.masked_mse(xd, rd, torch.zeros(n, h, w, device=dev), 37.5, add_to=add_to, grad=acc,
                         accumulate=True)
    assert float(out) == 0.0 and float(add_to) == -7.5
    assert torch.equal(bits(acc), bits(torch.from_numpy(g0).to(dev)))
    off = np.argwhere(mask == 0)
    assert len(off) >= 2
    xn, rn = x.copy(), ref.copy()
    (b0, i0, j0), (b1, i1, j1) = off[0], off[-1]
    xn[b0, :, i0, j0] = np.nan
    rn[b1, 1, i1, j1] = np.inf
    md = torch.from_numpy(mask).to(dev)
    clean_g, dirty_g = torch.empty_like(xd), torch.empty_like(xd)
    clean = ops.masked_mse(xd, rd, md, 37.5, grad=clean_g)
    dirty = ops.masked_mse(torch.from_numpy(xn).to(dev), torch.from_numpy(rn).to(dev), md, 37.5,
                           grad=dirty_g)
    assert torch.equal(bits(clean), bits(dirty)) and torch.equal(bits(clean_g), bits(dirty_g))
    # and under c = 1 it does get through
    md[b0, i0, j0] = 1
    assert bool(torch.isnan(ops.masked_mse(torch.from_numpy(xn).to(dev), rd, md, 37.5)).all())


def test_masked_mse_in_a_graph(dev):
    x, ref, mask, _ = mse_case((2, 3, 64, 64))
    xd, rd, md = (torch.from_numpy(t).to(dev) for t in (x, ref, mask))
    out, grad = torch.zeros(1, device=dev), torch.zeros_like(xd)
    eager = ops.masked_mse(xd, rd, md, 2.0, grad=torch.zeros_like(xd))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with ops.graph_capture(graph):
        ops.masked_mse(xd, rd, md, 2.0, out=out, grad=grad)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


# ============================================================================= engine
VGG_SEED = 1234
H = 64


@pytest.fixture(scope="module")
def feat(dev):
    return V.VGGFeatures(W.vgg19_synthetic(VGG_SEED, 5), dev)


def _img(seed, h=H, w=H):
    return torch.from_numpy(W.synthetic_image(seed, (1, 3, h, w)))


def _temporal(seed, dev, weight=500.0):
    """(ref, mask, weight): a random reference image and a mask with both values."""
    mask = torch.from_numpy((_rand((1, H, H), seed) > -0.5).astype(np.float32))
    return _img(seed + 1).to(dev), mask.to(dev), weight


@pytest.fixture(scope="module")
def frame_a(dev):
    return dict(style=_img(11).to(dev), content=_img(12).to(dev), init=_img(13).to(dev),
                temporal=_temporal(60, dev))


def test_engine_zero_term_changes_nothing(dev, feat, frame_a):
    """(a) an all-zero mask, and weight 0: x after 5 steps equals the engine without."""
    f = frame_a
    want = V.GatysEngine(feat, f["style"], f["content"], init=f["init"]).run(5).clone()
    ref, mask, weight = f["temporal"]
    e0 = V.GatysEngine(feat, f["style"], f["content"], init=f["init"],
                       temporal=(ref, torch.zeros_like(mask), weight))
    assert torch.equal(e0.run(5), want) and float(e0.tloss) == 0.0
    e1 = V.GatysEngine(feat, f["style"], f["content"], init=f["init"], temporal=(ref, mask, 0.0))
    assert torch.equal(e1.run(5), want)
    e2 = V.GatysEngine(feat, f["style"], f["content"], init=f["init"], temporal=f["temporal"])
    assert not torch.equal(e2.run(5), want)


@pytest.fixture(scope="module")
def one_iteration(dev, feat, frame_a):
    """One eager iteration with and without the term from the same x: (without, with)."""
    f = frame_a
    e0 = V.GatysEngine(feat, f["style"], f["content"], init=f["init"])
    e1 = V.GatysEngine(feat, f["style"], f["content"], init=f["init"], temporal=f["temporal"])
    e0._iteration()
    e1._iteration()
    torch.cuda.synchronize()
    return e0, e1


def _check_term(e0, e1, frame_a):
    """grad(with) - grad(without) = 2 gamma / (3 hw) c (x - omega) within the accumulate
    bound; total(with) - total(without) = the term within one rounding of total."""
    ref, mask, weight = frame_a["temporal"]
    L_ref, g_ref, mag = R.masked_mse(_np(frame_a["init"]), _np(ref), _np(mask), weight)
    g0 = _np(e0.grad).astype(np.float64)
    assert np.abs(g_ref).max() > 0
    within(_np(e1.grad), g0 + g_ref, (GRAD_R + 2) * U * (np.abs(g0) + np.abs(g_ref)),
           "engine gradient with the term")
    within(float(e1.tloss), L_ref, (chain((1, 3, H, H), True) + 16) * U * mag, "engine term")
    t0, t1, tl = float(e0.total), float(e1.total), float(e1.tloss)
    assert tl > 0 and abs(t1 - (t0 + tl)) <= U * abs(t1)
    assert float(e1.total) == float(e0.total + e1.tloss[0])


def test_engine_term_is_the_reference(dev, one_iteration, frame_a):
    """(b) at one fixed x (the init: the gradient of an iteration is taken before its Adam
    step), an engine with the term against one without."""
    _check_term(*one_iteration, frame_a)


def test_engine_eager_equals_replay(dev, feat, frame_a):
    """(c) 3 eager steps = 1 eager step + 2 replays, bit for bit."""
    f = frame_a
    kw = dict(init=f["init"], temporal=f["temporal"])
    a = V.GatysEngine(feat, f["style"], f["content"], **kw).run(3, graph=False)
    e = V.GatysEngine(feat, f["style"], f["content"], **kw)
    b = e.run(3)
    assert e.graph is not None and torch.equal(a, b)


def test_engine_retarget_equals_a_fresh_engine(dev, feat, frame_a):
    """(d) 3 steps on frame A, retarget to frame B, 3 replays = a fresh engine on B."""
    f = frame_a
    content_b, init_b = _img(14).to(dev), _img(15).to(dev)
    ref_b, mask_b, weight = _temporal(70, dev)
    mine = [t.clone() for t in (f["content"], f["init"], content_b, init_b, ref_b, mask_b)]
    e = V.GatysEngine(feat, f["style"], f["content"], init=f["init"], temporal=f["temporal"])
    e.run(3)
    graph = e.graph
    e.retarget(content_b, init=init_b, temporal_ref=ref_b, temporal_mask=mask_b)
    assert e.graph is graph
    for _ in range(3):
        e.step()
    fresh = V.GatysEngine(feat, f["style"], content_b, init=init_b,
                          temporal=(ref_b, mask_b, weight))
    assert torch.equal(e.x, fresh.run(3))
    assert torch.equal(e.c4, fresh.c4) and torch.equal(e.total, fresh.total)
    # without init: from the content; an engine without the term refuses temporal inputs
    e.retarget(f["content"])
    assert torch.equal(e.x, f["content"]) and torch.equal(e.temporal[0], ref_b)
    # the engine writes to none of the caller's tensors (it holds the content by reference)
    for kept, now in zip(mine, (f["content"], f["init"], content_b, init_b, ref_b, mask_b)):
        assert torch.equal(kept, now)
    with pytest.raises(ValueError, match="without a temporal term"):
        V.GatysEngine(feat, f["style"], f["content"]).retarget(content_b, temporal_ref=ref_b)


def test_lbfgs_closure_has_the_same_term(dev, feat, frame_a):
    """(e) GatysLBFGS with temporal: at the same x, (b)'s relations between the closure with
    the term and the one without, and the Adam engine's total and gradient bit for bit."""
    f = frame_a
    kw = dict(init=f["init"])
    lb0 = V.GatysLBFGS(feat, f["style"], f["content"], **kw)
    lb1 = V.GatysLBFGS(feat, f["style"], f["content"], temporal=f["temporal"], **kw)
    adam = V.GatysEngine(feat, f["style"], f["content"], temporal=f["temporal"], **kw)
    assert lb0.temporal is None and lb0.tloss is None
    lb0._closure()
    lb1._closure()
    adam._iteration()
    torch.cuda.synchronize()
    _check_term(lb0, lb1, frame_a)
    assert torch.equal(lb1.grad, adam.grad) and torch.equal(lb1.total, adam.total)
    assert torch.equal(lb1.tloss, adam.tloss)


# =========================================================================== workflow
T, DX, DY = 4, 2, 1


def clip_frames():
    """4 frames 64 x 64: one seeded texture seen through a window that moves by (2, 1) px
    (columns, rows) per frame; frame t (i, j) = texture (i + t, j + 2 t)."""
    tex = W.synthetic_image(81, (1, 3, H + DY * T, H + DX * T))
    return [torch.from_numpy(np.ascontiguousarray(tex[:, :, DY * t:DY * t + H, DX * t:DX * t + H]))
            for t in range(T)]


def clip_flows():
    """Exact flows: pixel (i, j) of frame t came from (i + 1, j + 2) of frame t-1."""
    bwd = np.zeros((T - 1, 2, H, H), np.float32)
    bwd[:, 0], bwd[:, 1] = DX, DY
    return -bwd, bwd


def test_clip_is_what_its_flows_say():
    frames, (fwd, bwd) = clip_frames(), clip_flows()
    for t in range(1, T):
        om, valid = R.warp(frames[t - 1].numpy(), bwd[t - 1:t])
        v = np.broadcast_to(valid[:, None], om.shape)
        assert np.array_equal(om[v], frames[t].numpy().astype(np.float64)[v])
        assert R.temporal_error(frames[t].numpy(), frames[t - 1].numpy(), fwd[t - 1:t],
                                bwd[t - 1:t]) == 0.0


def test_workflow_temporal_weight_lowers_the_temporal_error(dev, feat):
    """For every t >= 1 the masked temporal error sum c (y_t - W(y_{t-1}, bwd_t))^2 / sum c
    of a run with a large temporal weight is below that of the run with weight 0."""
    from styletransfer_amd import video
    frames, flows = clip_frames(), clip_flows()
    style = _img(11)

    def run(tw):
        ys = [_np(y) for y in video.gatys_video(feat, frames, style, flows, steps=20,
                                                temporal_weight=tw)]
        assert len(ys) == T and all(np.isfinite(y).all() for y in ys)
        return ys, [R.temporal_error(ys[t], ys[t - 1], flows[0][t - 1:t], flows[1][t - 1:t])
                    for t in range(1, T)]

    y0, e0 = run(0.0)
    y1, e1 = run(1e7)
    print("temporal error, weight 0:", e0, "weight 1e7:", e1)
    assert np.array_equal(y0[0], y1[0])  # frame 0: the term is exactly 0
    for t in range(T - 1):
        assert e1[t] < e0[t], (t + 1, e1[t], e0[t])


@pytest.mark.parametrize("flow", ["flows.npz", "static"])
def test_cli_writes_the_frames(dev, tmp_path, monkeypatch, flow):
    from click.testing import CliRunner
    from PIL import Image
    from conftest import REPO
    from styletransfer_amd.clis import cli
    monkeypatch.setattr(constants, "PROJECT_ROOT_PATH", str(tmp_path))
    monkeypatch.setattr(constants, "IMSIZE", H)
    monkeypatch.chdir(tmp_path)
    mean = np.array(constants.IMAGENET_MEAN, np.float32).reshape(1, 3, 1, 1)
    std = np.array(constants.IMAGENET_STD, np.float32).reshape(1, 3, 1, 1)
    clip = np.concatenate([np.clip((f.numpy() * std + mean) * 255, 0, 255) for f in clip_frames()])
    np.save(tmp_path / "clip.npy", np.ascontiguousarray(clip.transpose(0, 2, 3, 1)).astype(np.uint8))
    fwd, bwd = clip_flows()
    np.savez(tmp_path / "flows.npz", forward=fwd, backward=bwd)
    Image.open(os.path.join(REPO, "data", "styles", "picasso.jpg")).save(tmp_path / "style.jpg")
    r = CliRunner().invoke(cli, ["gatys_video", "clip.npy", "style.jpg", "--flow", flow, "-s", "3",
                                 "--first-steps", "4", "-tw", "100", "-o", "out"])
    assert r.exit_code == 0, r.output + repr(r.exception)
    assert sorted(os.listdir(tmp_path / "out")) == [f"{i}.png" for i in range(T)]
    imgs = [np.asarray(Image.open(tmp_path / "out" / f"{i}.png")) for i in range(T)]
    assert all(im.shape == (H, H, 3) for im in imgs)
    assert not np.array_equal(imgs[0], imgs[1])
