"""The HBM-bound kernels (elementwise.hip, vec.hip, the gradient-stats pair of lbfgs.hip,
stx_loss_finalize of gram.hip) against the fp64 references of tests/stream_ref.py, element
by element, at the sizes where their code changes path: scalar tails, more partials than
one finalize pass, grid caps, odd planes, unaligned bases.

Bounds come from the code, not from a run (u = 2^-24, the fp32 unit roundoff):
  selection kernels   bit-equal to the fp32 cast of the reference
  pointwise           |got - ref| <= (r + 1) u M, r the fp32 roundings of the header's
                      expression (stated at each use), M the magnitude sum of its terms
  reductions          |got - ref| <= (L + 16) u sum|terms|, L the longest serial chain one
                      thread adds for the shape (the chain_* helpers restate the kernels'
                      loop structure); never looser than 2^-16 sum|terms|; each reduction
                      runs twice and must give the same bits
NaN is ordinary data here: the last section pins where it must come out and where not."""
import functools

import numpy as np
import pytest
import torch

import stream_ref as R
from styletransfer_amd import _native as N
from styletransfer_amd import ops

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
CAP = 2.0 ** -16
NAN = float("nan")


def cdiv(a, b):
    return -(-a // b)


def data(*shape, seed, ties=False):
    """Signed, seeded; several elements exactly 0 and several pairs exactly equal."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(*shape, generator=g) * 2 - 1
    if ties:  # few distinct values: most neighbours tie
        x = torch.round(x * 2) / 2
    f = x.view(-1)
    f[5::53] = 0.0
    f[7::61] = f[6::61][:f[7::61].numel()]
    return x


def within(got, ref, bound, what):
    got = got.detach().cpu().double().numpy().reshape(np.shape(ref))
    err = np.abs(got - np.asarray(ref, dtype=np.float64))
    bad = ~(err <= bound)  # a NaN fails
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} beyond the bound; worst "
                           f"error {np.nanmax(err):.3e} at {int(np.nanargmax(err - bound))}, "
                           f"bound there {np.ravel(bound)[int(np.nanargmax(err - bound))]:.3e}")


def pointwise(got, ref, mag, r, what):
    within(got, ref, (r + 1) * U * np.asarray(mag, dtype=np.float64), what)


def reduction(got, ref, mag, L, what):
    assert (L + 16) * U <= CAP, (what, L)
    within(got, ref, (L + 16) * U * np.asarray(mag, dtype=np.float64), what)


def exact(got, ref, what=""):
    """Bit-equal to the fp32 cast of the reference (NaN matches NaN)."""
    g = got.detach().cpu().reshape(-1)
    w = torch.from_numpy(np.ascontiguousarray(ref)).to(torch.float32).reshape(-1)
    assert g.numel() == w.numel(), what
    gn, wn = torch.isnan(g), torch.isnan(w)
    assert torch.equal(gn, wn), f"{what}: NaN positions differ"
    assert torch.equal(g[~gn].view(torch.int32), w[~wn].view(torch.int32)), \
        f"{what}: {int((g[~gn] != w[~wn]).sum())} elements differ"


def twice(fn):
    a, b = fn().clone(), fn().clone()
    assert torch.equal(a, b), "not bit-reproducible run to run"
    return a


def with_tail(t, tail, dev):
    """t at the front of a longer device buffer that continues with `tail`: what a kernel
    would find if it read past the end of t, under this test's control."""
    return torch.cat([t.reshape(-1), tail.to(t.dtype)]).to(dev)


def refused(match):
    return pytest.raises(N.NativeError, match=match)


# ======================================================================= stx_mse
MSE_N = [1, 3, 4, 2049, 600_001, 2_097_152 + 1029]


def red_blocks(n):  # elementwise.hip: one block per 2048 elements, at most 1024
    return max(1, min(cdiv(n, 2048), 1024))


def chain_mse(n):  # sqdiff_partial_kernel: grid-stride, one term per pass
    return cdiv(n, red_blocks(n) * 256)


def chain_mse2(n):  # sqdiff2_partial_kernel: 4 terms per float4 pass + one tail term
    return 4 * cdiv(n // 4, red_blocks(n) * 256) + (1 if n % 4 else 0)


def square_over_n(L, ref):
    """Bound of mean^2 / n given mean within (L + 16) u mean: twice that relative error
    plus the two roundings of the square and the quotient."""
    k = 2 * (L + 16) + 2
    assert k * U <= CAP
    return k * U * np.asarray(ref)


@functools.lru_cache(maxsize=None)
def mse_pair(n):
    return data(n, seed=100 + n % 97), data(n, seed=200 + n % 97)


@functools.lru_cache(maxsize=None)
def mse_ref(n):
    a, b = mse_pair(n)
    return {(m, r): R.mse(a, b, m, relu_inputs=r)
            for m, r in ((0, False), (0, True), (1, False), (1, True), (2, False))}


@pytest.mark.parametrize("n", MSE_N)
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_mse(dev, n, mode):
    """n = 3 / 2049 / 600 001 / 2 098 181: mode-2 scalar tail of 3 / 1 / 1 / 1 elements;
    600 001: 293 partials, the finalize's strided loop; 2 098 181: above the 1024-block cap
    (9 passes).  The terms are non-negative, so sum|terms| is the value itself."""
    a, b = (t.to(dev) for t in mse_pair(n))
    L = chain_mse(n)
    if mode == 0:
        for relu in (False, True):  # relu: mode 0 with relu_inputs
            ref = mse_ref(n)[(0, relu)]
            got = twice(lambda: ops.mse(a, b, relu=relu, mode=0))
            reduction(got, ref, ref, L, f"mse mode 0 relu={relu}")
        return
    if mode == 1:
        for relu in (False, True):
            ref = mse_ref(n)[(1, relu)]
            got = twice(lambda: ops.mse(a, b, relu=relu, mode=1))
            reduction(got[1:], ref[1:], ref[1:], L, "mse mode 1 mean")
            within(got[:1], ref[:1], square_over_n(L, ref[:1]), "mse mode 1 mean^2/n")
        return
    L2 = chain_mse2(n)
    ref = mse_ref(n)[(2, False)]
    got = twice(lambda: ops.mse(a, b, mode=2))
    reduction(got[[0, 2]], ref[[0, 2]], ref[[0, 2]], L2, "mse mode 2 means")
    within(got[1:2], ref[1:2], square_over_n(L2, ref[1:2]), "mse mode 2 mean^2/n")
    # mode 2 = mode 0 and the relu'd mode 1 of the same inputs, each within its own bound
    m0 = ops.mse(a, b, mode=0)
    m1 = ops.mse(a, b, relu=True, mode=1)
    both = (L + 16) + (L2 + 16)
    within(got[:1], m0.double().cpu().numpy(), both * U * ref[:1], "mode 2 vs mode 0")
    within(got[2:], m1[1:].double().cpu().numpy(), both * U * ref[2:], "mode 2 vs mode 1 mean")
    within(got[1:2], m1[:1].double().cpu().numpy(),
           square_over_n(L, ref[1:2]) + square_over_n(L2, ref[1:2]), "mode 2 vs mode 1")


@pytest.mark.parametrize("n", MSE_N)
def test_mse_grad(dev, n):
    """Mode 0 with grad and gscale != 1.  r = 3: the host's (float)(gscale 2 / n), a - b,
    their product."""
    a, b = (t.to(dev) for t in mse_pair(n))
    grad = torch.full((n,), NAN, device=dev)
    out = ops.mse(a, b, mode=0, grad=grad, gscale=-3.5)
    ref, mag = R.mse_grad(*mse_pair(n), -3.5)
    pointwise(grad, ref, mag, 3, "mse grad")
    assert torch.equal(out, ops.mse(a, b, mode=0))  # the loss does not depend on grad


def test_mse_refusals(dev):
    buf = torch.zeros(65, device=dev)
    a, b = buf[:64], torch.zeros(64, device=dev)
    with refused("aligned"):  # mode 2 reads float4
        ops.mse(buf[1:], b, mode=2)
    with refused("aligned"):
        ops.mse(b, buf[1:], mode=2)
    for mode in (1, 2):
        with refused("invalid"):  # grad is mode 0's
            ops.mse(a, b, mode=mode, grad=torch.zeros(64, device=dev))


# ======================================================================= stx_diff_scale
@functools.lru_cache(maxsize=None)
def ds_inputs(n):
    a, b, old = data(n, seed=301), data(n, seed=302), data(n, seed=303)
    i = torch.arange(n)
    a[i % 10 == 0] = 0.0                                   # x > 0 fails at exactly 0
    a[i % 10 == 5] = -a[i % 10 == 5].abs() - 0.125         # ... and below
    b[i % 5 == 0] = b[i % 5 == 0].abs() + 0.25             # relu(a) - relu(b) != 0 there
    return a, b, old


@pytest.mark.parametrize("n", [1, 255, 257, 2_097_152 + 257])
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("sdev", [0, 1])
def test_diff_scale(dev, n, relu, acc, sdev):
    """2 097 409 is above the 8192 x 256 grid: a second grid-stride pass.  r = 2 (a - b,
    times the scale; the mask is exact) + 2 with s1 / s2 (s0 s1, then s2) + 1 with
    accumulate."""
    a, b, old = ds_inputs(n)
    s1 = torch.tensor(-0.3, device=dev) if sdev else None
    s2 = torch.tensor(2.5, device=dev) if sdev else None
    out = old.to(dev) if acc else torch.full((n,), NAN, device=dev)
    ops.diff_scale(a.to(dev), b.to(dev), 1.75, s1, s2, relu=bool(relu), out=out,
                   accumulate=bool(acc))
    ref, mag = R.diff_scale(a, b, 1.75, None if s1 is None else float(s1),
                            None if s2 is None else float(s2), relu_inputs=bool(relu),
                            old=old if acc else None)
    pointwise(out, ref, mag, 2 + 2 * sdev + acc, "diff_scale")


# ======================================================================= loss combine / finalize
@pytest.mark.parametrize("k", [1, 5, 16])
def test_loss_combine(dev, k):
    """One thread's chain of k products: L = k."""
    s = data(16, seed=310)
    w = [(-1) ** i * (0.5 + i) for i in range(k)]
    out = torch.full((1,), NAN, device=dev)
    got = twice(lambda: ops.loss_combine(s.to(dev), w, out))
    ref, mag = R.loss_combine(s, w)
    reduction(got, [ref], [mag], k, "loss_combine")


@pytest.mark.parametrize("k", [0, 17])
def test_loss_combine_refuses(dev, k):
    with refused("out of range"):
        ops.loss_combine(torch.zeros(32, device=dev), [1.0] * k, torch.zeros(1, device=dev))


FIN_PARTS = {1: [255], 5: [63, 256, 449, 1000, 1], 8: [1, 63, 64, 65, 255, 256, 449, 1000]}


def chain_parts(n):  # wave_sum_parts: s0 takes every unrolled pass and up to 3 remainders
    return n // 256 + 3


@pytest.mark.parametrize("k", [1, 5, 8])
@pytest.mark.parametrize("m", [0, 3])
@pytest.mark.parametrize("with_total", [False, True])
def test_loss_finalize(dev, k, m, with_total):
    """nparts 63 / 64 / 65 and 255 / 256 / 449 / 1000 sit on both sides of the i + 192 < n
    split of wave_sum_parts (remainder only; exactly one unrolled pass; unrolled + 1 ...)."""
    sizes = FIN_PARTS[k]
    parts = [data(n, seed=320 + n) for n in sizes]
    inv = [1.0 / (3 + i) for i in range(k)]
    inv32 = [float(np.float32(v)) for v in inv]
    extra = data(4, seed=330)[:m]
    w = [(-1) ** i * (1.0 + 0.5 * i) for i in range(k + m)]
    dparts = [p.to(dev) for p in parts]
    dextra = extra.to(dev) if m else None

    def run():
        losses = torch.full((10,), 77.0, device=dev)
        total = torch.full((1,), NAN, device=dev) if with_total else None
        ops.loss_finalize([(p.data_ptr(), p.numel(), iv) for p, iv in zip(dparts, inv)],
                          losses, dextra, w if with_total else None, total)
        return torch.cat([losses, total]) if with_total else losses

    got = twice(run)
    losses, mags, tot, tmag = R.loss_finalize(parts, inv32, extra, w if with_total else None)
    assert torch.all(got[k:10] == 77.0)  # only k losses written
    for i, n in enumerate(sizes):
        reduction(got[i:i + 1], losses[i:i + 1], mags[i:i + 1], chain_parts(n),
                  f"loss {i} ({n} parts)")
    if with_total:
        # one reduction over the terms w_i inv_i parts_i[j] and w_(k+j) extra_j: a term
        # passes its list's chain, then thread 0's chain of k + m
        full = sum(abs(w[i]) * mags[i] for i in range(k)) + tmag - sum(
            abs(w[i] * losses[i]) for i in range(k))
        reduction(got[10:], [tot], [full], max(map(chain_parts, sizes)) + k + m, "total")


def test_loss_finalize_refuses_17_terms(dev):
    p = torch.zeros(8, device=dev)
    with refused("invalid"):
        ops.loss_finalize([(p.data_ptr(), 8, 1.0)] * 8, torch.zeros(8, device=dev),
                          torch.zeros(9, device=dev), [1.0] * 17, torch.zeros(1, device=dev))


# ======================================================================= max-pool family
POOL_PLANES = [(3, 2, 2), (5, 7, 9), (4, 10, 14), (2, 1, 8), (3, 9, 2), (130, 128, 128)]


@functools.lru_cache(maxsize=None)
def pool_x(plane):
    """Plane 0 starts with a window of four equal values, plane 1 with one of all
    negatives (four-way tie at 0 under ReLU), plane 2 (where there is one) with -inf."""
    nc, h, w = plane
    x = data(nc, h, w, seed=340 + h, ties=True)
    if h >= 2 and w >= 2:
        x[0, :2, :2] = 0.5
        x[1, :2, :2] = torch.tensor([[-0.25, -1.0], [-0.5, -0.75]])
        x[2, :2, :2] = float("-inf")
    return x


@functools.lru_cache(maxsize=None)
def pool_ref(plane, relu):
    return R.maxpool_fwd(pool_x(plane), relu_input=bool(relu))


@pytest.mark.parametrize("plane", POOL_PLANES)
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("want_idx", [True, False])
def test_maxpool_fwd(dev, plane, relu, want_idx):
    """Odd h / w (floor mode), ties, -inf, idx == NULL; (2, 1, 8) has no output row: the
    refused-empty case."""
    nc, h, w = plane
    x = pool_x(plane).to(dev)[None]
    if h // 2 == 0:
        with refused("empty"):
            ops.maxpool2x2(x, relu_input=bool(relu), want_idx=want_idx)
        return
    y, idx = ops.maxpool2x2(x, relu_input=bool(relu), want_idx=want_idx)
    ry, ridx = pool_ref(plane, relu)
    exact(y, ry, "maxpool values")
    if want_idx:
        assert torch.equal(idx[0].cpu(), torch.from_numpy(ridx))


def pool_bwd(dev, dy, idx, nc, h, w):
    """stx_maxpool2x2_bwd with dy and idx followed in memory by 7.0 and by the flat indices
    of the odd trailing row: a read past their end would show up as 7.0 there."""
    dyb = with_tail(dy.cpu(), torch.full((64,), 7.0), dev)
    idxb = with_tail(idx.cpu(), 2 * (h // 2) * w + 2 * torch.arange(64), dev)
    dx = torch.full((nc, h, w), NAN, device=dev)
    N.check(N.lib().stx_maxpool2x2_bwd(dyb.data_ptr(), idxb.data_ptr(), dx.data_ptr(), nc, h, w,
                                       ops._stream()), "stx_maxpool2x2_bwd")
    return dx


@pytest.mark.parametrize("plane", POOL_PLANES)
def test_maxpool_bwd(dev, plane):
    """Every element outside an argmax, and the odd trailing row / column, gets exactly 0.
    (130, 128, 128): 2.13 M inputs, a second pass over the 8192 x 256 grid.  dy and idx are
    followed in memory by values under which a read past their end (the trailing row of the
    last plane looks one window row too far) would pick up 7.0; it must not show."""
    nc, h, w = plane
    ho, wo = h // 2, w // 2
    idx = torch.from_numpy(pool_ref(plane, 0)[1])
    dy = data(nc, ho, wo, seed=350)
    dx = pool_bwd(dev, dy, idx, nc, h, w)
    exact(dx, R.maxpool_bwd(dy, idx.numpy(), h, w), "maxpool bwd")
    assert not dx[:, 2 * ho:, :].any() and not dx[:, :, 2 * wo:].any()


@pytest.mark.parametrize("plane", POOL_PLANES)
def test_relupool_bwd(dev, plane):
    """Against the reference, and bit for bit maxpool2x2_bwd(idx of the relu'd forward)
    * (z > 0)."""
    nc, h, w = plane
    ho, wo = h // 2, w // 2
    z = pool_x(plane)
    dp = data(nc, ho, wo, seed=351)
    dpb = with_tail(dp, torch.full((64,), 7.0), dev)
    zd = z.to(dev)
    dz = torch.full((nc, h, w), NAN, device=dev)
    N.check(N.lib().stx_relupool_bwd(dpb.data_ptr(), zd.data_ptr(), dz.data_ptr(), nc, h, w,
                                     ops._stream()), "stx_relupool_bwd")
    exact(dz, R.relupool_bwd(dp, z), "relupool bwd")
    assert not dz[:, 2 * ho:, :].any() and not dz[:, :, 2 * wo:].any()
    if ho:
        _, idx = ops.maxpool2x2(zd[None], relu_input=True)
        dx = pool_bwd(dev, dp, idx[0], nc, h, w)
        want = torch.where(zd > 0, dx, torch.zeros_like(dx))
        assert torch.equal(dz.view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("n", [1, 257, 2_097_152 + 257])
def test_relu(dev, n):
    x, dy = data(n, seed=360, ties=True), data(n, seed=361)
    y = ops.relu(x.to(dev))
    exact(y, R.relu(x), "relu fwd")
    exact(ops.relu_bwd(dy.to(dev), y), R.relu_bwd(dy, R.relu(x)), "relu bwd")


# ======================================================================= upsample
@pytest.mark.parametrize("plane", [(1, 1, 1), (6, 5, 7), (3, 64, 33), (33, 128, 128)])
def test_upsample(dev, plane):
    """(33, 128, 128): 2.16 M outputs, a second grid pass.  Backward r = 3: the three
    additions of (s0 + s1) + (s2 + s3)."""
    nc, h, w = plane
    x, dy = data(nc, h, w, seed=370), data(nc, 2 * h, 2 * w, seed=371)
    exact(ops.upsample2x(x.to(dev)[None]), R.upsample_fwd(x), "upsample fwd")
    ref, mag = R.upsample_bwd(dy)
    pointwise(ops.upsample2x_bwd(dy.to(dev)[None]), ref, mag, 3, "upsample bwd")


# ======================================================================= stx_tv_loss
TV_SHAPES = [(1, 1, 1, 1), (2, 3, 1, 9), (2, 3, 9, 1), (2, 3, 5, 7), (1, 3, 20, 24),
             (1, 3, 300, 301)]
TV_FACTOR, TV_GSCALE, TV_GDEV = 0.375, -2.5, 0.3


def chain_tv(total):  # tv_kernel: grid-stride, one term per sum per pass
    return cdiv(total, red_blocks(total) * 256)


def run_tv(dev, y, with_grad, gdev):
    """Returns (loss, grad or None, reference tuple, rounding count of the grad)."""
    yd = y.to(dev)
    gd = torch.tensor(TV_GDEV, device=dev) if gdev else None
    grad = torch.full(y.shape, NAN, device=dev) if with_grad else None
    loss = twice(lambda: ops.tv_loss(yd, factor=TV_FACTOR, grad=grad, gscale=TV_GSCALE,
                                     gscale_dev=gd).reshape(1))
    ref = R.tv(y, TV_FACTOR, gscale=TV_GSCALE, gscale_dev=float(gd) if gdev else None)
    return loss, grad, ref, 2 + gdev  # gscale * factor, (* *gscale_dev,) * the sign sum


@pytest.mark.parametrize("shape", TV_SHAPES)
@pytest.mark.parametrize("with_grad", [False, True])
@pytest.mark.parametrize("gdev", [0, 1])
@pytest.mark.parametrize("ties", [False, True])
def test_tv(dev, shape, with_grad, gdev, ties):
    """h == 1, w == 1, 1 x 1; several planes (the last row of one is not a neighbour of
    the first row of the next); (1, 3, 300, 301): 270 900 elements in 133 blocks, 8
    grid-stride passes; ties: values from a grid of 0.5, so most neighbours are equal
    (sign 0).  grad == NULL drops the stores and must leave the loss's bits alone."""
    y = data(*shape, seed=380, ties=ties)
    loss, grad, (rl, rmag, rg, rgmag), r = run_tv(dev, y, with_grad, gdev)
    reduction(loss, [rl], [rmag], chain_tv(y.numel()), "tv loss")
    if with_grad:
        pointwise(grad, rg, rgmag, r, "tv grad")
        assert torch.equal(loss, run_tv(dev, y, False, gdev)[0])


def test_tv_constant_planes(dev):
    """Each plane a different constant: loss and gradient are exactly 0 unless rows of
    different planes are paired."""
    y = (torch.arange(6.0).reshape(2, 3, 1, 1) * 0.5 - 1).expand(2, 3, 5, 7).contiguous()
    loss, grad, _, _ = run_tv(dev, y, True, 1)
    assert float(loss) == 0.0 and not grad.any()


def test_tv_refuses_2_pow_29_elements(dev):
    """stx_tv_loss tests the element count before its workspace and before any launch, so
    a tiny tensor with large dims is safe to pass."""
    y = torch.zeros(16, device=dev)
    L = N.lib()
    wp, wn = ops.WS.get(L.stx_tv_ws(1, 1, 1 << 15, 1 << 14), dev)
    with refused("2\\^29"):
        N.check(L.stx_tv_loss(y.data_ptr(), y.data_ptr(), None, 1.0, None, 1, 1, 1 << 15, 1 << 14,
                              1.0, wp, wn, ops._stream()), "stx_tv_loss")


# ======================================================================= stx_bias_grad
BIAS_SHAPES = [(2, 16, 1024),     # one pass
               (2, 15, 1024),     # c just below the switch: two passes
               (4, 16, 16384),    # n hw == 65536 exactly: still one pass
               (4, 16, 16388),    # just above: two passes, float4
               (3, 7, 255),       # hw % 4 != 0: scalar loads
               (1, 3, 70_000)]    # long planes


def chain_bias(n, c, hw, aligned=True):
    if hw % 4 == 0 and aligned:
        if n * hw <= 65536 and c >= 16:
            return n * cdiv(hw // 4, 256)      # bias_grad_c_kernel: every plane, one lane sum
        return cdiv(hw // 4, 256) + n          # plane_sum_kernel, then sum_over_n_kernel
    return cdiv(hw, 256) + n


@pytest.mark.parametrize("shape", BIAS_SHAPES)
@pytest.mark.parametrize("acc", [0, 1])
def test_bias_grad(dev, shape, acc):
    n, c, hw = shape
    dy, old = data(n, c, hw, seed=390), data(c, seed=391) + 2.0
    dyd = dy.to(dev)
    start = old.to(dev) if acc else torch.full((c,), NAN, device=dev)
    got = twice(lambda: ops.bias_grad(dyd, start.clone(), accumulate=bool(acc)))
    ref, mag = R.bias_grad(dy, old=old if acc else None)
    reduction(got, ref, mag, chain_bias(n, c, hw) + acc, "bias_grad")


@pytest.mark.parametrize("acc", [0, 1])
def test_bias_grad_unaligned_base(dev, acc):
    """The one-pass shape from a base 4 bytes off a 16-byte boundary: scalar loads, two
    passes; the same sums as the aligned run within both bounds."""
    n, c, hw = BIAS_SHAPES[0]
    dy, old = data(n, c, hw, seed=390), data(c, seed=391) + 2.0
    buf = torch.empty(n * c * hw + 1, device=dev)
    view = buf[1:].view(n, c, hw)
    view.copy_(dy)
    assert view.data_ptr() % 16 == 4
    start = old.to(dev) if acc else torch.full((c,), NAN, device=dev)
    got = twice(lambda: ops.bias_grad(view, start.clone(), accumulate=bool(acc)))
    ref, mag = R.bias_grad(dy, old=old if acc else None)
    Lu, La = chain_bias(n, c, hw, aligned=False) + acc, chain_bias(n, c, hw) + acc
    reduction(got, ref, mag, Lu, "bias_grad unaligned")
    aligned = ops.bias_grad(dy.to(dev), start.clone(), accumulate=bool(acc))
    within(got, aligned.double().cpu().numpy(), (Lu + La + 32) * U * mag, "unaligned vs aligned")


# ======================================================================= stx_adam_step
@pytest.mark.parametrize("n", [1, 3, 1001])
def test_adam_three_steps(dev, n):
    """Three steps on 16-byte aligned buffers and on views one float off.  ops.adam_step and
    the ABI accept both: the kernel's `vec` switch holds, not the header's former "16-byte
    aligned buffers" (include/stx.h now says so); the two forms agree within the bound, not
    bit for bit (the compiler contracts the two loops differently).  Each step is compared with one fp64 torch.optim.Adam step from the state the kernel itself left.
    Hyper-parameters are exact in fp32.  Roundings: m' = m + w1 (g - m): r = 4 (w1, the
    difference, the product, the sum), M = |m| + w1 (|g| + |m|);  v' = v b2 + w2 g g: r = 5,
    all terms >= 0 so M = v';  p' = p - step m' / (sqrt(v') / sqrt(bc2) + eps): r = 16 (m'
    4, v' under the root 3, the root, step and sqrt(bc2) one cast each, two quotients, two
    products / sums of the denominator and update, the final sum, rounded up), M = |p| +
    step M_m / denom."""
    lr, b1, b2, eps = 2.0 ** -7, 0.875, 1 - 2.0 ** -6, 2.0 ** -20
    L = N.lib()
    p0 = data(n, seed=400)
    gs = [data(n, seed=401 + t, ties=(t == 1)) for t in range(3)]
    for off in (0, 1):
        p, g, m, v = (torch.zeros(n + 4, device=dev)[off:off + n] for _ in range(4))
        assert p.data_ptr() % 16 == 4 * off
        p.copy_(p0)
        step = torch.zeros(1, dtype=torch.int32, device=dev)
        ws = torch.empty(L.stx_adam_ws(), dtype=torch.uint8, device=dev)
        for t in range(1, 4):
            before = [x.cpu() for x in (p, m, v)]
            g.copy_(gs[t - 1])
            ops.adam_step(p, g, m, v, step, ws, lr=lr, beta1=b1, beta2=b2, eps=eps)
            rp, rm, rv = R.adam(before[0], gs[t - 1], before[1], before[2], t, lr=lr, b1=b1,
                                b2=b2, eps=eps)
            pb, mb, _ = (R.f64(x) for x in before)
            Mm = np.abs(mb) + (1 - b1) * (np.abs(R.f64(gs[t - 1])) + np.abs(mb))
            pointwise(m, rm, Mm, 4, f"adam m step {t} offset {off}")
            pointwise(v, rv, rv, 5, f"adam v step {t} offset {off}")
            denom = np.sqrt(rv) / np.sqrt(1 - b2 ** t) + eps
            Mp = np.abs(pb) + lr / (1 - b1 ** t) * Mm / denom
            pointwise(p, rp, Mp, 16, f"adam p step {t} offset {off}")
        assert int(step) == 3


# ======================================================================= vec.hip
VEC_N = [0, 1, 3, 4, 1027, 300_001]


def chain_vec(n):  # vred_partial_kernel: 256 x 256 threads, 4 terms per float4 pass + a tail
    return 4 * cdiv(n // 4, 256 * 256) + (1 if n % 4 else 0)


def vreduce(a, b, n, op, out, mul, add, sgn):
    L = N.lib()
    wp, wn = ops.WS.get(L.stx_vec_ws(), a.device)
    N.check(L.stx_vec_reduce(a.data_ptr(), ops._p(b), n, op, out.data_ptr(), ops._p(mul),
                             ops._p(add), float(sgn), wp, wn, ops._stream()), "stx_vec_reduce")
    return out


@pytest.mark.parametrize("n", VEC_N)
@pytest.mark.parametrize("op", [0, 1, 2])
@pytest.mark.parametrize("epi", [False, True])
def test_vec_reduce(dev, n, op, epi):
    """n = 0 gives *out = add (0 without add); 300 001: 75 000 float4 over 65 536 threads,
    two passes, and a tail of 1.  The epilogue add + sgn r mul scales sum|terms| by |mul|
    and adds |add|; its two roundings sit inside the + 16.  op 2 without epilogue is a
    selection: bit-exact."""
    a, b = data(max(n, 4), seed=410), data(max(n, 4), seed=411)  # (n = 0 still needs a pointer)
    ad, bd = a.to(dev), b.to(dev)
    mul = torch.tensor(-0.75, device=dev) if epi else None
    add = torch.tensor(1.5, device=dev) if epi else None
    sgn = -1.0 if epi else 1.0
    out = torch.full((1,), NAN, device=dev)
    got = twice(lambda: vreduce(ad, bd if op == 0 else None, n, op, out, mul, add, sgn))
    ref, mag = R.vec_reduce(a[:n], b[:n], op, -0.75 if epi else None, 1.5 if epi else None, sgn)
    if n == 0 or (op == 2 and not epi):
        exact(got, [ref], "vec_reduce")
    else:
        reduction(got, [ref], [mag], chain_vec(n), "vec_reduce")


def vaxpby(y, x, n, a, a_dev, a_sgn, b):
    N.check(N.lib().stx_vec_axpby(y.data_ptr(), ops._p(x), n, float(a), ops._p(a_dev),
                                  float(a_sgn), float(b), ops._stream()), "stx_vec_axpby")


@pytest.mark.parametrize("n", VEC_N)
@pytest.mark.parametrize("case", ["plain", "scale_only", "b0_nan_y", "a_dev"])
def test_vec_axpby(dev, n, case):
    """r = 5 at most: alpha = a_sgn *a_dev a (2), alpha x, b y, their sum.  b == 0 must not
    read y (pre-filled with NaN); x == NULL scales y."""
    x, y = data(max(n, 4), seed=420), data(max(n, 4), seed=421)
    a, b, a_dev, a_sgn, xs = {"plain": (1.5, -0.75, None, 1.0, x),
                              "scale_only": (1.5, -0.75, None, 1.0, None),
                              "b0_nan_y": (1.5, 0.0, None, 1.0, x),
                              "a_dev": (2.0, 0.5, 0.3, -1.0, x)}[case]
    if case == "b0_nan_y":
        y = torch.full_like(y, NAN)
    yd = y.to(dev)
    ad = None if a_dev is None else torch.tensor(a_dev, device=dev)
    vaxpby(yd, None if xs is None else xs.to(dev), n, a, ad, a_sgn, b)
    ref, mag = R.axpby(y[:n], None if xs is None else xs[:n], a, b,
                       None if ad is None else float(ad), a_sgn)
    pointwise(yd[:n], ref, mag, 5, "axpby")
    exact(yd[n:], y[n:].numpy(), "axpby beyond n")  # nothing past n is touched


def test_vec_refuse_unaligned(dev):
    buf, out = torch.zeros(68, device=dev), torch.zeros(1, device=dev)
    for a, b in ((buf[1:65], buf[4:68]), (buf[4:68], buf[1:65])):
        with refused("aligned"):
            vreduce(a, b, 64, 0, out, None, None, 1.0)
        with refused("aligned"):
            vaxpby(a, b, 64, 1.0, None, 1.0, 1.0)


@pytest.mark.parametrize("op,i,j,k", [(0, 0, 1, 3), (1, 0, 1, 3), (2, 0, 1, 3), (3, 0, 1, 3),
                                       (4, 0, 1, 3), (5, 0, 1, 3), (4, 2, -1, 2), (0, 2, 1, 2),
                                       (5, 2, 1, 2)])
def test_scalar_op(dev, op, i, j, k):
    """All six ops, j = -1 for the reciprocal, k aliasing i.  r = 1: one correctly rounded
    operation each (op 5's min is exact)."""
    s = torch.tensor([4.0, -0.3, 3.0, 9.0, 0.7, -5.0, 11.0, 13.0])
    sd = s.to(dev)
    N.check(N.lib().stx_scalar_op(sd.data_ptr(), op, i, j, k, ops._stream()), "stx_scalar_op")
    ref, mag = R.scalar_op(s, op, i, j, k)
    m = np.zeros(8)
    m[k] = mag
    pointwise(sd, ref, m, 1, "scalar_op")  # M = 0 elsewhere: untouched, bit for bit


# ======================================================================= stx_lbfgs_grad_stats
def chain_gstats(n):  # lb_gstats_kernel: 512 x 256 threads, 4 terms per float4 pass + a tail
    return 4 * cdiv(n // 4, 512 * 256) + (1 if n % 4 else 0)


def grad_stats(g, n, loss, scal, clear, clear_n):
    L = N.lib()
    wp, wn = ops.WS.get(2 * 512 * 4, g.device)
    N.check(L.stx_lbfgs_grad_stats(g.data_ptr(), n, ops._p(loss), scal.data_ptr(),
                                   ops._p(clear), clear_n, wp, wn, ops._stream()),
            "stx_lbfgs_grad_stats")
    return scal


@pytest.mark.parametrize("n", [1, 5, 4093, 786_432])
@pytest.mark.parametrize("with_loss,clear_n", [(True, 0), (False, 7), (True, 300)])
def test_lbfgs_grad_stats(dev, n, with_loss, clear_n):
    """4093: a tail of 1; 786 432: 196 608 float4 over 131 072 threads, two passes.
    scal[1] = max|g| is a selection (exact), scal[2] = sum|g| a reduction; scal[0] only
    with loss; scal[3..] and clear[clear_n..] stay."""
    g = data(n, seed=430)
    gd = g.to(dev)
    loss = torch.tensor(2.75, device=dev) if with_loss else None

    def run():
        scal = torch.arange(16.0, device=dev) + 100
        clear = torch.full((320,), 5.0, device=dev)
        grad_stats(gd, n, loss, scal, clear if clear_n else None, clear_n)
        return torch.cat([scal, clear])

    got = twice(run)
    _, mx, sm = R.grad_stats(g)
    assert float(got[0]) == (2.75 if with_loss else 100.0)
    exact(got[1:2], [mx], "max|g|")
    reduction(got[2:3], [sm], [sm], chain_gstats(n), "sum|g|")
    assert torch.equal(got[3:16].cpu(), torch.arange(3, 16.0) + 100)
    assert not got[16:16 + clear_n].any() and torch.all(got[16 + clear_n:] == 5.0)


# ======================================================================= NaN contract
def nan_at(x, where):
    x = x.clone()
    x.view(-1)[{"first": 0, "last": -1, "middle": x.numel() // 2}[where]] = NAN
    return x


WHERE = ["first", "last", "middle"]


@pytest.mark.parametrize("where", WHERE)
def test_nan_reaches_every_max_and_loss(dev, where):
    """One NaN at the first element, the last (inside the scalar tail: the sizes are no
    multiples of 4) or the middle must come out of stx_amax, stx_vec_reduce op 2,
    stx_lbfgs_grad_stats (max and, by arithmetic, the sum), stx_mse and stx_tv_loss."""
    x = nan_at(data(4099, seed=440), where).to(dev)
    o = data(4099, seed=441).to(dev)
    assert torch.isnan(ops.amax(x)).any(), "stx_amax"
    out = torch.zeros(1, device=dev)
    assert torch.isnan(vreduce(x, None, 4099, 2, out, None, None, 1.0)).all(), "vec_reduce max"
    scal = grad_stats(x, 4099, None, torch.zeros(16, device=dev), None, 0)
    assert torch.isnan(scal[1:3]).all(), "grad_stats"
    for a, b in ((x, o), (o, x)):
        assert torch.isnan(ops.mse(a, b, mode=0)).all(), "mse mode 0"
        assert torch.isnan(ops.mse(a, b, mode=1)).all(), "mse mode 1"
        assert torch.isnan(ops.mse(a, b, mode=2)[0]), "mse mode 2, the plain mean"
        # the relu'd sums read a NaN as 0 (fmaxf), as include/stx.h says of stx_mse
        assert not torch.isnan(ops.mse(a, b, relu=True, mode=0)).any()
    y = nan_at(data(1, 3, 19, 23, seed=442), where).to(dev)
    assert torch.isnan(ops.tv_loss(y, factor=1.0)), "tv loss"


def test_nan_plane_reaches_instnorm_out_amax(dev):
    x = data(1, 2, 8, 8, seed=443)
    x[0, 1, 3, 4] = NAN
    am = torch.zeros(N.STX_AMAX_SLOTS, device=dev)
    y, _, _ = ops.instnorm_fwd(x.to(dev), torch.ones(2, device=dev), torch.zeros(2, device=dev),
                               out_amax=am)
    assert torch.isnan(am).any() and not torch.isnan(y[0, 0]).any()


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("relu", [0, 1])
def test_nan_through_relu_and_maxpool(dev, where, relu):
    """stx_relu_fwd and stx_maxpool2x2_fwd stand in for torch's ReLU / MaxPool2d(ReLU(.)) on
    the generic path, where torch keeps a NaN: the window's output is NaN and idx points at
    it, with relu_input too (fmaxf(NaN, 0) = 0 used to heal it); the rest is untouched."""
    x = nan_at(data(3, 6, 10, seed=444), where)
    y, idx = ops.maxpool2x2(x.to(dev)[None], relu_input=bool(relu))
    ry, ridx = R.maxpool_fwd(x, relu_input=bool(relu))
    assert np.isnan(ry).sum() == 1
    exact(y, ry, "maxpool with a NaN")
    assert torch.equal(idx[0].cpu(), torch.from_numpy(ridx))
    if relu:
        exact(ops.relu(x.to(dev)), R.relu(x), "relu with a NaN")


def test_nan_gives_zero_in_relu_backwards(dev):
    """stx_relu_bwd at a NaN y and stx_relupool_bwd at a NaN z give 0, as torch's backward."""
    z = nan_at(data(2, 4, 6, seed=445), "middle")
    dy, dp = data(2, 4, 6, seed=446), data(2, 2, 3, seed=447)
    k = z.numel() // 2
    assert float(ops.relu_bwd(dy.to(dev), z.to(dev)).view(-1)[k]) == 0.0
    dz = ops.relupool_bwd(dp.to(dev)[None], z.to(dev)[None])
    assert float(dz.view(-1)[k]) == 0.0
    exact(ops.relu_bwd(dy.to(dev), z.to(dev)), R.relu_bwd(dy, z), "relu bwd with a NaN")


def test_nan_fused_pool_out_equals_generic_pool(dev):
    """The split conv's fused pool_out and stx_maxpool2x2_fwd(relu_input = 1) of the same
    pre-activation agree where it carries NaN (here one whole channel, through its bias):
    NaN in the same windows, the same bits elsewhere -- the shape of
    test_split_conv_pool_out, in the style of test_vgg_fused_pool_matches_unfused."""
    n, cin, cout, h, w = 2, 64, 64, 20, 70
    x = (data(n, cin, h, w, seed=448)).to(dev)
    wgt = (data(cout, cin, 3, 3, seed=449) * 0.1).to(dev)
    b = data(cout, seed=450) * 0.1
    b[3] = NAN
    pool = torch.zeros((n, cout, h // 2, w // 2), device=dev)
    y = ops.conv2d(x, ops.conv_weight_prep(wgt), cin, cout, 3, bias=b.to(dev),
                   wt16=ops.conv_weight_prep16(wgt), pool_out=pool)
    assert torch.isnan(y[:, 3]).all() and not torch.isnan(y[:, :3]).any()
    generic, _ = ops.maxpool2x2(y, relu_input=True, want_idx=False)
    assert torch.isnan(pool[:, 3]).all()
    exact(generic, pool.cpu().numpy(), "generic vs fused pool")
