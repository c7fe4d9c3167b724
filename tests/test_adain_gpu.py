"""The AdaIN kernels (csrc/adain.hip: stx_chan_stats, stx_adain, stx_stats_loss,
stx_stats_loss_bwd) against the fp64 restatement of tests/adain_ref.py, element by element,
the convs of the deep VGG tail and the decoder at channel counts nothing else runs, and the
whole path (trainer step, CLI) at 64^2.

Bounds come from the kernels' summation chains, not from a run.  u = 2^-24.  A sum whose
every term passes through at most D fp32 additions is within D u sum|x| of the exact sum
(first order); D per variant (chain_depth):

    register variants (hw % 4 == 0, aligned x):  a thread adds its R4 float4 groups, each
        group as (v0+v1)+(v2+v3): R4 + 2; the wave butterfly: 6; the waves' partials in
        series: NT/64.  (NT, R4) = (256, 4) to 4096 floats, (512, 8) to 16384, (1024, 16) to
        65536.
    loop variants: ceil(hw / (4 NT)) float4 trips (+2) or ceil(hw / NT) scalar trips per
        thread, then 6 + NT/64; NT = 256 below 16384 floats, 1024 from there.

    mean:  em = (D + 1) u mean|x|                       (the division rounds once more)
    Q^ = sum (x - mean^)^2 = Q + hw (mean - mean^)^2 exactly (sum (x - mean) = 0), each term
        rounded three times and summed through D additions:
        eQ = (D + 4) u (Q + hw em^2) + hw em^2
    std = sqrt(Q/(hw-1) + eps):  ev = eQ/(hw-1) + 2 u (var + eps),  es = ev / (2 std) + u std
    -- a mean error enters std through hw em^2 against var + eps, so a near-constant plane
    with a large mean (std near sqrt(eps) = 3.2e-3) has a visibly wider es: the bound says so.

    AdaIN  y = fma(x, a, b), r = G/std, a = fma(alpha, r, 1-alpha), b = alpha fma(-r, mean, M):
    the same r^ multiplies x and mean, so y^ = (1-alpha) x + alpha (r^ (x - mean^) + M^) up to
    the roundings of a, b and the fma:
        er = (eG + |G| es / std) / std + 2 u |r|,   eG = S u sum_s |mix sstd|  (eM alike)
        ey = alpha [er (|x - mean| + em) + |r| em + eM + u (|M| + |r mean|)]
             + u (2 |x a| + 2 |b| + |y|)
    |r| em is the amplification of a mean error by G/std (about 300 G at std = sqrt(eps)).

All bounds are first order; SLACK = 2 covers the second-order terms (the data keeps
ev <= var/2, checked)."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import adain_ref as R
from styletransfer_amd import _native as N
from styletransfer_amd import adain as M
from styletransfer_amd import autograd as A
from styletransfer_amd import ops
from styletransfer_amd import weights as W

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SLACK = 2.0
EPS = R.EPS32
TINY = 1e-44  # below the smallest fp32 subnormal: lets 0 <= 0 pass without admitting anything


# ------------------------------------------------------------------ variants and bounds
def variant(hw, aligned=True):
    """stx_*'s kernel choice (adain.hip launch_plane): (kind, threads, float4s per thread)."""
    reg = hw % 4 == 0 and aligned
    if reg and hw <= 4096:
        return "reg", 256, 4
    if reg and hw <= 16384:
        return "reg", 512, 8
    if reg and hw <= 65536:
        return "reg", 1024, 16
    return ("loop", 1024, 0) if hw >= 16384 else ("loop", 256, 0)


def chain_depth(hw, aligned=True):
    kind, nt, r4 = variant(hw, aligned)
    if kind == "reg":
        per_thread = r4 + 2
    elif hw % 4 == 0 and aligned:
        per_thread = math.ceil(hw / (4 * nt)) + 2
    else:
        per_thread = math.ceil(hw / nt)
    return per_thread + 6 + nt // 64


def stat_bounds(p, D):
    """p [P, hw] fp64 -> (mean, std, em, es) per plane."""
    hw = p.shape[1]
    m = p.mean(1)
    em = (D + 1) * U * np.abs(p).mean(1)
    Q = ((p - m[:, None]) ** 2).sum(1)
    eQ = (D + 4) * U * (Q + hw * em ** 2) + hw * em ** 2
    v = Q / (hw - 1) + EPS
    ev = eQ / (hw - 1) + 2 * U * v
    assert (ev <= 0.5 * v).all(), "test data: the first-order std bound needs ev <= var/2"
    s = np.sqrt(v)
    return m, s, SLACK * em, SLACK * (ev / (2 * s) + U * s)


def adain_bounds(p, smean, sstd, mix, alpha, c, D):
    """Reference y [P, hw] and its per-element bound; tables [S, c], mix [n, S] fp64."""
    m, s, em, es = stat_bounds(p, D)
    em, es = em / SLACK, es / SLACK
    S = smean.shape[0]
    Mx = (mix @ smean).reshape(-1)
    G = (mix @ sstd).reshape(-1)
    eM = S * U * (np.abs(mix) @ np.abs(smean)).reshape(-1)
    eG = S * U * (np.abs(mix) @ np.abs(sstd)).reshape(-1)
    r = G / s
    er = (eG + np.abs(G) * es / s) / s + 2 * U * np.abs(r)
    a = (1 - alpha) + alpha * r
    b = alpha * (Mx - r * m)
    y = p * a[:, None] + b[:, None]
    ey = alpha * (er[:, None] * (np.abs(p - m[:, None]) + em[:, None])
                  + (np.abs(r) * em + eM + U * (np.abs(Mx) + np.abs(r * m)))[:, None]) \
        + U * (2 * np.abs(p * a[:, None]) + 2 * np.abs(b)[:, None] + np.abs(y))
    return y, SLACK * ey + TINY


# ------------------------------------------------------------------------------- data
# (n, c, hw, aligned): hw 2..5; both sides of every dispatch threshold (4096 | 4100, 16384 |
# 16388, 65536 | 65540 for the register variants, 16382 | 16386 for the loop block size);
# the relu4_1 planes 1024 and 4096; a loop-path size >= 65536 with few planes; c in
# {5, 64, 512}; n c below and above the 256 planes one pass of the loss's final block takes;
# an unaligned base and hw % 4 != 0; 2048 | 2040 planes: stx_adain walks four small planes per
# block from 512 blocks (the one-hot check below compares its bits with one-plane blocks')
CASES = [
    (2, 5, 2, True), (2, 5, 3, True), (2, 5, 4, True), (2, 5, 5, True),
    (2, 512, 1024, True), (1, 64, 4096, True), (1, 5, 4100, True),
    (1, 3, 16384, True), (1, 3, 16388, True), (1, 3, 65536, True), (1, 3, 65540, True),
    (1, 3, 16382, True), (1, 3, 16386, True), (1, 3, 65537, True),
    (1, 5, 1024, False), (2, 64, 1023, True), (1, 5, 4096, False), (1, 3, 16384, False),
    (8, 256, 64, True), (8, 255, 64, True),
]
IDS = [f"n{n}c{c}hw{hw}{'' if al else 'u'}" for n, c, hw, al in CASES]
_cache = {}


def make(case, dev):
    """x [n, c, hw] fp32 on the device (at a 4-byte-aligned, not 16-byte-aligned base when
    not `aligned`) and its fp64 planes.  Plane 0 and every other plane carry end-of-plane
    markers (a large first and last element: a missed or doubled element moves the
    statistics far beyond the bound); plane 1: a mean that dwarfs its spread; plane 2:
    constant.  The arrays are shared by the tests and never modified."""
    if case in _cache:
        return _cache[case]
    n, c, hw, aligned = case
    P = n * c
    rng = np.random.default_rng(n * 1000003 + c * 1009 + hw * 7 + int(aligned))
    x = rng.standard_normal((P, hw)) * rng.uniform(0.2, 3.0, (P, 1)) + rng.uniform(-2, 2, (P, 1))
    x[:, 0] += 9.0
    x[:, -1] -= 7.0
    x[1] = 100.0 + 0.05 * rng.standard_normal(hw)
    x[2] = 1.5
    x = x.astype(np.float32)
    buf = torch.zeros(P * hw + 8, dtype=torch.float32, device=dev)
    off = 4 if aligned else 1
    xd = buf[off:off + P * hw].view(n, c, hw)
    xd.copy_(torch.from_numpy(x).view(n, c, hw))
    assert (xd.data_ptr() % 16 == 0) == aligned
    _cache[case] = (xd, x.astype(np.float64))
    return _cache[case]


def tables(case, S, dev, seed=0):
    n, c = case[:2]
    rng = np.random.default_rng(1000 + seed + S)
    smean = rng.standard_normal((S, c)).astype(np.float32)
    sstd = rng.uniform(0.3, 2.0, (S, c)).astype(np.float32)
    t = lambda a: torch.from_numpy(a).to(dev)
    return smean, sstd, t(smean), t(sstd)


def mixes(n, S, kind, dev):
    if kind == "onehot":
        m = np.zeros((n, S), np.float32)
        m[np.arange(n), (np.arange(n) + 1) % S] = 1.0
    else:
        rng = np.random.default_rng(n * 10 + S)
        m = rng.uniform(0.1, 1.0, (n, S))
        m = (m / m.sum(1, keepdims=True)).astype(np.float32)
    return m, torch.from_numpy(m).to(dev)


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def close(got, ref, bound, what):
    got = got.detach().double().cpu().numpy().reshape(ref.shape)
    err = np.abs(got - ref)
    bad = ~(err <= bound)
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} outside the bound; worst "
                           f"err/bound {np.nanmax(err / bound):.3g}")
    return float(np.max(err / bound))


# ------------------------------------------------------------------------- statistics
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_chan_stats_against_fp64(dev, case):
    n, c, hw, aligned = case
    xd, p = make(case, dev)
    D = chain_depth(hw, aligned)
    for relu in (False, True):
        q = np.where(p <= 0, 0.0, p) if relu else p
        m, s, em, es = stat_bounds(q, D)
        mean, std = ops.chan_stats(xd, EPS, relu_input=relu)
        mean2, std2 = ops.chan_stats(xd, EPS, relu_input=relu)
        assert torch.equal(bits(mean), bits(mean2)) and torch.equal(bits(std), bits(std2))
        r1 = close(mean, m, em + TINY, f"mean relu={relu}")
        r2 = close(std, s, es, f"std relu={relu}")
        print(f"{IDS[CASES.index(case)]} relu={relu} D={D}: mean {r1:.3g} std {r2:.3g} of bound")
    # the constant plane: every partial sum of 1.5 is exact, so the mean is 1.5, the squared
    # deviations are 0 and std = sqrt(eps) to fp32's rounding of the root
    mean, std = ops.chan_stats(xd, EPS)
    assert float(mean.view(-1)[2]) == 1.5
    assert abs(float(std.view(-1)[2]) - math.sqrt(EPS)) <= 2 * U * math.sqrt(EPS)


# ------------------------------------------------------------------------------ AdaIN
ADAIN_CASES = [CASES[i] for i in (0, 1, 3, 4, 5, 6, 8, 10, 12, 14, 15, 18, 19)]


@pytest.mark.parametrize("case", ADAIN_CASES, ids=[IDS[CASES.index(k)] for k in ADAIN_CASES])
def test_adain_against_fp64(dev, case):
    n, c, hw, aligned = case
    xd, p = make(case, dev)
    D = chain_depth(hw, aligned)
    mean0, std0 = ops.chan_stats(xd, EPS)
    combos = [(S, kind, alpha) for S in (1, 2, 3) for kind in ("onehot", "convex")
              for alpha in (0.0, 0.5, 1.0)]
    if n * c * hw > 70000:  # the large cases: every S, kind and alpha once, not their product
        combos = [(1, "onehot", 1.0), (2, "convex", 0.5), (3, "onehot", 0.0), (3, "convex", 1.0),
                  (2, "onehot", 0.5)]
    for S, kind, alpha in combos:
        smean, sstd, smd, ssd = tables(case, S, dev)
        mix, mixd = mixes(n, S, kind, dev)
        am = torch.zeros(N.STX_AMAX_SLOTS, device=dev)
        y, mean, std = ops.adain(xd, smd, ssd, mixd, alpha, EPS, out_amax=am, stats=True)
        y2 = ops.adain(xd, smd, ssd, mixd, alpha, EPS)
        assert torch.equal(bits(y), bits(y2)), "not reproducible"
        assert torch.equal(bits(mean), bits(mean0)) and torch.equal(bits(std), bits(std0))
        assert float(am.max()) == float(y.abs().max()), "out_amax is not the exact max"
        ref, bound = adain_bounds(p, smean.astype(np.float64), sstd.astype(np.float64),
                                  mix.astype(np.float64), alpha, c, D)
        close(y, ref, bound, f"S={S} {kind} alpha={alpha}")
        if alpha == 0.0:
            assert torch.equal(y, xd), "alpha = 0 must return x in value"
        if kind == "onehot" and S > 1:
            # routing only: the bits of S = 1 with the selected rows, sample by sample
            sel = mix.argmax(1)
            one = torch.ones(1, 1, device=dev)
            for k in range(n):
                r = int(sel[k])
                yk = ops.adain(xd[k:k + 1], smd[r:r + 1].contiguous(),
                               ssd[r:r + 1].contiguous(), one, alpha, EPS)
                assert torch.equal(bits(yk), bits(y[k:k + 1])), (S, k, alpha)


def test_adain_in_place_and_unaligned_output(dev):
    case = CASES[5]  # 4096: a register variant
    xd, p = make(case, dev)
    n, c, hw, _ = case
    smean, sstd, smd, ssd = tables(case, 2, dev)
    mix, mixd = mixes(n, 2, "convex", dev)
    y = ops.adain(xd, smd, ssd, mixd, 0.5, EPS)
    buf = torch.zeros(xd.numel() + 8, device=dev)
    yu = buf[1:1 + xd.numel()].view_as(xd)  # 4-byte aligned output: scalar stores
    ops.adain(xd, smd, ssd, mixd, 0.5, EPS, out=yu)
    assert torch.equal(bits(yu), bits(y))
    assert float(buf[0]) == 0.0 and float(buf[1 + xd.numel()]) == 0.0
    xi = xd.clone()
    ops.adain(xi, smd, ssd, mixd, 0.5, EPS, out=xi)
    assert torch.equal(bits(xi), bits(y))


# ------------------------------------------------------------------------------- loss
def _targets(case, dev, seed=5):
    n, c = case[:2]
    rng = np.random.default_rng(seed)
    tm = rng.standard_normal((n, c)).astype(np.float32)
    ts = rng.uniform(0.2, 2.0, (n, c)).astype(np.float32)
    return tm, ts, torch.from_numpy(tm).to(dev), torch.from_numpy(ts).to(dev)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_stats_loss_forward_against_fp64(dev, case):
    """Per plane (mean^ - tmean)^2 is within 2 |dm| em' + em'^2 of the exact square, em' = em +
    2 u |dm| (the subtraction and the square round once each); the final block sums P planes
    through ceil(P/256) + 6 + 4 additions and scales in fp64 (one rounding to fp32); out[0]
    is one more fp32 addition."""
    n, c, hw, aligned = case
    xd, p = make(case, dev)
    tm, ts, tmd, tsd = _targets(case, dev)
    m, s, em, es = stat_bounds(p, chain_depth(hw, aligned))
    P, weight = n * c, 3.5
    k = float(np.float32(weight)) / P
    DP = math.ceil(P / 256) + 10
    parts, bounds = [], []
    for ref, tgt, e in ((m, tm.reshape(-1).astype(np.float64), em),
                        (s, ts.reshape(-1).astype(np.float64), es)):
        d = np.abs(ref - tgt)
        e1 = e + 2 * U * d
        sq = d ** 2
        parts.append(k * sq.sum())
        bounds.append(SLACK * k * ((2 * d * e1 + e1 ** 2).sum() + (DP + 1) * U * sq.sum())
                      + U * k * sq.sum())
    add = torch.full((1,), 3.25, device=dev)
    out, mean, std = ops.stats_loss(xd, tmd, tsd, weight, EPS, add_to=add)
    out2, mean2, std2 = ops.stats_loss(xd, tmd, tsd, weight, EPS)
    assert torch.equal(bits(out), bits(out2)) and torch.equal(bits(mean), bits(mean2))
    m0, s0 = ops.chan_stats(xd, EPS)
    assert torch.equal(bits(mean), bits(m0)) and torch.equal(bits(std), bits(s0))
    o = out.double().cpu().numpy()
    print(f"{IDS[CASES.index(case)]}: L {o[0]:.8g} fp64 {parts[0] + parts[1]:.8g}; mean part "
          f"err/bound {abs(o[1] - parts[0]) / bounds[0]:.3g}, std part "
          f"{abs(o[2] - parts[1]) / bounds[1]:.3g}")
    assert abs(o[1] - parts[0]) <= bounds[0] and abs(o[2] - parts[1]) <= bounds[1]
    assert abs(o[0] - (parts[0] + parts[1])) <= bounds[0] + bounds[1] + U * (parts[0] + parts[1])
    oc = out.cpu()
    assert float(oc[0]) == float(oc[1] + oc[2])                       # one fp32 addition
    assert float(add) == float(torch.tensor(3.25) + oc[0])            # add_to += out[0]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_stats_loss_backward_element_by_element(dev, case):
    """dx = fma(B, x - mean, A) from the saved fp32 mean / std (the backward's inputs, taken
    as exact here; their own error is the forward test's).  A rounds 5 times (the
    subtraction, / hw, the fp32 k, k g, the product), B 6 times, x - mean once, the fma once:
    |dx^ - dx| <= 5 u |A| + 7 u |B (x - mean)| + u |dx|; accumulate adds u |old + dx|."""
    n, c, hw, aligned = case
    xd, p = make(case, dev)
    tm, ts, tmd, tsd = _targets(case, dev)
    weight, g = 3.5, 0.37
    _, mean, std = ops.stats_loss(xd, tmd, tsd, weight, EPS)
    m = mean.double().cpu().numpy().reshape(-1)
    s = std.double().cpu().numpy().reshape(-1)
    P = n * c

    def ref(gv):
        kk = gv * float(np.float32(weight)) / P
        A_ = kk * 2 * (m - tm.reshape(-1)) / hw
        B_ = kk * 2 * (s - ts.reshape(-1)) / ((hw - 1) * s)
        t = A_[:, None] + B_[:, None] * (p - m[:, None])
        e = 5 * U * np.abs(A_)[:, None] + 7 * U * np.abs(B_[:, None] * (p - m[:, None])) \
            + U * np.abs(t)
        return t, SLACK * e + TINY
    t1, e1 = ref(1.0)
    am = torch.zeros(N.STX_AMAX_SLOTS, device=dev)
    dx = ops.stats_loss_bwd(xd, mean, std, tmd, tsd, weight, out_amax=am)
    dx2 = ops.stats_loss_bwd(xd, mean, std, tmd, tsd, weight)
    assert torch.equal(bits(dx), bits(dx2))
    assert float(am.max()) == float(dx.abs().max())
    close(dx, t1, e1, "dx")
    # the constant plane: x - mean is exactly 0, so the std term is exactly 0 and every
    # element is the plane's A
    pl = dx.view(P, hw)[2]
    assert torch.equal(bits(pl), bits(pl[:1].expand(hw)))
    # g_dev: a power of two scales every bit pattern exactly; any g stays within the bound
    gd = torch.tensor([2.0], device=dev)
    assert torch.equal(ops.stats_loss_bwd(xd, mean, std, tmd, tsd, weight, g_dev=gd), 2 * dx)
    gd = torch.tensor([g], device=dev)
    tg, eg = ref(float(np.float32(g)))
    close(ops.stats_loss_bwd(xd, mean, std, tmd, tsd, weight, g_dev=gd), tg, eg, "dx g_dev")
    # accumulate
    rng = np.random.default_rng(3)
    old = rng.standard_normal((P, hw)).astype(np.float32)
    old[0, 0] = -0.0
    acc = torch.from_numpy(old).to(dev).view(n, c, hw).clone()
    ops.stats_loss_bwd(xd, mean, std, tmd, tsd, weight, dx=acc, accumulate=True)
    close(acc, old.astype(np.float64) + t1, e1 + SLACK * U * np.abs(old + t1), "dx accumulate")
    # where the added term is 0 the old contents stay bit for bit: the constant plane with
    # tmean = its saved mean (A = 0, B * 0 = 0), a -0.0 among them
    tm0 = tmd.clone()
    tm0.view(-1)[2] = mean.view(-1)[2]
    old[2, 0] = -0.0
    acc = torch.from_numpy(old).to(dev).view(n, c, hw).clone()
    ops.stats_loss_bwd(xd, mean, std, tm0, tsd, weight, dx=acc, accumulate=True)
    assert torch.equal(bits(acc.view(P, hw)[2]), bits(torch.from_numpy(old[2])))


# --------------------------------------------------------------------------- NaN / Inf
@pytest.mark.parametrize("poison", [float("nan"), float("inf"), float("-inf")])
@pytest.mark.parametrize("case", [CASES[4], CASES[6], CASES[16], CASES[18]],
                         ids=["reg1024", "reg4100", "loop4096u", "pipe64"])
def test_nonfinite_plane_stays_in_its_plane(dev, case, poison):
    n, c, hw, aligned = case
    xd, _ = make(case, dev)
    P, bad = n * c, 3
    xp = torch.zeros(xd.numel() + 8, device=dev)[(4 if aligned else 1):][:xd.numel()].view_as(xd)
    xp.copy_(xd)
    xp.view(P, hw)[bad, hw // 2] = poison
    smean, sstd, smd, ssd = tables(case, 2, dev)
    _, mixd = mixes(n, 2, "convex", dev)
    tm, ts, tmd, tsd = _targets(case, dev)
    keep = torch.arange(P) != bad

    def run(x):
        mean, std = ops.chan_stats(x, EPS)
        am = torch.zeros(N.STX_AMAX_SLOTS, device=dev)
        y = ops.adain(x, smd, ssd, mixd, 0.5, EPS, out_amax=am)
        out, lm, ls = ops.stats_loss(x, tmd, tsd, 1.0, EPS)
        dx = ops.stats_loss_bwd(x, lm, ls, tmd, tsd, 1.0)
        return [t.cpu() for t in (mean.view(P), std.view(P), y.view(P, hw), lm.view(P),
                                  ls.view(P), dx.view(P, hw))], out.cpu(), am.cpu()
    clean, _, _ = run(xd)
    dirty, out, am = run(xp)
    for a, b in zip(clean, dirty):
        assert torch.equal(bits(a[keep]), bits(b[keep])), "another plane changed"
        assert torch.isnan(b[bad]).all(), "the poisoned plane must be NaN throughout"
    assert torch.isnan(out).all() and torch.isnan(am).any()


# ------------------------------------------------------- channel counts nobody has run
# HIP error vs fp64 <= max(K * (torch-fp32 error vs fp64), FLOOR), relative norms: K and FLOOR
# as tests/test_itn_masks_gpu.py states and justifies them
K = 3.0
FLOOR = 2e-5


def _rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


@pytest.mark.parametrize("up", [False, True], ids=["raw", "up2"])
@pytest.mark.parametrize("ho,wo", [(4, 4), (8, 8), (6, 48)])
@pytest.mark.parametrize("cin,cout", [(256, 256), (256, 512), (512, 256), (256, 128), (128, 64),
                                      (64, 3)])
def test_conv_channel_counts_fp64(dev, cin, cout, ho, wo, up):
    """The convs of the VGG tail and the decoder, forward, data and weight gradient, raw and
    upsampled-input form (wo = 48: wo > 32 is a split-path rule)."""
    g = torch.Generator().manual_seed(cin * 7 + cout + ho + wo + up)
    hi, wi = (ho // 2, wo // 2) if up else (ho, wo)
    x0 = torch.randn(2, cin, hi, wi, generator=g)
    w0 = torch.randn(cout, cin, 3, 3, generator=g) * math.sqrt(2.0 / (9 * cin))
    b0 = torch.randn(cout, generator=g) * 0.1
    dy0 = torch.randn(2, cout, ho, wo, generator=g)
    x, w, b = (t.to(dev).requires_grad_() for t in (x0, w0, b0))
    y = A.conv2d(x, w, b, 1, 1, in_mode=N.STX_IN_UPSAMPLE2 if up else N.STX_IN_RAW)
    y.backward(dy0.to(dev))
    hip = {"y": y.detach().cpu(), "x": x.grad.cpu(), "w": w.grad.cpu(), "b": b.grad.cpu()}

    def ref(dtype):
        xr, wr, br = (t.to(dtype).requires_grad_() for t in (x0, w0, b0))
        xi = F.interpolate(xr, scale_factor=2, mode="nearest") if up else xr
        yr = F.conv2d(xi, wr, br, 1, 1)
        yr.backward(dy0.to(dtype))
        return {"y": yr.detach(), "x": xr.grad, "w": wr.grad, "b": br.grad}
    r64, r32 = ref(torch.float64), ref(torch.float32)
    for k in r64:
        e, r = _rel(hip[k], r64[k]), _rel(r32[k], r64[k])
        print(f"{k}: hip {e:.2e} fp32 {r:.2e}")
        assert e <= max(K * r, FLOOR), f"{k}: hip {e:.2e} vs fp32 {r:.2e}"


# ----------------------------------------------------------------- whole path at 64^2
def _images(seed, b=2, size=64):
    return torch.from_numpy(W.synthetic_image(seed, (b, 3, size, size)))


def _spy(net):
    """Forward hooks recording the ReLU masks (output > 0) and pool argmax of the decoder and
    of the encoder, per call, in execution order."""
    rec = {"dec": [], "enc": []}
    hs = []
    for name, mod in (("dec", net.decoder), ("enc", net.encoder.features)):
        for m in mod:
            if isinstance(m, torch.nn.ReLU):
                hs.append(m.register_forward_hook(
                    lambda m_, a, out, name=name: rec[name].append((out.detach() > 0).cpu())))
            elif isinstance(m, torch.nn.MaxPool2d):
                hs.append(m.register_forward_hook(
                    lambda m_, a, out, name=name: rec[name].append(
                        F.max_pool2d(a[0].detach().cpu(), 2, 2, return_indices=True)[1])))
    return rec, hs


@pytest.fixture(scope="module")
def step64(dev):
    """One AdaINTrainer step at 64^2 (relu4_1 is 8x8), B = 2, two different styles."""
    net = M.AdaINNet(decoder_seed=11)
    sd0 = {k: v.detach().cpu().numpy().copy() for k, v in net.decoder.state_dict().items()}
    tr = M.AdaINTrainer(net)
    content, style = _images(21), _images(22)
    flat0 = tr.flat.clone()
    ev0 = float(tr.evaluate(content, style))
    assert torch.equal(bits(tr.flat), bits(flat0)), "evaluate moved the parameters"
    assert not tr.flat_grad.any() and tr.k == 0
    rec, hs = _spy(net)
    loss = float(tr.step(content, style))
    for h in hs:
        h.remove()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().cpu().clone() for k, p in net.decoder.named_parameters()}
    return dict(net=net, tr=tr, sd0=sd0, content=content, style=style, ev0=ev0, loss=loss,
                grads=grads, rec=rec, flat0=flat0, flat1=tr.flat.clone())


def test_trainer_step_against_fp64_forced_branches(step64):
    s = step64
    vw = M.load_vgg19_deep_weights()
    dec = s["rec"]["dec"]                      # one decoder pass: 8 ReLUs
    enc = s["rec"]["enc"][-12:]                # the last of three encoder passes: 9 + 3
    assert len(dec) == 8 and len(s["rec"]["enc"]) == 36
    c_np, s_np = s["content"].numpy(), s["style"].numpy()
    g64, l64 = R.forced_grads(s["sd0"], vw, c_np, s_np, dec, enc, torch.float64)
    g32, l32 = R.forced_grads(s["sd0"], vw, c_np, s_np, dec, enc, torch.float32)
    nd, ne = R.natural_branches(s["sd0"], vw, c_np, s_np)
    flips = R.count_flips(dec, nd) + R.count_flips(enc, ne)
    print(f"loss hip {s['loss']:.7g} fp64 {l64:.7g} fp32 {l32:.7g}; flips {flips}")
    assert s["loss"] == s["ev0"], "evaluate and step disagree on the same parameters"
    assert abs(s["loss"] - l64) <= max(K * abs(l32 - l64), 1e-4 * abs(l64))
    for k, t in g64.items():
        e, r = _rel(s["grads"][k], t), _rel(g32[k], t)
        print(f"{k}: hip {e:.2e} fp32 {r:.2e}")
        assert e <= max(K * r, FLOOR), f"{k}: hip {e:.2e} vs fp32 {r:.2e} (forced branches)"


def test_trainer_step_updates_and_is_reproducible(step64, dev):
    s = step64
    assert not torch.equal(s["flat1"], s["flat0"]), "the step must move the decoder"
    assert s["tr"].k == 1 and s["tr"].opt.lr == s["tr"].lr_at(0) == 1e-4
    assert s["tr"].lr_at(20000) == 1e-4 / 2
    net = M.AdaINNet(decoder_seed=11)
    tr = M.AdaINTrainer(net)
    loss = float(tr.step(s["content"], s["style"]))
    assert loss == s["loss"] and torch.equal(bits(tr.flat), bits(s["flat1"]))
    l2a = float(s["tr"].step(s["content"], s["style"]))
    l2b = float(tr.step(s["content"], s["style"]))
    assert l2a == l2b and torch.equal(bits(tr.flat), bits(s["tr"].flat))
    with pytest.raises(RuntimeError, match="no backward"):
        x = torch.randn(1, 4, 4, 4, device=dev, requires_grad=True)
        M.AdaINFn.apply(x, torch.zeros(1, 4, device=dev), torch.ones(1, 4, device=dev),
                        torch.ones(1, 1, device=dev), 1.0, EPS).sum().backward()


def test_cli_round_trip(tmp_path, monkeypatch, dev):
    """adain train --synthetic, then convert-image / convert-video in a scratch project root:
    the written PNG equals AdaINNet.forward + imshow byte for byte."""
    from click.testing import CliRunner
    from PIL import Image
    from styletransfer_amd import color, constants, img_utils, video_io
    from styletransfer_amd.clis import cli
    monkeypatch.setattr(constants, "PROJECT_ROOT_PATH", str(tmp_path))
    monkeypatch.setattr(constants, "IMSIZE", 64)
    rng = np.random.default_rng(0)
    for name, (h, w) in (("c.png", (72, 80)), ("a.png", (64, 64)), ("b.png", (90, 70))):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(tmp_path / name)
    run = lambda *a: CliRunner().invoke(cli, ["adain", *a], catch_exceptions=False)
    r = run("train", "styles", "-n", "t", "--synthetic", "8", "-e", "1", "-b", "2")
    assert r.exit_code == 0, r.output
    ckpt = tmp_path / "data" / "models" / "adain_t_epoch0.pth"
    assert ckpt.is_file()
    assert list(torch.load(ckpt, weights_only=True).keys()) == R.DECODER_KEYS
    r = run("train", "styles", "-n", "t", "--synthetic", "8", "-e", "1", "-b", "2")
    assert r.exit_code == 0 and ckpt.is_file()  # the epoch exists: loaded and skipped
    png = tmp_path / "results" / "converted_adain_t.png"

    def convert(*a):
        r = run("convert-image", "c.png", *a, "-n", "t")
        assert r.exit_code == 0, r.output
        return png.read_bytes()
    got = convert("a.png", "b.png", "--mix", "a.png:0.3,b.png:0.7", "--alpha", "0.5",
                  "--preserve-color")
    net = M.AdaINNet()
    net.load(str(ckpt))
    image = img_utils.image_loader(str(tmp_path / "c.png"))
    styles = [img_utils.image_loader(str(tmp_path / n)) for n in ("a.png", "b.png")]
    with torch.no_grad():
        out = net(image, styles, mix=[0.3, 0.7], alpha=0.5)
    img_utils.imshow(color.merge_luminance(out, image), path=str(tmp_path / "ref.png"))
    assert got == (tmp_path / "ref.png").read_bytes()
    # alpha = 1 with a one-hot mix is the single-style run
    onehot = convert("a.png", "b.png", "--mix", "b.png:1")
    single = convert("b.png")
    assert onehot == single and onehot != got
    # a 4-frame clip to MJPEG
    np.save(tmp_path / "clip.npy", rng.integers(0, 256, (4, 72, 80, 3), dtype=np.uint8))
    r = run("convert-video", "clip.npy", "a.png", "-n", "t", "--format", "mjpeg")
    assert r.exit_code == 0, r.output
    fps, h, w, frames = video_io.read_mjpeg_avi(str(tmp_path / "results" / "adain_t.avi"))
    assert (h, w) == (64, 64) and len(list(frames)) == 4
