"""The InstanceNorm kernels (instnorm.hip: nine forward / backward variants behind
stx_instnorm_fwd / stx_instnorm_bwd) against the fp64 reference of tests/instnorm_ref.py,
element by element, on every variant at the plane sizes where the dispatch or a kernel's
own code changes path, with data that a norm ratio forgives: end-of-plane markers, planes
whose mean dwarfs their spread, a constant plane, var << eps, and planes full of elements
that sit on the ReLU threshold.

Bounds come from the code, not from a run (u = 2^-24; L the longest serial fp32 chain one
thread and the block tree add, restated per variant by chain_fwd / chain_bwd; never looser
than 2^-16):
  mean   (L + 16) u sum|u| / hw                                               = B_mean
  var    (L + 20) u var + B_mean^2   (sum(u - m) = 0: the mean's error enters squared)
  rstd   rstd (B_var / 2 (var + eps) + 4u)   (divide and sqrtf correctly rounded)   = B_rstd
  y      (r + 1) u (|u gsc| + |sh|) + |gamma| (rstd B_mean + |u - mean| B_rstd),  r = 3:
         gsc = gamma rstd, sh = fma(-mean, gsc, beta), y = fma(u, gsc, sh)
  sums   sg, sgx, sum du: (L + 16) u sum|terms|  (sum du: + the sum of its terms' bounds)
  du     (r + 1) u |k| (hw|g| + |sg| + |xh sgx|) + |k| (B_sg + |xh| B_sgx + |sgx| 2u|xh|),
         r = 7: k = gamma rstd / hw (2), hw g, xh sgx, the two subtractions, the product
         with k; the two roundings of xh = (u - mean) rstd are the last term
  dgamma, dbeta, dbias_in   sum over n of the plane bounds + (n + 1) u sum|parts|
         (+ u (|old| + |sum|) when accumulated)
The backward reference takes mean and rstd from the HIP forward and its ReLU mask from the
HIP forward's y > 0: a backward whose recomputed decision differs anywhere is an
O(|k| hw |dy|) error there (dy is non-zero everywhere) and fails the du bound.  Maxima
(out_amax) are exact; every call runs twice and must give the same bits.  The last section
pins where a NaN or Inf must come out."""
import functools

import numpy as np
import pytest
import torch

import instnorm_ref as R
from styletransfer_amd import _native as N
from styletransfer_amd import ops

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
CAP = 2.0 ** -16
EPS = float(np.float32(1e-5))
SLOTS = N.STX_AMAX_SLOTS
NAN, INF = float("nan"), float("inf")


def cdiv(a, b):
    return -(-a // b)


# ======================================================================= the dispatch
def piped(hw, planes):  # four 64^2 planes per block where that leaves >= 256 blocks
    return hw == 4096 and planes % 4 == 0 and planes // 4 >= 256


def fwd_variant(hw, planes):
    """stx_instnorm_fwd's kernel choice."""
    if piped(hw, planes):
        return "pipe"
    if hw % 4 == 0:
        for nt, r4 in ((512, 2), (256, 16), (1024, 16)):
            if hw <= 4 * nt * r4:
                return f"reg{nt}x{r4}"
    nt = 1024 if hw >= 4 * 1024 * 4 else 256
    return f"loop{nt}_vec" if hw % 4 == 0 else f"loop{nt}_scalar"


def bwd_variant(hw, planes, relu, res, aligned=True):
    """stx_instnorm_bwd's kernel choice (STX_IN_GREG at its default)."""
    al = aligned and hw % 4 == 0
    if al and piped(hw, planes):
        return "pipe"
    if al and hw <= 4 * 512 * 2:
        return "reg512x2"
    if al and hw <= 4 * 256 * 16:
        return "reg256x16"
    if al and hw <= 4 * 512 * 32 and relu and not res:
        return "greg"
    nt = 1024 if hw >= 4 * 1024 * 4 else 256
    return f"loop{nt}_vec" if al else f"loop{nt}_scalar"


def tree(nt):  # wave butterfly (6 adds), then the NT / 64 wave sums in order
    return 6 + nt // 64


def reg_shape(v):
    nt, r4 = v[3:].split("x")
    return int(nt), int(r4)


def chain_fwd(v, hw):
    """Sum and squared-deviation chains of the forward kernels."""
    if v == "pipe":
        v = "reg512x2"
    if v.startswith("reg"):  # R4 float4 groups, each (a + b) + (c + d), added in order
        nt, r4 = reg_shape(v)
        return r4 + 2 + tree(nt)
    nt = int(v[4:].split("_")[0])
    if v.endswith("vec"):  # one float4 group per trip
        return cdiv(hw // 4, nt) + 2 + tree(nt)
    return cdiv(hw, nt) + tree(nt)  # scalar: one element per trip


def chain_bwd(v, hw):
    """(chain of sg and sgx, chain of sum du) of the backward kernels."""
    if v == "pipe":
        v = "reg512x2"
    if v.startswith("reg") or v == "greg":  # sg, sgx element by element; sum du by float4
        nt, r4 = (512, 32) if v == "greg" else reg_shape(v)
        return 4 * r4 + tree(nt), r4 + 2 + tree(nt)
    nt = int(v[4:].split("_")[0])
    L = (4 * cdiv(hw // 4, nt) if v.endswith("vec") else cdiv(hw, nt)) + tree(nt)
    return L, L  # the loop kernels add all three element by element


# ======================================================================= data
def kind_of(i, ch, n, c):
    """The data kind of plane (i, ch): every call mixes all five, kinds by channel (ties
    need beta = 0), and exactly one constant plane among non-constant ones."""
    if c == 3:
        return (("signed", "offset", "ties"), ("tiny", "constant", "ties"))[i % 2][ch]
    if ch == 4 and i == min(1, n - 1):
        return "constant"
    return ("signed", "offset", "tiny", "ties", "signed")[ch % 5]


def tie_channels(c):
    ch = np.arange(c)
    return ch == 2 if c == 3 else ch % 5 == 3


@functools.lru_cache(maxsize=4)
def inputs(n, c, hw, res):
    """x, res, dy as CPU [n][c][hw] and the kind of each plane [n*c].  u = x (+ res):
      signed    uniform in [-1, 1] with exact zeros and equal pairs, and +-8 at the first
                float, the first float of the last float4 and the last float of the plane
                (a dropped or doubled end element moves the mean by far more than B_mean)
      offset    64 + N(0, 1) / 2: a one-pass variance fails here
      tiny      2 + 1e-4 N(0, 1): var << eps
      constant  0.7 (0.7 + 0.2 with res)
      ties      m + 0.3 {-1, 0, 1} with as many +1 as -1: a third of the plane has u = mean
                up to rounding, so y there is the residual of fma(mean, gsc, fl(-mean gsc))
    dy is non-zero everywhere: +-[0.25, 1]."""
    g = torch.Generator().manual_seed(9000 + 7 * hw + 13 * n * c + int(res))
    kinds = np.array([kind_of(i, ch, n, c) for i in range(n) for ch in range(c)])
    x = torch.empty(n * c, hw)
    r = torch.zeros(n * c, hw) if res else None
    for kind in sorted(set(kinds)):
        idx = torch.from_numpy(np.flatnonzero(kinds == kind))
        m = idx.numel()
        if kind == "signed":
            xs = torch.rand(m, hw, generator=g) * 2 - 1
            f = xs.view(-1)
            f[5::53] = 0.0
            f[7::61] = f[6::61][:f[7::61].numel()]
            xs[:, 0] = 8.0
            xs[:, 4 * ((hw - 1) // 4)] = 8.0
            xs[:, -1] = -8.0
            rs = torch.rand(m, hw, generator=g) - 0.5
        elif kind == "offset":
            xs = 64 + 0.5 * torch.randn(m, hw, generator=g)
            rs = 0.25 * torch.randn(m, hw, generator=g)
        elif kind == "tiny":
            xs = 2 + 1e-4 * torch.randn(m, hw, generator=g)
            rs = 1e-5 * torch.randn(m, hw, generator=g)
        elif kind == "constant":
            xs, rs = torch.full((m, hw), 0.7), torch.full((m, hw), 0.2)
        else:
            k = hw // 3
            t = torch.zeros(m, hw)
            t[:, :k], t[:, k:2 * k] = 1.0, -1.0
            t = torch.gather(t, 1, torch.argsort(torch.rand(m, hw, generator=g), dim=1))
            mid = (0.9 + 0.37 * (idx % 5).float())[:, None].expand(m, hw)
            xs, rs = (mid, 0.3 * t) if res else (mid + 0.3 * t, None)
        x[idx] = xs
        if res:
            r[idx] = rs
    dy = (0.25 + 0.75 * torch.rand(n * c, hw, generator=g)) * \
        (torch.randint(0, 2, (n * c, hw), generator=g) * 2 - 1)
    shape = (n, c, hw)
    return x.view(shape), (r.view(shape) if res else None), dy.view(shape), kinds


@functools.lru_cache(maxsize=None)
def affine(c):
    """A distinct gamma (of either sign) and beta per channel; beta = 0 where ties live."""
    ch = np.arange(c)
    gamma = np.where(ch % 2 == 0, 1.0, -1.0) * (0.5 + (ch % 97) / 64 + ch / 4096)
    beta = ((ch * 37) % 101 - 50) / 40 + ch / 8192
    beta[tie_channels(c)] = 0.0
    return torch.from_numpy(gamma).float(), torch.from_numpy(beta).float()


@functools.lru_cache(maxsize=4)
def ref_fwd(n, c, hw, res, aff):
    x, r, _, _ = inputs(n, c, hw, res)
    gamma, beta = affine(c) if aff else (None, None)
    return R.fwd(x.numpy(), None if gamma is None else gamma.numpy(),
                 None if beta is None else beta.numpy(),
                 res=None if r is None else r.numpy(), eps=1e-5)


# ======================================================================= checks
def held(got, ref, bound, what, rat):
    """|got - ref| <= bound everywhere (a NaN fails); notes the worst error / bound."""
    got = got.detach().cpu().double().numpy().reshape(np.shape(ref))
    ref = np.asarray(ref, dtype=np.float64)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), ref.shape)
    err = np.abs(got - ref)
    bad = ~(err <= bound)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / bound)
    rat[what] = max(rat.get(what, 0.0), float(q.max()))
    if bad.any():
        i = int(np.argmax(np.where(bad, q, 0.0)))
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {bad.size} beyond the bound; at {i} got "
            f"{got.ravel()[i]:.9g} ref {ref.ravel()[i]:.9g} error {err.ravel()[i]:.3e} "
            f"bound {bound.ravel()[i]:.3e}")


def same_bits(fn):
    a, b = fn(), fn()
    for s, t in zip(a, b):
        assert torch.equal(s.view(torch.int32), t.view(torch.int32)), \
            "not bit-reproducible run to run"
    return a


def amax_is(am, t, what):
    assert float(am.max()) == float(t.abs().max()), what


def one_float_in(t, dev):
    """t as a contiguous view one float into a longer device buffer (4-byte aligned)."""
    buf = torch.empty(t.numel() + 5, device=dev)
    buf[1:1 + t.numel()] = t.reshape(-1).to(dev)
    v = buf[1:1 + t.numel()].view(t.shape)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def own_workspace(monkeypatch):
    """A scratch buffer of the test's own in place of ops.WS: the backward's per-plane
    partials (sgx, sg, sum du) are read back from it."""
    ws = ops._Workspace()
    monkeypatch.setattr(ops, "WS", ws)
    return ws


def parts_of(ws, n, c):
    (buf,) = ws.buf.values()
    return buf[:12 * n * c].view(torch.float32).view(n, c, 3).clone()


def fwd_bounds(f, gamma, L):
    """(B_mean, B_rstd, B_y) of the docstring for the reference f."""
    assert (L + 20) * U <= CAP, L
    ga = 1.0 if gamma is None else np.abs(gamma.double().numpy())[None, :, None]
    b_mean = (L + 16) * U * f.absmean
    b_var = (L + 20) * U * f.var + b_mean ** 2
    b_rstd = f.rstd * (0.5 * b_var / (f.var + EPS) + 4 * U)
    b_y = 4 * U * f.ymag + ga * (f.rstd[..., None] * b_mean[..., None]
                                 + np.abs(f.u - f.mean[..., None]) * b_rstd[..., None])
    return b_mean, b_rstd, b_y


def bwd_bounds(b, Lsg, Lsdu):
    """(B_sg, B_sgx, B_du, B_sumdu) of the docstring for the reference b."""
    assert (max(Lsg, Lsdu) + 16) * U <= CAP, (Lsg, Lsdu)
    b_sg = (Lsg + 16) * U * b.sgmag
    b_sgx = (Lsg + 16) * U * b.sgxmag
    ak, axh = np.abs(b.k), np.abs(b.xh)
    b_du = 8 * U * ak * b.dumag + ak * (b_sg[..., None] + axh * b_sgx[..., None]
                                        + np.abs(b.sgx)[..., None] * 2 * U * axh)
    b_sdu = b_du.sum(axis=2) + (Lsdu + 16) * U * b.sdumag
    return b_sg, b_sgx, b_du, b_sdu


def run_case(dev, monkeypatch, n, c, hw, relu, res, aff=True, unaligned=None):
    """Forward and backward of one call against fp64; returns what the callers reuse."""
    x, r, dy, kinds = inputs(n, c, hw, res)
    gamma, beta = affine(c) if aff else (None, None)
    fv = fwd_variant(hw, n * c)
    bv = bwd_variant(hw, n * c, relu, res, aligned=unaligned is None)
    xd, dyd = x.to(dev), dy.to(dev)
    rd = r.to(dev) if res else None
    gd, bd = (gamma.to(dev), beta.to(dev)) if aff else (None, None)
    rat = {}

    # ---- forward (always on aligned bases: it refuses others)
    def forward():
        am = torch.zeros(SLOTS, device=dev)
        return ops.instnorm_fwd(xd, gd, bd, res=rd, relu=relu, out_amax=am) + (am,)

    y, mean, rstd, am = same_bits(forward)
    f = ref_fwd(n, c, hw, res, aff)
    b_mean, b_rstd, b_y = fwd_bounds(f, gamma, chain_fwd(fv, hw))
    held(mean, f.mean, b_mean, "mean", rat)
    held(rstd, f.rstd, b_rstd, "rstd", rat)
    held(y, np.where(f.y <= 0, 0.0, f.y) if relu else f.y, b_y, "y", rat)
    amax_is(am, y, "out_amax of y")
    mask = None
    if relu:
        # y_hip > 0 against y_ref > 0: they may differ only where |y_ref| <= B_y, on at
        # most 0.2 % of the elements -- except on planes that sit on the threshold: the
        # tie planes, and a constant plane without beta (y_ref = 0 exactly)
        mask = (y > 0).cpu().numpy()
        b0 = np.zeros(c) if beta is None else beta.numpy()
        free = (kinds == "ties") | (((kinds == "constant") | (hw == 1)) & (np.tile(b0, n) == 0))
        keep = ~free.reshape(n, c)
        diff = (mask != (f.y > 0))[keep]
        assert np.all(np.abs(f.y[keep][diff]) <= b_y[keep][diff]), "a ReLU decision off the edge"
        assert diff.sum() <= 0.002 * diff.size, (int(diff.sum()), diff.size)
        rat["flips %"] = 100.0 * diff.sum() / max(diff.size, 1)

    # ---- backward, from the HIP forward's mean, rstd and ReLU decisions
    ws = own_workspace(monkeypatch)
    if unaligned == "x":
        xd = one_float_in(x, dev)
    elif unaligned == "dy":
        dyd = one_float_in(dy, dev)
    elif unaligned == "res":
        rd = one_float_in(r, dev)

    def backward():
        am = torch.zeros(SLOTS, device=dev)
        du = ops.instnorm_bwd(dyd, bd, xd, rd, gd, mean, rstd, relu=relu, out_amax=am)
        return du, parts_of(ws, n, c), am

    du, parts, am = same_bits(backward)
    b = R.bwd(dy.numpy(), x.numpy(), None if gamma is None else gamma.numpy(),
              mean.cpu().numpy().reshape(n, c), rstd.cpu().numpy().reshape(n, c),
              res=None if r is None else r.numpy(), mask=mask)
    b_sg, b_sgx, b_du, b_sdu = bwd_bounds(b, *chain_bwd(bv, hw))
    held(du, b.du, b_du, "du", rat)
    held(parts[..., 0], b.sgx, b_sgx, "sgx", rat)
    held(parts[..., 1], b.sg, b_sg, "sg", rat)
    held(parts[..., 2], b.sdu, b_sdu, "sum du", rat)
    amax_is(am, du, "out_amax of du")
    print(f"{n}x{c} hw {hw} relu {int(relu)} res {int(res)} fwd {fv} bwd {bv}: err/bound "
          + " ".join(f"{k} {v:.3f}" for k, v in rat.items()))
    return SimpleCase(dev=dev, x=xd, r=rd, dy=dyd, gamma=gd, beta=bd, mean=mean, rstd=rstd,
                      y=y, du=du, parts=parts, ref=b, bounds=(b_sg, b_sgx, b_du, b_sdu))


class SimpleCase:
    def __init__(self, **kw):
        self.__dict__.update(kw)


# ======================================================================= every variant
def nc_for(hw):
    """39 planes where they fit (the 32 amax slots wrap; plane % c is not plane % 32)."""
    return (3, 13) if hw <= 16388 else (2, 3)


# hw -> the rows of the dispatch it is the edge of
SIZES = [
    4, 2052, 4092, 4096,            # reg<512,2>: one float4, R4 step 2 begins, last, full
    4100, 16380, 16384,             # reg<256,16>
    16388, 65532, 65536,            # fwd reg<1024,16>; bwd greg or loop<1024> vector
    28672, 28676,                   # greg's last register step / first LDS step (GREG_XL)
    65540,                          # loop kernels, vector
    1, 3, 63, 4097, 16385, 65537,   # loop kernels, scalar (bwd: <256> below 16384 floats)
]


def case_id(n, c, hw, relu, res, aligned=True):
    return (f"{n}x{c}-hw{hw}-relu{int(relu)}-res{int(res)}-fwd_{fwd_variant(hw, n * c)}"
            f"-bwd_{bwd_variant(hw, n * c, relu, res, aligned)}")


CASES = [(*nc_for(hw), hw, relu, res) for hw in SIZES
         for relu in (False, True) for res in (False, True)]
# the pipelined 64^2 kernels (256 and 257 blocks of four planes: the amax slots wrap) and
# their neighbours that must not take them: 1026 planes (no multiple of 4), 1020 (255 blocks)
PIPE_CASES = [(n, c, 4096, relu, res) for n, c in ((8, 128), (4, 257), (2, 513), (4, 255))
              for relu in (False, True) for res in (False, True)]


def test_the_table_is_covered():
    """Every variant of both entry points is among the ids below."""
    fwd = {fwd_variant(hw, n * c) for n, c, hw, _, _ in CASES + PIPE_CASES}
    bwd = {bwd_variant(hw, n * c, relu, res) for n, c, hw, relu, res in CASES + PIPE_CASES}
    assert fwd == {"pipe", "reg512x2", "reg256x16", "reg1024x16", "loop1024_vec",
                   "loop1024_scalar", "loop256_scalar"}
    assert bwd == {"pipe", "reg512x2", "reg256x16", "greg", "loop1024_vec", "loop1024_scalar",
                   "loop256_scalar"}
    assert bwd_variant(28672, 6, True, False) == "greg" == bwd_variant(65536, 6, True, False)
    assert bwd_variant(65540, 6, True, False) == "loop1024_vec"
    assert fwd_variant(4096, 1026) == "reg512x2" == fwd_variant(4096, 1020)
    assert max(n * c * hw for n, c, hw, _, _ in CASES + PIPE_CASES) <= 1028 * 4096


@pytest.mark.parametrize("n,c,hw,relu,res", CASES, ids=[case_id(*k) for k in CASES])
def test_instnorm_vs_fp64(dev, monkeypatch, n, c, hw, relu, res):
    run_case(dev, monkeypatch, n, c, hw, relu, res)


@pytest.mark.parametrize("n,c,hw,relu,res", PIPE_CASES, ids=[case_id(*k) for k in PIPE_CASES])
def test_instnorm_64x64_planes_vs_fp64(dev, monkeypatch, n, c, hw, relu, res):
    run_case(dev, monkeypatch, n, c, hw, relu, res)


UNALIGNED = [(3, 13, hw, which) for hw in (4096, 16384) for which in ("x", "dy", "res")]


@pytest.mark.parametrize("n,c,hw,which", UNALIGNED, ids=[
    f"{case_id(n, c, hw, True, True, aligned=False)}-unaligned_{w}" for n, c, hw, w in UNALIGNED])
def test_instnorm_bwd_unaligned_vs_fp64(dev, monkeypatch, n, c, hw, which):
    """A base that is not 16-byte aligned sends the backward to the loop kernel's scalar
    path (<256> at 4096 floats, <1024> at 16384); mean and rstd come from an aligned
    forward of the same values."""
    run_case(dev, monkeypatch, n, c, hw, True, True, unaligned=which)


def test_instnorm_fwd_refuses_unaligned_bases(dev):
    x = torch.zeros(2, 3, 64, device=dev)
    un = one_float_in(torch.zeros(2, 3, 64), dev)
    g, b = torch.ones(3, device=dev), torch.zeros(3, device=dev)
    for kw in (dict(x=un), dict(x=x, res=un), dict(x=x, out=un)):
        with pytest.raises(N.NativeError, match="alignment"):
            ops.instnorm_fwd(kw.pop("x"), g, b, **kw)


# one call per forward and per backward variant
NO_AFFINE = [(3, 13, 2052, True, True), (3, 13, 4100, True, False), (2, 3, 16388, True, False),
             (2, 3, 65540, False, True), (3, 13, 63, True, True), (3, 13, 16385, True, False),
             (4, 257, 4096, True, True)]


@pytest.mark.parametrize("n,c,hw,relu,res", NO_AFFINE, ids=[case_id(*k) for k in NO_AFFINE])
def test_instnorm_without_affine_vs_fp64(dev, monkeypatch, n, c, hw, relu, res):
    """gamma = beta = None: gsc = rstd, sh = -mean rstd, k = rstd / hw."""
    run_case(dev, monkeypatch, n, c, hw, relu, res, aff=False)


def test_pipelined_kernels_have_the_one_plane_kernels_bits(dev, monkeypatch):
    """instnorm.hip says the pipelined 64^2 kernels do the one-plane kernels' arithmetic in
    the same order: 1024 planes in one call (256 blocks of four planes) against the same
    planes as calls of 1020 and 4 (reg<512,2>), bit for bit."""
    n, c, hw = 1, 1024, 4096
    assert fwd_variant(hw, 1024) == "pipe" and fwd_variant(hw, 1020) == fwd_variant(hw, 4) \
        == "reg512x2"
    x, r, dy, _ = inputs(n, c, hw, True)
    gamma, beta = affine(c)
    xd, rd, dyd, gd, bd = (t.to(dev) for t in (x, r, dy, gamma, beta))
    ws = own_workspace(monkeypatch)
    for relu in (False, True):
        for res in (None, rd):
            def call(lo, hi):
                s = slice(lo, hi)
                rr = None if res is None else res[:, s]
                y, mean, rstd = ops.instnorm_fwd(xd[:, s], gd[s], bd[s], res=rr, relu=relu)
                du = ops.instnorm_bwd(dyd[:, s], bd[s], xd[:, s], rr, gd[s], mean, rstd,
                                      relu=relu)
                return y, mean, rstd, du, parts_of(ws, 1, hi - lo)
            whole = call(0, 1024)
            a, b = call(0, 1020), call(1020, 1024)
            for name, w, p, q in zip(("y", "mean", "rstd", "du", "parts"), whole, a, b):
                both = torch.cat([p, q], dim=0 if name in ("mean", "rstd") else 1)
                assert torch.equal(w.view(torch.int32), both.view(torch.int32)), \
                    (name, relu, res is not None, int((w != both).sum()))


# ======================================================================= parameter gradients
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("absent", [None, "dgamma", "dbeta", "dbias_in"])
def test_instnorm_param_grads_vs_fp64(dev, monkeypatch, accumulate, absent):
    """dgamma / dbeta / dbias_in written and accumulated, with any one of them None.
    dbias_in is mathematically 0: its bound is absolute (the du bounds summed and the chain
    term on sum|du|)."""
    n, c, hw = 5, 13, 2052
    k = run_case(dev, monkeypatch, n, c, hw, True, False)
    b, (b_sg, b_sgx, _, b_sdu) = k.ref, k.bounds
    g = torch.Generator().manual_seed(77)
    old = {name: (torch.rand(c, generator=g) * 4 - 2) for name in ("dgamma", "dbeta", "dbias_in")}

    def call():
        out = {name: (None if name == absent else old[name].clone().to(dev)) for name in old}
        du = ops.instnorm_bwd(k.dy, k.beta, k.x, None, k.gamma, k.mean, k.rstd, relu=True,
                              accumulate=accumulate, **out)
        assert torch.equal(du, k.du)
        return [t for t in out.values() if t is not None], out

    same_bits(lambda: call()[0])
    out = call()[1]
    rat = {}
    for name, plane_bound in (("dgamma", b_sgx), ("dbeta", b_sg), ("dbias_in", b_sdu)):
        if name == absent:
            continue
        ref, mag = getattr(b, name), getattr(b, name + "_mag")
        bound = plane_bound.sum(axis=0) + (n + 1) * U * mag
        if accumulate:
            o = old[name].double().numpy()
            bound = bound + U * (np.abs(o) + np.abs(ref))
            ref = ref + o
        held(out[name], ref, bound, name, rat)
    print(f"param grads accumulate {int(accumulate)} without {absent}: err/bound "
          + " ".join(f"{k} {v:.3f}" for k, v in rat.items()))


def test_param_grad_batch_past_its_job_table(dev):
    """33 accumulating backward calls inside a step: one more than STX_PGRAD_MAX, so the
    batch launches twice (32 jobs when the table fills, the last at flush()); bit-equal to
    the same calls made outside a step, for channel counts that mix within a launch."""
    assert N.STX_PGRAD_MAX == 32
    n, hw = 2, 36
    g = torch.Generator().manual_seed(78)
    calls = []
    for i in range(N.STX_PGRAD_MAX + 1):
        c = (3, 13, 64)[i % 3]
        x = (torch.rand(n, c, hw, generator=g) * 2 - 1).to(dev)
        dy = (torch.rand(n, c, hw, generator=g) * 2 - 1).to(dev)
        gamma = (torch.rand(c, generator=g) + 0.5).to(dev)
        beta = (torch.rand(c, generator=g) - 0.5).to(dev)
        _, mean, rstd = ops.instnorm_fwd(x, gamma, beta, relu=True)
        old = [(torch.rand(c, generator=g) - 0.5).to(dev) for _ in range(3)]
        calls.append((dy, beta, x, gamma, mean, rstd, old))

    def run():
        outs = []
        for dy, beta, x, gamma, mean, rstd, old in calls:
            dg, db, dbi = (t.clone() for t in old)
            ops.instnorm_bwd(dy, beta, x, None, gamma, mean, rstd, relu=True, dgamma=dg,
                             dbeta=db, dbias_in=dbi, accumulate=True)
            outs += [dg, db, dbi]
        return outs

    eager = run()
    assert not torch.equal(eager[0], calls[0][-1][0])
    ops.PGRADS.begin()
    try:
        batched = run()
        assert len(ops.PGRADS.jobs) == 1  # 32 went out when the table filled
        assert torch.equal(batched[-1], calls[-1][-1][2])  # the 33rd is still deferred
        ops.PGRADS.flush()
    finally:
        ops.PGRADS.active = False
        ops.PGRADS.jobs, ops.PGRADS.keep = [], []
    for i, (a, b) in enumerate(zip(eager, batched)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (i // 3, i % 3)


# ======================================================================= NaN and Inf
# (n, c, hw, the poisoned plane): one shape per variant; the pipelined kernels share a
# block among four planes, so theirs sits in the middle of one
NAN_FWD = [(2, 3, 2052, 1), (2, 3, 4100, 1), (2, 3, 16388, 1), (2, 3, 65540, 1), (2, 3, 63, 1),
           (2, 3, 16385, 1), (8, 128, 4096, 4 * 100 + 2)]


def rest_equal(a, b, p, what):
    """Every plane but p has the same bits in a and b."""
    a, b = a.reshape(a.shape[0] * a.shape[1], -1), b.reshape(a.shape[0] * a.shape[1], -1)
    keep = torch.arange(a.shape[0], device=a.device) != p
    assert torch.equal(a[keep].view(torch.int32), b[keep].view(torch.int32)), what


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("n,c,hw,p", NAN_FWD,
                         ids=[f"{n}x{c}-hw{hw}-fwd_{fwd_variant(hw, n * c)}" for n, c, hw, _ in NAN_FWD])
def test_nan_or_inf_in_a_plane_comes_out_of_the_forward(dev, n, c, hw, p, relu):
    """One NaN (then one +Inf) in plane p makes its mean NaN (Inf for +Inf), its rstd, gsc
    and sh NaN and so every y of the plane, under the ReLU too (y <= 0 ? 0 : y keeps a NaN;
    fmaxf(NaN, 0) = 0 handed on a clean zero plane with out_amax = 0); out_amax holds a
    NaN; every other plane keeps the bits of the clean call."""
    x, _, _, _ = inputs(n, c, hw, False)
    gamma, beta = (t.to(dev) for t in affine(c))
    xd = x.to(dev)

    def run(t):
        am = torch.zeros(SLOTS, device=dev)
        return ops.instnorm_fwd(t, gamma, beta, relu=relu, out_amax=am) + (am,)

    y0, mean0, rstd0, am0 = run(xd)
    assert not torch.isnan(am0).any()
    for bad in (NAN, INF):
        for at in (0, hw // 2, hw - 1):
            t = xd.clone()
            t.view(n * c, hw)[p, at] = bad
            y, mean, rstd, am = run(t)
            what = f"{bad} at {at}"
            assert torch.isnan(y.view(n * c, hw)[p]).all(), what
            assert torch.isnan(mean[p]) if bad != bad else float(mean[p]) == INF, what
            assert torch.isnan(rstd[p]), what
            assert torch.isnan(am).any(), what
            rest_equal(y, y0, p, what)
            rest_equal(mean.view(n, c), mean0.view(n, c), p, what)
            rest_equal(rstd.view(n, c), rstd0.view(n, c), p, what)


# (n, c, hw, relu, res, p): one shape per backward variant
# (plane 1 of the 2 x 3 calls is an offset plane whose ReLU lets a quarter through)
NAN_BWD = [(2, 3, 2052, True, True, 1), (2, 3, 4100, False, False, 1), (2, 3, 16388, True, False, 1),
           (2, 3, 16388, False, True, 1), (2, 3, 63, True, False, 1), (2, 3, 16385, True, True, 1),
           (8, 128, 4096, True, True, 4 * 100 + 2)]


@pytest.mark.parametrize("n,c,hw,relu,res,p", NAN_BWD, ids=[case_id(*k[:5]) for k in NAN_BWD])
def test_nan_in_dy_comes_out_of_the_backward(dev, monkeypatch, n, c, hw, relu, res, p):
    """One NaN in dy of plane p (at an element the ReLU lets through): sg and sgx of the
    plane are NaN, so its whole du, its three partials, its channel of dgamma / dbeta /
    dbias_in and out_amax; every other plane and channel keeps the clean call's bits."""
    x, r, dy, _ = inputs(n, c, hw, res)
    gamma, beta = (t.to(dev) for t in affine(c))
    xd, dyd = x.to(dev), dy.to(dev)
    rd = r.to(dev) if res else None
    y, mean, rstd = ops.instnorm_fwd(xd, gamma, beta, res=rd, relu=relu)
    open_ = torch.nonzero(y.view(n * c, hw)[p] > 0).view(-1)
    assert open_.numel() > 0
    at = int(open_[open_.numel() // 2])
    ws = own_workspace(monkeypatch)

    def run(d):
        am = torch.zeros(SLOTS, device=dev)
        pg = [torch.zeros(c, device=dev) for _ in range(3)]
        du = ops.instnorm_bwd(d, beta, xd, rd, gamma, mean, rstd, relu=relu, dgamma=pg[0],
                              dbeta=pg[1], dbias_in=pg[2], out_amax=am)
        return du, parts_of(ws, n, c), torch.stack(pg), am

    du0, parts0, pg0, am0 = run(dyd)
    assert not torch.isnan(am0).any() and not torch.isnan(pg0).any()
    d = dyd.clone()
    d.view(n * c, hw)[p, at] = NAN
    du, parts, pg, am = run(d)
    assert torch.isnan(du.view(n * c, hw)[p]).all()
    assert torch.isnan(parts.view(n * c, 3)[p]).all()
    assert torch.isnan(pg[:, p % c]).all() and torch.isnan(am).any()
    rest_equal(du, du0, p, "du")
    rest_equal(parts, parts0, p, "parts")
    rest_equal(pg.t()[None], pg0.t()[None], p % c, "parameter gradients")


@pytest.mark.parametrize("n,c,hw,relu,res,p", NAN_BWD, ids=[case_id(*k[:5]) for k in NAN_BWD])
def test_nan_in_x_makes_the_backward_plane_nan(dev, n, c, hw, relu, res, p):
    """A NaN in x reaches the backward through the saved mean and rstd (both NaN): the
    ReLU's recomputed !(NaN > 0) gives g = 0 on the whole plane, but k = gamma rstd / hw is
    NaN and du = k (...) is NaN at every element of the plane, with and without relu
    (include/stx.h); the other planes keep their bits."""
    x, r, dy, _ = inputs(n, c, hw, res)
    gamma, beta = (t.to(dev) for t in affine(c))
    xd, dyd = x.to(dev), dy.to(dev)
    rd = r.to(dev) if res else None

    def run(t):
        _, mean, rstd = ops.instnorm_fwd(t, gamma, beta, res=rd, relu=relu)
        return ops.instnorm_bwd(dyd, beta, t, rd, gamma, mean, rstd, relu=relu)

    du0 = run(xd)
    t = xd.clone()
    t.view(n * c, hw)[p, hw // 2] = NAN
    du = run(t)
    assert torch.isnan(du.view(n * c, hw)[p]).all()
    rest_equal(du, du0, p, "du")
