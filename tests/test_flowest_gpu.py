"""The optical-flow estimator (csrc/flowest.hip, video.FlowEstimator, gatys_video's
flows="auto") on the GPU, against the restatement tests/flowest_ref.py (pinned by
tests/test_flowest_host.py).

Bounds come from the expressions as include/stx.h writes them, not from a run (u = 2^-24;
the conventions of tests/test_flow_gpu.py):
  selections     bit-equal
  pointwise      |got - ref| <= (r + 1) u M, r the fp32 roundings along the longest path of
                 the expression (a constant rounded to fp32 counts as one), M the magnitude
                 sum of its terms
  estimator      three-way: max and RMS of |gpu - ref64| at most 2.5 x those of
                 |ref32 - ref64|, ref32 the restatement run at fp32 in the header's order"""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import flow_ref as R
import flowest_ref as E
import test_flow_gpu as TF
from styletransfer_amd import _native as N
from styletransfer_amd import constants, ops, video

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
SHAPES = [(1, 5, 7), (2, 64, 64), (1, 129, 67), (1, 96, 160)]  # (n, h, w)
IDS = ["x".join(map(str, s)) for s in SHAPES]
MAXFUSE = N.STX_FLOW_JACOBI_MAXFUSE

_np, _rand, within, bits = TF._np, TF._rand, TF.within, TF.bits


def _to(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


# =============================================================================== luma
LUMA_R = 6  # a channel: its fmaf (1), its coefficient in fp32 (1), the three roundings of
#             the sum (3), the product by 255 (1)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_luma(dev, shape):
    """Within (6 + 1) u M, M = 255 sum_k coef_k (|x_k| std_k + mean_k); a batch equals its
    images alone, a misaligned base (the scalar path) equals the aligned one, bit for bit."""
    n, h, w = shape
    img = _rand((n, 3, h, w), 61, -2.5, 2.5)
    ref = E.luma(img)
    mag = 255.0 * sum(k * (np.abs(img[:, c].astype(np.float64)) * float(E.STD[c]) + float(E.MEAN[c]))
                      for c, k in enumerate((0.299, 0.587, 0.114)))
    d = _to(img, dev)
    got = ops.flow_luma(d)
    within(_np(got), ref, (LUMA_R + 1) * U * mag, "luma")
    for b in range(n):
        assert torch.equal(bits(ops.flow_luma(d[b:b + 1].contiguous())), bits(got[b:b + 1]))
    assert torch.equal(bits(ops.flow_luma(TF.misaligned(d, dev))), bits(got))


# ========================================================================== linearize
LIN_R = 8   # Ix, Iy: a weight (3), a tap's difference (1; the half is exact), the sum (4)
LIN_RC = 10  # c: S(B) (7) and A - S(B) (1), or Ix / Iy (8), then the two fmaf (2)


def wild_flow(n, h, w):
    """The recipe's flow with NaN, +-inf and +-3e38 scattered over both channels."""
    f = TF.grid_flows(n, h, w)[0].copy()
    rng = np.random.default_rng(71)
    vals = np.array([np.nan, np.inf, -np.inf, 3e38, -3e38], np.float32)
    for k in range(max(h * w // 6, 10)):
        f[rng.integers(n), rng.integers(2), rng.integers(h), rng.integers(w)] = vals[k % 5]
    return f


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
@pytest.mark.parametrize("which", ["recipe", "large", "wild"])
def test_linearize_on_the_grid(dev, shape, which):
    """On 1/64-grid flows (exact coordinates) Ix, Iy within (8 + 1) u M and c within
    (10 + 1) u M of the fp64 restatement.  "large": flows up to the image size, most samples
    clamp.  "wild": NaN, +-inf and +-3e38 in the flow -- Ix and Iy there are the reference's
    clamped samples (c, which multiplies by the flow, is compared where the flow is finite
    and below 1e30).  A batch equals its images alone, bit for bit."""
    n, h, w = shape
    flow = wild_flow(n, h, w) if which == "wild" else TF.grid_flows(n, h, w)[which == "large"]
    a, b = _rand((n, h, w), 72, 0, 255), _rand((n, h, w), 73, 0, 255)
    ref, mag = E.linearize(a, b, flow, want_mag=True)
    with np.errstate(invalid="ignore"):
        tame = np.isfinite(flow).all(axis=1) & (np.abs(flow) < 1e30).all(axis=1)
        y, x = R.coords(flow)
        clamped = ~((y >= 0) & (y <= h - 1) & (x >= 0) & (x <= w - 1))
    if which == "large":
        assert clamped.mean() > 0.2
    if which == "wild":
        assert (~tame).sum() >= 8
    ad, bd, fd = _to(a, dev), _to(b, dev), torch.from_numpy(flow).to(dev)
    got = ops.flow_linearize(ad, bd, fd)
    g = _np(got)
    assert np.isfinite(g[:, :2]).all()
    within(g[:, :2], ref[:, :2], (LIN_R + 1) * U * mag[:, :2], f"linearize {which} Ix Iy")
    within(g[:, 2][tame], ref[:, 2][tame], (LIN_RC + 1) * U * mag[:, 2][tame],
           f"linearize {which} c")
    for k in range(n):
        alone = ops.flow_linearize(ad[k:k + 1].contiguous(), bd[k:k + 1].contiguous(),
                                   fd[k:k + 1].contiguous())
        assert torch.equal(bits(alone), bits(got[k:k + 1]))


# ============================================================================= jacobi
JAC_R = 12  # the longest path: ubar's edge sum (3), 1/6 in fp32 (1), its product (1), the
#             fmaf (1), a2 (1), a2 ubar (1), the outer fmaf (1), ru's fmaf and division (2),
#             the last product (1)


@functools.lru_cache(maxsize=None)
def jacobi_case(shape):
    n, h, w = shape
    coef = np.concatenate([_rand((n, 2, h, w), 81, -64, 64), _rand((n, 1, h, w), 82, -255, 255)], 1)
    return coef, _rand((n, 2, h, w), 83, -8, 8)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_one_jacobi_iteration(dev, shape):
    coef, uv = jacobi_case(shape)
    ref, mag = E.jacobi(coef, uv, 15.0, 1, want_mag=True)
    got = ops.flow_jacobi(_to(coef, dev), _to(uv, dev), alpha=15.0, iters=1)
    within(_np(got), ref, (JAC_R + 1) * U * mag, "one Jacobi iteration")


def jacobi_guarded(coef, uv, iters, fuse, dev):
    """stx_flow_jacobi into an output and a workspace that lie inside NaN-filled allocations;
    returns (out, the four guard bands)."""
    n, _, h, w = uv.shape
    G = 4096
    L = N.lib()
    need = L.stx_flow_jacobi_ws(n, h, w) // 4
    assert need == uv.numel()
    obuf = torch.full((G + uv.numel() + G,), float("nan"), device=dev)
    wbuf = torch.full((G + need + G,), float("nan"), device=dev)
    out, ws = obuf[G:G + uv.numel()].view(uv.shape), wbuf[G:G + need]
    N.check(L.stx_flow_jacobi(coef.data_ptr(), uv.data_ptr(), out.data_ptr(), n, h, w, 15.0, iters,
                              fuse, ws.data_ptr(), need * 4,
                              torch.cuda.current_stream().cuda_stream), "stx_flow_jacobi")
    return out, (obuf[:G], obuf[G + uv.numel():], wbuf[:G], wbuf[G + need:])


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
@pytest.mark.parametrize("iters", [1, 7, 8, 19, 40])
def test_fusion_changes_no_bit(dev, shape, iters):
    """fuse = 1, 2 and MAXFUSE equal the library's choice bit for bit; twice the same bits;
    a batch equals its images alone; uv_in is left as it was and nothing is written outside
    uv_out and the workspace."""
    n, h, w = shape
    coef, uv = (_to(t, dev) for t in jacobi_case(shape))
    uv0 = uv.clone()
    want = ops.flow_jacobi(coef, uv, iters=iters)
    assert bool(torch.isfinite(want).all())
    assert torch.equal(bits(ops.flow_jacobi(coef, uv, iters=iters)), bits(want))
    for fuse in (0, 1, 2, MAXFUSE):
        out, guards = jacobi_guarded(coef, uv, iters, fuse, dev)
        assert torch.equal(bits(out), bits(want)), fuse
        assert all(bool(torch.isnan(g).all()) for g in guards), fuse
    assert torch.equal(bits(uv), bits(uv0))
    for b in range(n):
        alone = ops.flow_jacobi(coef[b:b + 1].contiguous(), uv[b:b + 1].contiguous(), iters=iters)
        assert torch.equal(bits(alone), bits(want[b:b + 1]))


# ====================================================================== the estimator
CLIPS = [("translation", 48, 80), ("smooth", 48, 80), ("translation", 128, 160),
         ("smooth", 128, 160), ("smooth", 129, 67)]


@functools.lru_cache(maxsize=None)
def references(kind, h, w):
    A, B, f = E.clip(kind, h, w)
    return (A, B, f, np.concatenate(E.estimate_pair(B, A, np.float64)),
            np.concatenate(E.estimate_pair(B, A, np.float32)).astype(np.float64))


@pytest.mark.parametrize("kind,h,w", CLIPS, ids=[f"{k}-{h}x{w}" for k, h, w in CLIPS])
def test_estimator_three_way(dev, kind, h, w):
    """Per direction, max and RMS of |gpu - ref64| <= 2.5 x those of |ref32 - ref64|; the
    interior mean end-point error against the truth <= the reference's + 0.01 px."""
    A, B, f, ref64, ref32 = references(kind, h, w)
    est = video.FlowEstimator(h, w, dev)
    fwd, bwd = est.pair(_to(B, dev), _to(A, dev))
    got = np.concatenate([_np(fwd), _np(bwd)]).astype(np.float64)
    for k, name in enumerate(("fwd", "bwd")):
        dg, dr = np.abs(got[k] - ref64[k]), np.abs(ref32[k] - ref64[k])
        rms = lambda d: float(np.sqrt((d ** 2).mean()))
        print(f"{kind} {h}x{w} {name}: gpu max {dg.max():.3e} rms {rms(dg):.3e}; fp32 "
              f"restatement max {dr.max():.3e} rms {rms(dr):.3e}; ratios "
              f"{dg.max() / dr.max():.2f} {rms(dg) / rms(dr):.2f}")
        assert dg.max() <= 2.5 * dr.max() and rms(dg) <= 2.5 * rms(dr), name
    I = E.interior(f, h, w)
    e_gpu, e_ref = E.epe(got[1:], f)[I].mean(), E.epe(ref64[1:], f)[I].mean()
    print(f"interior EPE gpu {e_gpu:.4f} reference {e_ref:.4f}")
    assert e_gpu <= e_ref + 0.01


def test_estimator_replay_state_and_memory(dev):
    """Captured and replayed equals eager, bit for bit; a second pair on other frames
    leaves no trace of the first; pair allocates nothing."""
    h, w = 96, 80
    A, B, _ = E.clip("smooth", h, w)
    C_, D, _ = E.clip("translation", h, w, seed=3)
    a, b, c, d = (_to(t, dev) for t in (A, B, C_, D))
    est = video.FlowEstimator(h, w, dev)
    want_ab = [t.clone() for t in est.pair(a, b)]
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(dev)
    fwd, bwd = est.pair(c, d)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(dev) == before
    assert fwd.data_ptr() == est.fwd.data_ptr() and tuple(fwd.shape) == (1, 2, h, w)
    fresh = video.FlowEstimator(h, w, dev).pair(c, d)
    assert torch.equal(bits(fwd), bits(fresh[0])) and torch.equal(bits(bwd), bits(fresh[1]))
    assert not torch.equal(fwd, want_ab[0])
    # capture on static inputs, then replay on each pair
    x, y = torch.empty_like(a), torch.empty_like(a)
    graph = torch.cuda.CUDAGraph()
    with ops.graph_capture(graph):
        est.pair(x, y)
    for (p, q), want in (((a, b), want_ab), ((c, d), fresh)):
        x.copy_(p)
        y.copy_(q)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(est.fwd), bits(want[0]))
        assert torch.equal(bits(est.bwd), bits(want[1]))
    import gc
    assert not any(isinstance(o, torch.cuda.CUDAGraph) for o in gc.get_referents(est.__dict__))


# =========================================================================== workflow
@pytest.fixture(scope="module")
def feat(dev):
    from styletransfer_amd import vgg as V
    from styletransfer_amd import weights as W
    return V.VGGFeatures(W.vgg19_synthetic(TF.VGG_SEED, 5), dev)


def clip_frames():
    """3 grey frames 64 x 64: one texture seen through a window that moves by (2, 1) px
    (columns, rows) per frame, as tests/test_flow_gpu.py's clip does."""
    tex = E.texture(TF.H + 2 * TF.DY, TF.H + 2 * TF.DX, 4)
    return [torch.from_numpy(E.condition(tex[TF.DY * t:TF.DY * t + TF.H,
                                             TF.DX * t:TF.DX * t + TF.H])) for t in range(3)]


def test_workflow_auto_equals_estimated_flows(dev, feat):
    """gatys_video(flows="auto") = gatys_video(flows=estimate_flows(frames)), bit for bit
    (the first estimates between the frames' optimisations, the second up front); the flows
    are those of the clip: (2, 1) px per frame."""
    frames = clip_frames()
    style = TF._img(11)
    flows = video.estimate_flows(frames)
    assert flows[0].shape == (2, 2, TF.H, TF.H) and flows[0].dtype == np.float32
    core = (slice(None), slice(None), slice(12, -12), slice(12, -12))
    assert np.abs(flows[1][:, 0][core[0], core[2], core[3]].mean() - TF.DX) < 0.25
    assert np.abs(flows[1][:, 1][core[0], core[2], core[3]].mean() - TF.DY) < 0.25
    run = lambda fl: [y.clone() for y in video.gatys_video(feat, frames, style, fl, steps=5)]
    auto, given = run("auto"), run(flows)
    assert len(auto) == 3
    for t, (p, q) in enumerate(zip(auto, given)):
        assert bool(torch.isfinite(p).all()) and torch.equal(bits(p), bits(q)), t
    static = run("static")
    assert not torch.equal(auto[1], static[1])


def test_cli_auto_then_saved_flows(dev, tmp_path, monkeypatch):
    """--flow auto --save-flows f.npz, then --flow f.npz: identical PNGs."""
    from click.testing import CliRunner
    from PIL import Image
    from conftest import REPO
    from styletransfer_amd.clis import cli
    H = TF.H
    monkeypatch.setattr(constants, "PROJECT_ROOT_PATH", str(tmp_path))
    monkeypatch.setattr(constants, "IMSIZE", H)
    monkeypatch.chdir(tmp_path)
    mean = np.array(constants.IMAGENET_MEAN, np.float32).reshape(1, 3, 1, 1)
    std = np.array(constants.IMAGENET_STD, np.float32).reshape(1, 3, 1, 1)
    clip = np.concatenate([np.clip((f.numpy() * std + mean) * 255, 0, 255)
                           for f in clip_frames()])
    np.save(tmp_path / "clip.npy", np.ascontiguousarray(clip.transpose(0, 2, 3, 1)).astype(np.uint8))
    Image.open(os.path.join(REPO, "data", "styles", "picasso.jpg")).save(tmp_path / "style.jpg")
    common = ["gatys_video", "clip.npy", "style.jpg", "-s", "5", "-tw", "100"]
    r = CliRunner().invoke(cli, common + ["--flow", "auto", "--save-flows", "f.npz", "-o", "a"])
    assert r.exit_code == 0, r.output + repr(r.exception)
    f, b = video.load_flows(str(tmp_path / "f.npz"), 3, H)
    assert np.abs(f).max() > 0.5
    r = CliRunner().invoke(cli, common + ["--flow", "f.npz", "-o", "b"])
    assert r.exit_code == 0, r.output + repr(r.exception)
    r = CliRunner().invoke(cli, common + ["--flow", "auto", "-o", "c"])
    assert r.exit_code == 0, r.output + repr(r.exception)
    for i in range(3):
        pa, pb, pc = (np.asarray(Image.open(tmp_path / d / f"{i}.png")) for d in "abc")
        assert pa.shape == (H, H, 3) and np.array_equal(pa, pb) and np.array_equal(pa, pc), i
