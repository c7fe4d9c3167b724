"""Long-term consistency for gatys_video on the GPU: stx_flow_compose against
the existing flow ops (bit for bit) and against the fp64 restatement tests/longterm_ref.py
(pinned by tests/test_longterm_host.py), batched flow estimation, the engine's term, the
workflow and the command line.  Bounds and the margin rule are tests/test_flow_gpu.py's."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import flow_ref as R
import longterm_ref as LR
import test_flow_gpu as TF
from styletransfer_amd import _native as N
from styletransfer_amd import constants, ops, video
from styletransfer_amd import vgg as V
from styletransfer_amd import weights as W
from test_flow_gpu import U, WARP_R, _np, bits, sure, within

pytestmark = pytest.mark.gpu
IDS = ["x".join(map(str, s)) for s in LR.SHAPES]
COUNTS = [1, 2, 3, 4]


def _to(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@functools.lru_cache(maxsize=None)
def reference(shape, count):
    """(inputs, longterm_ref.compose of them): computed once, shared, never written."""
    case = LR.case(shape, count)
    return case, LR.compose(*case)


def device_case(shape, count, dev):
    (prevs, fwds, bwds, fill), _ = reference(shape, count)
    return [_to(p, dev) for p in prevs], [_to(f, dev) for f in fwds], \
        [_to(b, dev) for b in bwds], _to(fill, dev)


def chain_of_ops(prevs, fwds, bwds, fill):
    """(ref, cmask, init, which) as the composition of the existing ops: the torch.where
    chain over ops.flow_consistency and ops.flow_warp, nearest offset last so it wins."""
    n, c, h, w = prevs[0].shape
    ref = torch.zeros_like(prevs[0])
    init = ops.flow_warp(prevs[0], bwds[0], fill=fill)
    cmask = torch.zeros((n, h, w), device=ref.device)
    which = torch.full((n, h, w), 255, device=ref.device, dtype=torch.uint8)
    for q in reversed(range(len(prevs))):
        on = ops.flow_consistency(fwds[q], bwds[q]) != 0
        om = ops.flow_warp(prevs[q], bwds[q])
        ref = torch.where(on[:, None], om, ref)
        init = torch.where(on[:, None], om, init)
        cmask = torch.where(on, torch.ones_like(cmask), cmask)
        which = torch.where(on, torch.full_like(which, q), which)
    return ref, cmask, init, which


def same(got, want):
    for g, w_, name in zip(got, want, ("ref", "cmask", "init", "which")):
        if g.dtype == torch.uint8:
            assert torch.equal(g, w_), name
        else:
            assert torch.equal(bits(g), bits(w_)), name


# ================================================================================ compose
@pytest.mark.parametrize("shape", LR.SHAPES, ids=IDS)
@pytest.mark.parametrize("count", COUNTS)
def test_compose_equals_the_existing_ops(dev, shape, count):
    """ref, cmask, init and which bit for bit; at count 1 (cmask, init) are the short-term
    set-up's flow_consistency and flow_warp(fill), and ref is flow_warp's under the mask."""
    prevs, fwds, bwds, fill = device_case(shape, count, dev)
    got = ops.flow_compose(prevs, fwds, bwds, fill)
    same(got, chain_of_ops(prevs, fwds, bwds, fill))
    if count == 1:
        ref, cmask, init, _ = got
        assert torch.equal(bits(cmask), bits(ops.flow_consistency(fwds[0], bwds[0])))
        assert torch.equal(bits(init), bits(ops.flow_warp(prevs[0], bwds[0], fill=fill)))
        om = ops.flow_warp(prevs[0], bwds[0])
        assert torch.equal(bits(ref), bits(torch.where(cmask[:, None] != 0, om, torch.zeros_like(om))))
    # a batch equals its images alone
    for b in range(shape[0]):
        one = lambda ts: [t[b:b + 1].contiguous() for t in ts]
        alone = ops.flow_compose(one(prevs), one(fwds), one(bwds), fill[b:b + 1].contiguous())
        same(alone, [g[b:b + 1] for g in got])


@pytest.mark.parametrize("shape", LR.SHAPES, ids=IDS)
@pytest.mark.parametrize("count", COUNTS)
def test_compose_against_the_reference(dev, shape, count):
    """Where every offset's predicate is clear of its threshold (test_flow_gpu.sure; at most
    0.5 % of the pixels are not: test_longterm_host pins that on the reference alone): cmask
    and which equal the reference's; ref and init within (7 + 1) u sum|w_k a_k| (WARP_R)."""
    (prevs, fwds, bwds, fill), r = reference(shape, count)
    ok = np.logical_and.reduce([sure(q) for q in r["rs"]])
    assert (~ok).mean() <= 0.005, (~ok).mean()
    ref, cmask, init, which = (_np(t) for t in ops.flow_compose(*device_case(shape, count, dev)))
    assert set(np.unique(cmask)) <= {0.0, 1.0}
    assert np.array_equal(cmask[ok], r["cmask"][ok].astype(np.float32))
    assert np.array_equal(which[ok], r["which"][ok])
    okc = np.broadcast_to(ok[:, None], ref.shape)
    tol = (WARP_R + 1) * U * r["mag"]
    within(ref[okc], r["ref"][okc], tol[okc], "compose ref")
    # init: the selected warp, or the start (its own warp's magnitude, or the exact fill)
    _, _, mag0 = R.warp(prevs[0], bwds[0], want_mag=True)
    tol_init = np.where(r["cmask"][:, None] > 0, tol, (WARP_R + 1) * U * mag0)
    within(init[okc], r["init"][okc], tol_init[okc], "compose init")
    print(shape, count, "selected per offset",
          [int((which == q).sum()) for q in range(count)], "none", int((which == 255).sum()))


def read_by_unsettled(which, bwd, q):
    """The pixels of offset q's planes that a pixel still unsettled at q (which >= q, 255
    included) can read: bwd[q] at itself and its four neighbours, fwd[q] and prev[q] at the
    four taps of its source."""
    n, h, w = which.shape
    need = which >= q
    rb = need.copy()
    rb[:, 1:] |= need[:, :-1]
    rb[:, :-1] |= need[:, 1:]
    rb[:, :, 1:] |= need[:, :, :-1]
    rb[:, :, :-1] |= need[:, :, 1:]
    y, x = R.coords(bwd)
    with np.errstate(invalid="ignore"):
        valid = (y >= 0) & (y <= h - 1) & (x >= 0) & (x <= w - 1) & need
    y0 = np.minimum(np.floor(np.where(valid, y, 0)), h - 2).astype(np.int64)
    x0 = np.minimum(np.floor(np.where(valid, x, 0)), w - 2).astype(np.int64)
    rt = np.zeros_like(need)
    b = np.broadcast_to(np.arange(n)[:, None, None], need.shape)
    for dy in (0, 1):
        for dx in (0, 1):
            rt[b[valid], y0[valid] + dy, x0[valid] + dx] = True
    return rb, rt


@pytest.mark.parametrize("shape", LR.SHAPES[1:], ids=IDS[1:])
def test_compose_priority_and_early_exit(dev, shape):
    """A settled pixel looks at no later offset.  For every q >= 1, prev[q], fwd[q] and bwd[q]
    are set to NaN wherever no pixel that is still unsettled at q reads them (a pixel of
    another offset's region may read a settled pixel's planes: its neighbour's bwd in the
    boundary test, its source's taps), which covers most of the area settled before q: the
    outputs keep their bits.  Then a NaN in bwd[0] at a pixel hands it to offset 1."""
    count = 4
    (prevs, fwds, bwds, fill), _ = reference(shape, count)
    clean = ops.flow_compose(*device_case(shape, count, dev))
    which = _np(clean[3])
    prevs, fwds, bwds = ([a.copy() for a in t] for t in (prevs, fwds, bwds))
    for q in range(1, count):
        rb, rt = read_by_unsettled(which, bwds[q], q)
        settled = which < q
        assert (~rb & settled).sum() >= 0.5 * settled.sum() > 0, q
        assert (~rt & settled).sum() >= 0.25 * settled.sum(), q
        bwds[q][np.broadcast_to(~rb[:, None], bwds[q].shape)] = np.nan
        fwds[q][np.broadcast_to(~rt[:, None], fwds[q].shape)] = np.nan
        prevs[q][np.broadcast_to(~rt[:, None], prevs[q].shape)] = np.nan
    dirty = ops.flow_compose([_to(p, dev) for p in prevs], [_to(f, dev) for f in fwds],
                             [_to(b, dev) for b in bwds], _to(fill, dev))
    same(dirty, clean)
    # hand-over: a pixel of offset 0 that offset 1 would also take
    (prevs, fwds, bwds, fill), _ = reference(shape, 2)
    c1 = _np(ops.flow_consistency(_to(fwds[1], dev), _to(bwds[1], dev))) != 0
    b, i, j = np.argwhere((which == 0) & c1)[len(np.argwhere((which == 0) & c1)) // 2]
    bwd0 = bwds[0].copy()
    bwd0[b, 0, i, j] = np.nan
    d = device_case(shape, 2, dev)
    ref, cmask, init, wh = ops.flow_compose(d[0], d[1], [_to(bwd0, dev), d[2][1]], d[3])
    om1 = ops.flow_warp(d[0][1], d[2][1])
    assert int(wh[b, i, j]) == 1 and float(cmask[b, i, j]) == 1.0
    assert torch.equal(bits(ref[b, :, i, j]), bits(om1[b, :, i, j]))
    assert torch.equal(bits(init[b, :, i, j]), bits(om1[b, :, i, j]))


def test_compose_nan_in_a_selected_tap(dev):
    """A NaN in prev[q] at a tap of a selected pixel makes ref and init NaN there; the same
    NaN at an offset that is not selected there reaches nothing."""
    shape = LR.SHAPES[2]
    (prevs, fwds, bwds, fill), r = reference(shape, 2)
    clean = ops.flow_compose(*device_case(shape, 2, dev))
    which = _np(clean[3])
    y, x = R.coords(bwds[0])
    inner = np.zeros_like(which, dtype=bool)
    inner[:, 8:-8, 8:-8] = True
    b, i, j = np.argwhere((which == 0) & inner)[0]
    ty, tx = int(y[b, i, j]), int(x[b, i, j])
    p0 = prevs[0].copy()
    p0[b, 1, ty, tx] = np.nan
    d = device_case(shape, 2, dev)
    ref, _, init, _ = ops.flow_compose([_to(p0, dev), d[0][1]], d[1], d[2], d[3])
    assert bool(torch.isnan(ref[b, 1, i, j])) and bool(torch.isnan(init[b, 1, i, j]))
    assert not bool(torch.isnan(ref[b, 0, i, j]))
    # offset 1 poisoned at every tap that only pixels settled at offset 0 would read
    _, rt = read_by_unsettled(which, bwds[1], 1)
    p1 = prevs[1].copy()
    p1[np.broadcast_to(~rt[:, None], p1.shape)] = np.nan
    same(ops.flow_compose([d[0][0], _to(p1, dev)], d[1], d[2], d[3]), clean)


@pytest.mark.parametrize("shape", LR.SHAPES, ids=IDS)
def test_compose_pixels_without_a_source(dev, shape):
    """cmask 0, which 255, ref +0 (the bits), init = the warp of prev[0] along bwd[0], or
    fill where that leaves the image: both kinds occur."""
    count = 2
    prevs, fwds, bwds, fill = device_case(shape, count, dev)
    ref, cmask, init, which = ops.flow_compose(prevs, fwds, bwds, fill)
    none = which == 255
    assert bool(none.any()) and bool(((cmask == 0) == none).all())
    nc = none[:, None].expand_as(ref)
    assert bool((bits(ref)[nc] == 0).all())
    start, valid = ops.flow_warp(prevs[0], bwds[0], fill=fill, want_valid=True)
    assert torch.equal(bits(init)[nc], bits(start)[nc])
    out = none & (valid == 0)
    assert bool(out.any()) and bool((none & (valid != 0)).any())
    assert torch.equal(bits(init)[out[:, None].expand_as(ref)], bits(fill)[out[:, None].expand_as(ref)])


def test_compose_argument_checks_launch_nothing(dev):
    """count 0 and 5, a null entry and h = 1: an error, and the outputs keep their sentinel."""
    prevs, fwds, bwds, fill = device_case(LR.SHAPES[0], 4, dev)
    n, c, h, w = LR.SHAPES[0]
    outs = [torch.full_like(fill, -3.0), torch.full((n, h, w), -3.0, device=dev),
            torch.full_like(fill, -3.0), torch.full((n, h, w), 77, device=dev, dtype=torch.uint8)]
    tab = lambda ts: (C.c_void_p * 5)(*[t.data_ptr() for t in ts])
    L = N.lib()

    def call(p=prevs, count=4, hh=h, ww=w):
        t = tab(p)
        if p is not prevs:
            t[1] = None
        return L.stx_flow_compose(t, tab(fwds), tab(bwds), count, fill.data_ptr(),
                                  *[o.data_ptr() for o in outs], n, c, hh, ww, None)

    assert call(count=0) == 1001 and call(count=5) == 1001 and call(p=list(prevs)) == 1001
    assert call(hh=1, ww=h * w) == 1001
    with pytest.raises(N.NativeError, match="stx_flow_compose"):
        ops.flow_compose(prevs + prevs[:1], fwds + fwds[:1], bwds + bwds[:1], fill)
    with pytest.raises(N.NativeError):
        ops.flow_compose([], [], [], fill)
    torch.cuda.synchronize()
    assert all(bool((o == (77 if o.dtype == torch.uint8 else -3.0)).all()) for o in outs)
    assert call() == 0  # and the same call with nothing wrong runs
    torch.cuda.synchronize()
    assert not bool((outs[1] == -3.0).any())


def test_compose_in_a_graph(dev):
    """Captured once; after the inputs change in place a replay gives the eager bits."""
    shape = LR.SHAPES[1]
    prevs, fwds, bwds, fill = device_case(shape, 3, dev)
    outs = ops.flow_compose(prevs, fwds, bwds, fill)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with ops.graph_capture(graph):
        ops.flow_compose(prevs, fwds, bwds, fill, *outs)
    other = device_case(shape, 3, dev)
    # the offsets change places and the images change: other selections, other values
    for dst, src in zip(prevs + fwds + bwds, other[0][::-1] + other[1][::-1] + other[2][::-1]):
        dst.copy_(src * 1.0)
    prevs[0].mul_(0.5)
    eager = [t.clone() for t in ops.flow_compose(prevs, fwds, bwds, fill)]
    for o in outs:
        o.zero_()
    graph.replay()
    torch.cuda.synchronize()
    same(outs, eager)
    assert not torch.equal(eager[3], chain_of_ops(*device_case(shape, 3, dev))[3])


# ===================================================================== batched estimation
def _frames(h, w, count, seed):
    """count + 1 conditioned frames: one smooth texture seen through a window moving
    (2, 1) px per frame."""
    import flowest_ref as E
    tex = E.texture(h + count, w + 2 * count, seed)
    return [E.condition(tex[t:t + h, 2 * t:2 * t + w]) for t in range(count + 1)]


@pytest.mark.parametrize("h,w", [(48, 80), (33, 65)])
def test_pairs_flow_equals_pair_calls(dev, h, w):
    """FlowEstimator(pairs=3).pairs_flow over (frame t-k, frame t), k = 1, 2, 3, equals three
    pair calls of a one-pair estimator bit for bit; so does a 2-pair list, and pair() itself,
    on the 3-pair estimator (the leading part of the batch); nothing is allocated."""
    fr = [_to(f, dev) for f in _frames(h, w, 3, 5)]
    one = video.FlowEstimator(h, w, dev)
    want = [[t.clone() for t in one.pair(fr[3 - k], fr[3])] for k in (1, 2, 3)]
    assert not torch.equal(want[0][0], want[1][0])
    est = video.FlowEstimator(h, w, dev, pairs=3)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(dev)
    got = est.pairs_flow([(fr[3 - k], fr[3]) for k in (1, 2, 3)])
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(dev) == before
    assert len(got) == 3 and tuple(got[0][0].shape) == (1, 2, h, w)
    for (f, b), (wf, wb) in zip(got, want):
        assert torch.equal(bits(f), bits(wf)) and torch.equal(bits(b), bits(wb))
    assert got[0][0].data_ptr() == est.fwd.data_ptr()
    two = est.pairs_flow([(fr[0], fr[3]), (fr[2], fr[3])])  # other pairs, other slots
    assert len(two) == 2
    for (f, b), (wf, wb) in zip(two, (want[2], want[0])):
        assert torch.equal(bits(f), bits(wf)) and torch.equal(bits(b), bits(wb))
    f, b = est.pair(fr[1], fr[3])
    assert torch.equal(bits(f), bits(want[1][0])) and torch.equal(bits(b), bits(want[1][1]))
    with pytest.raises(ValueError, match="1..3"):
        est.pairs_flow([(fr[0], fr[1])] * 4)
    with pytest.raises(ValueError, match="1..1"):
        one.pairs_flow([(fr[0], fr[1])] * 2)


def test_estimate_flows_with_offsets(dev):
    """estimate_flows(offsets=(1, 2)): key 1 is the two-array form's result bit for bit, key 2
    the flows over two frames ([T-2]), about twice the clip's (2, 1) px."""
    fr = [torch.from_numpy(f) for f in _frames(64, 64, 3, 4)]
    d = video.estimate_flows(fr, offsets=(1, 2))
    f1, b1 = video.estimate_flows(fr)
    assert sorted(d) == [1, 2] and d[2][0].shape == (2, 2, 64, 64) and d[1][0].shape == (3, 2, 64, 64)
    assert np.array_equal(d[1][0], f1) and np.array_equal(d[1][1], b1)
    core = d[2][1][:, :, 14:-14, 14:-14]
    assert abs(core[:, 0].mean() - 4) < 0.5 and abs(core[:, 1].mean() - 2) < 0.5


# ================================================================================= engine
@pytest.fixture(scope="module")
def feat(dev):
    return V.VGGFeatures(W.vgg19_synthetic(TF.VGG_SEED, 5), dev)


def test_engine_term_is_the_long_term_loss(dev, feat):
    """One iteration of GatysEngine(temporal=(ref*, c*, w)) on flow_compose's outputs: tloss
    equals longterm_ref.long_loss, the explicit fp64 sum over the offsets, within the bound
    of test_flow_gpu.test_engine_term_is_the_reference.  The flows are the occlusion clip's
    (whole pixels: every warp is exact, so the bound is the masked loss's alone)."""
    flows = LR.occlusion_flows((1, 2))
    t = 3
    fwds = [flows[k][0][t - k:t - k + 1] for k in (1, 2)]
    bwds = [flows[k][1][t - k:t - k + 1] for k in (1, 2)]
    prevs = [W.synthetic_image(31 + k, (1, 3, 64, 64)) for k in (1, 2)]
    x0 = W.synthetic_image(13, (1, 3, 64, 64))
    weight = 500.0
    ref, cmask, _, which = ops.flow_compose([_to(p, dev) for p in prevs], [_to(f, dev) for f in fwds],
                                            [_to(b, dev) for b in bwds], _to(x0, dev))
    assert {0, 1, 255} == set(np.unique(_np(which)))
    want, mag = LR.long_loss(x0, prevs, fwds, bwds, weight)
    e = V.GatysEngine(feat, TF._img(11).to(dev), TF._img(12).to(dev), init=_to(x0, dev),
                      temporal=(ref, cmask, weight))
    e._iteration()
    torch.cuda.synchronize()
    assert want > 0
    within(float(e.tloss), want, (TF.chain((1, 3, 64, 64), True) + 16) * U * mag,
           "engine term, long-term")


# =============================================================================== workflow
STEPS, WEIGHT = 20, 1e7  # as test_flow_gpu.test_workflow_temporal_weight_lowers_the_temporal_error


def test_workflow_long_term_lowers_the_error_on_uncovered_pixels(dev, feat):
    """On the occlusion clip with its exact flows: the error sum m (y_t - W(y_{t-2}, bwd2_t))^2
    / sum m over the pixels m that frame t-1 does not explain and frame t-2 does, averaged
    over t >= 2, is lower with long_term=(1, 2) than with long_term=None."""
    frames = [torch.from_numpy(f) for f in LR.occlusion_clip()]
    flows = LR.occlusion_flows((1, 2))
    style = TF._img(11)

    def run(flows_, long_term):
        ys = [_np(y) for y in video.gatys_video(feat, frames, style, flows_, steps=STEPS,
                                                temporal_weight=WEIGHT, long_term=long_term)]
        assert len(ys) == LR.CLIP_T and all(np.isfinite(y).all() for y in ys)
        return ys

    short, long_ = run(flows[1], None), run(flows, (1, 2))
    e_short, e_long = LR.uncovered_error(short, flows), LR.uncovered_error(long_, flows)
    print(f"uncovered-pixel error: long_term=None {e_short:.6g}, long_term=(1, 2) {e_long:.6g}")
    assert np.array_equal(short[0], long_[0]) and np.array_equal(short[1], long_[1])
    assert e_long < e_short, (e_long, e_short)


@pytest.mark.parametrize("flows,optimizer", [("given", "adam"), ("static", "adam"),
                                             ("auto", "adam"), ("given", "lbfgs")])
def test_long_term_of_one_offset_is_the_short_term_workflow(dev, feat, flows, optimizer):
    """long_term=(1,) yields the frames of long_term=None, bit for bit."""
    frames, fl = TF.clip_frames(), TF.clip_flows()
    style = TF._img(11)
    steps = 5 if optimizer == "adam" else 1
    run = lambda lt: [y.clone() for y in video.gatys_video(
        feat, frames, style, fl if flows == "given" else flows, steps=steps,
        temporal_weight=1e4, optimizer=optimizer, long_term=lt)]
    a, b = run(None), run((1,))
    assert len(a) == len(b) == TF.T
    for t, (p, q) in enumerate(zip(a, b)):
        assert torch.equal(bits(p), bits(q)), t


def test_long_term_auto_equals_estimated_flows(dev, feat):
    """gatys_video("auto", long_term=(1, 2)) = gatys_video(estimate_flows(offsets=(1, 2))),
    and the second offset matters."""
    frames = [torch.from_numpy(f) for f in LR.occlusion_clip()[:4]]
    style = TF._img(11)
    d = video.estimate_flows(frames, offsets=(1, 2))
    run = lambda fl, lt: [y.clone() for y in video.gatys_video(feat, frames, style, fl, steps=5,
                                                               temporal_weight=1e4, long_term=lt)]
    auto, given = run("auto", (1, 2)), run(d, (1, 2))
    for t, (p, q) in enumerate(zip(auto, given)):
        assert bool(torch.isfinite(p).all()) and torch.equal(bits(p), bits(q)), t
    with pytest.raises(ValueError, match=r"no flows given for offsets \[2\]"):
        run(d[1], (1, 2))


# ==================================================================================== CLI
def test_cli_long_term(dev, tmp_path, monkeypatch):
    """--long-term 1,2 with an .npz of both offsets, with static and with auto --save-flows
    (the saved file reloads through load_long_flows and gives auto's frames); a file without
    the second offset exits with the named error."""
    from click.testing import CliRunner
    from PIL import Image
    from conftest import REPO
    from styletransfer_amd.clis import cli
    H, T = LR.CLIP_H, 4
    monkeypatch.setattr(constants, "PROJECT_ROOT_PATH", str(tmp_path))
    monkeypatch.setattr(constants, "IMSIZE", H)
    monkeypatch.chdir(tmp_path)
    mean = np.array(constants.IMAGENET_MEAN, np.float32).reshape(1, 3, 1, 1)
    std = np.array(constants.IMAGENET_STD, np.float32).reshape(1, 3, 1, 1)
    clip = np.concatenate([np.clip((f * std + mean) * 255, 0, 255)
                           for f in LR.occlusion_clip()[:T]])
    np.save(tmp_path / "clip.npy", np.ascontiguousarray(clip.transpose(0, 2, 3, 1)).astype(np.uint8))
    flows = LR.occlusion_flows((1, 2))
    cut = {k: tuple(a[:T - k] for a in v) for k, v in flows.items()}
    video.save_flows(str(tmp_path / "both.npz"), *cut[1], longer={2: cut[2]})
    video.save_flows(str(tmp_path / "short.npz"), *cut[1])
    Image.open(os.path.join(REPO, "data", "styles", "picasso.jpg")).save(tmp_path / "style.jpg")
    common = ["gatys_video", "clip.npy", "style.jpg", "-s", "3", "-tw", "100", "--long-term", "1,2"]
    pngs = lambda d: [np.asarray(Image.open(tmp_path / d / f"{i}.png")) for i in range(T)]
    for flow, out in (("both.npz", "a"), ("static", "b")):
        r = CliRunner().invoke(cli, common + ["--flow", flow, "-o", out])
        assert r.exit_code == 0, r.output + repr(r.exception)
        assert sorted(os.listdir(tmp_path / out)) == sorted(f"{i}.png" for i in range(T))
        assert all(im.shape == (H, H, 3) for im in pngs(out))
    assert not np.array_equal(pngs("a")[2], pngs("b")[2])
    r = CliRunner().invoke(cli, common + ["--flow", "auto", "--save-flows", "f.npz", "-o", "c"])
    assert r.exit_code == 0, r.output + repr(r.exception)
    d = video.load_long_flows(str(tmp_path / "f.npz"), T, H, (1, 2))
    assert d[2][0].shape == (T - 2, 2, H, H) and np.abs(d[2][1]).max() > 0.5
    r = CliRunner().invoke(cli, common + ["--flow", "f.npz", "-o", "d"])
    assert r.exit_code == 0, r.output + repr(r.exception)
    assert all(np.array_equal(p, q) for p, q in zip(pngs("c"), pngs("d")))
    r = CliRunner().invoke(cli, common + ["--flow", "short.npz", "-o", "e"])
    assert r.exit_code == 2 and "_2' array for offset 2" in r.output and "--save-flows" in r.output
    assert not os.path.exists(tmp_path / "e")
