"""Long-term consistency for gatys_video, the parts that need no GPU: the identity that
ops.flow_compose rests on, checked on the fp64 restatement tests/longterm_ref.py (which is
written as Ruder et al. write the loss, not through the identity); the inputs of
tests/test_longterm_gpu.py; the flow files; offset validation; the C ABI's argument
checks."""
import itertools

import numpy as np
import pytest
import torch

import flow_ref as R
import longterm_ref as LR

E_INVALID = 1001
COUNTS = [1, 2, 3, 4]


def sure(r):
    """tests/test_flow_gpu.py's margin rule (restated here: that module needs a GPU to
    import): both reference margins exceed 1e-4, so an fp32 evaluation decides alike."""
    with np.errstate(invalid="ignore"):
        return (r["margin_occluded"] > 1e-4) & (r["margin_boundary"] > 1e-4)


# ================================================================================ identity
@pytest.mark.parametrize("shape", LR.SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("count", COUNTS)
def test_long_loss_is_one_masked_loss_on_the_composition(shape, count):
    """sum_j masked_mse(x, omega^j, c_long^j) = masked_mse(x, omega*, c*) to 1e-12 relative,
    on the recipe flows; the c_long^j are pairwise disjoint, their sum is the OR of the c^j,
    and `which` names the nearest consistent offset."""
    prevs, fwds, bwds, fill = LR.case(shape, count)
    x = np.random.default_rng(5).uniform(-1, 1, shape)
    r = LR.compose(prevs, fwds, bwds, fill)
    want, _ = LR.long_loss(x, prevs, fwds, bwds, 37.5)
    got, _, _ = R.masked_mse(x, r["ref"], r["cmask"], 37.5)
    assert abs(got - want) <= 1e-12 * abs(want)
    assert want > 0 or shape[2] == 5  # (the 5 x 7 recipe has no consistent pixel: all fill)
    longs = r["longs"]
    assert set(np.unique(longs)) <= {0.0, 1.0}
    for a, b in itertools.combinations(range(count), 2):
        assert not (longs[a] * longs[b]).any(), (a, b)
    cs = np.stack([q["c"] for q in r["rs"]])
    assert np.array_equal(r["cmask"] != 0, cs.any(axis=0))
    nearest = np.where(cs.any(axis=0), cs.argmax(axis=0), 255)
    assert np.array_equal(r["which"], nearest.astype(np.uint8))
    # init: the composed reference where there is one, else the short-term start
    start, _ = R.warp(prevs[0], bwds[0], fill=fill)
    on = np.broadcast_to(r["cmask"][:, None] != 0, shape)
    assert np.array_equal(r["init"][on], r["ref"][on])
    assert np.array_equal(r["init"][~on], start[~on]) and not r["ref"][~on].any()


@pytest.mark.parametrize("shape", LR.SHAPES[1:], ids=lambda s: "x".join(map(str, s)))
def test_every_offset_and_no_offset_is_selected(shape):
    """The inputs exercise the composition: at count 4 every offset supplies pixels and some
    pixels have no source; the band's start leaves the image (fill)."""
    prevs, fwds, bwds, fill = LR.case(shape, 4)
    r = LR.compose(prevs, fwds, bwds, fill)
    assert set(np.unique(r["which"])) == {0, 1, 2, 3, 255}
    none = r["which"] == 255
    assert (~r["rs"][0]["valid"] & none).any()
    assert np.array_equal(r["init"][:, 0][~r["rs"][0]["valid"] & none],
                          fill.astype(np.float64)[:, 0][~r["rs"][0]["valid"] & none])


@pytest.mark.parametrize("shape", LR.SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("count", COUNTS)
def test_reference_margins_stay_under_the_cap(shape, count):
    """The pixels at which some offset's predicate sits within 1e-4 of its threshold are left
    out of the GPU comparison; on these inputs they are at most 0.5 % (the cap of
    test_flow_gpu.test_consistency_on_the_recipe)."""
    _, fwds, bwds, _ = LR.case(shape, count)
    ok = np.logical_and.reduce([sure(R.consistency(f, b)) for f, b in zip(fwds, bwds)])
    assert (~ok).mean() <= 0.005, (~ok).mean()


# ====================================================================== the occlusion clip
def test_occlusion_clip_is_what_its_flows_say():
    """Each frame is its predecessors warped along the exact flows wherever the masks say
    consistent; the uncovered pixels (c1 = 0 and c2 = 1) are at least 1 % of every frame
    t >= 2; the occluder is narrower than twice its speed."""
    frames, flows = LR.occlusion_clip(), LR.occlusion_flows((1, 2))
    assert len(frames) == LR.CLIP_T >= 6 and frames[0].shape == (1, 3, 64, 64)
    assert LR.OCC_W < 2 * LR.OCC_SPEED
    assert np.abs(np.diff(frames[0], axis=-1)).mean() > 0.1  # textured
    for k in (1, 2):
        assert flows[k][0].shape == (LR.CLIP_T - k, 2, 64, 64)
        for t in range(k, LR.CLIP_T):
            fwd, bwd = flows[k][0][t - k:t - k + 1], flows[k][1][t - k:t - k + 1]
            om, _ = R.warp(frames[t - k], bwd)
            c = np.broadcast_to(R.consistency(fwd, bwd)["c"][:, None], om.shape)
            assert c.mean() > 0.8
            assert np.array_equal(om[c], frames[t].astype(np.float64)[c]), (k, t)
    for t in range(2, LR.CLIP_T):
        m = LR.uncovered(flows, t)
        assert m.mean() >= 0.01, (t, m.mean())
        a, b = LR.occluder_cols(t - 1)  # where the occluder stood a frame ago
        assert m[0, LR.OCC_ROWS[0] + 1:LR.OCC_ROWS[1] - 1, a:b].all()
    # every predicate of the clip is far from its threshold: the GPU decides as the reference
    for k in (1, 2):
        for t in range(k, LR.CLIP_T):
            assert sure(R.consistency(flows[k][0][t - k:t - k + 1],
                                      flows[k][1][t - k:t - k + 1])).all()


def test_uncovered_error_of_the_clip_itself_is_zero():
    frames, flows = LR.occlusion_clip(), LR.occlusion_flows((1, 2))
    assert LR.uncovered_error(frames, flows) == 0.0
    other = [f + t for t, f in enumerate(frames)]
    assert LR.uncovered_error(other, flows) == pytest.approx(3 * 2.0 ** 2)  # 3 channels, d = 2


# ============================================================================ offsets, files
def test_offsets_are_validated():
    from styletransfer_amd import video
    assert video.check_offsets((1, 2, 4)) == (1, 2, 4) and video.check_offsets([1]) == (1,)
    assert video.check_offsets((1, 5, 9, 16)) == (1, 5, 9, 16)
    for bad, match in (((2, 4), "first must be 1"), ((1, 2, 2), "strictly increasing"),
                       ((1, 4, 2), "strictly increasing"), ((1, 2, 3, 4, 5), "1 to 4 entries"),
                       ((), "1 to 4 entries"), ((1, 17), "at most 16"),
                       ((1, 2.5), "integers"), ((0, 1), "first must be 1")):
        with pytest.raises(ValueError, match=match):
            video.check_offsets(bad)
    # the workflow checks before it touches the device or the frames
    with pytest.raises(ValueError, match="first must be 1"):
        next(video.gatys_video(None, [], None, "static", 1, long_term=(2, 3)))


def _long(T=5, S=16, offsets=(1, 2, 4), seed=0):
    rng = np.random.default_rng(seed)
    return {k: tuple(rng.normal(size=(T - k, 2, S, S)).astype(np.float32) for _ in range(2))
            for k in offsets}


def test_long_flows_round_trip(tmp_path):
    from styletransfer_amd import video
    d = _long()
    path = str(tmp_path / "f.npz")
    video.save_flows(path, *d[1], longer={k: v for k, v in d.items() if k > 1})
    with np.load(path) as z:
        assert sorted(z.files) == ["backward", "backward_2", "backward_4", "forward",
                                   "forward_2", "forward_4"]
    back = video.load_long_flows(path, 5, 16, (1, 2, 4))
    assert sorted(back) == [1, 2, 4]
    for k in d:
        for got, want in zip(back[k], d[k]):
            assert np.array_equal(got, want) and got.dtype == np.float32 and got.flags.c_contiguous
    assert sorted(video.load_long_flows(path, 5, 16, (1, 4))) == [1, 4]
    # the short-term reader and writer are what they were
    f, b = video.load_flows(path, 5, 16)
    assert np.array_equal(f, d[1][0]) and np.array_equal(b, d[1][1])
    video.save_flows(path, *d[1])
    with np.load(path) as z:
        assert sorted(z.files) == ["backward", "forward"]


def test_load_long_flows_names_what_is_wrong(tmp_path):
    from styletransfer_amd import video
    d = _long(offsets=(1, 2))
    arrays = dict(forward=d[1][0], backward=d[1][1], forward_2=d[2][0], backward_2=d[2][1])
    nan = d[2][1].copy()
    nan[0, 0, 1, 1] = np.nan
    cases = [
        ({"backward_2": None}, r"no 'backward_2' array for offset 2.*--flow auto --save-flows"),
        ({"forward_2": None}, r"no 'forward_2' array for offset 2"),
        ({"forward": None}, r"no 'forward' array \(found"),
        ({"forward_2": d[2][0][:2]}, "'forward_2' holds 2 flows.*5 frames need 3"),
        ({"backward_2": d[2][1][:, :, :8]}, r"'backward_2' has shape \(3, 2, 8, 16\).*T-2"),
        ({"forward_2": d[2][0].astype(np.float64)}, "'forward_2' is float64"),
        ({"backward_2": nan}, "'backward_2' holds 1 non-finite"),
        ({"backward": d[1][1][:3]}, "'backward' holds 3 flows.*5 frames need 4"),
    ]
    for i, (change, match) in enumerate(cases):
        a = {k: v for k, v in {**arrays, **change}.items() if v is not None}
        path = str(tmp_path / f"bad{i}.npz")
        np.savez(path, **a)
        with pytest.raises(ValueError, match=match):
            video.load_long_flows(path, 5, 16, (1, 2))
    with pytest.raises(ValueError, match="first must be 1"):
        video.load_long_flows(str(tmp_path / "bad0.npz"), 5, 16, (2,))
    with pytest.raises(ValueError, match="one shape expected"):
        video.save_flows(str(tmp_path / "x.npz"), *d[1], longer={2: (d[2][0], d[2][1][:1])})


# ================================================================================ C ABI
def test_flow_compose_is_exported_and_checks_its_arguments():
    """Refused before any launch (fake pointers: nothing is dereferenced, no GPU here)."""
    import ctypes as C
    from styletransfer_amd import _native as N
    L = N.lib()
    assert "stx_flow_compose" in N.SIGNATURES
    p = 4096
    tab = lambda *v: (C.c_void_p * 5)(*v)
    good = tab(p, p, p, p, p)

    def call(prev=good, fwd=good, bwd=good, count=2, fill=2 * p, ref=3 * p, cmask=4 * p,
             init=5 * p, which=6 * p, n=1, c=3, h=8, w=8):
        return L.stx_flow_compose(prev, fwd, bwd, count, fill, ref, cmask, init, which, n, c, h, w,
                                  None)

    hole = tab(p, None, p, p, p)
    for kw in (dict(count=0), dict(count=5), dict(count=-1), dict(prev=hole), dict(fwd=hole),
               dict(bwd=hole), dict(prev=None), dict(fill=None), dict(ref=None),
               dict(cmask=None), dict(h=1), dict(w=1), dict(n=0), dict(c=0), dict(n=70000),
               dict(ref=p), dict(init=p), dict(cmask=p), dict(h=65536, w=65536)):
        assert call(**kw) == E_INVALID, kw
        assert b"stx_flow_compose" in L.stx_last_error_string()


def test_flow_compose_refuses_cpu_tensors():
    from styletransfer_amd import _native as N
    from styletransfer_amd import ops
    x, f = torch.zeros(1, 3, 4, 4), torch.zeros(1, 2, 4, 4)
    with pytest.raises(N.NativeError):
        ops.flow_compose([x], [f], [f], x)


# =================================================================================== CLI
def test_cli_long_term_option(tmp_path, monkeypatch):
    """--long-term is parsed, validated and handed on; a flow file is read for its offsets."""
    from click.testing import CliRunner
    from styletransfer_amd import constants, img_utils, network, video
    from styletransfer_amd.clis import cli
    monkeypatch.setattr(constants, "PROJECT_ROOT_PATH", str(tmp_path))
    calls = []

    class FakeNet:
        def __init__(self, style):
            pass

        def train_gatys_video(self, frames, style_image, flows, **kw):
            calls.append((flows, kw))
            return iter([torch.zeros(1, 3, 16, 16) for _ in frames])

    monkeypatch.setattr(network, "StyleNetwork", FakeNet)
    monkeypatch.setattr(video, "iterate_frames",
                        lambda src, *a, **k: iter([torch.zeros(1, 3, 16, 16)] * 5))
    monkeypatch.setattr(img_utils, "image_loader", lambda path, imsize=None: path)
    monkeypatch.setattr(img_utils, "imshow", lambda img, path=None, **k: None)
    d = _long(offsets=(1, 2))
    video.save_flows(str(tmp_path / "both.npz"), *d[1], longer={2: d[2]})
    video.save_flows(str(tmp_path / "short.npz"), *d[1])
    run = lambda *a: CliRunner().invoke(cli, ["gatys_video", "clip.npy", "s.jpg", *a])
    r = run("--flow", "both.npz", "--long-term", "1,2")
    assert r.exit_code == 0, r.output + repr(r.exception)
    flows, kw = calls[-1]
    assert kw["long_term"] == (1, 2) and sorted(flows) == [1, 2]
    assert np.array_equal(flows[2][1], d[2][1])
    r = run("--flow", "static", "--long-term", "1,2,4")
    assert r.exit_code == 0 and calls[-1][0] == "static" and calls[-1][1]["long_term"] == (1, 2, 4)
    r = run("--flow", "both.npz")
    assert r.exit_code == 0 and calls[-1][1]["long_term"] is None and len(calls[-1][0]) == 2
    n = len(calls)
    r = run("--flow", "short.npz", "--long-term", "1,2")
    assert r.exit_code == 2 and "backward_2" not in r.output and "forward_2" in r.output
    assert "--save-flows" in r.output
    for bad in ("2,4", "1,1", "1,x", "1,2,3,4,5", "1,32"):
        r = run("--flow", "static", "--long-term", bad)
        assert r.exit_code == 2 and "--long-term" in r.output, bad
    assert len(calls) == n
    assert "--long-term" in run("--help").output
