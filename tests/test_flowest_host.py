"""Optical-flow estimation, the parts that need no GPU: stx_flow_pyramid, the command
line's `--flow auto` / `--save-flows`, save_flows, and the pin of the fp64 restatement
tests/flowest_ref.py (the yardstick of tests/test_flowest_gpu.py) against clips whose true
flow is exact by construction.

Conditions of the pin (from the method's prototype; they hold for the reference, at fp64
and at fp32 alike, which shows that precision does not decide them): interior mean
end-point error <= 0.15 px (interior: a margin of ceil(max|f|) + 4), and
flow_ref.consistency of the two estimated directions keeps >= 0.99 of the interior.

What tests/flowest_ref.py gives (fp64; fp32 agrees to the digits shown):

    size     true flow                  EPE mean  EPE max  kept    max|fp32 - fp64|
    48x80    (5.25, -3.5) translation   0.0728    1.416    0.9982  4.4e-5
    48x80    the smooth field           0.0835    0.207    1.0000  1.1e-5
    128x160  (5.25, -3.5) translation   0.0204    0.765    1.0000  4.4e-5
    128x160  the smooth field           0.0187    0.405    1.0000  2.1e-5

Occlusion (96 x 128, a 32 x 40 rectangle of octave-(4, 8) texture over the background, moved
by (rows, cols)); conditions >= 0.9, >= 0.95, >= 0.9 and the core's mean backward flow
within 0.1 px of the motion:

    motion  disoccluded masked  far field kept  core kept  mean bwd in the core (dx, dy)
    (0, 6)  0.990               0.972           0.932      (-5.953, -0.084)
    (3, 4)  0.975               0.972           0.996      (-3.966, -2.983)

The texture seed is part of the input: Horn-Schunck falls into local minima on some
textures (seed 5 leaves a patch of the 48 x 80 translation at 8 px error), and a clip was
chosen on which the reference meets the conditions."""
import numpy as np
import pytest
import torch

import flow_ref as R
import flowest_ref as E

E_INVALID = 1001


# ---------------------------------------------------------------------------- pyramid
@pytest.mark.parametrize("min_side", [8, 16])
@pytest.mark.parametrize("hw", [(5, 7), (48, 80), (129, 67), (512, 512)])
def test_pyramid_sizes(hw, min_side):
    from styletransfer_amd import ops
    want = E.pyramid(*hw, min_side)
    assert ops.flow_pyramid(*hw, min_side) == want
    assert want[0] == hw and all(min(s) >= 2 for s in want)


def test_pyramid_known_and_arguments():
    import ctypes as C
    from styletransfer_amd import _native as N
    from styletransfer_amd import ops
    assert ops.flow_pyramid(512, 512) == [(512, 512), (256, 256), (128, 128), (64, 64), (32, 32),
                                          (16, 16)]
    assert ops.flow_pyramid(48, 80) == [(48, 80), (24, 40)]
    assert ops.flow_pyramid(129, 67, 8) == [(129, 67), (65, 34), (33, 17), (17, 9)]
    assert ops.flow_pyramid(5, 7) == [(5, 7)]
    L = N.lib()
    for bad in ((1, 8, 16), (8, 1, 16), (8, 8, 1), (8, 8, 0)):
        assert L.stx_flow_pyramid(*bad, None, None, 0) == -E_INVALID, bad
        assert b"stx_flow_pyramid" in L.stx_last_error_string()
    # a short array receives the first `cap` levels; the count is still the whole pyramid's
    hs, ws = (C.c_int * 2)(), (C.c_int * 2)()
    assert L.stx_flow_pyramid(512, 512, 16, hs, ws, 2) == 6
    assert list(hs) == [512, 256] and list(ws) == [512, 256]


def test_entry_points_refuse_bad_arguments():
    """Before any launch (fake pointers: nothing is dereferenced, no GPU here)."""
    from styletransfer_amd import _native as N
    L = N.lib()
    p, q, r, s = 4096, 8192, 12288, 16384
    import ctypes as C
    m = (C.c_float * 3)(0.5, 0.5, 0.5)
    for bad in ((None, q, 1, 8, 8), (p, None, 1, 8, 8), (p, q, 0, 8, 8), (p, q, 1, 1, 8),
                (p, q, 1, 8, 1), (p, q, 70000, 8, 8)):
        assert L.stx_flow_luma(*bad, m, m, None) == E_INVALID, bad
    assert L.stx_flow_luma(p, q, 1, 8, 8, None, m, None) == E_INVALID
    for bad in ((None, q, r, s, 1, 8, 8), (p, None, r, s, 1, 8, 8), (p, q, None, s, 1, 8, 8),
                (p, q, r, None, 1, 8, 8), (p, q, r, r, 1, 8, 8), (p, q, r, s, 1, 1, 8)):
        assert L.stx_flow_linearize(*bad, None) == E_INVALID, bad
        assert b"stx_flow_linearize" in L.stx_last_error_string()
    ws = L.stx_flow_jacobi_ws(2, 64, 64)
    assert ws == 2 * 2 * 64 * 64 * 4

    def jac(coef=p, uv=q, out=r, n=2, h=64, w=64, alpha=15.0, iters=40, fuse=0, wp=s, wn=ws):
        return L.stx_flow_jacobi(coef, uv, out, n, h, w, alpha, iters, fuse, wp, wn, None)

    for kw in (dict(coef=None), dict(uv=None), dict(out=None), dict(out=q), dict(n=0), dict(h=1),
               dict(iters=0), dict(fuse=-1), dict(fuse=N.STX_FLOW_JACOBI_MAXFUSE + 1),
               dict(alpha=0.0), dict(alpha=float("nan")), dict(wp=q), dict(wp=r)):
        assert jac(**kw) == E_INVALID, kw
        assert b"stx_flow_jacobi" in L.stx_last_error_string()
    assert jac(wp=None) == 1002 and jac(wn=ws - 1) == 1002  # STX_E_WORKSPACE
    assert L.stx_flow_scale(None, 1, 8, 8, 2.0, 2.0, None) == E_INVALID


def test_ops_refuse_cpu_tensors():
    from styletransfer_amd import _native as N
    from styletransfer_amd import ops
    with pytest.raises(N.NativeError):
        ops.flow_luma(torch.zeros(1, 3, 4, 4))
    with pytest.raises(N.NativeError):
        ops.flow_linearize(torch.zeros(1, 4, 4), torch.zeros(1, 4, 4), torch.zeros(1, 2, 4, 4))
    with pytest.raises(N.NativeError):
        ops.flow_jacobi(torch.zeros(1, 3, 4, 4), torch.zeros(1, 2, 4, 4))
    with pytest.raises(N.NativeError):
        ops.flow_scale(torch.zeros(1, 2, 4, 4), 2.0, 2.0)


# -------------------------------------------------------------------------------- CLI
def test_parser_accepts_auto(tmp_path, monkeypatch):
    import click
    from styletransfer_amd import constants
    from styletransfer_amd.clis import gatys_video as G
    monkeypatch.setattr(constants, "PROJECT_ROOT_PATH", str(tmp_path))
    assert G.parse_flow(None, None, "auto") == "auto"
    assert G.parse_flow(None, None, "static") == "static"
    with pytest.raises(click.BadParameter, match="auto"):
        G.parse_flow(None, None, "nothing.npz")


@pytest.fixture
def stubbed_cli(tmp_path, monkeypatch):
    """The command with loading, estimation and the transfer stubbed: only the argument
    handling runs.  Returns (invoke, calls)."""
    from click.testing import CliRunner
    from styletransfer_amd import constants, img_utils, network, video
    from styletransfer_amd.clis import cli
    monkeypatch.setattr(constants, "PROJECT_ROOT_PATH", str(tmp_path))
    calls = []

    class FakeNet:
        def __init__(self, style):
            pass

        def train_gatys_video(self, frames, style_image, flows, **kw):
            calls.append(flows)
            return iter([torch.zeros(1, 3, 16, 16) for _ in frames])

    est = (np.full((3, 2, 16, 16), 1.5, np.float32), np.full((3, 2, 16, 16), -1.5, np.float32))
    monkeypatch.setattr(network, "StyleNetwork", FakeNet)
    monkeypatch.setattr(video, "iterate_frames",
                        lambda src, *a, **k: iter([torch.zeros(1, 3, 16, 16)] * 4))
    monkeypatch.setattr(video, "estimate_flows", lambda frames, **k: est)
    monkeypatch.setattr(img_utils, "image_loader", lambda path, imsize=None: path)
    monkeypatch.setattr(img_utils, "imshow", lambda img, path=None, **k: None)
    np.savez(tmp_path / "flows.npz", forward=est[0], backward=est[1])
    return (lambda *args: CliRunner().invoke(cli, ["gatys_video", *args])), calls, est


def test_cli_auto_and_save_flows(stubbed_cli, tmp_path):
    from styletransfer_amd import video
    invoke, calls, est = stubbed_cli
    r = invoke("--help")
    assert r.exit_code == 0 and "auto" in r.output and "--save-flows" in r.output
    r = invoke("clip.npy", "s.jpg", "--flow", "auto")
    assert r.exit_code == 0, r.output + repr(r.exception)
    assert calls == ["auto"]
    r = invoke("clip.npy", "s.jpg", "--flow", "auto", "--save-flows", "est.npz")
    assert r.exit_code == 0, r.output + repr(r.exception)
    assert np.array_equal(calls[-1][0], est[0]) and np.array_equal(calls[-1][1], est[1])
    f, b = video.load_flows(str(tmp_path / "est.npz"), 4, 16)
    assert np.array_equal(f, est[0]) and np.array_equal(b, est[1])


@pytest.mark.parametrize("flow", ["static", "flows.npz"])
def test_cli_save_flows_needs_auto(stubbed_cli, flow):
    invoke, calls, _ = stubbed_cli
    r = invoke("clip.npy", "s.jpg", "--flow", flow, "--save-flows", "est.npz")
    assert r.exit_code == 2 and "--save-flows" in r.output and "auto" in r.output
    assert not calls


def test_save_flows_round_trips_the_bits(tmp_path):
    from styletransfer_amd import video
    rng = np.random.default_rng(3)
    fwd = rng.normal(size=(3, 2, 16, 16)).astype(np.float32)
    bwd = rng.normal(size=(3, 2, 16, 16)).astype(np.float32)
    fwd[0, 0, 0, :3] = [-0.0, 1e-42, 3e38]  # a signed zero, a subnormal, a large value
    path = str(tmp_path / "f.npz")
    video.save_flows(path, fwd, bwd)
    f, b = video.load_flows(path, 4, 16)
    assert f.dtype == np.float32 and np.array_equal(f.view(np.int32), fwd.view(np.int32))
    assert np.array_equal(b.view(np.int32), bwd.view(np.int32))
    with pytest.raises(ValueError, match="one shape"):
        video.save_flows(path, fwd, bwd[:2])


# ------------------------------------------------------------------ the reference's pin
CLIPS = [("translation", 48, 80), ("smooth", 48, 80), ("translation", 128, 160),
         ("smooth", 128, 160)]


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("kind,h,w", CLIPS, ids=[f"{k}-{h}x{w}" for k, h, w in CLIPS])
def test_reference_recovers_the_true_flow(kind, h, w, dtype):
    A, B, f = E.clip(kind, h, w)
    fwd, bwd = E.estimate_pair(B, A, dtype)  # bwd = estimate(A, B): the true flow
    assert bwd.dtype == dtype
    I = E.interior(f, h, w)
    e = E.epe(bwd, f)[I]
    kept = R.consistency(fwd.astype(np.float32), bwd.astype(np.float32))["c"][I].mean()
    print(f"{kind} {h}x{w} {np.dtype(dtype).name}: EPE mean {e.mean():.4f} max {e.max():.3f}, "
          f"kept {kept:.4f}")
    assert e.mean() <= 0.15
    assert kept >= 0.99


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("motion", [(0, 6), (3, 4)], ids=["0,6", "3,4"])
def test_reference_masks_the_disocclusion(motion, dtype):
    dr, dc = motion
    prev, cur, (r0, c0, rh, rw) = E.occlusion_clip(dr, dc)
    fwd, bwd = E.estimate_pair(prev, cur, dtype)
    c = R.consistency(fwd.astype(np.float32), bwd.astype(np.float32))["c"][0]
    h, w = c.shape
    old, new, core = (np.zeros((h, w), bool) for _ in range(3))
    old[r0:r0 + rh, c0:c0 + rw] = True
    new[r0 + dr:r0 + dr + rh, c0 + dc:c0 + dc + rw] = True
    core[r0 + dr + 6:r0 + dr + rh - 6, c0 + dc + 6:c0 + dc + rw - 6] = True
    ii, jj = np.nonzero(old | new)  # the rectangle's sweep
    far = np.ones((h, w), bool)
    far[max(ii.min() - 12, 0):ii.max() + 13, max(jj.min() - 12, 0):jj.max() + 13] = False
    far[:4] = far[-4:] = far[:, :4] = far[:, -4:] = False
    masked, far_kept, core_kept = 1 - c[old & ~new].mean(), c[far].mean(), c[core].mean()
    mean_bwd = np.array([bwd[0, 0][core].mean(), bwd[0, 1][core].mean()])
    print(f"{motion} {np.dtype(dtype).name}: disoccluded masked {masked:.3f}, far kept "
          f"{far_kept:.3f}, core kept {core_kept:.3f}, core bwd {mean_bwd}")
    assert masked >= 0.9 and far_kept >= 0.95 and core_kept >= 0.9
    # the rectangle moved by (dr, dc): frame t's pixel came from (-dc, -dr) as (dx, dy)
    assert np.abs(mean_bwd - np.array([-dc, -dr])).max() <= 0.1


def test_reference_conventions():
    """An integer translation of two pixels: the finest level alone recovers it, with the
    sign convention A(i, j) = B(i + f[1], j + f[0]); one Jacobi iteration of a zero data
    term is the 9-point average."""
    tex = E.texture(40, 44, 2)
    A, B = E.condition(tex[2:34, 4:40]), E.condition(tex[3:35, 2:38])  # A(i, j) = B(i-1, j+2)
    f = E.estimate(A, B, min_side=64)
    assert f.shape == (1, 2, 32, 36)
    assert np.abs(f[0, 0, 8:-8, 8:-8].mean() - 2.0) < 0.1
    assert np.abs(f[0, 1, 8:-8, 8:-8].mean() + 1.0) < 0.1
    uv = np.random.default_rng(0).normal(size=(1, 2, 6, 7))
    out = E.jacobi(np.zeros((1, 3, 6, 7)), uv, iters=1)
    q = np.pad(uv, ((0, 0), (0, 0), (1, 1), (1, 1)), mode="edge")
    want = (q[..., :-2, 1:-1] + q[..., 2:, 1:-1] + q[..., 1:-1, :-2] + q[..., 1:-1, 2:]) / 6 + \
        (q[..., :-2, :-2] + q[..., :-2, 2:] + q[..., 2:, :-2] + q[..., 2:, 2:]) / 12
    assert np.allclose(out, want, rtol=0, atol=1e-14)
    g = E.luma(E.condition(tex))
    assert np.abs(g[0] - tex).max() < 1e-3  # a grey frame's luma is its grey level
