"""Temporally consistent Gatys video, the parts that need no GPU: the C ABI of the three
flow entry points, video.load_flows and the `gatys_video` command line."""
import os
import subprocess

import numpy as np
import pytest
import torch

NEW = ("stx_flow_warp", "stx_flow_consistency", "stx_masked_mse_ws", "stx_masked_mse")
E_INVALID, E_WORKSPACE = 1001, 1002


def test_flow_symbols_exported_and_bound():
    from styletransfer_amd import _native as N
    N.lib()
    out = subprocess.check_output(["nm", "-D", "--defined-only", N.LIB_PATH]).decode()
    syms = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for name in NEW:
        assert name in syms, name
        assert name in N.SIGNATURES, name


def test_flow_invalid_args_rejected():
    """Refused before any launch (fake pointers: nothing is dereferenced, no GPU here)."""
    from styletransfer_amd import _native as N
    L = N.lib()
    p = 4096
    for bad in ((None, p, 2 * p, 1, 3, 8, 8), (p, None, 2 * p, 1, 3, 8, 8),
                (p, p, None, 1, 3, 8, 8), (p, p, p, 1, 3, 8, 8),  # out == src
                (p, p, 2 * p, 0, 3, 8, 8), (p, p, 2 * p, 1, 0, 8, 8),
                (p, p, 2 * p, 1, 3, 1, 8), (p, p, 2 * p, 1, 3, 8, 1),
                (p, p, 2 * p, 70000, 3, 8, 8), (p, p, 2 * p, 1, 3, 65536, 65536)):
        src, flow, out, n, c, h, w = bad
        assert L.stx_flow_warp(src, flow, None, out, None, n, c, h, w, None) == E_INVALID, bad
        assert b"stx_flow_warp" in L.stx_last_error_string()
    for bad in ((None, p, p, 1, 8, 8), (p, None, p, 1, 8, 8), (p, p, None, 1, 8, 8),
                (p, p, p, 0, 8, 8), (p, p, p, 1, 1, 8), (p, p, p, 1, 8, 1)):
        assert L.stx_flow_consistency(*bad, None) == E_INVALID, bad
        assert b"stx_flow_consistency" in L.stx_last_error_string()
    ws = L.stx_masked_mse_ws()
    assert ws > 0

    def mse(x=p, ref=p, mask=p, n=1, c=3, hw=64, out=p, ws_ptr=p, ws_bytes=ws):
        return L.stx_masked_mse(x, ref, mask, n, c, hw, 1.0, out, None, None, 0, ws_ptr, ws_bytes,
                                None)

    for kw in (dict(x=None), dict(ref=None), dict(mask=None), dict(out=None), dict(n=0),
               dict(c=0), dict(hw=0), dict(n=1024, c=1024, hw=4096)):
        assert mse(**kw) == E_INVALID, kw
        assert b"stx_masked_mse" in L.stx_last_error_string()
    assert mse(ws_ptr=None) == E_WORKSPACE
    assert mse(ws_bytes=ws - 1) == E_WORKSPACE


def test_ops_refuse_cpu_tensors():
    """The product path still raises without a GPU: no CPU fallback."""
    from styletransfer_amd import _native as N
    from styletransfer_amd import ops
    x = torch.zeros(1, 3, 4, 4)
    f = torch.zeros(1, 2, 4, 4)
    with pytest.raises(N.NativeError):
        ops.flow_warp(x, f)
    with pytest.raises(N.NativeError):
        ops.flow_consistency(f, f)
    with pytest.raises(N.NativeError):
        ops.masked_mse(x, x, torch.zeros(1, 4, 4), 1.0)


# ------------------------------------------------------------------------- load_flows
def _save(path, **arrays):
    np.savez(path, **arrays)
    return str(path)


def test_load_flows_accepts_a_good_file(tmp_path):
    from styletransfer_amd import video
    rng = np.random.default_rng(0)
    fwd = rng.normal(size=(3, 2, 16, 16)).astype(np.float32)
    bwd = rng.normal(size=(3, 2, 16, 16)).astype(np.float32)
    f, b = video.load_flows(_save(tmp_path / "ok.npz", forward=fwd, backward=bwd), 4, 16)
    assert np.array_equal(f, fwd) and np.array_equal(b, bwd)
    assert f.dtype == np.float32 and f.flags.c_contiguous


def test_load_flows_names_what_is_wrong(tmp_path):
    from styletransfer_amd import video
    good = np.zeros((3, 2, 16, 16), np.float32)
    nan = good.copy()
    nan[1, 0, 2, 3] = np.nan
    inf = good.copy()
    inf[0, 1, 0, 0] = np.inf
    cases = [
        (dict(forward=good, backward=good[:2]), "holds 2 flows.*4 frames need 3"),
        (dict(forward=good[:, :, :8], backward=good), r"'forward' has shape \(3, 2, 8, 16\)"),
        (dict(forward=good, backward=np.zeros((3, 3, 16, 16), np.float32)), "'backward' has shape"),
        (dict(forward=good.astype(np.float64), backward=good), "'forward' is float64"),
        (dict(forward=good), "no 'backward' array"),
        (dict(backward=good), "no 'forward' array"),
        (dict(forward=good, backward=nan), "'backward' holds 1 non-finite"),
        (dict(forward=inf, backward=good), "'forward' holds 1 non-finite"),
    ]
    for k, (arrays, match) in enumerate(cases):
        with pytest.raises(ValueError, match=match):
            video.load_flows(_save(tmp_path / f"bad{k}.npz", **arrays), 4, 16)


# ------------------------------------------------------------------------------- CLI
@pytest.fixture
def stubbed_cli(tmp_path, monkeypatch):
    """The `gatys_video` command with the frame and image loading and the transfer stubbed:
    only the argument handling runs.  Returns (invoke, calls, written)."""
    from click.testing import CliRunner
    from styletransfer_amd import constants, img_utils, network, video
    from styletransfer_amd.clis import cli
    monkeypatch.setattr(constants, "PROJECT_ROOT_PATH", str(tmp_path))
    calls, written = [], []

    class FakeNet:
        def __init__(self, style):
            pass

        def train_gatys_video(self, frames, style_image, flows, **kw):
            calls.append((frames, flows, kw))
            return iter([torch.zeros(1, 3, 16, 16) for _ in frames])

    monkeypatch.setattr(network, "StyleNetwork", FakeNet)
    monkeypatch.setattr(video, "iterate_frames",
                        lambda src, *a, **k: iter([torch.zeros(1, 3, 16, 16)] * 4))
    monkeypatch.setattr(img_utils, "image_loader", lambda path, imsize=None: path)
    monkeypatch.setattr(img_utils, "imshow", lambda img, path=None, **k: written.append(path))
    good = np.zeros((3, 2, 16, 16), np.float32)
    np.savez(tmp_path / "flows.npz", forward=good, backward=good)
    np.savez(tmp_path / "short.npz", forward=good[:2], backward=good[:2])

    def invoke(*args):
        return CliRunner().invoke(cli, ["gatys_video", *args])
    return invoke, calls, written


def test_cli_help_lists_the_options(stubbed_cli):
    invoke, calls, _ = stubbed_cli
    r = invoke("--help")
    assert r.exit_code == 0
    for opt in ("--flow", "-s", "--first-steps", "-tw", "-sw", "-cw", "--optimizer",
                "--layer-weights", "-o", "static"):
        assert opt in r.output, opt
    assert not calls


def test_cli_passes_its_arguments_on(stubbed_cli):
    invoke, calls, written = stubbed_cli
    r = invoke("clip.npy", "s.jpg", "--flow", "flows.npz", "-s", "7", "--first-steps", "9", "-tw",
               "50", "-sw", "10", "-cw", "2", "--optimizer", "lbfgs", "--layer-weights",
               "1,1,1,0,0", "-o", "out")
    assert r.exit_code == 0, r.output + repr(r.exception)
    (frames, flows, kw), = calls
    assert len(frames) == 4 and flows[0].shape == (3, 2, 16, 16)
    assert (kw["steps"], kw["first_steps"], kw["temporal_weight"], kw["style_weight"],
            kw["content_weight"], kw["optimizer"]) == (7, 9, 50.0, 10, 2, "lbfgs")
    assert kw["style_layer_weights"] == [1, 1, 1, 0, 0]
    assert [os.path.basename(p) for p in written] == ["0.png", "1.png", "2.png", "3.png"]
    assert all(os.path.basename(os.path.dirname(p)) == "out" for p in written)
    r = invoke("clip.npy", "s.jpg", "--flow", "static")
    assert r.exit_code == 0, r.output + repr(r.exception)
    assert calls[-1][1] == "static" and calls[-1][2]["temporal_weight"] is None
    assert calls[-1][2]["first_steps"] is None and calls[-1][2]["optimizer"] == "adam"


def test_cli_usage_errors(stubbed_cli):
    invoke, calls, _ = stubbed_cli
    r = invoke("clip.npy", "s.jpg", "--flow", "nothing.npz")
    assert r.exit_code == 2 and "static" in r.output and "--flow" in r.output
    r = invoke("clip.npy", "s.jpg")
    assert r.exit_code == 2 and "--flow" in r.output
    r = invoke("clip.npy", "s.jpg", "--flow", "short.npz")
    assert r.exit_code == 2 and "4 frames need 3" in r.output
    r = invoke("clip.npy", "s.jpg", "--flow", "static", "--optimizer", "sgd")
    assert r.exit_code == 2
    assert not calls
