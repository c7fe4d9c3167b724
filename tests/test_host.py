"""Host-side logic that needs no GPU: the C-ABI library loads and exports every
declared symbol; image I/O parity with the reference; checkpoint helpers; module
structure / state_dict keys; the product path fails loudly without a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO


def test_library_exports_header_symbols():
    from styletransfer_amd import _native as N
    L = N.lib()
    assert L.stx_version() == 1
    out = subprocess.check_output(["nm", "-D", "--defined-only", N.LIB_PATH]).decode()
    syms = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    hdr = open(os.path.join(REPO, "include", "stx.h")).read()
    decl = set(re.findall(r"\b(stx_[a-z0-9_]+)\s*\(", hdr))
    assert len(decl) >= 30
    assert decl <= syms, decl - syms
    assert decl == set(N.SIGNATURES), decl ^ set(N.SIGNATURES)
    # the ABI revision the binding checks at load (a library of another revision is
    # refused, never driven with arguments whose meaning changed)
    rev = re.search(r"#define STX_ABI_VERSION (\d+)", hdr).group(1)
    assert L.stx_abi_version() == N.STX_ABI_VERSION == int(rev)


def test_struct_mirrors_match_the_library():
    """Every ctypes mirror has the size and last-member offset the compiled library has
    (stx_abi_layout): a member added to include/stx.h but not to _native.py, or the other
    way round, fails here instead of shifting fields on the GPU."""
    import ctypes as C
    from styletransfer_amd import _native as N
    mirrors = [(N.ConvParams, "unpool_out"), (N.WprepJob, "pad_"), (N.LossParts, "k"),
               (N.GramFinJob, "coef_amax"), (N.PGradJob, "pad_"), (N.ImageMeta, "tmp_offset"),
               (N.CinJob, "accumulate"), (N.StyleLossParams, "defer"),
               (N.WgradParams, "no_split")]
    count = N.lib().stx_abi_layout(None, 0)
    assert count == 2 * len(mirrors)
    out = (C.c_longlong * count)()
    assert N.lib().stx_abi_layout(C.cast(out, C.c_void_p), count) == count
    for i, (S, last) in enumerate(mirrors):
        assert S._fields_[-1][0] == last, S
        assert (C.sizeof(S), getattr(S, last).offset) == (out[2 * i], out[2 * i + 1]), S


def test_host_queries_without_gpu():
    from styletransfer_amd import ops
    assert ops.conv_weight_dims(3, 64, 3) == (4, 64)
    assert ops.conv_weight_dims(128, 256, 3) == (128, 256)
    assert ops.coef_pitch(64) == 64 and ops.coef_pitch(96) == 128
    from styletransfer_amd import _native as N
    assert N.lib().stx_gram_ws(1, 64, 262144) > 0
    need = C.c_size_t()
    p = N.WgradParams(n=8, cin=128, h=64, w=64, cout=128, ks=3, stride=1, pad=1, ho=64, wo=64)
    assert N.lib().stx_conv2d_wgrad_plan(C.byref(p), C.byref(need)) > 0 and need.value > 0


def _wgrad_dims(n, cin, h, w, cout, ks, stride=1, mode=0, **kw):
    """stx_wgrad_params dims of a pad ks // 2 conv over x [n][cin][h][w] read with `mode`."""
    from styletransfer_amd import _native as N
    hv, wv = (2 * h, 2 * w) if mode == N.STX_IN_UPSAMPLE2 else (h, w)
    pad = ks // 2
    f = dict(n=n, cin=cin, h=h, w=w, cout=cout, ks=ks, stride=stride, pad=pad, in_mode=mode,
             ho=(hv + 2 * pad - ks) // stride + 1, wo=(wv + 2 * pad - ks) // stride + 1)
    f.update(kw)
    return f


def _wgrad_plan(**f):
    from styletransfer_amd import _native as N
    need = C.c_size_t()
    return N.lib().stx_conv2d_wgrad_plan(C.byref(N.WgradParams(**f)), C.byref(need)), need.value


def test_wgrad_path_table():
    """The kernel stx_conv2d_wgrad picks is pinned per layer: every trained conv of
    ImageTransformNet at B = 8, 256^2 and the VGG-style ReLU-input 3x3 convs take the path
    the Python ladder over the per-kernel workspace probes gave them before the choice moved
    into the library (run by hand on a build of that revision).  A plan function that sent
    one of them to the fp32 kernel would pass every fp64 comparison and only be slower."""
    from styletransfer_amd import _native as N
    RELU, UP = N.STX_IN_RELU, N.STX_IN_UPSAMPLE2
    table = [((8, 3, 256, 256, 32, 9), N.STX_WGRAD_FEW16),            # conv0
             ((8, 32, 256, 256, 64, 3, 2), N.STX_WGRAD_F16S2),        # the two downs
             ((8, 64, 128, 128, 128, 3, 2), N.STX_WGRAD_F16S2),
             ((8, 128, 64, 64, 128, 3), N.STX_WGRAD_F16),             # residual blocks
             ((8, 128, 64, 64, 64, 3, 1, UP), N.STX_WGRAD_F16),       # the two upsampled convs
             ((8, 64, 128, 128, 32, 3, 1, UP), N.STX_WGRAD_F16),
             ((8, 32, 256, 256, 3, 9), N.STX_WGRAD_FEW16),            # conv22
             ((8, 64, 256, 256, 64, 3, 1, RELU), N.STX_WGRAD_F16),    # VGG-style
             ((8, 64, 128, 128, 128, 3, 1, RELU), N.STX_WGRAD_F16)]
    for args, want in table:
        path, need = _wgrad_plan(**_wgrad_dims(*args))
        assert path == want and need > 0, (args, path, need)
        assert _wgrad_plan(**_wgrad_dims(*args, no_split=1))[0] == N.STX_WGRAD_F32, args
    # shapes the split kernels do not cover fall through to the fp32 kernel
    for args in ((2, 3, 32, 40, 32, 9),        # 9x9, w % 16 != 0
                 (2, 32, 16, 24, 32, 3),       # 3x3 stride 1, wo % 16 != 0
                 (2, 8, 16, 16, 32, 3),        # 3x3 stride 1, cin 8
                 (2, 32, 17, 32, 32, 3, 2)):   # 3x3 stride 2, odd h
        path, need = _wgrad_plan(**_wgrad_dims(*args))
        assert path == N.STX_WGRAD_F32 and need > 0, (args, path, need)
    # no kernel at all
    for f in (_wgrad_dims(2, 32, 16, 16, 32, 5), _wgrad_dims(2, 32, 16, 16, 32, 3, 3),
              _wgrad_dims(2, 32, 16, 16, 32, 3, 1, N.STX_IN_DILATE2)):
        assert _wgrad_plan(**f) == (N.STX_WGRAD_NONE, 0), f


def test_wgrad_malformed_params_rejected():
    """stx_conv2d_wgrad validates the whole stx_wgrad_params before any launch (no GPU is
    present here and the pointers are fake): invalid, or the workspace code."""
    from styletransfer_amd import _native as N
    L = N.lib()
    dims = _wgrad_dims(8, 128, 64, 64, 128, 3)
    path, need = _wgrad_plan(**dims)
    assert path == N.STX_WGRAD_F16

    def refused(code, **kw):
        f = dict(dims, x=16, dy=32, dw=48, x_amax=64, dy_amax=192, ws=4096, ws_bytes=need)
        f.update(kw)
        rc = L.stx_conv2d_wgrad(C.byref(N.WgradParams(**f)), None)
        msg = L.stx_last_error_string()
        assert rc == code and b"stx_conv2d_wgrad" in msg, (kw, rc, msg)

    rc = L.stx_conv2d_wgrad(C.byref(N.WgradParams()), None)  # all zero
    assert rc == 1001 and b"stx_conv2d_wgrad" in L.stx_last_error_string()
    refused(1001, dw=None)
    refused(1001, x=None)
    refused(1001, dy_amax=None)             # a split path reads both amax groups
    refused(1001, x_amax=None)
    refused(1002, ws_bytes=need - 1)
    refused(1002, ws=None)
    refused(1001, ho=63)                    # ho does not follow from (h, ks, stride, pad)
    refused(1001, in_mode=N.STX_IN_UPSAMPLE2)  # (ho would be 128)
    refused(1001, x=20)                     # misaligned x on a split path: no fallback
    refused(1001, dy=36)
    refused(1001, ks=5)
    # the fp32 path needs neither amax groups nor alignment, but its own workspace
    need32 = _wgrad_plan(**dict(dims, no_split=1))[1]
    refused(1002, no_split=1, x=20, x_amax=None, dy_amax=None, ws_bytes=need32 - 1)


def test_invalid_args_rejected():
    from styletransfer_amd import _native as N
    import ctypes as C
    p = N.ConvParams()  # all zero: must be rejected before any launch
    rc = N.lib().stx_conv2d(C.byref(p), None)
    assert rc == 1001
    assert b"unsupported" in N.lib().stx_last_error_string()


def test_pool_sum_contract_rejected():
    """stx_conv_params.pool_sum (the fused nearest-x2 upsampling backward) is refused
    before any launch unless it comes with pool_out on the split path's plain epilogue."""
    from styletransfer_amd import _native as N
    import ctypes as C
    cp, op = N.lib(), None
    # a well-formed split-path data gradient geometry (64 -> 128 at 64x64), fake pointers
    p = N.ConvParams(x=16, y=32, n=1, cin=64, h=64, w=64, cout=128, ks=3, stride=1, pad=1,
                     in_mode=0, hv=64, wv=64, ho=64, wo=64, cin_pad=64, cout_pad=128,
                     wt16=48, w_amax=64, in_amax=80, pool_sum=1)
    rc = cp.stx_conv2d(C.byref(p), op)  # no pool_out
    assert rc == 1001 and b"pool_sum" in cp.stx_last_error_string()
    p.pool_out, p.relu_out = 96, 1      # pool_out given, but a ReLU epilogue
    rc = cp.stx_conv2d(C.byref(p), op)
    assert rc == 1001 and b"pool_sum" in cp.stx_last_error_string()
    p.relu_out, p.ho, p.wo, p.hv, p.wv, p.h, p.w = 0, 63, 63, 63, 63, 63, 63  # odd output
    rc = cp.stx_conv2d(C.byref(p), op)
    assert rc == 1001 and b"pool_sum" in cp.stx_last_error_string()


def test_style_loss_malformed_params_rejected():
    """stx_style_loss refuses a malformed stx_style_loss_params before any launch (no GPU
    is present here and the pointers are fake): invalid, or the workspace code."""
    from styletransfer_amd import _native as N
    import ctypes as C
    L = N.lib()
    b, c, hw = 2, 64, 96
    gram_ws, content_ws = L.stx_gram_ws(b, c, hw), L.stx_style_content_ws(b, c, hw)
    assert 0 < gram_ws < content_ws
    job = N.GramFinJob()

    def refused(code, **kw):
        f = dict(target=16, coef=32, b=b, c=c, hw=hw, weight=1.0, ws=4096, ws_bytes=content_ws)
        f.update(kw)
        rc = L.stx_style_loss(C.byref(N.StyleLossParams(**f)), None)
        msg = L.stx_last_error_string()
        assert rc == code and b"stx_style_loss" in msg, (kw, rc, msg)

    rc = L.stx_style_loss(C.byref(N.StyleLossParams()), None)  # all zero
    assert rc == 1001 and b"stx_style_loss" in L.stx_last_error_string()
    refused(1001, z=48, parts=64, nparts=3)                     # both sources
    refused(1001)                                               # neither
    refused(1001, z=48, target=None)
    refused(1001, parts=64, nparts=3, c=96)
    refused(1001, parts=64, nparts=0)
    refused(1001, z=48, content=80)                             # content without mse_out
    refused(1001, z=48, mse_out=96)                             # mse_out without content
    refused(1001, z=48, mse_parts=80, mse_out=96)               # mse_parts with z
    refused(1001, parts=64, nparts=3, content=80, mse_out=96)   # content with parts
    refused(1001, z=48, loss=112, defer=C.pointer(job))         # defer excludes loss
    refused(1002, z=48, ws_bytes=gram_ws - 1)
    refused(1002, parts=64, nparts=3, ws_bytes=gram_ws - 1)
    refused(1002, z=48, ws=None)
    refused(1002, z=48, content=80, mse_out=96, ws_bytes=gram_ws)  # < stx_style_content_ws
    assert bytes(job) == bytes(N.GramFinJob())                  # a refused call writes no job


def test_phase2_contract_rejected():
    """The fused Gram-backward phase (p2_z) on the split path needs a raw-input data
    gradient; any other loader mode is refused before a launch, not dropped."""
    from styletransfer_amd import _native as N
    import ctypes as C
    L = N.lib()
    for mode, (hv, wv) in ((N.STX_IN_RELU, (64, 64)), (N.STX_IN_RELU_POOL2, (32, 32)),
                           (N.STX_IN_UPSAMPLE2, (128, 128))):
        p = N.ConvParams(x=16, y=32, n=1, cin=64, h=64, w=64, cout=64, ks=3, stride=1, pad=1,
                         in_mode=mode, hv=hv, wv=wv, ho=hv, wo=wv, cin_pad=64, cout_pad=64,
                         wt16=48, w_amax=64, in_amax=80, p2_z=96, p2_wt=112, p2_c=64,
                         p2_amax=128)
        rc = L.stx_conv2d(C.byref(p), None)
        assert rc == 1001 and b"raw-input" in L.stx_last_error_string(), mode


def test_grayscale_frames_expand_to_rgb():
    """iterate_raw_frames: 2-D (grayscale) frames become HxWx3 like PIL's L -> RGB."""
    from PIL import Image
    from styletransfer_amd import video
    arr = (np.arange(2 * 5 * 7) % 251).astype(np.uint8).reshape(2, 5, 7)
    out = list(video.iterate_raw_frames(arr))
    assert len(out) == 2
    for f, g in zip(out, arr):
        assert f.shape == (5, 7, 3)
        assert np.array_equal(f, np.asarray(Image.fromarray(g).convert("RGB")))


def test_image_loader_matches_reference():
    from styletransfer_amd import img_utils
    d = np.load(os.path.join(GOLDEN, "images.npz"))
    x = img_utils.image_loader(os.path.join(REPO, "data", "dancing.jpg"))
    assert torch.equal(x.cpu(), torch.from_numpy(d["dancing_256"]))
    y = img_utils.image_loader(os.path.join(REPO, "data", "styles", "picasso.jpg"))
    assert torch.equal(y.cpu(), torch.from_numpy(d["picasso_256"]))


def test_imshow_bytes_match_reference(tmp_path):
    from PIL import Image
    from styletransfer_amd import img_utils
    d = np.load(os.path.join(GOLDEN, "images.npz"))
    p = tmp_path / "o.png"
    img_utils.imshow(torch.from_numpy(d["imshow_in"]), path=str(p))
    assert np.array_equal(np.asarray(Image.open(p)), d["imshow_out"])


def test_golden_io_split_round_trip(tmp_path):
    """oracle/golden_io.py: a fixture over the file-size limit is written as several files,
    each within it, and loads back as the same arrays byte for byte (an incompressible
    array larger than one file is cut; scalars and small arrays ride along); a small one
    stays a single <name>.npz.  No fixture file of the suite is above 1 MiB."""
    from oracle import golden_io
    rng = np.random.default_rng(5)
    arrays = {"n": np.asarray(3), "big": rng.random((3, 401, 257)).astype(np.float32),
              "bits": rng.integers(0, 256, 700_001, dtype=np.uint8), "s": np.float64(0.25),
              "m": rng.random((2, 64, 65))}
    paths = golden_io.save(str(tmp_path), "case", arrays)
    assert len(paths) > 1 and all(os.path.getsize(p) <= golden_io.LIMIT for p in paths)
    back = golden_io.load(str(tmp_path), "case")
    assert list(back) == list(arrays)
    for k, a in arrays.items():
        a = np.asarray(a)
        assert back[k].dtype == a.dtype and back[k].shape == a.shape
        assert back[k].tobytes() == a.tobytes(), k
    small = {"a": np.arange(5), "b": np.float32(1.5)}
    assert [os.path.basename(p) for p in golden_io.save(str(tmp_path), "case", small)] == ["case.npz"]
    assert sorted(os.listdir(tmp_path)) == ["case.npz"]  # (the split files were replaced)
    assert np.array_equal(golden_io.load(str(tmp_path), "case")["a"], np.arange(5))
    with pytest.raises(FileNotFoundError):
        golden_io.load(str(tmp_path), "absent")
    assert all(os.path.getsize(os.path.join(GOLDEN, f)) <= 1 << 20 for f in os.listdir(GOLDEN))


def test_latest_weights_lexicographic(tmp_path, monkeypatch):
    from styletransfer_amd import constants, network
    mdir = tmp_path / "data" / "models"
    mdir.mkdir(parents=True)
    for e in (1, 9, 10):
        torch.save({"w": torch.tensor([float(e)])}, mdir / f"fast_st_wave_epoch{e}.pth")
    monkeypatch.setattr(constants, "PROJECT_ROOT_PATH", str(tmp_path))
    sd = network._load_latest_model_weigths("fast_st", "wave")
    assert float(sd["w"]) == 9.0  # reference quirk: 'epoch9' sorts after 'epoch10'
    with pytest.raises(AssertionError):
        network._load_latest_model_weigths("fast_st", "nope")


def test_itn_structure_cpu():
    from styletransfer_amd import network
    from styletransfer_amd import weights as W
    net = network.ImageTransformNet(torch.rand(3, 8, 8), batch_size=2)
    keys = list(net.state_dict().keys())
    assert keys == [k for k, _ in W.itn_synthetic(4321)]
    assert sum(p.numel() for p in net.parameters()) == 1_679_235
    assert isinstance(net[0], torch.nn.Conv2d) and net[0].padding_mode == "zeros"
    vnet = network.VideoTransformNet(torch.rand(3, 8, 8))
    assert vnet[0].in_channels == 6 and not vnet.has_external_weights


@pytest.mark.skipif(torch.cuda.device_count() > 0, reason="checks the no-GPU failure mode")
def test_product_path_fails_loudly_without_gpu():
    from styletransfer_amd import _native as N
    from styletransfer_amd import network
    net = network.ImageTransformNet(torch.rand(3, 8, 8), batch_size=1)
    with pytest.raises(N.NativeError, match="no CPU fallback"):
        net(torch.rand(1, 3, 16, 16))


def test_vgg_weights_from_local_state_dict(tmp_path):
    from styletransfer_amd import vgg as V
    sd = {}
    for idx, (co, ci) in zip((0, 2, 5, 7, 10), V.VGG_CONV_SHAPES):
        sd[f"features.{idx}.weight"] = torch.full((co, ci, 3, 3), float(idx))
        sd[f"features.{idx}.bias"] = torch.zeros(co)
    p = tmp_path / "vgg19.pth"
    torch.save(sd, p)
    ws = V.load_vgg19_weights(str(p))
    assert [float(w.flat[0]) for w, _ in ws] == [0.0, 2.0, 5.0, 7.0, 10.0]


def test_cli_help():
    from click.testing import CliRunner
    from styletransfer_amd.clis import cli
    r = CliRunner().invoke(cli, ["gatys_st", "--help"])
    assert r.exit_code == 0 and "--steps" in r.output and "-cw" in r.output
    r = CliRunner().invoke(cli, ["fast_st", "train", "--help"])
    assert r.exit_code == 0 and "--batch-size" in r.output
    r = CliRunner().invoke(cli, ["fast_st", "convert-image", "--help"])
    assert r.exit_code == 0 and "--out-dir" in r.output


def test_loader_workers_per_rank(monkeypatch):
    """The GPU-conditioned COCO loader's decode workers are sized per rank: the usable
    CPUs (affinity, cgroup quota) split over the node's ranks (LOCAL_WORLD_SIZE), minus one
    for the rank's training loop, at most 16 (stransfer/dataset.py:141-197's loader, fed
    at the data-parallel step rate)."""
    from styletransfer_amd import dataset as D
    n = D.usable_cpus()
    assert n >= 1
    for lw in (1, 2, 8):
        assert D.default_workers(lw) == max(0, min(16, n // lw - 1))
    monkeypatch.setenv("LOCAL_WORLD_SIZE", "4")
    assert D.default_workers() == max(0, min(16, n // 4 - 1))


def test_parity_and_gram128_host_contracts():
    """Round-5 host logic without a GPU: the 128-channel fused Gram's slab geometry and its
    single-round gate, the parity-class upsampling slab size, the trained network's slab
    jobs (the two up convs get a parity-class job), and the new stx_conv2d contracts
    (wt16_up only on an upsampled-input split conv; mse_ref only with a 128-channel
    fused Gram) refused before any launch."""
    import ctypes as C
    import torch
    from styletransfer_amd import _native as N
    from styletransfer_amd import network, ops
    assert [ops.gram_tile_units(c) for c in (3, 64, 128, 256)] == [1, 1, 3, 10]
    # conv2_2 at Gatys 512^2 (256 tiles: one round) vs fast_st's B = 8 (512 blocks)
    assert ops.conv_gram_tiles(128, 128, 256, 256, n=1, in_mode=N.STX_IN_RELU) == 256
    assert ops.conv_gram_tiles(64, 128, 256, 256, n=1, in_mode=N.STX_IN_RAW) == 256
    assert ops.conv_gram_tiles(128, 128, 128, 128, n=8, in_mode=N.STX_IN_RELU) == 0
    assert ops.conv_gram_tiles(128, 128, 256, 256, n=1, in_mode=N.STX_IN_UPSAMPLE2) == 0
    L = N.lib()
    # [a][cin16][ry][b, rx][hi, lo][cout64] fp16
    assert L.stx_conv_weight16up_bytes(64, 32) == 2 * 64 * 2 * 4 * 2 * 64 * 2
    assert L.stx_conv_weight16up_bytes(20, 40) == 2 * 32 * 2 * 4 * 2 * 64 * 2
    net = network.ImageTransformNet(torch.rand(3, 8, 8), batch_size=1).to("cpu")
    convs = [m for m in net.modules() if isinstance(m, network.Conv2d)]
    ups = [c for c in convs if c._up_input]
    assert [tuple(c.weight.shape[:2]) for c in ups] == [(64, 128), (32, 64)]
    slabs = ops.TrainedSlabs(convs)
    kinds = [slabs._jobs[i].kind for i in range(slabs._njobs)]
    assert kinds.count(N.STX_WPREP_F16UP) == 2
    assert sum(s[5] is not None for s in slabs.slabs) == 2
    base = dict(x=16, y=32, n=1, cin=64, h=32, w=32, cout=64, ks=3, stride=1, pad=1,
                cin_pad=64, cout_pad=64, wt16=48, w_amax=64, in_amax=80)
    p = N.ConvParams(in_mode=N.STX_IN_RAW, hv=32, wv=32, ho=32, wo=32, wt16_up=96, **base)
    assert L.stx_conv2d(C.byref(p), None) == 1001 and b"wt16_up" in L.stx_last_error_string()
    # the parity-class taps assume the full x2 image: a truncated virtual size (hv < 2h or
    # wv < 2w, which UPSAMPLE2 otherwise accepts) is refused, not computed with the wrong
    # border
    for hv, wv in ((64, 63), (63, 64), (62, 64)):
        p = N.ConvParams(in_mode=N.STX_IN_UPSAMPLE2, hv=hv, wv=wv, ho=hv, wo=wv, wt16_up=96,
                         **base)
        assert L.stx_conv2d(C.byref(p), None) == 1001 and b"wt16_up" in L.stx_last_error_string()
    # unpool_out: only a raw-input split data gradient with cout 64 and its operands
    p = N.ConvParams(in_mode=N.STX_IN_RAW, hv=32, wv=32, ho=32, wo=32, unpool_out=1, **base)
    assert L.stx_conv2d(C.byref(p), None) == 1001 and b"unpool_out" in L.stx_last_error_string()
    p = N.ConvParams(in_mode=N.STX_IN_RAW, hv=32, wv=64, ho=32, wo=64, gram_part=112,
                     mse_ref=128, mse_parts=144, **dict(base, w=64))
    assert L.stx_conv2d(C.byref(p), None) == 1001 and b"mse_ref" in L.stx_last_error_string()
