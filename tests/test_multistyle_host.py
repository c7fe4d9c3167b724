"""Multi-style fast_st (conditional instance norm), the parts that need no GPU: the new
ABI struct and the argument checks of its two entry points, the network's structure and
checkpoint round trip, the style schedule of the trainer and the CLI's mix parser."""
import ctypes as C
import json

import pytest
import torch

from styletransfer_amd import _native as N
from styletransfer_amd import constants, network, train
from styletransfer_amd import weights as W

E_INVALID = 1001


def test_cin_job_mirror_matches_the_library():
    mirrors = 9  # stx_abi_layout's table (include/stx.h); stx_cin_job is its seventh entry
    count = N.lib().stx_abi_layout(None, 0)
    assert count == 2 * mirrors
    out = (C.c_longlong * count)()
    assert N.lib().stx_abi_layout(C.cast(out, C.c_void_p), count) == count
    assert N.CinJob._fields_[-1][0] == "accumulate"
    assert (C.sizeof(N.CinJob), N.CinJob.accumulate.offset) == (out[12], out[13])


def _job(**kw):
    """A well-formed job for both entry points (fake, never dereferenced pointers)."""
    f = dict(gtab=16, btab=32, gamma_n=48, beta_n=64, parts=80, dgtab=96, dbtab=112,
             dbias_in=128, c=32, accumulate=0)
    f.update(kw)
    return N.CinJob(**f)


@pytest.mark.parametrize("fn", ["stx_cin_mix", "stx_cin_param_grads"])
def test_cin_entry_points_refuse_malformed_arguments(fn):
    """STX_E_INVALID with a message, before any launch (no GPU is present here and the
    pointers are fake): njobs outside 1..STX_CIN_MAX, S <= 0, n <= 0, NULL mix, a job
    with c <= 0 or a NULL required pointer."""
    L = N.lib()
    f = getattr(L, fn)
    mix = 256

    def refused(jobs, njobs, mix, n, S, word):
        arr = (N.CinJob * max(len(jobs), 1))(*jobs)
        rc = f(arr, njobs, mix, n, S, None)
        msg = L.stx_last_error_string()
        assert rc == E_INVALID and fn.encode() in msg and word in msg, (rc, msg)

    refused([_job()], 0, mix, 4, 3, b"njobs")
    refused([_job()], -1, mix, 4, 3, b"njobs")
    refused([_job()] * (N.STX_CIN_MAX + 1), N.STX_CIN_MAX + 1, mix, 4, 3, b"njobs")
    assert f(None, 1, mix, 4, 3, None) == E_INVALID
    refused([_job()], 1, mix, 4, 0, b"S > 0")
    refused([_job()], 1, mix, 4, -2, b"S > 0")
    refused([_job()], 1, mix, 0, 3, b"n > 0")
    refused([_job()], 1, None, 4, 3, b"mix")
    refused([_job(), _job(c=0)], 2, mix, 4, 3, b"job 1")
    refused([_job(c=-5)], 1, mix, 4, 3, b"job 0")
    required = ("gtab", "btab", "gamma_n", "beta_n") if fn == "stx_cin_mix" else ("parts",)
    for name in required:
        refused([_job(), _job(), _job(**{name: None})], 3, mix, 4, 3, b"job 2")


S3 = 3


def _net():
    return network.MultiStyleTransformNet([torch.rand(3, 8, 8)] * S3, batch_size=2,
                                          style_names=["a.jpg", "b.jpg", "c.jpg"]).to("cpu")


def test_multistyle_net_structure_and_checkpoint_round_trip(tmp_path, monkeypatch):
    from styletransfer_amd.layers import ConditionalInstanceNorm2d, InstanceNorm2d
    net = _net()
    sd = net.state_dict()
    ref = W.itn_synthetic(4321)
    assert list(sd) == [k for k, _ in ref] and len(sd) == 62
    cin = [m for m in net.modules() if isinstance(m, ConditionalInstanceNorm2d)]
    assert len(cin) == 15 and all(isinstance(m, InstanceNorm2d) for m in cin)
    assert len({id(m.state) for m in cin}) == 1 and cin[0].state is net.cin
    n_in = 0
    for (k, v) in ref:
        if sd[k].dim() == 2:  # an IN tensor: a row per style
            assert tuple(sd[k].shape) == (S3,) + v.shape, k
            n_in += 1
        else:
            assert tuple(sd[k].shape) == v.shape, k
    assert n_in == 30 and sum(sd[k].shape[1] for k in sd if sd[k].dim() == 2) == 2 * 1600
    # the default ResidualBlock / ImageTransformNet are unchanged
    blk = network.ResidualBlock(8, 8)
    assert type(blk.insn1) is InstanceNorm2d and tuple(blk.insn1.weight.shape) == (8,)
    # checkpoint (state_dict only) + sidecar, written where static_train writes them
    monkeypatch.setattr(constants, "PROJECT_ROOT_PATH", str(tmp_path))
    monkeypatch.chdir(tmp_path)
    (tmp_path / "data" / "models").mkdir(parents=True)
    with torch.no_grad():
        for i, p in enumerate(net.parameters()):
            p.copy_(torch.randn(p.shape, generator=torch.Generator().manual_seed(i)))
    torch.save(net.state_dict(), "data/models/fast_mst_trio_epoch0.pth")
    net._checkpoint_written("trio")
    # a single-style checkpoint of a style with the same name is not picked up, nor is the
    # multi-style one by the single-style loader
    torch.save({"w": torch.zeros(1)}, "data/models/fast_st_trio_epoch0.pth")
    assert json.load(open("data/models/fast_mst_trio.styles.json")) == ["a.jpg", "b.jpg", "c.jpg"]
    assert network.MultiStyleTransformNet.load_style_names("trio") == ["a.jpg", "b.jpg", "c.jpg"]
    assert list(network._load_latest_model_weigths("fast_st", "trio")) == ["w"]
    back = _net()
    back.load_latest("trio")  # (adaptive_torch_load: weights_only=True)
    for k, v in net.state_dict().items():
        assert torch.equal(back.state_dict()[k], v), k
    with pytest.raises(AssertionError):
        back.load_latest("absent")


def test_mix_of_accepts_ids_and_weights():
    net = _net()
    assert torch.equal(net.mix_of(None, 2, "cpu"), torch.tensor([[1., 0, 0], [1, 0, 0]]))
    assert torch.equal(net.mix_of(2, 2, "cpu"), torch.tensor([[0., 0, 1], [0, 0, 1]]))
    assert torch.equal(net.mix_of(torch.tensor([1, 0]), 2, "cpu"),
                       torch.tensor([[0., 1, 0], [1, 0, 0]]))
    assert torch.equal(net.mix_of(torch.tensor([.25, .75, 0]), 2, "cpu"),
                       torch.tensor([[.25, .75, 0], [.25, .75, 0]]))
    m = torch.tensor([[.5, .5, 0], [0, 0, 1.]])
    assert torch.equal(net.mix_of(m, 2, "cpu"), m)
    for bad in (3, -1, torch.tensor([0, 3]), torch.tensor([0, 1, 2]), torch.rand(2, 4),
                torch.rand(4)):
        with pytest.raises(ValueError):
            net.mix_of(bad, 2, "cpu")


@pytest.mark.parametrize("B,S,world", [(8, 3, 2), (8, 3, 8), (4, 4, 1)])
def test_style_ids_slices_and_period(B, S, world):
    for t in range(2 * S + 1):
        full = train.style_ids(t, B, S)
        assert full == [(t * B + j) % S for j in range(B)]
        parts = [train.style_ids(t, B, S, r, world) for r in range(world)]
        assert all(len(p) == B // world for p in parts)
        assert sum(parts, []) == full
        # the schedule repeats after S steps, and after fewer only where t*B = 0 mod S
        assert train.style_ids(t + S, B, S) == full
        for d in range(1, S):
            assert (train.style_ids(t + d, B, S) == full) == ((d * B) % S == 0)
    # every style equally often over a period
    seen = sum((train.style_ids(t, B, S) for t in range(S)), [])
    assert all(seen.count(s) == B for s in range(S))
    with pytest.raises(ValueError):
        train.style_ids(0, B, S, 0, 3 if B % 3 else 5)
    with pytest.raises(ValueError):
        train.style_ids(0, B, S, world, world)


def test_parse_mix():
    names = ["a.jpg", "b.jpg", "c.jpg"]
    assert network.parse_mix(None, names) == [1.0, 0.0, 0.0]
    assert network.parse_mix("", names) == [1.0, 0.0, 0.0]
    assert network.parse_mix("b.jpg", names) == [0.0, 1.0, 0.0]
    assert network.parse_mix("a.jpg:0.3,b.jpg:0.9", names) == [0.25, 0.75, 0.0]
    assert network.parse_mix(" c.jpg:2 , a.jpg:2", names) == [0.5, 0.0, 0.5]
    for bad, word in (("d.jpg:1", "unknown style"), ("a.jpg:-0.5,b.jpg:1", ">= 0"),
                      ("a.jpg:0,b.jpg:0", "sum to 0"), ("a.jpg:x", "not a number"),
                      ("a.jpg:1,a.jpg:2", "twice"), ("a.jpg:nan", ">= 0"),
                      ("a.jpg:inf", "finite")):
        with pytest.raises(ValueError, match=word):
            network.parse_mix(bad, names)


def test_cli_multi_help_and_mix_rejection(tmp_path, monkeypatch):
    from click.testing import CliRunner
    from styletransfer_amd.clis import cli
    r = CliRunner().invoke(cli, ["fast_st", "train-multi", "--help"])
    assert r.exit_code == 0 and "--name" in r.output and "--synthetic" in r.output
    r = CliRunner().invoke(cli, ["fast_st", "convert-image-multi", "--help"])
    assert r.exit_code == 0 and "--mix" in r.output and "--out-dir" in r.output
    monkeypatch.setattr(constants, "PROJECT_ROOT_PATH", str(tmp_path))
    (tmp_path / "data" / "models").mkdir(parents=True)
    (tmp_path / "data" / "models" / "fast_mst_duo.styles.json").write_text('["a.jpg", "b.jpg"]')
    for mix, word in (("z.jpg:1", "unknown style"), ("a.jpg:-1", ">= 0"), ("a.jpg:0", "sum to 0")):
        r = CliRunner().invoke(cli, ["fast_st", "convert-image-multi", "x.jpg", "duo", "--mix", mix])
        assert r.exit_code == 2 and word in r.output, r.output
    r = CliRunner().invoke(cli, ["fast_st", "convert-image-multi", "x.jpg", "nobody"])
    assert r.exit_code == 2
