"""Scale control without a GPU: the fp64 restatement (tests/scale_ref.py) against torch's
antialiased interpolate on the CPU, the library's host plan against the restatement, the
argument checks of the resampler, scale.check_sizes, the per-tap weight helper and the
command-line switches."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import scale_ref as SR

PAIRS = [((5, 7), (3, 2)), ((3, 2), (9, 11)), ((37, 53), (19, 27)), ((37, 53), (74, 106)),
         ((64, 64), (128, 128)), ((128, 128), (64, 64)), ((100, 100), (141, 141)),
         ((141, 141), (100, 100)), ((96, 96), (96, 96))]
IDS = [f"{a[0]}x{a[1]}-{b[0]}x{b[1]}" for a, b in PAIRS]
FILTERS = {"triangle": (0, "bilinear"), "cubic": (1, "bicubic")}
AXES = sorted({(a[i], b[i]) for a, b in PAIRS for i in (0, 1)})


@pytest.mark.parametrize("filter", list(FILTERS))
@pytest.mark.parametrize("pair", PAIRS, ids=IDS)
def test_ref_is_torch_antialiased_interpolate(pair, filter):
    (hi, wi), (ho, wo) = pair
    x = torch.randn(2, 3, hi, wi, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    ref = F.interpolate(x, size=(ho, wo), mode=FILTERS[filter][1], align_corners=False,
                        antialias=True)
    got = SR.resize(x.numpy(), ho, wo, filter)
    err = float(np.abs(got - ref.numpy()).max())
    print(f"{filter} {pair}: {err:.2e}")
    assert err <= 1e-13


@pytest.mark.parametrize("filter", list(FILTERS))
@pytest.mark.parametrize("axis", AXES, ids=[f"{a}-{b}" for a, b in AXES])
def test_plan_is_the_restatement(axis, filter):
    from styletransfer_amd import _native as N
    L = N.lib()
    n_in, n_out = axis
    first, count, w64, k = SR.plan(n_in, n_out, filter)
    code = FILTERS[filter][0]
    assert L.stx_resample_plan(n_in, n_out, code, None, None, None, 0) == k
    kk = k + 2  # room to spare: the padding must be zero
    f = np.full(n_out, -7, np.int32)
    c = np.full(n_out, -7, np.int32)
    w = np.full((n_out, kk), 9.0, np.float32)
    assert L.stx_resample_plan(n_in, n_out, code, f.ctypes.data, c.ctypes.data, w.ctypes.data,
                               kk) == k
    assert np.array_equal(f, first) and np.array_equal(c, count)
    assert np.all(np.abs(w[:, :k].astype(np.float64) - w64) <= 2.0 ** -24 * np.abs(w64))
    for i in range(n_out):
        assert not w[i, count[i]:].any()
    # the ops wrapper hands out the same tables
    from styletransfer_amd import ops
    f2, c2, w2, k2 = ops.resample_plan(n_in, n_out, filter)
    assert k2 == k and np.array_equal(f2, first) and np.array_equal(c2, count)
    assert np.array_equal(w2, w[:, :k])


def _err(L):
    return L.stx_last_error_string().decode()


def test_plan_rejections():
    from styletransfer_amd import _native as N
    L = N.lib()
    for args in ((0, 4, 0), (4, 0, 1), (-3, 4, 0), (4, -1, 1), (8, 4, 2), (8, 4, -1)):
        rc = L.stx_resample_plan(*args, None, None, None, 0)
        assert rc < 0, args
        assert "stx_resample_plan" in _err(L)
    f = np.zeros(4, np.int32)
    w = np.zeros((4, 1), np.float32)
    assert L.stx_resample_plan(8, 4, 0, f.ctypes.data, f.ctypes.data, w.ctypes.data, 1) < 0
    assert "room for 1" in _err(L)
    assert L.stx_resample_plan(8, 4, 0, f.ctypes.data, None, w.ctypes.data, 4) < 0


def test_resample2d_rejections_before_launch():
    """Every call fails in the argument checks: no pointer is read and nothing is launched
    (the addresses are made up)."""
    from styletransfer_amd import _native as N
    L = N.lib()
    x, y, t, ws = 0x10000, 0x900000, 0x2000000, 0x3000000
    nc, hi, wi, ho, wo = 3, 8, 8, 16, 16
    need = L.stx_resample2d_ws(nc, hi, wi, ho, wo)
    assert need == nc * hi * wo * 4
    assert L.stx_resample2d_ws(nc, hi, wi, hi, wo) == 0 == L.stx_resample2d_ws(nc, hi, wi, ho, wi)

    def call(x=x, y=y, nc=nc, hi=hi, wi=wi, ho=ho, wo=wo, xt=(t, t, t, 4), yt=(t, t, t, 4), ws=ws,
             ws_bytes=need):
        return L.stx_resample2d(x, y, nc, hi, wi, ho, wo, *xt, *yt, ws, ws_bytes, None)

    cases = {
        "hi=0": dict(hi=0), "wo=-1": dict(wo=-1), "nc=0": dict(nc=0), "nc": dict(nc=65536),
        "side": dict(wo=4100), "x tables": dict(xt=(None, None, None, 0)),
        "y tables": dict(yt=(t, None, t, 4)), "y k": dict(yt=(t, t, t, 0)),
        "ws short": dict(ws_bytes=need - 1), "ws null": dict(ws=None),
        "alias": dict(y=x), "overlap": dict(y=x + 64), "x null": dict(x=None),
    }
    for name, kw in cases.items():
        # STX_E_INVALID / STX_E_WORKSPACE, not a HIP error: refused by the checks
        assert call(**kw) in (1001, 1002), name
        assert "stx_resample2d" in _err(L), name
    call(y=x)
    assert "alias" in _err(L)
    call(ws_bytes=need - 1)
    assert "workspace" in _err(L)


def test_check_sizes():
    from styletransfer_amd import scale
    for bad in ([], [256, 256], [512, 256], [130, 256], [256, scale.MAX_SIDE + 4], [0, 64],
                [-64, 64], [64.5, 128]):
        with pytest.raises(ValueError):
            scale.check_sizes(bad)
    assert scale.check_sizes([64, 100]) == [64, 100]
    assert scale.check_sizes((scale.MAX_SIDE,)) == [scale.MAX_SIDE]
    assert scale.level_steps(3, 2) == [3, 3] and scale.level_steps([1, 2], 2) == [1, 2]
    with pytest.raises(ValueError):
        scale.level_steps([1, 2, 3], 2)


def test_tap_weights():
    from styletransfer_amd import vgg as V
    sw = 100_000.0
    got = V.tap_weights(sw)
    assert got == [sw] * 5 and all(type(v) is float for v in got)
    assert V.tap_weights(100_000) == [sw] * 5
    assert V.tap_weights(sw, [1, 0.5, 2, 0, 0.25]) == [sw, 0.5 * sw, 2 * sw, 0.0, 0.25 * sw]
    assert V.tap_weights([1.0, 2.0, 3.0, 4.0, 5.0]) == [1.0, 2.0, 3.0, 4.0, 5.0]
    for bad in ([1, 1, 1, 1], [1, 1, 1, 1, -1], [1, 1, 1, 1, float("nan")]):
        with pytest.raises(ValueError):
            V.tap_weights(sw, bad)
    with pytest.raises(ValueError):
        V.tap_weights([1.0, 2.0])
    # an engine without per-tap multipliers passes the plain float on, as before
    assert V._folded_style(100_000, None) == sw and type(V._folded_style(100_000, None)) is float


BAD_CLI = [
    (["gatys_st", "c.jpg", "s.jpg", "--scales", "64,x"], "--scales"),
    (["gatys_st", "c.jpg", "s.jpg", "--scales", "128,64"], "--scales"),
    (["gatys_st", "c.jpg", "s.jpg", "--scales", "64,130"], "--scales"),
    (["gatys_st", "c.jpg", "s.jpg", "--scales", ""], "--scales"),
    (["gatys_st", "c.jpg", "s.jpg", "--scales", "64,128", "--scale-steps", "5"], "--scale-steps"),
    (["gatys_st", "c.jpg", "s.jpg", "--scales", "64,128", "--scale-steps", "5,a"],
     "--scale-steps"),
    (["gatys_st", "c.jpg", "s.jpg", "--scale-steps", "5,5"], "--scale-steps"),
    (["gatys_st", "c.jpg", "s.jpg", "--layer-weights", "0,0,0,0,0"], "--layer-weights"),
    (["gatys_st", "c.jpg", "s.jpg", "--layer-weights", "1,1,1,1"], "--layer-weights"),
    (["gatys_st", "c.jpg", "s.jpg", "--layer-weights", "1,1,-1,1,1"], "--layer-weights"),
    (["gatys_st", "c.jpg", "s.jpg", "--coarse-style", "t.jpg", "--fine-taps", "0"], "--fine-taps"),
    (["gatys_st", "c.jpg", "s.jpg", "--coarse-style", "t.jpg", "--fine-taps", "5"], "--fine-taps"),
    (["gatys_guided", "c.jpg", "-r", "s.jpg:m.png", "--scales", "64,64"], "--scales"),
    (["gatys_guided", "c.jpg", "-r", "s.jpg:m.png", "--scales", "64,128", "--scale-steps",
      "1,2,3"], "--scale-steps"),
]


@pytest.mark.parametrize("argv,option", BAD_CLI, ids=[" ".join(a[1:]) for a, _ in BAD_CLI])
def test_cli_refuses_bad_values_before_loading(argv, option):
    """The image paths do not exist: a run that got as far as loading them would fail with
    another error, one that does not name the option."""
    from click.testing import CliRunner
    from styletransfer_amd.clis import cli
    r = CliRunner().invoke(cli, argv)
    assert r.exit_code == 2, r.output + repr(r.exception)
    assert option in r.output


def test_cli_help_names_the_switches():
    from click.testing import CliRunner
    from styletransfer_amd.clis import cli
    out = CliRunner().invoke(cli, ["gatys_st", "--help"]).output
    for name in ("--scales", "--scale-steps", "--layer-weights", "--coarse-style", "--fine-taps",
                 "--mix-steps"):
        assert name in out
    out = CliRunner().invoke(cli, ["gatys_guided", "--help"]).output
    assert "--scales" in out and "--scale-steps" in out
