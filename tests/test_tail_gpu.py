"""The tail of a Gatys iteration without its two one-block launches: the
loss finalize and Adam's step-counter kernel run as rider blocks of the backward's compose
launch (stx_conv_weight_compose16_tail), and the Adam update reads the scalars the rider
left (stx_adam_step_prepared).  The riders run the bodies of the launches they replace, so
every value of an iteration must be the same bits with them and without (STX_TAIL_LOSS /
STX_TAIL_ADAM = 0 under STX_AB=1 put the two launches back), eagerly and as a graph replay.

128 x 128 images are the smallest at which the five taps take the paths they take at 512^2
(fused Gram in the conv epilogue for conv1_x and conv2_x, the 256-channel triangle kernel
on 32^2 pixels for conv3_1, the compose launch at B = 1)."""
import os

import pytest
import torch

from styletransfer_amd import _native as N
from styletransfer_amd import ops
from styletransfer_amd import vgg as V
from styletransfer_amd import weights as W

pytestmark = pytest.mark.gpu

H = 128
OFF = {"STX_TAIL_LOSS": "0", "STX_TAIL_ADAM": "0"}


class _Env:
    """A/B switches of the host path for the duration (N.knob reads them under STX_AB=1)."""

    def __init__(self, kv):
        self.kv, self.old = dict(kv, STX_AB="1"), {}

    def __enter__(self):
        for k, v in self.kv.items():
            self.old[k] = os.environ.get(k)
            os.environ[k] = v

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def feat(dev):
    return V.VGGFeatures(W.vgg19_synthetic(1234, 5), dev)


def _img(seed, b=1):
    return torch.from_numpy(W.synthetic_image(seed, (b, 3, H, H)))


def _state(e):
    torch.cuda.synchronize()
    return [t.detach().clone() for t in (e.x, e.grad, e.m, e.v, e.total, e.losses(),
                                         e.step_dev)]


def _engine_steps(feat, dev, env, graph, steps=4):
    """The engine's state after each of `steps` iterations (eager; or one eager iteration,
    which allocates every buffer, a capture, and steps - 1 replays), and the riders each
    compose call was given."""
    seen = []
    orig = ops.conv_weight_compose16

    def spy(*a, **k):
        seen.append((k.get("loss_job") is not None, k.get("adam_prepare") is not None))
        return orig(*a, **k)

    out = []
    with _Env(env):
        e = V.GatysEngine(feat, _img(11).to(dev), _img(12).to(dev), init=_img(13).to(dev))
        ops.conv_weight_compose16 = spy
        try:
            for it in range(steps):
                if graph and it == 0:
                    e.capture(warmup=1)  # (runs the one eager iteration)
                else:
                    e.step()
                out.append(_state(e))
                assert float(e.st.amax.abs().max()) == 0.0  # cleared for the next forward
        finally:
            ops.conv_weight_compose16 = orig
    return out, seen


@pytest.fixture(scope="module")
def eager_off(feat, dev):
    return _engine_steps(feat, dev, OFF, graph=False)


def _same(got, want):
    names = ("x", "grad", "m", "v", "total", "losses", "step_dev")
    for it, (g, w) in enumerate(zip(got, want)):
        for n, a, b in zip(names, g, w):
            assert not torch.isnan(b.float()).any(), (it, n)
            assert torch.equal(a, b), (it, n)


def test_riders_eager(feat, dev, eager_off):
    want, seen_off = eager_off
    assert seen_off and not any(l or a for l, a in seen_off)  # compose taken, no riders
    got, seen = _engine_steps(feat, dev, {}, graph=False)
    assert len(seen) == 4 and all(l and a for l, a in seen)   # both riders, every iteration
    _same(got, want)
    assert [int(s[-1]) for s in got] == [1, 2, 3, 4]


@pytest.mark.parametrize("env", [{}, {"STX_TAIL_LOSS": "0"}, {"STX_TAIL_ADAM": "0"}, OFF])
def test_riders_graph_replay(feat, dev, eager_off, env):
    """Three replays of a captured iteration against the eager run without riders: both
    riders, each alone, and neither."""
    got, seen = _engine_steps(feat, dev, env, graph=True)
    # (the eager iteration and the captured one)
    assert seen == [(env.get("STX_TAIL_LOSS") != "0", env.get("STX_TAIL_ADAM") != "0")] * 2
    _same(got, eager_off[0])


def test_deferred_loss_without_compose(feat, dev):
    """B = 2 takes no compose launch: loss_backward launches the deferred finalize itself,
    and the losses and total are those of the undeferred run when it returns."""
    targets = [t.reshape(t.shape[-2:]).contiguous() for t in feat.style_targets(_img(11).to(dev))]
    x = _img(21, b=2).to(dev).contiguous()
    c4 = V.content_target(feat, _img(22, b=2).to(dev)).clone()
    res = []
    for defer in (False, True):
        total = torch.full((), float("nan"), device=dev)
        st = V.loss_forward(feat, targets, x, c4, folded_weights=(1e5, 1.0), total=total,
                            defer_loss=defer)
        assert (st.loss_job is not None) == defer
        prep = ops.AdamPrepare(torch.zeros(1, dtype=torch.int32, device=dev),
                               torch.zeros(16, device=dev))
        dx = V.loss_backward(feat, st, feature_grad=False, adam_prepare=prep)
        torch.cuda.synchronize()
        assert st.loss_job is None and not prep.done
        res.append((total.clone(), V.loss_values(st).clone(), dx.clone()))
    for a, b in zip(*res):
        assert not torch.isnan(a).any() and torch.equal(a, b)


def test_lbfgs_deferred_loss(feat, dev):
    """GatysLBFGS defers the loss finalize onto the compose launch: two outer steps give the
    total, x and evaluation count of the run with the finalize as its own launch."""
    res = []
    for env in (OFF, {}):
        with _Env(env):
            e = V.GatysLBFGS(feat, _img(11).to(dev), _img(12).to(dev), init=_img(13).to(dev))
            e.run(2)
            torch.cuda.synchronize()
            res.append((e.total.clone(), e.x.clone(), e.func_evals))
    assert res[0][2] == res[1][2] and res[0][2] > 2
    assert torch.isfinite(res[0][0]) and torch.equal(res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1])


def test_adam_split(dev):
    """stx_adam_step_prepared after the prepare rider of a real compose launch (C = 64)
    against stx_adam_step_clear: the same p, m, v over three steps on n = 1003 elements (a
    scalar tail after the 16-byte body), `clear` zeroed, the counter advanced by one per
    step; the loss rider beside it gives stx_loss_finalize's values, and the slab and its
    bound are those of the plain compose launch."""
    g = torch.Generator(device="cpu").manual_seed(3)
    n, cout, cin = 1003, 64, 8
    w = (torch.randn(cout, cin, 3, 3, generator=g) * 0.05).to(dev)
    A = (torch.randn(1, cout, cout, generator=g) * 1e-3).to(dev)
    w_amax, a_amax = ops.amax(w), ops.amax(A)
    parts = [torch.randn(k, generator=g).to(dev) for k in (64, 192, 640, 5)]
    lparts = [(p.data_ptr(), p.numel(), 1.0 / (i + 3)) for i, p in enumerate(parts)]
    extra = torch.randn(2, generator=g).to(dev)
    wts = [0.5, 2.0, 3.0, 1e5, 1.0, 0.25]
    want_l, want_t = torch.zeros(4, device=dev), torch.zeros((), device=dev)
    ops.loss_finalize(lparts, want_l, extra=extra, weights=wts, total=want_t)
    b0 = torch.zeros(N.STX_AMAX_SLOTS, device=dev)
    slab0 = ops.conv_weight_compose16(A, a_amax, w, w_amax, b0).clone()

    p0 = torch.randn(n, generator=g).to(dev)
    st = [[p0.clone(), torch.zeros(n, device=dev), torch.zeros(n, device=dev),
           torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(16, device=dev)]
          for _ in range(2)]
    clear = torch.empty(1000, device=dev)
    for it in range(3):
        grad = (torch.randn(n, generator=g) * (it + 1)).to(dev)
        p, m, v, step, ws = st[0]
        clear.fill_(5.0)
        ops.adam_step(p, grad, m, v, step, ws, lr=0.01, beta1=0.8, beta2=0.99, clear=clear)
        assert float(clear.abs().max()) == 0.0
        p, m, v, step, ws = st[1]
        clear.fill_(5.0)
        got_l = torch.full((4,), float("nan"), device=dev)
        got_t = torch.full((), float("nan"), device=dev)
        job = ops.LossFinalizeJob(lparts, got_l, extra=extra, weights=wts, total=got_t)
        prep = ops.AdamPrepare(step, ws, 0.01, 0.8, 0.99)
        b1 = torch.zeros(N.STX_AMAX_SLOTS, device=dev)
        slab1 = ops.conv_weight_compose16(A, a_amax, w, w_amax, b1, loss_job=job,
                                          adam_prepare=prep)
        assert job.done and prep.done
        assert float(clear.min()) == 5.0  # the rider clears nothing
        ops.adam_step_prepared(p, grad, m, v, ws, beta1=0.8, beta2=0.99, clear=clear)
        torch.cuda.synchronize()
        assert float(clear.abs().max()) == 0.0
        assert int(step) == it + 1 == int(st[0][3])
        for a, b in zip(st[0][:3] + [want_l, want_t, slab0, b0],
                        st[1][:3] + [got_l, got_t, slab1, b1]):
            assert torch.equal(a, b)
    # each rider alone
    got_l.fill_(float("nan"))
    ops.conv_weight_compose16(A, a_amax, w, w_amax, b1, loss_job=ops.LossFinalizeJob(
        lparts, got_l, extra=extra, weights=wts, total=got_t))
    ops.conv_weight_compose16(A, a_amax, w, w_amax, b1,
                              adam_prepare=ops.AdamPrepare(st[1][3], st[1][4], 0.01, 0.8, 0.99))
    torch.cuda.synchronize()
    assert torch.equal(got_l, want_l) and int(st[1][3]) == 4
