"""Multi-style fast_st on the GPU: conditional instance norm (N styles per network).

The reference project has no multi-style network, so the yardstick is the torch CPU
functional restatement (tests/cin_ref.py over tests/forced_ref.py) in fp64 and fp32 under
the three-way protocol of tests/test_itn_masks_gpu.py: the HIP error against fp64 is at
most max(K x the torch-fp32 error against fp64, FLOOR), with the HIP branch decisions
forced where a gradient crosses a ReLU.  Where the new code only re-routes bits the
single-style path already produces (a one-hot mix, all samples on one style), equality is
exact.
"""
import ctypes as C
import os
import shutil

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

import cin_ref as CR
import forced_ref as R
from conftest import REPO
from styletransfer_amd import _native as N
from styletransfer_amd import autograd as A
from styletransfer_amd import constants, network, ops
from styletransfer_amd import vgg as V
from styletransfer_amd import weights as W
from styletransfer_amd.train import FastStTrainer, MultiStyleTrainer, style_ids

pytestmark = pytest.mark.gpu

K, FLOOR = 3.0, 2e-5  # tests/test_itn_masks_gpu.py
U = 2.0 ** -24        # fp32 unit roundoff
SEEDS = (4321, 4322, 4323)  # style tables: independent seeds; convolutions of the first


def _rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _within(name, hip, r32, r64):
    e, r = _rel(hip, r64), _rel(r32, r64)
    print(f"{name}: hip {e:.2e} fp32 {r:.2e}")
    assert e <= max(K * r, FLOOR), f"{name}: hip {e:.2e} vs fp32 {r:.2e}"


@pytest.fixture
def project_root(tmp_path, monkeypatch):
    """A scratch PROJECT_ROOT with the data layout the CLI reads and the CWD there."""
    for rel_path in ("data/dancing.jpg", "data/styles/picasso.jpg"):
        dst = tmp_path / rel_path
        dst.parent.mkdir(parents=True, exist_ok=True)
        shutil.copy(os.path.join(REPO, rel_path), dst)
    monkeypatch.setattr(constants, "PROJECT_ROOT_PATH", str(tmp_path))
    monkeypatch.chdir(tmp_path)
    return tmp_path


def _tables(S, cs, seed):
    g = torch.Generator().manual_seed(seed)
    return [(1 + 0.1 * torch.randn(S, c, generator=g), 0.1 * torch.randn(S, c, generator=g))
            for c in cs]


def _convex(n, S, seed):
    m = torch.rand(n, S, generator=torch.Generator().manual_seed(seed)) + 0.05
    return (m / m.sum(1, keepdim=True)).float()


# ------------------------------------------------------------------ the two kernels
def test_cin_mix_one_hot_exact_and_convex_fp64(dev):
    """stx_cin_mix, S=3, n=4, two layers (c = 32, 128) in one launch: one-hot rows
    reproduce the table rows bit for bit; convex rows are within the fma chain's bound
    S * 2^-24 * sum_s |w * table| per element of fp64."""
    S, n, ids = 3, 4, [0, 2, 1, 2]
    tabs = _tables(S, (32, 128), 7)
    dtabs = [(g.to(dev), b.to(dev)) for g, b in tabs]
    rows = ops.cin_mix(dtabs, CR.one_hot(ids, S, torch.float32).to(dev))
    for (g, b), (gn, bn) in zip(tabs, rows):
        assert torch.equal(gn.cpu(), g[ids]) and torch.equal(bn.cpu(), b[ids])
    mix = _convex(n, S, 8)
    rows = ops.cin_mix(dtabs, mix.to(dev))
    for (g, b), (gn, bn) in zip(tabs, rows):
        for t, out in ((g, gn), (b, bn)):
            want = mix.double() @ t.double()
            bound = S * U * (mix.double().abs() @ t.double().abs())
            err = (out.cpu().double() - want).abs()
            print(f"cin_mix c={t.shape[1]}: max err/bound {float((err / bound).max()):.3f}")
            assert bool((err <= bound).all())


def _cin_grads(parts, mix, outs, accumulate, dev):
    """stx_cin_param_grads over [(parts [n*c][3], (dg, db, dbias))] in ONE launch."""
    n, S = mix.shape
    jobs = [N.CinJob(None, None, None, None, p.data_ptr(), dg.data_ptr(), db.data_ptr(),
                     dc.data_ptr(), dg.shape[1], int(accumulate))
            for p, (dg, db, dc) in zip(parts, outs)]
    N.check(N.lib().stx_cin_param_grads((N.CinJob * len(jobs))(*jobs), len(jobs),
                                        mix.data_ptr(), n, S, ops._stream()), "cin grads")


def _in_grads(parts, n, outs, accumulate):
    """The single-style reduction (stx_instnorm_param_grads) of the same partials."""
    jobs = [N.PGradJob(p.data_ptr(), dg.data_ptr(), db.data_ptr(), dc.data_ptr(), n,
                       dg.shape[0], int(accumulate), 0) for p, (dg, db, dc) in zip(parts, outs)]
    N.check(N.lib().stx_instnorm_param_grads((N.PGradJob * len(jobs))(*jobs), len(jobs),
                                             ops._stream()), "in grads")


def test_cin_param_grads_single_style_bits_and_mixed_fp64(dev):
    """stx_cin_param_grads, S=3, n=4, c = 32 and 128 in one launch.  All samples on one
    style: that row has stx_instnorm_param_grads' bits on the same partials, the other
    rows are exactly 0 (untouched with accumulate), the conv-bias sums are the same bits.
    Mixed ids and a convex mix: within n * 2^-24 * sum_k |w * parts| of fp64."""
    S, n, cs, s = 3, 4, (32, 128), 1
    g = torch.Generator().manual_seed(11)
    parts_h = [torch.randn(n * c, 3, generator=g) for c in cs]
    parts = [p.to(dev) for p in parts_h]

    def fresh(shape_g, fill):
        return [(torch.full((*shape_g, c), fill, device=dev), torch.full((*shape_g, c), fill,
                                                                         device=dev),
                 torch.full((c,), fill, device=dev)) for c in cs]
    mix = CR.one_hot([s] * n, S, torch.float32).to(dev)
    got, want = fresh((S,), float("nan")), fresh((), float("nan"))
    _cin_grads(parts, mix, got, False, dev)
    _in_grads(parts, n, want, False)
    for (dg, db, dc), (wg, wb, wc) in zip(got, want):
        assert torch.equal(dg[s], wg) and torch.equal(db[s], wb) and torch.equal(dc, wc)
        for o in (r for r in range(S) if r != s):
            assert not dg[o].any() and not db[o].any()
    # accumulate: onto random contents; the other rows keep theirs
    pre = [tuple(torch.randn(t.shape, generator=g).to(dev) for t in o) for o in got]
    got = [tuple(t.clone() for t in o) for o in pre]
    want = [(o[0][s].clone(), o[1][s].clone(), o[2].clone()) for o in pre]
    _cin_grads(parts, mix, got, True, dev)
    _in_grads(parts, n, want, True)
    for (dg, db, dc), (wg, wb, wc), (pg, pb, _) in zip(got, want, pre):
        assert torch.equal(dg[s], wg) and torch.equal(db[s], wb) and torch.equal(dc, wc)
        for o in (r for r in range(S) if r != s):
            assert torch.equal(dg[o], pg[o]) and torch.equal(db[o], pb[o])
    # mixed ids / convex weights against fp64
    for mixh in (CR.one_hot([0, 2, 1, 2], S, torch.float32), _convex(n, S, 12)):
        got = fresh((S,), float("nan"))
        _cin_grads(parts, mixh.to(dev), got, False, dev)
        for p, (dg, db, dc) in zip(parts_h, got):
            p3 = p.double().reshape(n, -1, 3)
            m = mixh.double()
            for j, out in ((0, dg), (1, db)):
                err = (out.cpu().double() - m.t() @ p3[..., j]).abs()
                assert bool((err <= n * U * (m.t().abs() @ p3[..., j].abs())).all())
            err = (dc.cpu().double() - p3[..., 2].sum(0)).abs()
            assert bool((err <= n * U * p3[..., 2].abs().sum(0)).all())


# ------------------------------------------------------------------ the layer
@pytest.mark.parametrize("res", [0, 1])
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("shape", [(8, 128, 64, 64), (2, 32, 256, 256), (4, 128, 16, 16),
                                   (3, 5, 7, 9)])
def test_cond_instance_norm_fwd_bwd_fp64(dev, shape, relu, res):
    """ConditionalInstanceNorm2d forward + backward (outside a training step: the table
    gradients are reduced per call) against fp64 with the ReLU mask forced from the HIP
    output, at shapes that reach the pipelined 64^2 kernels, the 256^2 register kernel,
    the small register kernel and the unaligned loop kernel: y, dx, dres, both tables,
    and the conv-bias gradient.

    The conv-bias gradient sum(du) is 0 in exact arithmetic (IN removes the plane mean),
    so it is bounded absolutely: du = gamma rstd / hw * (hw g - sum g - xhat sum(g xhat))
    per element, so per channel the rounding of the terms and of the three block sums
    (depth <= 64 serial + 10 tree levels each) is at most
    128 * 2^-24 * sum_k |gamma_k| rstd_k (sum|g| + |sum g| + |sum g xhat|)."""
    from styletransfer_amd.layers import ConditionalInstanceNorm2d
    n, c, h, w = shape
    S = 3
    g = torch.Generator().manual_seed(1000 * n + 10 * relu + res)
    x0, up = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    r0 = torch.randn(shape, generator=g) if res else None
    (gt, bt), = _tables(S, (c,), 5)
    mix = _convex(n, S, 6)
    mix[::2] = CR.one_hot([k % S for k in range(0, n, 2)], S, torch.float32)  # some one-hot
    layer = ConditionalInstanceNorm2d(S, c).to(dev)
    layer.load_state_dict({"weight": gt, "bias": bt})
    layer.state.set(mix.to(dev))
    cb = torch.nn.Parameter(torch.zeros(c, device=dev))
    x = x0.to(dev).requires_grad_()
    r = r0.to(dev).requires_grad_() if res else None
    y = layer(x, relu=bool(relu), res=r, conv_bias=cb)
    y.backward(up.to(dev))
    mask = (y.detach() > 0).cpu()
    hip = {"y": y.detach().cpu(), "x": x.grad.cpu(), "gtab": layer.weight.grad.cpu(),
           "btab": layer.bias.grad.cpu()}
    if res:
        hip["res"] = r.grad.cpu()

    def ref(dtype):
        t = {"x": x0.to(dtype).clone().requires_grad_(),
             "gtab": gt.to(dtype).clone().requires_grad_(),
             "btab": bt.to(dtype).clone().requires_grad_(),
             "cb": torch.zeros(c, dtype=dtype, requires_grad=True)}
        # the conv bias is already inside x: it enters with value 0 and gradient sum(du)
        u = t["x"] + (t["cb"] - t["cb"].detach())[None, :, None, None]
        if res:
            t["res"] = r0.to(dtype).clone().requires_grad_()
            u = u + t["res"]
        yr = CR.cond_norm(u, t["gtab"], t["btab"], mix.to(dtype))
        if relu:
            yr = yr * mask.to(dtype)
        yr.backward(up.to(dtype))
        return {"y": yr.detach(), **{k: v.grad for k, v in t.items()}}, u.detach()
    (r64, u64), (r32, _) = ref(torch.float64), ref(torch.float32)
    for k in hip:
        _within(f"{shape} relu={relu} res={res} {k}", hip[k], r32[k], r64[k])
    gg = up.double() * (mask.double() if relu else 1.0)
    var, mu = torch.var_mean(u64, dim=(2, 3), unbiased=False, keepdim=True)
    rstd = (var + 1e-5).rsqrt()
    xh = (u64 - mu) * rstd
    terms = gg.abs().sum((2, 3)) + gg.sum((2, 3)).abs() + (gg * xh).sum((2, 3)).abs()
    bound = 128 * U * ((mix.double() @ gt.double()).abs() * rstd[:, :, 0, 0] * terms).sum(0)
    err = cb.grad.cpu().double().abs()
    print(f"{shape} relu={relu} res={res} conv bias: max |sum du| / bound "
          f"{float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())


# ------------------------------------------------------------------ the network
B4, H64, S3 = 4, 64, 3


def _styles(n, h, seed=71):
    return [torch.from_numpy(W.synthetic_image(seed + i, (1, 3, h, h))) for i in range(n)]


def _multi(sd, styles, dev, batch_size=B4):
    net = network.MultiStyleTransformNet([s.to(dev) for s in styles], batch_size)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd})
    return net


def test_one_style_is_the_single_style_path_bit_for_bit(dev):
    """B=4, 64^2, S=3, every sample on style s: the forward equals ImageTransformNet loaded
    with row s, and after one _fwd_bwd every conv gradient equals the single-style
    trainer's, table row s equals its IN gradients and the other rows are zero -- the same
    kernels see the same bits."""
    s = 1
    styles = _styles(S3, H64)
    batch = torch.from_numpy(W.synthetic_image(81, (B4, 3, H64, H64))).to(dev)
    sd = CR.multi_sd(SEEDS)
    mnet = _multi(sd, styles, dev)
    snet = network.ImageTransformNet(styles[s].to(dev), B4)
    snet.load_state_dict({k: torch.from_numpy(v) for k, v in CR.single_sd(sd, s)})
    with torch.no_grad():
        assert torch.equal(mnet(batch, style=s), snet(batch))
        assert torch.equal(mnet(batch, style=torch.tensor([s] * B4)), snet(batch))
    trm = MultiStyleTrainer(mnet, [t.to(dev) for t in styles])
    trs = FastStTrainer(snet, styles[s].to(dev))
    trm.set_styles(B4, [s] * B4)
    lm, ls = trm._fwd_bwd(batch), trs._fwd_bwd(batch)
    torch.cuda.synchronize()
    assert torch.equal(lm, ls), (float(lm), float(ls))
    pm = dict(mnet.named_parameters())
    for k, p in snet.named_parameters():
        gm = pm[k].grad
        if k in CR.IN_KEYS:
            assert tuple(gm.shape) == (S3,) + tuple(p.shape)
            assert torch.equal(gm[s], p.grad), k
            assert not gm[[o for o in range(S3) if o != s]].any(), k
        else:
            assert torch.equal(gm, p.grad), k


def test_mixed_style_step_three_way(dev, monkeypatch):
    """One MultiStyleTrainer forward/backward at B=4, 64^2, S=3, ids [0, 2, 1, 2] against
    the forced-branch fp64 restatement: every parameter gradient (the tables included)
    within max(3 x fp32's error, 2e-5), the loss within 1e-4, and the flips against an
    unforced fp64 run at most max(3 x the fp32 run's, 16) (the golden case's 8 at twice
    its batch)."""
    ids = [0, 2, 1, 2]
    styles = _styles(S3, H64)
    batch = torch.from_numpy(W.synthetic_image(82, (B4, 3, H64, H64)))
    sd = CR.multi_sd(SEEDS)
    vgg = V.load_vgg19_weights()
    net = _multi(sd, styles, dev)
    tr = MultiStyleTrainer(net, [t.to(dev) for t in styles])
    tr.set_styles(B4, ids)
    with R.HipBranchSpy(net, V, monkeypatch) as spy:
        loss_hip = float(tr._fwd_bwd(batch.to(dev)))
    torch.cuda.synchronize()
    bi, bv = spy.itn, spy.vgg
    g_hip = {k: p.grad.detach().cpu().clone() for k, p in net.named_parameters()}
    s_np, b_np = [s.numpy() for s in styles], batch.numpy()
    ni, nv = CR.natural_branches_cond(sd, vgg, b_np, ids, S3)
    ni32, nv32 = CR.natural_branches_cond(sd, vgg, b_np, ids, S3, torch.float32)
    flips = R.count_flips(bi, ni) + R.count_flips(bv, nv)
    flips32 = R.count_flips(ni32, ni) + R.count_flips(nv32, nv)
    g64, l64 = CR.forced_grads_cond(sd, vgg, s_np, b_np, ids, bi, bv, torch.float64)
    g32, _ = CR.forced_grads_cond(sd, vgg, s_np, b_np, ids, bi, bv, torch.float32)
    gmax = max(float(g.norm()) for g in g64.values())
    worst = []
    for k, t in g64.items():
        assert g_hip[k].shape == t.shape, k
        if float(t.norm()) < 1e-7 * gmax:
            # conv bias feeding an InstanceNorm: exactly 0 in exact arithmetic
            assert float(g_hip[k].norm()) < 1e-5 * gmax, k
            continue
        e, r = _rel(g_hip[k], t), _rel(g32[k], t)
        worst.append((e / max(r, FLOOR), e, r, k))
    worst.sort()
    print(f"flips {flips} (fp32 reference: {flips32}); loss hip {loss_hip:.7g} fp64 {l64:.7g}; "
          f"worst (ratio, hip, fp32, param): {worst[-3:]}")
    for _, e, r, k in worst:
        assert e <= max(K * r, FLOOR), f"{k}: hip {e:.2e} vs fp32 {r:.2e} (forced branches)"
    assert abs(loss_hip - l64) <= 1e-4 * abs(l64)
    assert flips <= max(3 * flips32, 16), (flips, flips32)


@pytest.mark.parametrize("hw", [(64, 64), (24, 40)])
def test_vgg_loss_per_sample_gram_targets_fp64(dev, monkeypatch, hw):
    """The loss network alone with a DISTINCT Gram target per sample ([B][C][C], B=3) --
    the kernels' target_batched path, which the multi-style trainer is the first to use:
    the seven loss values and dx against fp64 with the VGG branches forced, at 64x64 (Gram
    partials fused into the conv epilogues) and 24x40 (the unfused Gram path)."""
    B = 3
    h, w = hw
    feat = V.VGGFeatures(V.load_vgg19_weights(), dev)
    vgg = V.load_vgg19_weights()
    x0 = torch.from_numpy(W.synthetic_image(91, (B, 3, h, w)))
    c0 = torch.from_numpy(W.synthetic_image(92, (B, 3, h, w)))
    st0 = [torch.from_numpy(W.synthetic_image(93 + i, (1, 3, h, w))) for i in range(B)]
    per = [feat.style_targets(s.to(dev)) for s in st0]
    targets = [torch.cat([p[i].reshape(1, *p[i].shape[-2:]) for p in per]).contiguous()
               for i in range(5)]
    assert all(t.shape[0] == B and not torch.equal(t[0], t[1]) for t in targets)
    c4 = V.content_target(feat, c0.to(dev)).clone()
    gw = torch.tensor([1e5, 2e5, 3e5, 2e5, 1e5, 1.0, 1e3])
    x = x0.to(dev).requires_grad_()
    with R.HipBranchSpy(torch.nn.Sequential(), V, monkeypatch) as spy:
        losses = A.VGGLossFn.apply(x, c4, feat, targets, True)
        (losses * gw.to(dev)).sum().backward()
    torch.cuda.synchronize()
    bv = spy.vgg

    def ref(dtype):
        vw = [(torch.tensor(a, dtype=dtype), torch.tensor(b, dtype=dtype)) for a, b in vgg]
        xr = x0.to(dtype).clone().requires_grad_()
        with torch.no_grad():
            tg = [torch.cat([R.gram(z) for z in zs]) for zs in
                  zip(*[R.vgg_forward(vw, s.to(dtype)) for s in st0])]
            c4r = R.vgg_forward(vw, c0.to(dtype))[3]
        zs = R.vgg_forward(vw, xr, R.Branches(bv))
        ls = [F.mse_loss(R.gram(z), t) for z, t in zip(zs, tg)]
        ls.append(F.mse_loss(zs[3], c4r))
        # FeatureReconstructionLoss on the ReLU'd tap: mse^2 / numel (mask of Z4 forced)
        ls.append(F.mse_loss(zs[3] * bv[3][0].to(dtype), F.relu(c4r)).pow(2) / zs[3].numel())
        ls = torch.stack(ls)
        (ls * gw.to(dtype)).sum().backward()
        return ls.detach(), xr.grad
    (l64, d64), (l32, d32) = ref(torch.float64), ref(torch.float32)
    for i in range(7):
        _within(f"{hw} loss {i}", losses[i], l32[i], l64[i])
    _within(f"{hw} dx", x.grad, d32, d64)


def _flat_sd_trainer(sd, styles, dev):
    net = _multi(sd, styles, dev)
    return MultiStyleTrainer(net, [t.to(dev) for t in styles])


def test_graph_replay_equals_eager_with_changing_styles(dev):
    """Three train_steps whose style ids change every step: flat parameters and losses of
    graph=True (the warm-up step, then two replays of the captured graphs) equal
    graph=False bit for bit -- ids, mix or targets baked into the capture would not."""
    styles = _styles(S3, H64)
    sd = CR.multi_sd(SEEDS)
    ids = [[0, 1, 2, 0], [2, 2, 1, 0], [1, 0, 0, 2]]
    batches = [torch.from_numpy(W.synthetic_image(85 + t, (B4, 3, H64, H64))).to(dev)
               for t in range(3)]
    trg, tre = _flat_sd_trainer(sd, styles, dev), _flat_sd_trainer(sd, styles, dev)
    for t in range(3):
        lg = trg.train_step(batch=batches[t], graph=True, ids=ids[t]).clone()
        le = tre.train_step(batch=batches[t], graph=False, ids=ids[t]).clone()
        assert torch.equal(lg, le), (t, float(lg), float(le))
        assert torch.equal(trg.flat, tre.flat), t
    assert trg._graph is not None and trg.t == tre.t == 3
    # the default schedule drives the same buffers
    lg, le = trg.train_step(batches[0]).clone(), tre.train_step(batches[0], graph=False).clone()
    assert torch.equal(lg, le) and torch.equal(trg.flat, tre.flat)
    assert trg._buffers(B4)[0].tolist() == style_ids(3, B4, S3)


def test_dp_shards_sum_to_the_full_batch_gradient(dev):
    """Two shards with the world=2 scaling (mean / W + TV sum) and their style_ids slices,
    summed by hand, == the full-batch gradient within 1e-5 (test_dp_gradient_equivalence's
    bound)."""
    styles = _styles(S3, H64)
    sd = CR.multi_sd(SEEDS)
    batch = torch.from_numpy(W.synthetic_image(88, (B4, 3, H64, H64))).to(dev)

    def grads(world, rank):
        tr = _flat_sd_trainer(sd, styles, dev)
        tr.world, tr.rank = world, rank  # scaling and slice only; summed by hand below
        b = B4 // world
        tr.set_styles(b)
        assert tr._buffers(b)[0].tolist() == style_ids(0, B4, S3, rank, world)
        tr._fwd_bwd(batch[rank * b:(rank + 1) * b].contiguous())
        return tr.flat_grad.clone()
    full = grads(1, 0)
    summed = grads(2, 0) + grads(2, 1)
    e = _rel(summed, full)
    print(f"dp: summed shards vs full batch {e:.2e}")
    assert e < 1e-5


def test_inference_blend_fp64(dev):
    """A (0.25, 0.75, 0) blend of two styles against the fp64 functional restatement, and
    a (1, 0, 0) mix == style 0 == the single-style network of row 0, bit for bit."""
    styles = _styles(S3, H64)
    sd = CR.multi_sd(SEEDS)
    net = _multi(sd, styles, dev)
    x0 = torch.from_numpy(W.synthetic_image(89, (2, 3, H64, H64)))
    w = torch.tensor([0.25, 0.75, 0.0])
    with torch.no_grad():
        y = net(x0.to(dev), style=w).cpu()
        y0 = net(x0.to(dev), style=torch.tensor([1.0, 0.0, 0.0]))
        assert torch.equal(y0, net(x0.to(dev), style=0)) and torch.equal(y0, net(x0.to(dev)))
        snet = network.ImageTransformNet(styles[0].to(dev), 2)
        snet.load_state_dict({k: torch.from_numpy(v) for k, v in CR.single_sd(sd, 0)})
        assert torch.equal(y0, snet(x0.to(dev)))

        def ref(dtype):
            t = {k: torch.tensor(v, dtype=dtype) for k, v in sd}
            return CR.itn_forward_cond(t, x0.to(dtype), w.to(dtype).expand(2, -1), R.Branches())
        _within("blend y", y, ref(torch.float32), ref(torch.float64))
    assert not torch.equal(y, y0.cpu())


def test_cli_train_multi_then_convert_image_multi(dev, project_root):
    """`fast_st train-multi A B -n duo --synthetic 8 -e 1 -b 4` writes the checkpoint and
    the style-name sidecar; `fast_st convert-image-multi IMG duo --mix ...` writes a PNG
    whose bytes are img_utils.to_pil of an in-process process_image forward of the same
    checkpoint."""
    import json
    from click.testing import CliRunner
    from styletransfer_amd import img_utils
    from styletransfer_amd.clis import cli
    r = CliRunner().invoke(cli, ["fast_st", "train-multi", "data/styles/picasso.jpg",
                                 "data/dancing.jpg", "-n", "duo", "--synthetic", "8", "-e", "1",
                                 "-b", "4"])
    assert r.exit_code == 0, r.output + repr(r.exception)
    models = project_root / "data" / "models"
    ck = models / "fast_mst_duo_epoch0.pth"
    assert ck.is_file()
    names = json.load(open(models / "fast_mst_duo.styles.json"))
    assert names == ["picasso.jpg", "dancing.jpg"]
    saved = torch.load(ck, weights_only=True)
    assert list(saved) == [k for k, _ in W.itn_synthetic(4321)]
    assert tuple(saved["1.weight"].shape) == (2, 32)
    r = CliRunner().invoke(cli, ["fast_st", "convert-image-multi", "data/dancing.jpg", "duo",
                                 "--mix", "picasso.jpg:0.5,dancing.jpg:0.5"])
    assert r.exit_code == 0, r.output + repr(r.exception)
    got = np.asarray(Image.open(project_root / "results" / "converted_fast_mst_duo.png"))
    net = network.MultiStyleTransformNet([torch.rand(3, 8, 8)] * 2, style_names=names)
    out = net.process_image("data/dancing.jpg", "duo", mix=[0.5, 0.5], out_dir="again/")
    assert np.array_equal(got, np.asarray(img_utils.to_pil(out)))
    # and it is a blend: neither pure style gives these bytes
    with torch.no_grad():
        x = img_utils.image_loader(str(project_root / "data/dancing.jpg"))
        assert not torch.equal(out, net(x, style=0)) and not torch.equal(out, net(x, style=1))
