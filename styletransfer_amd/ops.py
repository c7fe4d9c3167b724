"""Functional wrappers over libstx (include/stx.h) for torch tensors.

PyTorch supplies device memory, the current HIP stream and autograd plumbing;
every arithmetic op here is a hand-written HIP kernel in libstx.so.  Nothing in
this module falls back to a torch/CPU implementation: a non-CUDA tensor or a
missing library raises.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import functools
import gc

import torch

from . import _native as N
from ._native import ConvParams, check, lib

__all__ = [
    "conv_weight_dims", "conv_weight_prep", "conv_weight_prep16", "split_eligible", "amax",
    "conv2d", "conv_out_hw", "conv2d_wgrad", "wgrad_path",
    "bias_grad", "gram", "style_loss", "gram_bwd", "guided_style_loss", "guided_gram_bwd", "mse", "diff_scale", "loss_combine",
    "maxpool2x2", "maxpool2x2_bwd", "relupool_bwd", "relu", "relu_bwd", "adam_step",
    "instnorm_fwd", "instnorm_bwd", "cin_mix", "upsample2x", "upsample2x_bwd", "tv_loss",
    "temporal_loss", "temporal_loss_bwd", "flow_warp", "flow_consistency", "flow_compose", "masked_mse",
    "chan_stats", "adain", "stats_loss", "stats_loss_bwd",
    "color_stats", "color_affine", "resample_plan",
    "resample2d",
    "flow_pyramid", "flow_luma", "flow_linearize", "flow_jacobi", "flow_scale",
]


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _req(t: torch.Tensor, name: str = "tensor"):
    if not t.is_cuda:
        raise N.NativeError(f"{name}: the HIP path needs a device tensor (got {t.device}); "
                            "there is no CPU fallback")
    if t.dtype != torch.float32:
        raise N.NativeError(f"{name}: fp32 required (got {t.dtype})")
    if not t.is_contiguous():
        raise N.NativeError(f"{name}: contiguous NCHW required")
    return t


class _Workspace:
    """Per-device scratch buffer, grown on demand.  All users are stream-ordered
    on the same stream and finish with the scratch inside one C call.

    A captured hipGraph (GatysEngine, FastStTrainer.capture, FrameEngine) bakes the
    scratch pointer of its capture into its kernels, so a buffer is never freed
    once handed out: when a larger one is needed the old one is retired, not
    released to the caching allocator (growth is geometric, so the retired
    buffers sum to less than the live one)."""

    def __init__(self):
        self.buf = {}
        self.retired = []

    def get(self, nbytes: int, device) -> tuple:
        nbytes = max(int(nbytes), 256)
        key = (device.index if isinstance(device, torch.device) else device)
        b = self.buf.get(key)
        if b is None or b.numel() < nbytes:
            size = max(nbytes, 1 << 20) if b is None else max(nbytes, 2 * b.numel())
            if b is not None:
                self.retired.append(b)
            b = torch.empty(size, dtype=torch.uint8, device=device)
            self.buf[key] = b
        return b.data_ptr(), b.numel()


WS = _Workspace()
WS_SIDE = _Workspace()  # the weight-gradient side stream's own scratch (SideStream)


class SideStream:
    """Weight gradients off the data-gradient chain.  In a training step's backward
    (train.FastStTrainer / VideoTrainer between begin() and end()) every conv's dW --
    which nothing in the backward reads -- runs on a side stream that waits for the
    work issued so far (dy is ready), while the data gradients continue on the main
    stream; end() joins the side stream back before the gradient exchange / Adam.  The
    small B=8 grids of the ImageTransformNet (2 blocks per CU) leave room for a
    concurrent kernel.  The side work has its own scratch (WS_SIDE) and keeps its
    inputs referenced until the join (no cross-stream reuse of their memory, eager or
    captured).  Opt-in (STX_WGRAD_SIDE=1) until measured."""

    def __init__(self):
        self.active = False
        self.streams = {}
        self.stream = None
        self.keep = []

    def begin(self, device):
        if N.knob("STX_WGRAD_SIDE", "0") != "1":
            return
        key = torch.device(device).index or 0
        if key not in self.streams:
            self.streams[key] = torch.cuda.Stream(device)
        self.stream = self.streams[key]
        self.active = True
        self.keep = []

    def on_side(self):
        return self.active and torch.cuda.current_stream() == self.stream

    def run(self, fn, *keep):
        if not self.active:
            return fn()
        self.stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self.stream):
            r = fn()
        self.keep.extend(t for t in keep if t is not None)
        return r

    def end(self):
        if self.active:
            torch.cuda.current_stream().wait_stream(self.stream)
            self.keep = []
            self.active = False


SIDE = SideStream()


def _scratch():
    return WS_SIDE if SIDE.on_side() else WS


@contextlib.contextmanager
def graph_capture(graph, **kw):
    """torch.cuda.graph(graph, **kw) with Python's cyclic garbage collector held off for
    the capture (after one collection): a CUDAGraph left in a reference cycle by earlier
    work (a finished engine) and collected while this stream captures would be destroyed
    mid-capture, which HIP refuses (hipErrorStreamCaptureUnsupported -> abort)."""
    gc.collect()
    was = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(graph, **kw):
            yield
    finally:
        if was:
            gc.enable()


class AmaxArena:
    """Pre-zeroed amax groups for producers that annotate their outputs (InstanceNorm
    forward/backward -> the next split conv's input scale).  A training step calls
    begin() (one fill of all groups) and end(); outside a step take() returns None
    and consumers compute max|x| themselves.  Annotations carry the arena epoch, so a
    tensor kept across steps is never trusted with a re-zeroed group."""

    def __init__(self, groups=128):
        self.groups = groups
        self.buf = None
        self.i = 0
        self.epoch = 0
        self.active = False

    def begin(self, device):
        dev = torch.device(device)
        if self.buf is None or self.buf.device != dev:
            self.buf = torch.zeros((self.groups, N.STX_AMAX_SLOTS), device=dev,
                                   dtype=torch.float32)
        else:
            self.buf.zero_()
        self.i = 0
        self.epoch += 1
        self.active = True

    def end(self):
        self.active = False

    def take(self, device):
        if not self.active or self.i >= self.groups or self.buf.device != device:
            return None
        g = self.buf[self.i]
        self.i += 1
        return g

    def take_span(self, k, device):
        """k consecutive zeroed groups as one flat slot vector (vgg.slot layout)."""
        if not self.active or self.i + k > self.groups or self.buf.device != device:
            return None
        g = self.buf[self.i:self.i + k].view(-1)
        self.i += k
        return g

    def annotate(self, t, g):
        if g is not None:
            t._stx_amax = (g, self.epoch)
        return t

    def lookup(self, t):
        a = getattr(t, "_stx_amax", None)
        if a is None or not self.active or a[1] != self.epoch:
            return None
        return a[0]


ARENA = AmaxArena()


class ParamGradBatch:
    """Deferred InstanceNorm parameter reductions of one training step: between
    begin() and flush() each instnorm_bwd given dgamma/dbeta/dbias_in keeps its
    per-plane partials in a buffer of its own and records a job; flush() reduces all
    of them in one launch (stx_instnorm_param_grads).  Outside a step the reductions
    run per call."""

    def __init__(self):
        self.active = False
        self.jobs, self.keep = [], []

    def begin(self):
        self.active = True
        self.jobs, self.keep = [], []

    def add(self, parts, n, c, dgamma, dbeta, dbias, accumulate):
        self.keep.append(parts)
        self.jobs.append(N.PGradJob(parts.data_ptr(), _p(dgamma), _p(dbeta), _p(dbias), n, c,
                                    int(accumulate), 0))
        if len(self.jobs) == N.STX_PGRAD_MAX:
            self._launch()

    def _launch(self):
        if self.jobs:
            arr = (N.PGradJob * len(self.jobs))(*self.jobs)
            check(lib().stx_instnorm_param_grads(arr, len(self.jobs), _stream()),
                  "stx_instnorm_param_grads")
        self.jobs, self.keep = [], []

    def flush(self):
        self._launch()
        self.active = False


PGRADS = ParamGradBatch()


class CinGradBatch:
    """ParamGradBatch for conditional instance norm (stx_cin_param_grads): the style
    tables' and conv biases' gradients of every per-sample IN layer of a step in one
    launch.  Same life cycle: between begin() and flush() each instnorm_bwd(per_sample=
    True) keeps its partials and records a job; outside a step add() reduces at once.
    All jobs of a launch share the step's mix [n][S]."""

    def __init__(self):
        self.active = False
        self.jobs, self.keep, self.mix = [], [], None

    def begin(self):
        self.active = True
        self.jobs, self.keep, self.mix = [], [], None

    def add(self, parts, mix, c, dgtab, dbtab, dbias, accumulate, defer=True):
        if self.mix is not None and (self.mix.data_ptr() != mix.data_ptr() or
                                     self.mix.shape != mix.shape):
            self._launch()
        self.mix = mix
        self.keep.append(parts)
        self.jobs.append(N.CinJob(None, None, None, None, parts.data_ptr(), _p(dgtab), _p(dbtab),
                                  _p(dbias), c, int(accumulate)))
        if len(self.jobs) == N.STX_CIN_MAX or not (self.active and defer):
            self._launch()  # (with any jobs pending: their partials are written too)

    def _launch(self):
        if self.jobs:
            arr = (N.CinJob * len(self.jobs))(*self.jobs)
            n, S = self.mix.shape
            check(lib().stx_cin_param_grads(arr, len(self.jobs), self.mix.data_ptr(), n, S,
                                            _stream()), "stx_cin_param_grads")
        self.jobs, self.keep, self.mix = [], [], None

    def flush(self):
        self._launch()
        self.active = False


CINGRADS = CinGradBatch()


# ----------------------------------------------------------------------- conv
def conv_weight_dims(cin, cout, ks):
    a, b = C.c_int(), C.c_int()
    check(lib().stx_conv_weight_dims(cin, cout, ks, C.byref(a), C.byref(b)), "weight_dims")
    return a.value, b.value


def conv_weight_prep(w: torch.Tensor, transpose: bool = False) -> torch.Tensor:
    """[cout][cin][k][k] -> k-major GEMM slab (transpose=True: data-gradient slab)."""
    _req(w, "weight")
    cout, cin, ks, _ = w.shape
    gin, gout = (cout, cin) if transpose else (cin, cout)
    cp, op = conv_weight_dims(gin, gout, ks)
    wt = torch.empty((cp * ks * ks, op), device=w.device, dtype=torch.float32)
    check(lib().stx_conv_weight_prep(w.data_ptr(), wt.data_ptr(), cout, cin, ks, int(transpose),
                                     _stream()), "conv_weight_prep")
    return wt


def conv_weight_prep16(w: torch.Tensor, transpose: bool = False):
    """[cout][cin][3][3] -> (fp16 hi/lo split slab, device max|w|) for the split-MFMA
    path of stx_conv2d (transpose=True: the data-gradient slab)."""
    _req(w, "weight")
    cout, cin, ks, _ = w.shape
    L = lib()
    nb = L.stx_conv_weight16_bytes(cin, cout, ks, int(transpose))
    if nb == 0:
        raise N.NativeError(f"no fp16-split slab for a {ks}x{ks} conv")
    wt16 = torch.empty(nb, device=w.device, dtype=torch.uint8)
    w_amax = torch.empty(N.STX_AMAX_SLOTS, device=w.device, dtype=torch.float32)
    check(L.stx_conv_weight_prep16(w.data_ptr(), wt16.data_ptr(), w_amax.data_ptr(), cout, cin,
                                   ks, int(transpose), _stream()), "conv_weight_prep16")
    return wt16, w_amax


def conv_weight_prep16_up(w: torch.Tensor):
    """[cout][cin][3][3] -> (parity-class split slab, device max|w|) of a conv over a
    nearest x2 upsampled input (stx_conv_weight_prep16_up; conv2d(wt16_up=...))."""
    _req(w, "weight")
    cout, cin, ks, _ = w.shape
    assert ks == 3, ks
    L = lib()
    slab = torch.empty(L.stx_conv_weight16up_bytes(cin, cout), device=w.device, dtype=torch.uint8)
    w_amax = torch.empty(N.STX_AMAX_SLOTS, device=w.device, dtype=torch.float32)
    check(L.stx_conv_weight_prep16_up(w.data_ptr(), slab.data_ptr(), w_amax.data_ptr(), cout,
                                      cin, _stream()), "conv_weight_prep16_up")
    return slab, w_amax


def conv_weight_compose16(coef, coef_amax, w: torch.Tensor, w_amax, out_amax, scale=None,
                          out=None, loss_job=None, adam_prepare=None):
    """The data-gradient split slab of w' = scale * A w (A = coef [cout][pitch], one image's
    Gram-backward operator, coef_amax >= max|A|; w [cout][cin][3][3], w_amax >= max|w|):
    conv^T_w(A z) = conv^T_{w'}(z) (stx_conv_weight_compose16, one launch).  out_amax (an
    amax group) receives the slab's scale bound; the conv takes wt16=(slab, out_amax).
    out: the slab buffer to reuse.  Returns the slab.

    loss_job (a LossFinalizeJob) / adam_prepare (an AdamPrepare): run as rider blocks of
    this launch instead of as one-block launches of their own
    (stx_conv_weight_compose16_tail); both are marked done."""
    _req(w, "weight")
    _req(coef, "coef")
    cout, cin, ks, _ = w.shape
    assert ks == 3 and coef.shape[-2] == cout and coef.numel() == cout * coef.shape[-1], coef.shape
    L = lib()
    if out is None:
        out = torch.empty(L.stx_conv_weight16_bytes(cin, cout, ks, 1), device=w.device,
                          dtype=torch.uint8)
    if loss_job is None and adam_prepare is None:
        check(L.stx_conv_weight_compose16(coef.data_ptr(), coef.shape[-1], coef_amax.data_ptr(),
                                          w.data_ptr(), w_amax.data_ptr(), cout, cin, _p(scale),
                                          out.data_ptr(), out_amax.data_ptr(), _stream()),
              "stx_conv_weight_compose16")
        return out
    j, a = loss_job, adam_prepare
    check(L.stx_conv_weight_compose16_tail(
        coef.data_ptr(), coef.shape[-1], coef_amax.data_ptr(), w.data_ptr(), w_amax.data_ptr(),
        cout, cin, _p(scale), out.data_ptr(), out_amax.data_ptr(),
        C.byref(j.lp) if j else None, j.losses.data_ptr() if j else None,
        _p(j.extra) if j else None, j.m if j else 0, j.w if j else None,
        _p(j.total) if j else None,
        a.step_dev.data_ptr() if a else None, a.ws.data_ptr() if a else None,
        a.lr if a else 0.0, a.beta1 if a else 0.0, a.beta2 if a else 0.0, _stream()),
        "stx_conv_weight_compose16_tail")
    if j:
        j.done = True
    if a:
        a.done = True
    return out


def conv_weight_prep16_pair(w: torch.Tensor):
    """(forward slab, data-gradient slab), sharing one device max|w| (two launches)."""
    _req(w, "weight")
    cout, cin, ks, _ = w.shape
    L = lib()
    wt16 = torch.empty(L.stx_conv_weight16_bytes(cin, cout, ks, 0), device=w.device,
                       dtype=torch.uint8)
    wtT16 = torch.empty(L.stx_conv_weight16_bytes(cin, cout, ks, 1), device=w.device,
                        dtype=torch.uint8)
    w_amax = torch.empty(N.STX_AMAX_SLOTS, device=w.device, dtype=torch.float32)
    check(L.stx_conv_weight_prep16_pair(w.data_ptr(), wt16.data_ptr(), wtT16.data_ptr(),
                                        w_amax.data_ptr(), cout, cin, ks, _stream()),
          "conv_weight_prep16_pair")
    return (wt16, w_amax), (wtT16, w_amax)


class TrainedSlabs:
    """The GEMM weight slabs of a trained network's conv layers, re-prepped after
    every parameter update in two launches (stx_conv_weight_prep_batch) instead of
    ~2 per slab.  For each layer the slabs the forward and the input-gradient kernels
    of autograd.Conv2dFn will select: the fp16 hi/lo split slab (shapes the split
    kernel takes) or the fp32 k-major slab, for the forward and the transposed
    data-gradient GEMM; forward and data-gradient split slabs share one max|w| group.

    `prep()` enqueues the batch and hands each layer `_train_slabs = (key, wt, wt16,
    wtT, wtT16, wt16_up)` keyed on the weight's (pointer, version): layers.Conv2d uses
    the slabs only while the key matches, so a weight changed behind the trainer's back
    falls back to per-call preps.  wt16_up: the parity-class slab of a conv that reads a
    nearest x2 upsampled input (layers.Conv2d._up_input), sharing the max|w| group."""

    def __init__(self, convs):
        self.convs = list(convs)
        self.generation = 0
        self._retired = []
        self.slabs = None
        self._build()

    def _build(self):
        split = N.knob("STX_CONV_SPLIT", "1") != "0"
        L = lib()
        jobs = []
        if self.slabs is not None:
            # a hipGraph captured earlier still holds the old slab / job pointers: keep
            # them alive (as _Workspace retires scratch buffers) and bump the generation
            # so the owner re-captures (train.FastStTrainer checks it before a replay)
            self._retired.append((self.slabs, self._jobs))
            self.generation += 1
        self.slabs = []
        for conv in self.convs:
            w = conv.weight
            cout, cin, ks, _ = w.shape
            stride, pad = conv.stride[0], conv.padding[0]
            f16 = split and pad == 1 and split_eligible(cin, cout, ks, stride)
            b16 = split and pad == 1 and split_eligible(cout, cin, ks, 1)
            dev = w.device
            am = torch.empty(N.STX_AMAX_SLOTS, device=dev, dtype=torch.float32) \
                if (f16 or b16) else None
            out = []
            for t, is16 in ((0, f16), (1, b16)):
                if is16:
                    slab = torch.empty(L.stx_conv_weight16_bytes(cin, cout, ks, t), device=dev,
                                       dtype=torch.uint8)
                    jobs.append(N.WprepJob(w.data_ptr(), slab.data_ptr(), am.data_ptr(),
                                           N.STX_WPREP_F16, cout, cin, ks, t, 0))
                    out.append((None, (slab, am)))
                else:
                    gin, gout = (cout, cin) if t else (cin, cout)
                    cp, op = conv_weight_dims(gin, gout, ks)
                    slab = torch.empty((cp * ks * ks, op), device=dev, dtype=torch.float32)
                    jobs.append(N.WprepJob(w.data_ptr(), slab.data_ptr(), None,
                                           N.STX_WPREP_F32, cout, cin, ks, t, 0))
                    out.append((slab, None))
            up = None
            if f16 and stride == 1 and ks == 3 and getattr(conv, "_up_input", False) and \
                    N.knob("STX_UPAR", "1") != "0":
                up = torch.empty(L.stx_conv_weight16up_bytes(cin, cout), device=dev,
                                 dtype=torch.uint8)
                jobs.append(N.WprepJob(w.data_ptr(), up.data_ptr(), am.data_ptr(),
                                       N.STX_WPREP_F16UP, cout, cin, ks, 0, 0))
            self.slabs.append((w.data_ptr(), out[0][0], out[0][1], out[1][0], out[1][1], up))
        if len(jobs) > N.STX_WPREP_MAX:
            raise N.NativeError(f"{len(jobs)} weight slabs > STX_WPREP_MAX")
        self._jobs = (N.WprepJob * len(jobs))(*jobs)
        self._njobs = len(jobs)

    def release_retired(self):
        """Drop the slabs of earlier generations: call after the owner re-captured its
        graphs (a graph of an older generation refuses to replay, so nothing reads
        them any more)."""
        self._retired.clear()

    def prep(self):
        if any(c.weight.data_ptr() != s[0] for c, s in zip(self.convs, self.slabs)):
            self._build()  # a parameter was re-homed
        if self._njobs:
            check(lib().stx_conv_weight_prep_batch(self._jobs, self._njobs, _stream()),
                  "conv_weight_prep_batch")
        for c, (_, wt, wt16, wtT, wtT16, up) in zip(self.convs, self.slabs):
            w = c.weight
            c._train_slabs = ((w.data_ptr(), w._version, w.device), wt, wt16, wtT, wtT16,
                              None if up is None else (up, wt16[1]))


_S2_FWD = N.knob("STX_S2_FWD", "1") != "0"


def split_eligible(cin, cout, ks, stride=1):
    """Shapes stx_conv2d runs on the fp16 hi/lo split MFMA kernel (conv16.hip)."""
    # stride 2 (raw input only): STX_S2_FWD=0 keeps it on the fp32 kernel (A/B switch)
    return ks == 3 and cin >= 16 and cout > 4 and (
        stride == 1 or (stride == 2 and _S2_FWD))


def amax(x: torch.Tensor, out=None):
    """max|x| as an amax group (STX_AMAX_SLOTS floats whose max is the value)."""
    _req(x, "x")
    if out is None:
        out = torch.empty(N.STX_AMAX_SLOTS, device=x.device, dtype=torch.float32)
    check(lib().stx_amax(x.data_ptr(), x.numel(), out.data_ptr(), _stream()), "stx_amax")
    return out


def vdot(a, b, out, mul=None, add=None, sgn=1.0, op=0):
    """*out = add + sgn * mul * r, r = dot(a, b) (op 0), sum|a| (1), max|a| (2); a
    fixed-order reduction (stx_vec_reduce).  out/mul/add: 1-element device tensors."""
    _req(a, "a")
    L = lib()
    wp, wn = WS.get(L.stx_vec_ws(), a.device)
    check(L.stx_vec_reduce(a.data_ptr(), _p(b), a.numel(), op, out.data_ptr(), _p(mul), _p(add),
                           float(sgn), wp, wn, _stream()), "stx_vec_reduce")
    return out


def virtual_hw(h, w, in_mode, hv=None, wv=None):
    if in_mode in (N.STX_IN_RAW, N.STX_IN_RELU):
        return h, w
    if in_mode == N.STX_IN_RELU_POOL2:
        return h // 2, w // 2
    if in_mode == N.STX_IN_UPSAMPLE2:
        return 2 * h, 2 * w
    return hv, wv  # DILATE2: explicit


def conv_out_hw(hv, wv, ks, stride, pad):
    return (hv + 2 * pad - ks) // stride + 1, (wv + 2 * pad - ks) // stride + 1


def conv2d(x, wt, cin, cout, ks, stride=1, pad=None, in_mode=N.STX_IN_RAW, bias=None,
           out=None, mask=None, aux=None, aux_scale=0.0, acc_scale=None, accumulate=False,
           relu_out=False, wt_batch_stride=0, hv=None, wv=None, p2_z=None, p2_coef=None,
           p2_scale=None, up_dp=None, up_z=None, wt16=None, in_amax=None, out_amax=None,
           pool_out=None, p2_amax=None, split_1x1=False, gram_part=None, pool_sum=False,
           gram_cnt=None, p2_wt_amax=None, mse_ref=None, mse_parts=None, wt16_up=None,
           unpool_out=None, pool_only=False):
    """stx_conv2d on x [n][cin][h][w] with a prepped slab `wt`.
    p2_z/p2_coef: fused Gram-backward phase (value += s2 * A[n] . p2_z[n]);
    up_dp/up_z: fused ReLU+MaxPool2d backward epilogue.
    wt16=(slab, w_amax) from conv_weight_prep16 selects the fp16 hi/lo split MFMA
    kernel for eligible shapes; in_amax (device >= max|x|) is computed when absent;
    out_amax (device scalar, zeroed by the caller) receives max|out|; pool_out
    [n][cout][ho/2][wo/2] receives maxpool2x2(relu(out)) (split path, wo > 32);
    gram_part [n * conv_gram_tiles(...) * 4096] receives the fused per-tile Gram
    partials of out (stx_conv_params.gram_part); pool_sum: pool_out receives the 2x2
    SUM of the output instead and the full-resolution output is not written (returned:
    pool_out) -- the nearest-x2 upsampling backward fused into a data gradient.
    p2_wt_amax: amax group >= max|p2_coef| over the batch (a FinalizeBatch job's
    coef_amax): the split path's Gram-backward phase then runs on the fp16 split MFMA.
    mse_ref/mse_parts (with gram_part, cout 128): the content target and the per-tile
    content / feature MSE sums of the output (stx_conv_params.mse_ref).
    wt16_up=(slab, w_amax) from conv_weight_prep16_up: an upsampled-input conv with the
    plain epilogue runs as four output-parity 2x2 convs (stx_conv_params.wt16_up).
    unpool_out=(z, coef, coef_amax, z_amax, scale): the result d is the gradient of
    maxpool2x2(relu(z)) and `out` [n][cout][2 ho][2 wo] receives unpool(d) [z > 0] +
    scale * A[n] . z (stx_conv_params.unpool_out: a pooled tap's ReLU+MaxPool and Gram
    backward in this data gradient's epilogue).
    pool_only (with pool_out, split path): the full-resolution output is not written
    (stx_conv_params.y = NULL); returns pool_out."""
    _req(x, "x")
    n, c, h, w = x.shape
    assert c == cin, (c, cin)
    if pad is None:
        pad = ks // 2
    hv, wv = virtual_hw(h, w, in_mode, hv, wv)
    ho, wo = conv_out_hw(hv, wv, ks, stride, pad)
    if pool_sum:
        assert pool_out is not None and out is None, "pool_sum writes pool_out only"
        out = pool_out  # p.y must be set; the kernel never writes it with pool_sum
    elif unpool_out is not None:
        oshape = (n, cout, 2 * ho, 2 * wo)
        if out is None:
            out = torch.empty(oshape, device=x.device, dtype=torch.float32)
        _req(out, "out")
        assert out.shape == oshape, (out.shape, oshape)
    elif out is None:
        out = torch.empty((n, cout, ho, wo), device=x.device, dtype=torch.float32)
    else:
        _req(out, "out")
        assert out.shape == (n, cout, ho, wo), (out.shape, (n, cout, ho, wo))
    cp, op = conv_weight_dims(cin, cout, ks)
    p = ConvParams(x=x.data_ptr(), wt=_p(wt), bias=_p(bias), y=out.data_ptr(),
                   mask=_p(mask), aux=_p(aux), aux_scale=float(aux_scale),
                   acc_scale=_p(acc_scale), accumulate=int(accumulate), relu_out=int(relu_out),
                   n=n, cin=cin, h=h, w=w, cout=cout, ks=ks, stride=stride, pad=pad,
                   in_mode=in_mode, hv=hv, wv=wv, ho=ho, wo=wo, cin_pad=cp, cout_pad=op,
                   wt_batch_stride=int(wt_batch_stride))
    if p2_z is not None:
        assert p2_coef is not None and p2_coef.shape[-1] == op, (p2_coef.shape, op)
        p.p2_z, p.p2_wt, p.p2_scale = p2_z.data_ptr(), p2_coef.data_ptr(), _p(p2_scale)
        p.p2_c = p2_z.shape[1]
        p.p2_wt_batch_stride = p2_coef.shape[-1] * p2_coef.shape[-2]
    if up_dp is not None:
        p.up_dp, p.up_z = up_dp.data_ptr(), up_z.data_ptr()
    if wt16 is not None and split_eligible(cin, cout, ks, stride) and wt_batch_stride == 0:
        if in_amax is None:
            in_amax = amax(x)
        p.wt16, p.w_amax, p.in_amax = wt16[0].data_ptr(), wt16[1].data_ptr(), in_amax.data_ptr()
        if wt16_up is not None and in_mode == N.STX_IN_UPSAMPLE2 and ks == 3 and stride == 1 \
                and pad == 1 and wo > 32 and (hv, wv) == (2 * h, 2 * w) and not any(
                    v is not None for v in (mask, aux, acc_scale, p2_z, up_dp, pool_out,
                                            gram_part)) and not accumulate:
            p.wt16_up, p.w_amax = wt16_up[0].data_ptr(), wt16_up[1].data_ptr()
        if p2_z is not None:
            p.p2_amax = (p2_amax if p2_amax is not None else amax(p2_z)).data_ptr()
            if p2_wt_amax is not None:
                p.p2_wt_amax = p2_wt_amax.data_ptr()
    elif split_1x1:
        # Gram backward as the split phase alone (per-image weights, include/stx.h)
        assert ks == 1 and wt_batch_stride and mask is None and p2_z is None
        p.wt16 = 1
        p.in_amax = (in_amax if in_amax is not None else amax(x)).data_ptr()
    if unpool_out is not None:
        uz, ucoef, ucoef_amax, uz_amax, uscale = unpool_out
        _req(uz, "unpool z")
        assert uz.shape == out.shape and ucoef.shape[-1] == op, (uz.shape, ucoef.shape, op)
        p.unpool_out = 1
        p.up_z, p.p2_wt, p.p2_scale = uz.data_ptr(), ucoef.data_ptr(), _p(uscale)
        p.p2_c = uz.shape[1]
        p.p2_wt_batch_stride = ucoef.shape[-1] * ucoef.shape[-2]
        p.p2_amax = (uz_amax if uz_amax is not None else amax(uz)).data_ptr()
        p.p2_wt_amax = ucoef_amax.data_ptr()
    if in_amax is not None and not p.in_amax:
        # the non-split kernels that take an input bound (convfew.hip's split 64->3
        # data gradient) read it too; the others ignore it
        p.in_amax = in_amax.data_ptr()
    if out_amax is not None:
        p.out_amax = out_amax.data_ptr()
    if pool_out is not None:
        _req(pool_out, "pool_out")
        assert pool_out.shape == (n, cout, ho // 2, wo // 2), pool_out.shape
        p.pool_out = pool_out.data_ptr()
        p.pool_sum = int(bool(pool_sum))
    assert mse_ref is None or gram_part is not None, "mse_ref rides on the fused Gram"
    if gram_part is not None:
        _req(gram_part, "gram_part")
        nt = lib().stx_conv_gram_tiles(C.byref(p))
        ng = lib().stx_conv_gram_groups(C.byref(p)) if gram_cnt is not None else 0
        ntu = gram_tile_units(cout)
        assert nt > 0 and gram_part.numel() >= n * (ntu * nt + ng) * 4096, \
            (nt, ng, gram_part.numel())
        p.gram_part = gram_part.data_ptr()
        if mse_ref is not None:
            _req(mse_ref, "mse_ref")
            _req(mse_parts, "mse_parts")
            assert mse_ref.shape == out.shape and mse_parts.numel() >= 2 * n * nt, \
                (mse_ref.shape, mse_parts.numel(), n * nt)
            p.mse_ref, p.mse_parts = mse_ref.data_ptr(), mse_parts.data_ptr()
        if gram_cnt is not None:
            assert gram_cnt.is_cuda and gram_cnt.dtype == torch.int32 and \
                gram_cnt.numel() >= n * ng, (gram_cnt.dtype, gram_cnt.numel(), n * ng)
            p.gram_cnt = gram_cnt.data_ptr()
    if pool_only:
        assert pool_out is not None and not pool_sum and gram_part is None, "pool_only"
        p.y = None
        out = pool_out
    check(lib().stx_conv2d(C.byref(p), _stream()), "stx_conv2d")
    return out


def gram_tile_units(c):
    """64 x 64 tiles of the upper triangle of a c x c Gram (the partial slab's U)."""
    nt = (c + 63) // 64
    return nt * (nt + 1) // 2


def conv_gram_tiles(cin, cout, ho, wo, n=1, in_mode=N.STX_IN_RAW):
    """Gram partials per image (one per output tile) of a split 3x3 stride-1 conv with a
    fused Gram over a batch of n (stx_conv_gram_tiles; 0: not fusable)."""
    p = ConvParams(cin=cin, cout=cout, ks=3, stride=1, pad=1, ho=ho, wo=wo, wt16=2, n=n,
                   in_mode=in_mode)
    return lib().stx_conv_gram_tiles(C.byref(p))


def conv_gram_groups(cin, cout, ho, wo, n=1, in_mode=N.STX_IN_RAW):
    """In-kernel group sums per image of the fused Gram with gram_cnt
    (stx_conv_gram_groups: ceil(tiles / STX_GRAM_GROUP); 0: not fusable).  The slab then
    holds n * (tiles + groups) * 4096 floats: the per-tile scratch, then the group sums
    (conv2d(gram_part=slab, gram_cnt=counters); style_loss_from_parts on the sums)."""
    p = ConvParams(cin=cin, cout=cout, ks=3, stride=1, pad=1, ho=ho, wo=wo, wt16=2, n=n,
                   in_mode=in_mode)
    return lib().stx_conv_gram_groups(C.byref(p))


@functools.lru_cache(maxsize=None)
def _wgrad_plan(n, cin, h, w, cout, ks, stride, pad, in_mode, ho, wo, no_split):
    """(path, workspace bytes) of stx_conv2d_wgrad_plan; they depend on these dims alone."""
    p = N.WgradParams(n=n, cin=cin, h=h, w=w, cout=cout, ks=ks, stride=stride, pad=pad,
                      in_mode=in_mode, ho=ho, wo=wo, no_split=no_split)
    need = C.c_size_t()
    return lib().stx_conv2d_wgrad_plan(C.byref(p), C.byref(need)), need.value


def wgrad_path(n, cin, h, w, cout, ks, stride=1, pad=None, in_mode=N.STX_IN_RAW, split=True):
    """The N.STX_WGRAD_* path conv2d_wgrad takes for an x [n][cin][h][w]; above
    N.STX_WGRAD_F32 it is a split one, which reads the amax groups of x and dy."""
    pad = ks // 2 if pad is None else pad
    ho, wo = conv_out_hw(*virtual_hw(h, w, in_mode, 0, 0), ks, stride, pad)
    no_split = int(not (split and N.knob("STX_CONV_SPLIT", "1") != "0"))
    return _wgrad_plan(n, cin, h, w, cout, ks, stride, pad, in_mode, ho, wo, no_split)[0]


def conv2d_wgrad(x, dy, cin, cout, ks, stride=1, pad=None, in_mode=N.STX_IN_RAW, dw=None,
                 accumulate=False, split=True, x_amax=None, dy_amax=None):
    """dW (+)= sum dy * V(x) (stx_conv2d_wgrad: the library picks the kernel -- wgrad_path);
    split=False or STX_CONV_SPLIT=0 keeps every shape on the fp32 MFMA."""
    _req(x, "x")
    _req(dy, "dy")
    n, _, h, w = x.shape
    if pad is None:
        pad = ks // 2
    if dw is None:
        dw = torch.empty((cout, cin, ks, ks), device=x.device, dtype=torch.float32)
    p = N.WgradParams(x=x.data_ptr(), dy=dy.data_ptr(), dw=dw.data_ptr(),
                      accumulate=int(accumulate), n=n, cin=cin, h=h, w=w, cout=cout, ks=ks,
                      stride=stride, pad=pad, in_mode=in_mode, ho=dy.shape[2], wo=dy.shape[3],
                      no_split=int(not (split and N.knob("STX_CONV_SPLIT", "1") != "0")))
    path, need = _wgrad_plan(n, cin, h, w, cout, ks, stride, pad, in_mode, p.ho, p.wo, p.no_split)
    if path > N.STX_WGRAD_F32:  # (xa / da stay referenced until the launch is queued)
        xa = x_amax if x_amax is not None else amax(x)
        da = dy_amax if dy_amax is not None else amax(dy)
        p.x_amax, p.dy_amax = xa.data_ptr(), da.data_ptr()
    p.ws, p.ws_bytes = _scratch().get(need, x.device)
    check(lib().stx_conv2d_wgrad(C.byref(p), _stream()), "stx_conv2d_wgrad")
    return dw


def bias_grad(dy, db=None, accumulate=False):
    _req(dy, "dy")
    n, c = dy.shape[:2]
    hw = dy[0, 0].numel()
    if db is None:
        db = torch.empty(c, device=dy.device, dtype=torch.float32)
    L = lib()
    wp, wn = WS.get(L.stx_bias_grad_ws(n, c), dy.device)
    check(L.stx_bias_grad(dy.data_ptr(), db.data_ptr(), n, c, hw, int(accumulate), wp, wn,
                          _stream()), "stx_bias_grad")
    return db


# ----------------------------------------------------------------------- gram
def gram(z, scale=None, z_amax=None):
    """G[b] = F F^T * scale (default 1/(C*H*W), StyleLoss.gram_matrix).  z_amax
    (device >= max|z|) selects the fp16 hi/lo split MFMA partials."""
    _req(z, "z")
    b, c = z.shape[:2]
    hw = z[0, 0].numel()
    if scale is None:
        scale = 1.0 / (c * hw)
    g = torch.empty((b, c, c), device=z.device, dtype=torch.float32)
    L = lib()
    wp, wn = WS.get(L.stx_gram_ws(b, c, hw), z.device)
    check(L.stx_gram(z.data_ptr(), g.data_ptr(), b, c, hw, float(scale), _p(z_amax), wp, wn,
                     _stream()),
          "stx_gram")
    return g


def coef_pitch(c):
    return lib().stx_gram_coef_pitch(c)


class FinalizeBatch:
    """Deferred Gram finalizes of one forward (stx_gram_finalize_batch): the style-loss ops
    given `fin=` append a job instead of launching their finalize; flush() runs them all
    in one launch.  The job structs (and what they point at, via `keep`) live until then."""

    def __init__(self):
        self.jobs, self.keep = [], []

    def new(self):
        j = N.GramFinJob()
        self.jobs.append(j)
        return j

    def flush(self):
        if self.jobs:
            arr = (N.GramFinJob * len(self.jobs))(*self.jobs)
            check(lib().stx_gram_finalize_batch(arr, len(self.jobs), _stream()),
                  "stx_gram_finalize_batch")
        self.jobs, self.keep = [], []


@functools.lru_cache(maxsize=None)
def _style_dims(b, c, hw, content):
    """A tap's host-side constants: workspace bytes (stx_style_content_ws with the content
    companion), byte offset and count of its loss partials in it, coef pitch."""
    L = lib()
    npart = C.c_int()
    off = L.stx_style_loss_parts(b, c, hw, C.byref(npart))
    need = (L.stx_style_content_ws if content else L.stx_gram_ws)(b, c, hw)
    return need, off, npart.value, L.stx_gram_coef_pitch(c)


def _style_loss(b, c, hw, target, device, weight, diag_alpha, coef, defer_ws, fin, *,
                want_coef=True, loss=None, nparts=0, **source):
    """The one stx_style_loss call behind style_loss, style_content_loss and
    style_loss_from_parts.  source: the tensors (or None) of N.StyleLossParams by field
    name -- z, z_amax, g_out, content, mse_out, or parts (with nparts), mse_parts, mse_out.
    Returns (loss, coef), the loss as the deferred (ptr, nparts, inv) triple with defer_ws."""
    _req(target, "target")
    # target [c][c] / [1][c][c] broadcast over the batch (expand_as), or [b][c][c]
    tb = target.numel() == b * c * c and b > 1
    if not tb and target.numel() != c * c:
        raise ValueError(f"style target {tuple(target.shape)} cannot expand to ({b},{c},{c})")
    need, off, npart, cp = _style_dims(b, c, hw, source.get("content") is not None)
    if not want_coef:
        coef = None
    elif coef is None:
        coef = torch.empty((b, cp, cp), device=device, dtype=torch.float32)
    if defer_ws is not None:
        assert defer_ws.numel() >= need, (defer_ws.numel(), need)
        wp, wn = defer_ws.data_ptr(), defer_ws.numel()
    else:
        wp, wn = WS.get(need, device)
    source.update(target=target, coef=coef, loss=loss)
    p = N.StyleLossParams(target_batched=int(tb), b=b, c=c, hw=hw, weight=float(weight),
                          diag_alpha=float(diag_alpha), ws=wp, ws_bytes=wn, nparts=int(nparts),
                          **{k: t.data_ptr() for k, t in source.items() if t is not None})
    if fin is not None:  # finalize deferred to fin.flush()
        assert defer_ws is not None
        p.defer = C.pointer(fin.new())
    check(lib().stx_style_loss(C.byref(p), _stream()), "stx_style_loss")
    if defer_ws is None:
        return loss, coef
    return (wp + off, npart, 1.0 / (b * c * c)), coef


def style_loss(z, target, weight=1.0, diag_alpha=0.0, want_coef=True, g_out=None, loss=None,
               coef=None, z_amax=None, defer_ws=None, fin=None):
    """mean((gram(z) - target)^2) -> 0-d loss; coef = d(weight*loss)/dz operator.
    defer_ws (uint8 device buffer >= stx_gram_ws): the loss is not reduced here; its
    partials stay in defer_ws for loss_finalize (returns (LossPart, coef))."""
    _req(z, "z")
    b, c = z.shape[:2]
    if loss is None and defer_ws is None:
        loss = torch.empty((), device=z.device, dtype=torch.float32)
    if fin is not None:
        assert g_out is None and want_coef
    return _style_loss(b, c, z[0, 0].numel(), target, z.device, weight, diag_alpha, coef,
                       defer_ws, fin, want_coef=want_coef, loss=loss, z=z, z_amax=z_amax,
                       g_out=g_out)


def style_content_loss(z, target, content, mse_out, weight=1.0, diag_alpha=0.0, coef=None,
                       z_amax=None, defer_ws=None, fin=None):
    """style_loss(z, target, ..., defer_ws=...) and mse(z, content, mode=2, out=mse_out) in
    one pass over z where the Gram kernel allows it.  defer_ws >= stx_style_content_ws.
    Returns (deferred LossPart, coef)."""
    _req(z, "z")
    _req(content, "content")
    assert content.numel() == z.numel() and mse_out.numel() >= 3
    assert defer_ws is not None
    b, c = z.shape[:2]
    return _style_loss(b, c, z[0, 0].numel(), target, z.device, weight, diag_alpha, coef,
                       defer_ws, fin, z=z, z_amax=z_amax, content=content, mse_out=mse_out)


def style_loss_from_parts(gparts, nparts, b, c, hw, target, weight=1.0, diag_alpha=0.0,
                          coef=None, defer_ws=None, fin=None, mse_parts=None, mse_out=None):
    """style_loss from the fused Gram partials a conv wrote (conv2d(gram_part=...)):
    gparts [b][U][nparts][64][64] (U = 3 for c = 128, else 1).  mse_parts (the content
    tap: conv2d(mse_ref=content, mse_parts=...)) with mse_out [3]: the content, feature
    and feature-mse values as style_content_loss writes them, from the same launch.
    Returns (deferred LossPart, coef) as style_loss with defer_ws."""
    _req(gparts, "gram partials")
    if (mse_parts is None) != (mse_out is None):
        raise ValueError("mse_parts and mse_out go together")
    if mse_parts is not None:
        _req(mse_parts, "mse_parts")
        assert mse_parts.numel() >= 2 * b * nparts and mse_out.numel() >= 3
    assert defer_ws is not None
    return _style_loss(b, c, hw, target, gparts.device, weight, diag_alpha, coef, defer_ws, fin,
                       parts=gparts, nparts=nparts, mse_parts=mse_parts, mse_out=mse_out)


class LossFinalizeJob:
    """One stx_loss_finalize call, described: launch() runs it as a launch of its own;
    conv_weight_compose16(loss_job=...) runs it as a rider of the compose launch.  Either
    way once (done)."""

    def __init__(self, parts, losses, extra=None, weights=None, total=None):
        self.lp = N.LossParts()
        assert len(parts) <= 8
        for i, (ptr, n, inv) in enumerate(parts):
            self.lp.parts[i], self.lp.nparts[i], self.lp.inv[i] = ptr, n, inv
        self.lp.k = len(parts)
        self.losses, self.extra, self.total = losses, extra, total
        self.m = 0 if extra is None else extra.numel()
        self.w = None
        if weights is not None:
            self.w = (C.c_float * len(weights))(*[float(x) for x in weights])
        self.done = False

    def launch(self):
        if not self.done:
            check(lib().stx_loss_finalize(C.byref(self.lp), self.losses.data_ptr(),
                                          _p(self.extra), self.m, self.w, _p(self.total),
                                          _stream()), "stx_loss_finalize")
            self.done = True
        return self.losses


def loss_finalize(parts, losses, extra=None, weights=None, total=None):
    """One launch: losses[i] = reduced deferred style-loss partials (parts from
    style_loss(defer_ws=...)), and optionally total = sum w_i losses_i + sum w extra."""
    return LossFinalizeJob(parts, losses, extra, weights, total).launch()


def gram_bwd_fused(coef, z, out=None, acc_scale=None, up_dp=None, aux=None, aux_scale=0.0,
                   out_amax=None, z_amax=None):
    """out = s*A[n].z[n] (+ unpool(up_dp)*(z>0)) (+ aux_scale*aux): the Gram backward
    as a 1x1 MFMA conv with the ReLU+MaxPool backward fused into its epilogue.
    z_amax (device >= max|z|) runs it on the fp16 hi/lo split MFMA."""
    b, c = z.shape[:2]
    return conv2d(z, coef, c, c, 1, pad=0, out=out, acc_scale=acc_scale, aux=aux,
                  aux_scale=aux_scale, wt_batch_stride=coef.shape[-1] * coef.shape[-2],
                  up_dp=up_dp, up_z=z if up_dp is not None else None, out_amax=out_amax,
                  in_amax=z_amax, split_1x1=z_amax is not None)


def gram_bwd(coef, z, dz=None, acc_scale=None, mask=None, aux=None, aux_scale=0.0,
             accumulate=False):
    _req(z, "z")
    b, c, h, w = z.shape
    if dz is None:
        dz = torch.empty_like(z)
    check(lib().stx_gram_bwd(coef.data_ptr(), z.data_ptr(), dz.data_ptr(), b, c, h, w,
                             _p(acc_scale), _p(mask), _p(aux), float(aux_scale), int(accumulate),
                             _stream()), "stx_gram_bwd")
    return dz


# ----------------------------------------------------------------------- guided gram
def guided_style_loss(z, wts, targets, lam, weight=1.0, z_amax=None, w_max=None, g_out=None,
                      coef=None, loss_r=None, want_coef=True, ws=None):
    """Region-weighted style loss (stx_guided_style_loss): R regions with pixel weights
    wts [R][hw] (each row normalised to sum hw), targets [R][c][c], lam = R host floats.
    Returns (loss_r [R] device floats, coef [b][R][cpad][cpad]) with
    coef[b][r] = weight * lam[r] * d loss_r / dG . 2/(c hw), the operator guided_gram_bwd
    applies.  z_amax (amax group >= max|z|) selects the fp16 hi/lo split MFMA where
    hw % 8 == 0.  w_max (host float >= wts.max()) is read from wts when absent (a host
    sync: pass it inside a captured iteration).  ws: a uint8 device buffer >=
    stx_guided_style_ws to use instead of the shared scratch."""
    _req(z, "z")
    _req(wts, "wts")
    _req(targets, "targets")
    b, c = z.shape[:2]
    hw = z[0, 0].numel()
    R = wts.shape[0]
    if wts.numel() != R * hw:
        raise ValueError(f"wts {tuple(wts.shape)} does not cover {hw} pixels per region")
    if targets.numel() != R * c * c:
        raise ValueError(f"targets {tuple(targets.shape)} is not ({R},{c},{c})")
    lam = [float(v) for v in lam]
    if len(lam) != R:
        raise ValueError(f"{len(lam)} region weights for {R} regions")
    if w_max is None:
        w_max = float(wts.max())
    if loss_r is None:
        loss_r = torch.empty(R, device=z.device, dtype=torch.float32)
    if want_coef and coef is None:
        cp = coef_pitch(c)
        coef = torch.empty((b, R, cp, cp), device=z.device, dtype=torch.float32)
    L = lib()
    need = L.stx_guided_style_ws(b, c, hw, R)
    if ws is not None:
        assert ws.numel() >= need > 0, (ws.numel(), need)
        wp, wn = ws.data_ptr(), ws.numel()
    else:
        wp, wn = WS.get(need, z.device)
    arr = (C.c_float * max(R, 1))(*lam)
    check(L.stx_guided_style_loss(z.data_ptr(), wts.data_ptr(), float(w_max), targets.data_ptr(),
                                  _p(g_out), _p(coef) if want_coef else None, loss_r.data_ptr(),
                                  b, c, hw, R, arr, float(weight), _p(z_amax), wp, wn,
                                  _stream()), "stx_guided_style_loss")
    return loss_r, (coef if want_coef else None)


def guided_gram_bwd(coef, z, wts, dz=None, acc_scale=None, accumulate=False, z_amax=None,
                    coef_amax=None):
    """dz (+)= s * sum_r wts[r] o (coef[:, r] . z) (stx_guided_gram_bwd), one pass over z.
    With z_amax and coef_amax (amax groups) the products run on the fp16 hi/lo split MFMA,
    else on the fp32 MFMA."""
    _req(z, "z")
    _req(wts, "wts")
    _req(coef, "coef")
    b, c, h, w = z.shape
    R = wts.shape[0]
    cp = coef_pitch(c)
    if wts.numel() != R * h * w or coef.numel() != b * R * cp * cp:
        raise ValueError(f"wts {tuple(wts.shape)} / coef {tuple(coef.shape)} do not match z "
                         f"{tuple(z.shape)} with {R} regions")
    if dz is None:
        if accumulate:
            raise ValueError("accumulate needs dz")
        dz = torch.empty_like(z)
    _req(dz, "dz")
    assert dz.shape == z.shape, (dz.shape, z.shape)
    check(lib().stx_guided_gram_bwd(coef.data_ptr(), z.data_ptr(), wts.data_ptr(), dz.data_ptr(),
                                    b, c, h, w, R, _p(acc_scale), int(accumulate), _p(z_amax),
                                    _p(coef_amax), _stream()), "stx_guided_gram_bwd")
    return dz


# ----------------------------------------------------------------------- mse etc
def mse(a, b, relu=False, mode=0, out=None, grad=None, gscale=1.0):
    """mode 0: F.mse_loss (mean); mode 1: FeatureReconstructionLoss (out[1] = mean)."""
    _req(a, "a")
    _req(b, "b")
    assert a.numel() == b.numel()
    n = a.numel()
    if out is None:
        out = torch.empty({0: 1, 1: 2, 2: 3}[mode], device=a.device, dtype=torch.float32)
    L = lib()
    wp, wn = WS.get(L.stx_mse_ws(n), a.device)
    check(L.stx_mse(a.data_ptr(), b.data_ptr(), n, int(relu), mode, out.data_ptr(), _p(grad),
                    float(gscale), wp, wn, _stream()), "stx_mse")
    return out


def diff_scale(a, b, s0, s1=None, s2=None, relu=False, out=None, accumulate=False):
    if out is None:
        out = torch.empty_like(a)
    check(lib().stx_diff_scale(a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), float(s0),
                               _p(s1), _p(s2), int(relu), int(accumulate), _stream()),
          "stx_diff_scale")
    return out


def loss_combine(s, weights, out):
    k = len(weights)
    arr = (C.c_float * k)(*[float(x) for x in weights])
    check(lib().stx_loss_combine(s.data_ptr(), k, arr, out.data_ptr(), _stream()),
          "stx_loss_combine")
    return out


# ----------------------------------------------------------------------- pooling / relu
def maxpool2x2(x, relu_input=False, want_idx=True):
    _req(x, "x")
    n, c, h, w = x.shape
    y = torch.empty((n, c, h // 2, w // 2), device=x.device, dtype=torch.float32)
    idx = torch.empty(y.shape, device=x.device, dtype=torch.int64) if want_idx else None
    check(lib().stx_maxpool2x2_fwd(x.data_ptr(), y.data_ptr(), _p(idx), n * c, h, w,
                                   int(relu_input), _stream()), "stx_maxpool2x2_fwd")
    return y, idx


def maxpool2x2_bwd(dy, idx, h, w):
    n, c = dy.shape[:2]
    dx = torch.empty((n, c, h, w), device=dy.device, dtype=torch.float32)
    check(lib().stx_maxpool2x2_bwd(dy.data_ptr(), idx.data_ptr(), dx.data_ptr(), n * c, h, w,
                                   _stream()), "stx_maxpool2x2_bwd")
    return dx


def relupool_bwd(dp, z, out=None):
    n, c, h, w = z.shape
    if out is None:
        out = torch.empty_like(z)
    check(lib().stx_relupool_bwd(dp.data_ptr(), z.data_ptr(), out.data_ptr(), n * c, h, w,
                                 _stream()), "stx_relupool_bwd")
    return out


def relu(x):
    _req(x, "x")
    y = torch.empty_like(x)
    check(lib().stx_relu_fwd(x.data_ptr(), y.data_ptr(), x.numel(), _stream()), "stx_relu_fwd")
    return y


def relu_bwd(dy, y):
    dx = torch.empty_like(dy)
    check(lib().stx_relu_bwd(dy.data_ptr(), y.data_ptr(), dx.data_ptr(), dy.numel(), _stream()),
          "stx_relu_bwd")
    return dx


# ----------------------------------------------------------------------- adam
def adam_step(p, g, m, v, step_dev, ws, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8,
              clear=None):
    """Adam update (stx_adam_step); clear: a float32 device tensor (<= 2^31 elements)
    zeroed in the same launch sequence (stx_adam_step_clear)."""
    if clear is not None:
        _req(clear, "clear")
        check(lib().stx_adam_step_clear(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(),
                                        p.numel(), float(lr), float(beta1), float(beta2),
                                        float(eps), step_dev.data_ptr(), ws.data_ptr(),
                                        clear.data_ptr(), clear.numel(), _stream()),
              "stx_adam_step_clear")
        return
    check(lib().stx_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(),
                              float(lr), float(beta1), float(beta2), float(eps),
                              step_dev.data_ptr(), ws.data_ptr(), _stream()), "stx_adam_step")


class AdamPrepare:
    """The first half of an Adam step (step counter + bias-corrected scalars into ws) for
    conv_weight_compose16(adam_prepare=...) to run as a rider of the compose launch; done
    tells the caller whether a launch took it (adam_step_prepared then, else adam_step)."""

    def __init__(self, step_dev, ws, lr=1e-3, beta1=0.9, beta2=0.999):
        self.step_dev, self.ws = step_dev, ws
        self.lr, self.beta1, self.beta2 = float(lr), float(beta1), float(beta2)
        self.done = False


def adam_step_prepared(p, g, m, v, ws, beta1=0.9, beta2=0.999, eps=1e-8, clear=None):
    """The Adam update alone, with the scalars an AdamPrepare rider left in ws for this step
    (stx_adam_step_prepared); clear: a float32 device tensor zeroed by the same launch."""
    if clear is not None:
        _req(clear, "clear")
    check(lib().stx_adam_step_prepared(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(),
                                       p.numel(), float(beta1), float(beta2), float(eps),
                                       ws.data_ptr(), _p(clear),
                                       0 if clear is None else clear.numel(), _stream()),
          "stx_adam_step_prepared")


# ----------------------------------------------------------------------- instance norm
def _mix_of(mix, n):
    """A step's style weights as the kernels take them: fp32 [n][S] on the device."""
    _req(mix, "mix")
    if mix.dim() != 2 or mix.shape[0] != n:
        raise ValueError(f"mix {tuple(mix.shape)}: [{n}][S] expected")
    return mix


def cin_mix(tables, mix):
    """Per-sample affine rows of conditional instance norm layers in one launch
    (stx_cin_mix).  tables: [(gtab, btab)] per layer, each [S][c]; mix [n][S].  Returns
    [(gamma_n, beta_n)] per layer, each [n][c] = mix @ table (fma chain, s ascending: a
    one-hot row reproduces the table row's bits)."""
    tables = list(tables)
    if not tables:
        return []
    n, S = _mix_of(mix, mix.shape[0]).shape
    jobs, out = [], []
    buf = torch.empty(2 * n * sum(g.shape[1] for g, _ in tables), device=mix.device,
                      dtype=torch.float32)
    o = 0
    for g, b in tables:
        _req(g, "gtab")
        _req(b, "btab")
        c = g.shape[1]
        if tuple(g.shape) != (S, c) or tuple(b.shape) != (S, c):
            raise ValueError(f"style tables {tuple(g.shape)} / {tuple(b.shape)}: [{S}][c] expected")
        gn, bn = buf[o:o + n * c].view(n, c), buf[o + n * c:o + 2 * n * c].view(n, c)
        o += 2 * n * c
        out.append((gn, bn))
        jobs.append(N.CinJob(g.data_ptr(), b.data_ptr(), gn.data_ptr(), bn.data_ptr(), None, None,
                             None, None, c, 0))
    for i in range(0, len(jobs), N.STX_CIN_MAX):
        chunk = jobs[i:i + N.STX_CIN_MAX]
        check(lib().stx_cin_mix((N.CinJob * len(chunk))(*chunk), len(chunk), mix.data_ptr(), n, S,
                                _stream()), "stx_cin_mix")
    return out


def instnorm_fwd(x, gamma, beta, res=None, eps=1e-5, relu=False, out=None, out_amax=None,
                 per_sample=False):
    """per_sample: gamma / beta are [n][c] (a row per sample: conditional instance norm);
    the kernels index their affine vectors by plane % c only, so the ABI is called with
    (1, n*c) -- the same kernel selection and bits as the shared-affine call."""
    _req(x, "x")
    n, c = x.shape[:2]
    hw = x[0, 0].numel()
    if per_sample:
        for t in (gamma, beta):
            if t is None or tuple(_req(t, "per-sample affine").shape) != (n, c):
                raise ValueError(f"per_sample: gamma and beta must be [{n}][{c}]")
        n, c = 1, n * c
    if out is None:
        out = torch.empty_like(x)
    mean = torch.empty(n * c, device=x.device, dtype=torch.float32)
    rstd = torch.empty_like(mean)
    check(lib().stx_instnorm_fwd(x.data_ptr(), _p(res), _p(gamma), _p(beta), out.data_ptr(),
                                 mean.data_ptr(), rstd.data_ptr(), n, c, hw, float(eps),
                                 int(relu), _p(out_amax), _stream()), "stx_instnorm_fwd")
    return out, mean, rstd


def instnorm_bwd(dy, beta, x, res, gamma, mean, rstd, relu=False, dgamma=None, dbeta=None,
                 accumulate=False, out_amax=None, dbias_in=None, per_sample=False, mix=None):
    """du of y = [relu](IN(x (+res))*gamma + beta); dgamma / dbeta / dbias_in (the bias
    gradient of the conv that produced x, sum du) written or accumulated when given.
    beta: the forward's beta (None if it had none): with relu the kernel recomputes the
    forward's y > 0 from x (+ res), mean, rstd, gamma, beta bit for bit (include/stx.h).
    per_sample (conditional instance norm): gamma / beta are the forward's [n][c] rows and
    the ABI is called with (1, n*c) as in instnorm_fwd; dgamma / dbeta are then the style
    tables' gradients [S][c] and mix [n][S] the step's style weights -- they and dbias_in
    come from the layer's partials through CINGRADS (one launch per step inside a
    training step, else one here)."""
    n, c = x.shape[:2]
    hw = x[0, 0].numel()
    du = torch.empty_like(x)
    L = lib()
    need = L.stx_instnorm_bwd_ws(n, c)
    if per_sample:
        if gamma is None or tuple(gamma.shape) != (n, c) or beta is None or \
                tuple(beta.shape) != (n, c):
            raise ValueError(f"per_sample: gamma and beta must be [{n}][{c}]")
        want = dgamma is not None or dbeta is not None or dbias_in is not None
        if want:
            S = _mix_of(mix, n).shape[1]
            for t in (dgamma, dbeta):
                if t is not None and tuple(_req(t, "table gradient").shape) != (S, c):
                    raise ValueError(f"per_sample: table gradients must be [{S}][{c}]")
            parts = torch.empty(need, device=x.device, dtype=torch.uint8)
            wp, wn = parts.data_ptr(), need
        else:
            wp, wn = WS.get(need, x.device)
        check(L.stx_instnorm_bwd(dy.data_ptr(), beta.data_ptr(), x.data_ptr(), _p(res),
                                 gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                 du.data_ptr(), None, None, None, 1, n * c, hw, int(relu), 0,
                                 _p(out_amax), wp, wn, _stream()), "stx_instnorm_bwd")
        if want:
            # deferred to the step's launch only when accumulating into persistent
            # buffers; a fresh gradient tensor must be complete on return
            CINGRADS.add(parts, mix, c, dgamma, dbeta, dbias_in, accumulate,
                         defer=bool(accumulate))
        return du
    # deferred only when accumulating into persistent buffers (.grad views): a fresh
    # gradient tensor handed back to autograd must be complete on return
    defer = PGRADS.active and accumulate and (
        dgamma is not None or dbeta is not None or dbias_in is not None)
    job = None
    if defer:  # partials kept for the step's single parameter-reduction launch
        parts = torch.empty(need, device=x.device, dtype=torch.uint8)
        job = (parts, n, c, dgamma, dbeta, dbias_in, accumulate)
        wp, wn = parts.data_ptr(), need
        dgamma = dbeta = dbias_in = None
    else:
        wp, wn = WS.get(need, x.device)
    check(L.stx_instnorm_bwd(dy.data_ptr(), _p(beta), x.data_ptr(), _p(res), _p(gamma),
                             mean.data_ptr(), rstd.data_ptr(), du.data_ptr(), _p(dgamma),
                             _p(dbeta), _p(dbias_in), n, c, hw, int(relu), int(accumulate),
                             _p(out_amax), wp,
                             wn, _stream()), "stx_instnorm_bwd")
    if job is not None:
        PGRADS.add(*job)  # after the kernel that writes its partials
    return du


# ----------------------------------------------------------------------- upsample / tv
def upsample2x(x):
    n, c, h, w = x.shape
    y = torch.empty((n, c, 2 * h, 2 * w), device=x.device, dtype=torch.float32)
    check(lib().stx_upsample2x_fwd(x.data_ptr(), y.data_ptr(), n * c, h, w, _stream()),
          "stx_upsample2x_fwd")
    return y


def upsample2x_bwd(dy):
    n, c, H, W = dy.shape
    dx = torch.empty((n, c, H // 2, W // 2), device=dy.device, dtype=torch.float32)
    check(lib().stx_upsample2x_bwd(dy.data_ptr(), dx.data_ptr(), n * c, H // 2, W // 2,
                                   _stream()), "stx_upsample2x_bwd")
    return dx


def tv_loss(y, factor=1e-6, grad=None, gscale=1.0, gscale_dev=None, out=None):
    _req(y, "y")
    n, c, h, w = y.shape
    if out is None:
        out = torch.empty((), device=y.device, dtype=torch.float32)
    L = lib()
    wp, wn = WS.get(L.stx_tv_ws(n, c, h, w), y.device)
    check(L.stx_tv_loss(y.data_ptr(), out.data_ptr(), _p(grad), float(gscale), _p(gscale_dev),
                        n, c, h, w, float(factor), wp, wn, _stream()), "stx_tv_loss")
    return out


# ----------------------------------------------------------------------- temporal loss
def temporal_loss(y, y_old, x, x_old, weight=1.0, out=None):
    """[loss, ||y - y_old||, ||x - x_old||] (device [3]), loss =
    ||y - y_old|| / (||x - x_old|| + 1) * weight (get_temporal_loss)."""
    for t, nm in ((y, "y"), (y_old, "y_old"), (x, "x"), (x_old, "x_old")):
        _req(t, nm)
    assert y.numel() == y_old.numel() == x.numel() == x_old.numel(), \
        (y.shape, y_old.shape, x.shape, x_old.shape)
    if out is None:
        out = torch.empty(3, device=y.device, dtype=torch.float32)
    L = lib()
    wp, wn = WS.get(L.stx_temporal_loss_ws(), y.device)
    check(L.stx_temporal_loss(y.data_ptr(), y_old.data_ptr(), x.data_ptr(), x_old.data_ptr(),
                              y.numel(), float(weight), out.data_ptr(), wp, wn, _stream()),
          "stx_temporal_loss")
    return out


def temporal_loss_bwd(y, y_old, fwd, weight=1.0, g=None, grad=None, accumulate=False):
    """d loss / d y of temporal_loss (fwd: its output), times the device scalar g."""
    if grad is None:
        grad = torch.empty_like(y)
    check(lib().stx_temporal_loss_bwd(y.data_ptr(), y_old.data_ptr(), y.numel(), fwd.data_ptr(),
                                      float(weight), _p(g), grad.data_ptr(), int(accumulate),
                                      _stream()), "stx_temporal_loss_bwd")
    return grad


# --------------------------------------------------------- flow-warped temporal consistency
def _flow2(t, name, like=None):
    _req(t, name)
    if t.dim() != 4 or t.shape[1] != 2 or min(t.shape[2:]) < 2:
        raise N.NativeError(f"{name}: a flow [n, 2, h, w] with h, w >= 2 required "
                            f"(got {tuple(t.shape)})")
    if like is not None and (t.shape[0], *t.shape[2:]) != (like.shape[0], *like.shape[2:]):
        raise N.NativeError(f"{name}: {tuple(t.shape)} does not match {tuple(like.shape)}")
    return t


def flow_warp(src, flow, fill=None, out=None, want_valid=False):
    """src [n, c, h, w] sampled bilinearly at (i + flow[:, 1], j + flow[:, 0]) (stx_flow_warp):
    a pixel whose source lies outside the image takes fill's value (0 without fill).
    want_valid: True returns (out, valid), valid [n, h, w] of 1.0 / 0.0; a tensor is filled
    and returned in that place.  out must not alias src."""
    _req(src, "src")
    if src.dim() != 4:
        raise N.NativeError(f"src: [n, c, h, w] required (got {tuple(src.shape)})")
    _flow2(flow, "flow", src)
    n, c, h, w = src.shape
    if out is None:
        out = torch.empty_like(src)
    for t, nm in ((fill, "fill"), (out, "out")):
        if t is not None:
            _req(t, nm)
            assert t.shape == src.shape, (nm, t.shape, src.shape)
    valid = None
    if want_valid is True:
        valid = torch.empty((n, h, w), device=src.device, dtype=torch.float32)
    elif want_valid is not False and want_valid is not None:
        valid = _req(want_valid, "valid")
        assert valid.numel() == n * h * w, (valid.shape, src.shape)
    check(lib().stx_flow_warp(src.data_ptr(), flow.data_ptr(), _p(fill), out.data_ptr(),
                              _p(valid), n, c, h, w, _stream()), "stx_flow_warp")
    return out if valid is None else (out, valid)


def flow_consistency(fwd, bwd, out=None):
    """The consistency mask [n, h, w] (1.0 / 0.0) of frame t given fwd (t-1 -> t) and bwd
    (t -> t-1): 0 where the backward flow leaves the image, at disocclusions and at motion
    boundaries (stx_flow_consistency; Ruder et al. 2016, eq. 5 and 6)."""
    _flow2(bwd, "bwd")
    _flow2(fwd, "fwd", bwd)
    n, _, h, w = bwd.shape
    if out is None:
        out = torch.empty((n, h, w), device=bwd.device, dtype=torch.float32)
    _req(out, "out")
    assert out.numel() == n * h * w, (out.shape, bwd.shape)
    check(lib().stx_flow_consistency(fwd.data_ptr(), bwd.data_ptr(), out.data_ptr(), n, h, w,
                                     _stream()), "stx_flow_consistency")
    return out


FLOW_COMPOSE_MAX = 4  # offsets one stx_flow_compose launch takes (include/stx.h)


def flow_compose(prevs, fwds, bwds, fill, ref=None, cmask=None, init=None, which=None):
    """(ref, cmask, init, which) of the long-term consistency loss in one launch
    (stx_flow_compose): prevs, fwds, bwds are lists of 1..4 tensors, nearest frame first --
    prevs[q] [n, c, h, w] an earlier result, (fwds[q], bwds[q]) the flows between that frame
    and this one.  Per pixel the first q whose flow_consistency predicate holds gives
    ref = init = flow_warp(prevs[q], bwds[q]), cmask = 1, which = q; a pixel with none has
    cmask = 0, which = 255, ref = 0 and init = flow_warp(prevs[0], bwds[0], fill).  which is
    uint8 [n, h, w]."""
    count = len(prevs)
    if not (len(fwds) == len(bwds) == count):
        raise N.NativeError(f"flow_compose: {count} prevs, {len(fwds)} fwds, {len(bwds)} bwds")
    if count:
        src = _req(prevs[0], "prevs[0]")
        if src.dim() != 4:
            raise N.NativeError(f"prevs[0]: [n, c, h, w] required (got {tuple(src.shape)})")
        for q in range(count):
            _req(prevs[q], f"prevs[{q}]")
            assert prevs[q].shape == src.shape, (q, prevs[q].shape, src.shape)
            _flow2(bwds[q], f"bwds[{q}]", src)
            _flow2(fwds[q], f"fwds[{q}]", src)
    else:
        src = _req(fill, "fill")
    n, c, h, w = src.shape
    if ref is None:
        ref = torch.empty_like(src)
    if cmask is None:
        cmask = torch.empty((n, h, w), device=src.device, dtype=torch.float32)
    if init is None:
        init = torch.empty_like(src)
    if which is None:
        which = torch.empty((n, h, w), device=src.device, dtype=torch.uint8)
    for t, nm in ((fill, "fill"), (ref, "ref"), (init, "init")):
        _req(t, nm)
        assert t.shape == src.shape, (nm, t.shape, src.shape)
    _req(cmask, "cmask")
    assert cmask.numel() == n * h * w, (cmask.shape, src.shape)
    if which.dtype != torch.uint8 or not which.is_contiguous() or which.numel() != n * h * w \
            or which.device != src.device:
        raise N.NativeError(f"which: a contiguous uint8 [n, h, w] on {src.device} required")
    table = lambda ts: (C.c_void_p * max(count, 1))(*[t.data_ptr() for t in ts])
    check(lib().stx_flow_compose(table(prevs), table(fwds), table(bwds), count, fill.data_ptr(),
                                 ref.data_ptr(), cmask.data_ptr(), init.data_ptr(),
                                 which.data_ptr(), n, c, h, w, _stream()), "stx_flow_compose")
    return ref, cmask, init, which


def masked_mse(x, ref, mask, weight, out=None, add_to=None, grad=None, accumulate=False):
    """out[0] = weight / x.numel() * sum over mask != 0 of (x - ref)^2 (stx_masked_mse), x and
    ref [n, c, h, w], mask [n, h, w] shared by the channels.  add_to: a device scalar that
    receives += the loss; grad: written, or with accumulate added to, 2 weight / x.numel() *
    (x - ref) under the mask (a masked-out element is 0, or left as it is)."""
    _req(x, "x")
    _req(ref, "ref")
    _req(mask, "mask")
    if x.dim() != 4 or ref.shape != x.shape:
        raise N.NativeError(f"x, ref: equal [n, c, h, w] required (got {tuple(x.shape)}, "
                            f"{tuple(ref.shape)})")
    n, c, h, w = x.shape
    if mask.numel() != n * h * w:
        raise N.NativeError(f"mask: [n, h, w] of x {tuple(x.shape)} required "
                            f"(got {tuple(mask.shape)})")
    if out is None:
        out = torch.empty(1, device=x.device, dtype=torch.float32)
    for t, nm in ((out, "out"), (add_to, "add_to"), (grad, "grad")):
        if t is not None:
            _req(t, nm)
    if grad is not None:
        assert grad.shape == x.shape, (grad.shape, x.shape)
    L = lib()
    wp, wn = _scratch().get(L.stx_masked_mse_ws(), x.device)
    check(L.stx_masked_mse(x.data_ptr(), ref.data_ptr(), mask.data_ptr(), n, c, h * w,
                           float(weight), out.data_ptr(), _p(add_to), _p(grad),
                           int(bool(accumulate)), wp, wn, _stream()), "stx_masked_mse")
    return out


# ------------------------------------------------- adaptive instance norm (arbitrary style)
def _planes(x, name="x"):
    _req(x, name)
    if x.dim() < 3:
        raise N.NativeError(f"{name}: [n, c, ...] planes required (got {tuple(x.shape)})")
    n, c = x.shape[:2]
    return n, c, x[0, 0].numel()


def _nc(t, n, c, name):
    if t is not None and (_req(t, name).numel() != n * c):
        raise N.NativeError(f"{name}: [{n}][{c}] required (got {tuple(t.shape)})")
    return t


def chan_stats(x, eps=1e-5, relu_input=False):
    """(mean, std) [n, c] of the planes of x (stx_chan_stats): unbiased variance, eps inside
    the root; relu_input takes them of max(x, 0) with a NaN kept."""
    n, c, hw = _planes(x)
    mean = torch.empty(n, c, device=x.device, dtype=torch.float32)
    std = torch.empty_like(mean)
    check(lib().stx_chan_stats(x.data_ptr(), mean.data_ptr(), std.data_ptr(), n, c, hw,
                               float(eps), int(bool(relu_input)), _stream()), "stx_chan_stats")
    return mean, std


def adain(x, smean, sstd, mix, alpha=1.0, eps=1e-5, out=None, out_amax=None, stats=False):
    """y = fma(x, a, b) per plane (stx_adain): style tables smean, sstd [S, c], mix [n, S],
    strength alpha.  stats=True also returns the content (mean, std) [n, c]."""
    n, c, hw = _planes(x)
    _req(smean, "smean")
    _req(sstd, "sstd")
    _req(mix, "mix")
    if smean.dim() != 2 or smean.shape[1] != c or sstd.shape != smean.shape:
        raise N.NativeError(f"smean, sstd: equal [S][{c}] required (got {tuple(smean.shape)}, "
                            f"{tuple(sstd.shape)})")
    S = smean.shape[0]
    if tuple(mix.shape) != (n, S):
        raise N.NativeError(f"mix: [{n}][{S}] required (got {tuple(mix.shape)})")
    if out is None:
        out = torch.empty_like(x)
    elif _req(out, "out").shape != x.shape:
        raise N.NativeError(f"out: the shape of x required (got {tuple(out.shape)})")
    mean = std = None
    if stats:
        mean = torch.empty(n, c, device=x.device, dtype=torch.float32)
        std = torch.empty_like(mean)
    check(lib().stx_adain(x.data_ptr(), smean.data_ptr(), sstd.data_ptr(), mix.data_ptr(),
                          float(alpha), out.data_ptr(), _p(mean), _p(std), n, c, hw, S,
                          float(eps), _p(out_amax), _stream()), "stx_adain")
    return (out, mean, std) if stats else out


def stats_loss(x, tmean, tstd, weight=1.0, eps=1e-5, out=None, add_to=None, save=True):
    """out[0] = weight / (n c) * sum [(mean - tmean)^2 + (std - tstd)^2], out[1] / out[2] the
    two parts (stx_stats_loss); returns (out, mean, std) with the statistics saved for
    stats_loss_bwd (None, None with save=False)."""
    n, c, hw = _planes(x)
    _nc(tmean, n, c, "tmean")
    _nc(tstd, n, c, "tstd")
    if tmean is None or tstd is None:
        raise N.NativeError("tmean, tstd required")
    if out is None:
        out = torch.empty(3, device=x.device, dtype=torch.float32)
    elif _req(out, "out").numel() < 3:
        raise N.NativeError("out: 3 floats required")
    if add_to is not None:
        _req(add_to, "add_to")
    mean = std = None
    if save:
        mean = torch.empty(n, c, device=x.device, dtype=torch.float32)
        std = torch.empty_like(mean)
    L = lib()
    wp, wn = _scratch().get(L.stx_stats_loss_ws(n, c), x.device)
    check(L.stx_stats_loss(x.data_ptr(), tmean.data_ptr(), tstd.data_ptr(), n, c, hw, float(eps),
                           float(weight), out.data_ptr(), _p(add_to), _p(mean), _p(std), wp, wn,
                           _stream()), "stx_stats_loss")
    return out, mean, std


def stats_loss_bwd(x, mean, std, tmean, tstd, weight=1.0, g_dev=None, dx=None, accumulate=False,
                   out_amax=None):
    """dx (+)= d stats_loss / dx scaled by *g_dev (stx_stats_loss_bwd), from the forward's
    saved mean, std.  accumulate needs dx."""
    n, c, hw = _planes(x)
    for t, nm in ((mean, "mean"), (std, "std"), (tmean, "tmean"), (tstd, "tstd")):
        if t is None:
            raise N.NativeError(f"{nm} required")
        _nc(t, n, c, nm)
    if g_dev is not None:
        _req(g_dev, "g_dev")
    if dx is None:
        if accumulate:
            raise N.NativeError("accumulate: dx required")
        dx = torch.empty_like(x)
    elif _req(dx, "dx").shape != x.shape:
        raise N.NativeError(f"dx: the shape of x required (got {tuple(dx.shape)})")
    check(lib().stx_stats_loss_bwd(x.data_ptr(), mean.data_ptr(), std.data_ptr(),
                                   tmean.data_ptr(), tstd.data_ptr(), n, c, hw, float(weight),
                                   _p(g_dev), dx.data_ptr(), int(bool(accumulate)),
                                   _p(out_amax), _stream()), "stx_stats_loss_bwd")
    return dx


# ---------------------------------------------------------------------- colour control
def _img3(t, name):
    _req(t, name)
    if t.dim() != 4 or t.shape[1] != 3:
        raise N.NativeError(f"{name}: [n, 3, h, w] required (got {tuple(t.shape)})")
    return t


def _host_f32(v, count, name):
    """A small host array (numpy / list / None) as a ctypes float array, or None."""
    if v is None:
        return None
    flat = [float(e) for row in v for e in (row if hasattr(row, "__len__") else [row])]
    if len(flat) != count:
        raise ValueError(f"{name}: {count} values expected, got {len(flat)}")
    return (C.c_float * count)(*flat)


def color_stats(x, out=None):
    """Per image of x [n, 3, h, w]: RGB mean[3] and the population covariance's upper
    triangle [rr, rg, rb, gg, gb, bb], a device fp64 tensor [n, 9] (stx_color_stats)."""
    _img3(x, "x")
    n, _, h, w = x.shape
    if out is None:
        out = torch.empty((n, 9), device=x.device, dtype=torch.float64)
    assert out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() \
        and out.numel() == 9 * n, (out.shape, out.dtype)
    L = lib()
    wp, wn = _scratch().get(L.stx_color_stats_ws(n, h, w), x.device)
    check(L.stx_color_stats(x.data_ptr(), out.data_ptr(), n, h, w, wp, wn, _stream()),
          "stx_color_stats")
    return out


def color_affine(x, M, b=None, base=None, lo=None, hi=None, out=None):
    """out[c] = clamp(base[c] + sum_d M[c][d] (x[d] - base[d]) + b[c]) per pixel of
    [n, 3, h, w] (stx_color_affine).  M [3][3], b, lo, hi [3]: host values, baked into the
    launch; base None reads as zeros; lo / hi None: no clamp.  out may be x or base."""
    _img3(x, "x")
    if out is None:
        out = torch.empty_like(x)
    for t, nm in ((base, "base"), (out, "out")):
        if t is not None:
            _img3(t, nm)
            assert t.shape == x.shape, (nm, t.shape, x.shape)
    n, _, h, w = x.shape
    check(lib().stx_color_affine(x.data_ptr(), _p(base), out.data_ptr(), n, h, w,
                                 _host_f32(M, 9, "M"), _host_f32(b, 3, "b"),
                                 _host_f32(lo, 3, "lo"), _host_f32(hi, 3, "hi"), _stream()),
          "stx_color_affine")
    return out


# ------------------------------------------------------------------------ scale control
FILTERS = {"triangle": 0, "cubic": 1}  # STX_FILTER_* (include/stx.h)
_RESAMPLE_TABLES = {}  # (in, out, filter, device) -> (first, count, w, k) on the device


def resample_plan(n_in, n_out, filter="cubic"):
    """(first [out] int32, count [out] int32, w [out][k] fp32, k) of one axis, numpy arrays
    (stx_resample_plan: a host function, no GPU needed)."""
    import numpy as np
    if filter not in FILTERS:
        raise ValueError(f"filter {filter!r}: expected one of {tuple(FILTERS)}")
    L = lib()
    k = L.stx_resample_plan(int(n_in), int(n_out), FILTERS[filter], None, None, None, 0)
    if k <= 0:
        check(-k, "stx_resample_plan")
    first = np.zeros(n_out, np.int32)
    count = np.zeros(n_out, np.int32)
    w = np.zeros((n_out, k), np.float32)
    rc = L.stx_resample_plan(int(n_in), int(n_out), FILTERS[filter], first.ctypes.data,
                             count.ctypes.data, w.ctypes.data, k)
    if rc != k:
        check(-rc if rc < 0 else 1001, "stx_resample_plan")  # (1001: STX_E_INVALID)
    return first, count, w, k


def _resample_tables(n_in, n_out, filter, device):
    """The device copy of an axis plan, uploaded once per (in, out, filter, device): a
    later call with the same sizes makes no host-to-device copy (and can be captured)."""
    key = (int(n_in), int(n_out), filter, torch.device(device))
    t = _RESAMPLE_TABLES.get(key)
    if t is None:
        first, count, w, k = resample_plan(n_in, n_out, filter)
        t = (torch.from_numpy(first).to(device), torch.from_numpy(count).to(device),
             torch.from_numpy(w).to(device), k)
        _RESAMPLE_TABLES[key] = t
    return t


def resample2d(x, size, filter="cubic", out=None):
    """x [n, c, h, w] or [r, h, w] resized to size = (ho, wo) (an int: both), antialiased,
    half-pixel centres (stx_resample2d; torch's interpolate(..., align_corners=False,
    antialias=True) with "bilinear" for "triangle" and "bicubic" for "cubic").  out must
    not alias x; an unchanged size gives an exact copy."""
    _req(x, "x")
    if x.dim() not in (3, 4):
        raise N.NativeError(f"x: [n, c, h, w] or [r, h, w] required (got {tuple(x.shape)})")
    ho, wo = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
    lead, (hi, wi) = tuple(x.shape[:-2]), x.shape[-2:]
    nc = 1
    for d in lead:
        nc *= d
    if out is None:
        out = torch.empty(lead + (ho, wo), device=x.device, dtype=torch.float32)
    _req(out, "out")
    assert tuple(out.shape) == lead + (ho, wo), (out.shape, lead, ho, wo)
    none = (None, None, None, 0)
    xf, xc, xw, xk = _resample_tables(wi, wo, filter, x.device) if wi != wo else none
    yf, yc, yw, yk = _resample_tables(hi, ho, filter, x.device) if hi != ho else none
    L = lib()
    wp, wn = _scratch().get(L.stx_resample2d_ws(nc, hi, wi, ho, wo), x.device)
    check(L.stx_resample2d(x.data_ptr(), out.data_ptr(), nc, hi, wi, ho, wo, _p(xf), _p(xc),
                           _p(xw), xk, _p(yf), _p(yc), _p(yw), yk, wp, wn, _stream()),
          "stx_resample2d")
    return out


# ----------------------------------------------------------------- optical-flow estimation
def flow_pyramid(h, w, min_side=16):
    """[(h_0, w_0), (h_1, w_1), ...]: the levels of the flow estimator's pyramid, finest
    first (stx_flow_pyramid: a host function, no GPU needed)."""
    L = lib()
    n = L.stx_flow_pyramid(int(h), int(w), int(min_side), None, None, 0)
    if n <= 0:
        check(-n, "stx_flow_pyramid")
    hs, ws = (C.c_int * n)(), (C.c_int * n)()
    if L.stx_flow_pyramid(int(h), int(w), int(min_side), hs, ws, n) != n:
        check(1001, "stx_flow_pyramid")  # (1001: STX_E_INVALID)
    return list(zip(hs, ws))


def flow_luma(img, mean=None, std=None, out=None):
    """grey [n, h, w] = 255 (0.299 R + 0.587 G + 0.114 B) of a conditioned image
    [n, 3, h, w], R = r std[0] + mean[0] and so on (stx_flow_luma; mean, std default to
    ImageNet's, as image conditioning applies them)."""
    from . import constants
    _img3(img, "img")
    n, _, h, w = img.shape
    if out is None:
        out = torch.empty((n, h, w), device=img.device, dtype=torch.float32)
    _req(out, "out")
    assert out.numel() == n * h * w, (out.shape, img.shape)
    check(lib().stx_flow_luma(img.data_ptr(), out.data_ptr(), n, h, w,
                              _host_f32(constants.IMAGENET_MEAN if mean is None else mean, 3, "mean"),
                              _host_f32(constants.IMAGENET_STD if std is None else std, 3, "std"),
                              _stream()), "stx_flow_luma")
    return out


def _grey(t, name, flow):
    _req(t, name)
    if t.dim() != 3 or (t.shape[0], *t.shape[1:]) != (flow.shape[0], *flow.shape[2:]):
        raise N.NativeError(f"{name}: [n, h, w] of the flow {tuple(flow.shape)} required "
                            f"(got {tuple(t.shape)})")
    return t


def flow_linearize(a, b, flow, out=None):
    """coef [n, 3, h, w] = (Ix, Iy, c) of luma planes a, b [n, h, w] at the flow [n, 2, h, w]:
    b and its central-difference gradient sampled at the clamped (i + flow[1], j + flow[0]),
    c = a - b_warped + Ix u + Iy v (stx_flow_linearize)."""
    _flow2(flow, "flow")
    _grey(a, "a", flow)
    _grey(b, "b", flow)
    n, _, h, w = flow.shape
    if out is None:
        out = torch.empty((n, 3, h, w), device=flow.device, dtype=torch.float32)
    _req(out, "out")
    assert tuple(out.shape) == (n, 3, h, w), (out.shape, flow.shape)
    check(lib().stx_flow_linearize(a.data_ptr(), b.data_ptr(), flow.data_ptr(), out.data_ptr(),
                                   n, h, w, _stream()), "stx_flow_linearize")
    return out


def flow_jacobi(coef, uv, out=None, alpha=15.0, iters=40, fuse=0):
    """`iters` Jacobi iterations of the Horn-Schunck system of coef [n, 3, h, w] from uv
    [n, 2, h, w] (stx_flow_jacobi).  fuse: iterations per launch (0: the library's choice);
    the result does not depend on it.  out must not alias uv."""
    _flow2(uv, "uv")
    _req(coef, "coef")
    n, _, h, w = uv.shape
    if tuple(coef.shape) != (n, 3, h, w):
        raise N.NativeError(f"coef: {(n, 3, h, w)} required (got {tuple(coef.shape)})")
    if out is None:
        out = torch.empty_like(uv)
    _flow2(out, "out", uv)
    L = lib()
    wp, wn = _scratch().get(L.stx_flow_jacobi_ws(n, h, w), uv.device)
    check(L.stx_flow_jacobi(coef.data_ptr(), uv.data_ptr(), out.data_ptr(), n, h, w,
                            float(alpha), int(iters), int(fuse), wp, wn, _stream()),
          "stx_flow_jacobi")
    return out


def flow_scale(flow, sx, sy):
    """flow[:, 0] *= sx, flow[:, 1] *= sy in place (stx_flow_scale: a prolonged flow's
    displacements in the finer level's pixels)."""
    _flow2(flow, "flow")
    n, _, h, w = flow.shape
    check(lib().stx_flow_scale(flow.data_ptr(), n, h, w, float(sx), float(sy), _stream()),
          "stx_flow_scale")
    return flow
