"""Arbitrary-style transfer by adaptive instance normalisation (Huang & Belongie 2017,
"Arbitrary Style Transfer in Real-time with Adaptive Instance Normalization"): a style
never trained on, given at conversion time, in one forward pass, blendable (`mix`) and
with a strength knob (`alpha`).

    t = AdaIN(f(content), f(style));   image = g(t)

f is the frozen VGG-19 prefix through relu4_1 (Encoder), g its mirror (Decoder, the only
trained part).  The statistics, the transform and the mean/std style loss are HIP kernels
(csrc/adain.hip: stx_chan_stats, stx_adain, stx_stats_loss, stx_stats_loss_bwd); the convs
are the project's own.  Padding is zeros (layers.Conv2d), where the paper reflects.
The reference project has no counterpart.  Nothing here falls back to torch compute: a CPU
tensor raises.
"""
from __future__ import annotations

import os
import random

import numpy as np
import torch
import torch.nn as nn

from . import _native as N
from . import autograd as A
from . import c_logging, constants, img_utils, ops
from . import weights as W
from .layers import Conv2d, MaxPool2d, ReLU, Upsample
from .optim import FlatAdam

LOGGER = c_logging.get_logger()

EPS = 1e-5
MODEL_NAME = "adain"
# torchvision `features` indices of the nine convs through conv4_1
ENCODER_CONVS = (0, 2, 5, 7, 10, 12, 14, 16, 19)
# the encoder as a list: a conv's (cin, cout) followed by its ReLU, "M" a MaxPool2d(2, 2),
# "T" a tap (relu1_1, relu2_1, relu3_1, relu4_1)
ENCODER_PLAN = ((3, 64), "T", (64, 64), "M", (64, 128), "T", (128, 128), "M", (128, 256), "T",
                (256, 256), (256, 256), (256, 256), "M", (256, 512), "T")
TAP_CHANNELS = (64, 128, 256, 512)
# the decoder: (cin, cout, relu after it), "U" a nearest x2 upsample
DECODER_PLAN = ((512, 256, True), "U", (256, 256, True), (256, 256, True), (256, 256, True),
                (256, 128, True), "U", (128, 128, True), (128, 64, True), "U", (64, 64, True),
                (64, 3, False))
IMAGE_EXTS = (".jpg", ".jpeg", ".png", ".bmp")


def load_vgg19_deep_weights(path: str | None = None, seed: int = 1234):
    """The nine VGG-19 convs through conv4_1 as [(w, b)] numpy arrays: from a local
    torchvision state dict (keys `features.{0,2,5,7,10,12,14,16,19}.*` or without the prefix)
    when `path` or $STX_VGG19_WEIGHTS names one (weights_only=True), else deterministic
    synthetic weights.  The first five entries equal vgg.load_vgg19_weights' for the same
    arguments."""
    path = path or os.environ.get("STX_VGG19_WEIGHTS")
    if path and os.path.exists(path):
        sd = torch.load(path, map_location="cpu", weights_only=True)
        out = []
        for idx in ENCODER_CONVS:
            for pre in ("features.", ""):
                if f"{pre}{idx}.weight" in sd:
                    out.append((sd[f"{pre}{idx}.weight"].float().numpy(),
                                sd[f"{pre}{idx}.bias"].float().numpy()))
                    break
            else:
                raise KeyError(f"VGG-19 weights file {path} lacks conv index {idx}")
        return out
    return W.vgg19_synthetic(seed, len(ENCODER_CONVS))


# ----------------------------------------------------------------------------- autograd
class AdaINFn(torch.autograd.Function):
    """stx_adain, forward only: in training its input comes from the frozen encoder.  A
    gradient requested through it is an error, not zeros."""

    @staticmethod
    def forward(ctx, x, smean, sstd, mix, alpha, eps):
        x = A._c(x)
        g = ops.ARENA.take(x.device)  # max|y|: the first decoder conv's input scale
        y = ops.adain(x, smean, sstd, mix, alpha, eps, out_amax=g)
        return ops.ARENA.annotate(y, g)

    @staticmethod
    def backward(ctx, dy):
        raise RuntimeError("AdaINFn has no backward: the AdaIN transform is applied to the "
                           "frozen encoder's features (detach its inputs)")


class StatsLossFn(torch.autograd.Function):
    """(x, loss) = tap(x): x passes through, loss = weight / (n c) * sum [(mean - tmean)^2 +
    (std - tstd)^2] (stx_stats_loss).  The backward adds the loss's gradient into the
    gradient arriving for x from the deeper layers in the same pass (stx_stats_loss_bwd with
    accumulate: that buffer is updated in place), or writes it when nothing arrives."""

    @staticmethod
    def forward(ctx, x, tmean, tstd, weight, eps):
        x = A._c(x)
        out, mean, std = ops.stats_loss(x, tmean, tstd, weight, eps)
        ctx.save_for_backward(x, mean, std, tmean, tstd)
        ctx.weight = weight
        ctx.set_materialize_grads(False)
        return x.view_as(x), out[0]

    @staticmethod
    def backward(ctx, dy, gl):
        if gl is None:
            return dy, None, None, None, None
        x, mean, std, tmean, tstd = ctx.saved_tensors
        g = A._c(gl.reshape(1))
        if dy is None:
            dx = ops.stats_loss_bwd(x, mean, std, tmean, tstd, ctx.weight, g_dev=g)
        else:
            dx = ops.stats_loss_bwd(x, mean, std, tmean, tstd, ctx.weight, g_dev=g,
                                    dx=A._c(dy), accumulate=True)
        return dx, None, None, None, None


def stats_loss(x, tmean, tstd, weight=1.0, eps=EPS):
    """The differentiable statistics loss alone (the pass-through output dropped)."""
    return StatsLossFn.apply(x, tmean, tstd, float(weight), float(eps))[1]


# ------------------------------------------------------------------------------ networks
class Encoder(nn.Module):
    """The frozen VGG-19 prefix through relu4_1 on layers.Conv2d / ReLU / MaxPool2d;
    forward returns the taps [relu1_1, relu2_1, relu3_1, relu4_1].  requires_grad=False on
    every weight lets Conv2d.prepped() cache its slabs."""

    def __init__(self, weights=None, device=None):
        super().__init__()
        params = weights if isinstance(weights, list) else load_vgg19_deep_weights(weights)
        mods, k = [], 0
        for item in ENCODER_PLAN:
            if item == "M":
                mods.append(MaxPool2d(2, 2))
            elif item == "T":
                mods.append(nn.Identity())  # a tap: after the ReLU before it
            else:
                cin, cout = item
                conv = Conv2d(cin, cout, kernel_size=3, padding=1)
                w, b = params[k]
                assert tuple(w.shape) == (cout, cin, 3, 3), (k, w.shape)
                with torch.no_grad():
                    conv.weight.copy_(torch.as_tensor(np.ascontiguousarray(w)))
                    conv.bias.copy_(torch.as_tensor(np.ascontiguousarray(b)))
                mods += [conv, ReLU()]
                k += 1
        self.features = nn.Sequential(*mods)
        self.to(device or constants.DEVICE).eval()
        for p in self.parameters():
            p.requires_grad_(False)

    def convs(self):
        return [m for m in self.features if isinstance(m, nn.Conv2d)]

    def forward(self, x, tap_fn=None, last_only=False):
        """tap_fn(i, x) -> x: called at tap i with the tap's tensor, its result goes on
        (StatsLossFn in training).  last_only: return relu4_1 alone."""
        taps = []
        for m in self.features:
            if isinstance(m, nn.Identity):
                if tap_fn is not None:
                    x = tap_fn(len(taps), x)
                taps.append(x)
            else:
                x = m(x)
        return taps[-1] if last_only else taps


class Decoder(nn.Sequential):
    """The mirror of the encoder: 3x3 stride-1 zero-padded convs, a ReLU after each but the
    last, nearest x2 upsampling before the convs that leave relu4_1's, relu3_1's and
    relu2_1's resolution.  A conv behind an Upsample reads its input through the conv
    loader's upsampling mode (_up_input: it gets the parity-class slab).  seed: He-scaled
    deterministic initial weights (weights.he_conv); None keeps torch's default init."""

    def __init__(self, seed: int | None = None, device=None):
        mods, up, k = [], False, 0
        for item in DECODER_PLAN:
            if item == "U":
                mods.append(Upsample(mode="nearest", scale_factor=2))
                up = True
                continue
            cin, cout, relu = item
            conv = Conv2d(cin, cout, kernel_size=3, padding=1)
            conv._up_input = up
            up = False
            if seed is not None:
                w, b = W.he_conv(seed * 1000 + k, cout, cin, 3)
                with torch.no_grad():
                    conv.weight.copy_(torch.from_numpy(w))
                    conv.bias.copy_(torch.from_numpy(b))
            k += 1
            mods.append(conv)
            if relu:
                mods.append(ReLU())
        super().__init__(*mods)
        self.to(device or constants.DEVICE)

    def forward(self, x):
        up = False
        for m in self._modules.values():
            if isinstance(m, Upsample):
                up = True  # fused into the next conv's loader
            elif isinstance(m, nn.Conv2d):
                x = m(x, N.STX_IN_UPSAMPLE2 if up else N.STX_IN_RAW)
                up = False
            else:
                x = m(x)
        return x


def parse_style_mix(spec, names):
    """--mix 'a.jpg:0.3,b.jpg:0.7' over the given style names -> weights in their order,
    normalised to sum 1; None / '' weighs every given style equally.  Errors as
    network.parse_mix (unknown or repeated name, malformed or negative weight, zero sum)."""
    from .network import parse_mix
    names = list(names)
    if len(set(names)) != len(names):
        raise ValueError(f"style names must differ: {names}")
    if not spec:
        return [1.0 / len(names)] * len(names)
    return parse_mix(spec, names)


def _to_device_image(t):
    t = torch.as_tensor(t)
    if t.dim() == 3:
        t = t.unsqueeze(0)
    return t.to(constants.DEVICE, torch.float32).contiguous()


class AdaINNet(nn.Module):
    """Encoder + AdaIN + Decoder.  state: only the decoder is trained and saved."""

    def __init__(self, vgg_weights=None, decoder_seed: int | None = None, device=None):
        super().__init__()
        self.encoder = Encoder(vgg_weights, device)
        self.decoder = Decoder(decoder_seed, device)

    @property
    def device(self):
        return self.decoder[0].weight.device

    @torch.no_grad()
    def style_stats(self, style_images):
        """(smean, sstd) [S, 512] at relu4_1 of a batch [S, 3, h, w] or a sequence of images
        (each [3, h, w] or [1, 3, h, w], sizes may differ)."""
        if isinstance(style_images, torch.Tensor):
            groups = [style_images if style_images.dim() == 4 else style_images.unsqueeze(0)]
        else:
            groups = [s if s.dim() == 4 else s.unsqueeze(0) for s in style_images]
        means, stds = [], []
        for g in groups:
            m, s = ops.chan_stats(self.encoder(g.to(self.device, torch.float32).contiguous(),
                                               last_only=True), EPS)
            means.append(m)
            stds.append(s)
        return torch.cat(means).contiguous(), torch.cat(stds).contiguous()

    def mix_of(self, mix, n, S):
        """None (the first style), weights [S] or rows [n][S] -> fp32 [n][S] on the device."""
        if mix is None:
            mix = [1.0] + [0.0] * (S - 1)
        mix = torch.as_tensor(mix, dtype=torch.float32)
        if mix.dim() == 1:
            mix = mix.expand(n, -1)
        if tuple(mix.shape) != (n, S):
            raise ValueError(f"mix {tuple(mix.shape)}: [{n}][{S}] or [{S}] expected")
        return mix.to(self.device, torch.float32).contiguous()

    def forward(self, content, style, mix=None, alpha=1.0):
        """content [n, 3, h, w]; style: images (see style_stats) or their (smean, sstd);
        mix: see mix_of; alpha: 0 keeps the content features, 1 is the full transfer."""
        if isinstance(style, tuple) and len(style) == 2 and style[0].dim() == 2:
            smean, sstd = style
        else:
            smean, sstd = self.style_stats(style)
        with torch.no_grad():
            fc = self.encoder(content, last_only=True)
        m = self.mix_of(mix, fc.shape[0], smean.shape[0])
        t = AdaINFn.apply(fc, smean, sstd, m, float(alpha), EPS)
        return self.decoder(t)

    # ---------------------------------------------------------------- checkpoints
    @staticmethod
    def checkpoint_path(name, epoch, models_path="data/models/"):
        return os.path.join(constants.PROJECT_ROOT_PATH, models_path,
                            f"{MODEL_NAME}_{name}_epoch{epoch}.pth")

    def save(self, name, epoch, models_path="data/models/"):
        path = self.checkpoint_path(name, epoch, models_path)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        torch.save(self.decoder.state_dict(), path)
        return path

    def load(self, path):
        loc = "cuda" if self.device.type == "cuda" else "cpu"
        self.decoder.load_state_dict(torch.load(path, map_location=loc, weights_only=True))

    def load_latest(self, name, models_path="data/models/"):
        """Load the lexicographically last `adain_{name}_epoch*.pth` (the decoder)."""
        root = os.path.join(constants.PROJECT_ROOT_PATH, models_path)
        pre = f"{MODEL_NAME}_{name}_epoch"
        found = sorted(f for f in (os.listdir(root) if os.path.isdir(root) else [])
                       if f.startswith(pre) and f.endswith(".pth"))
        if not found:
            raise AssertionError(f"There are no AdaIN decoder weights named {name!r} in {root}")
        self.load(os.path.join(root, found[-1]))
        return found[-1]

    # ---------------------------------------------------------------- workflows
    def convert(self, image, styles, mix=None, alpha=1.0, preserve_color=False):
        """One conditioned image [1, 3, h, w] through the net (no gradient)."""
        with torch.no_grad():
            out = self(image, styles, mix=mix, alpha=alpha)
        if preserve_color:
            from . import color
            out = color.merge_luminance(out, image)
        return out

    def process_image(self, image_path, style_paths, mix=None, alpha=1.0, preserve_color=False,
                      name="nsp", out_dir="results/"):
        """Convert an image with the latest decoder of `name` and the styles at style_paths;
        mix: None (the first style) or weights over style_paths.  Returns the output."""
        self.load_latest(name)
        root = constants.PROJECT_ROOT_PATH
        image = img_utils.image_loader(os.path.join(root, image_path))
        styles = [img_utils.image_loader(os.path.join(root, p)) for p in style_paths]
        out = self.convert(image, styles, mix, alpha, preserve_color)
        out_dir = os.path.join(root, out_dir)
        os.makedirs(out_dir, exist_ok=True)
        img_utils.imshow(out, path=os.path.join(out_dir, f"converted_{MODEL_NAME}_{name}.png"))
        return out

    def process_video(self, video_path, style_paths, mix=None, alpha=1.0, preserve_color=False,
                      name="nsp", working_dir="workdir/", out_dir="results/", fps=24.0,
                      format="png", quality=90, subsampling="4:2:0", max_frames=90 * 24):
        """Every frame of a clip through encoder -> stx_adain -> decoder; the style statistics
        are computed once.  format "png": frames 0.png, 1.png, ... in working_dir; "mjpeg":
        out_dir/adain_<name>.avi through the GPU JPEG encoder.  Returns the path."""
        from . import video
        if format not in ("png", "mjpeg"):
            raise ValueError(f"format {format!r}: 'png' or 'mjpeg'")
        self.load_latest(name)
        root = constants.PROJECT_ROOT_PATH
        stats = self.style_stats([img_utils.image_loader(os.path.join(root, p))
                                  for p in style_paths])
        src = video_path if isinstance(video_path, np.ndarray) else os.path.join(root, video_path)
        working_dir, out_dir = os.path.join(root, working_dir), os.path.join(root, out_dir)
        os.makedirs(out_dir, exist_ok=True)
        sink = None
        if format == "mjpeg":
            sink = video.MjpegSink(os.path.join(out_dir, f"{MODEL_NAME}_{name}.avi"), fps,
                                   quality, subsampling, self.device)
        else:
            os.makedirs(working_dir, exist_ok=True)
        cond = None
        try:
            for i, frame in enumerate(video.iterate_raw_frames(src, max_frames)):
                if cond is None or (cond.h, cond.w) != tuple(frame.shape[:2]):
                    cond = img_utils.ImageConditioner(constants.IMSIZE, self.device).fixed(
                        *frame.shape[:2])
                cond.load(frame)
                y = self.convert(cond.run(), stats, mix, alpha, preserve_color)
                if sink is not None:
                    sink.write(y)
                else:
                    img_utils.imshow(y[0], path=os.path.join(working_dir, f"{i}.png"))
        finally:
            if sink is not None:
                sink.close()
        return sink.path if sink is not None else working_dir


# ------------------------------------------------------------------------------- training
class AdaINTrainer:
    """One training step of the decoder:

        t = AdaIN(f(c), f(s)) at alpha = 1, sample k on style k;   out = g(t)
        L = content_weight MSE(relu4_1(out), t)
            + style_weight sum_i statsloss(relu{i}_1(out), stats(relu{i}_1(s)))

    Adam on the decoder only, lr_k = lr / (1 + lr_decay k) applied by value per step.  The
    decoder's parameters live in one flat buffer (FlatAdam, one launch), its conv slabs are
    re-prepped in one batch per step (ops.TrainedSlabs), the frozen encoder's once.  Eager:
    no graph capture, one GPU."""

    def __init__(self, net: AdaINNet, style_weight=10.0, content_weight=1.0, lr=1e-4,
                 lr_decay=5e-5):
        from .train import flatten_parameters
        self.net = net
        self.device = net.device
        self.sw, self.cw = float(style_weight), float(content_weight)
        self.lr0, self.lr_decay = float(lr), float(lr_decay)
        self.k = 0  # steps taken
        self.flat, self.flat_grad = flatten_parameters(net.decoder, self.device)
        self.params = list(net.decoder.parameters())
        self.opt = FlatAdam(self.flat, self.flat_grad, lr=self.lr0, params=self.params)
        self.slabs = ops.TrainedSlabs(m for m in net.decoder if isinstance(m, Conv2d))
        self.enc_slabs = ops.TrainedSlabs(net.encoder.convs())
        self.enc_slabs.prep()  # frozen: the slabs (forward and data gradient) stay valid
        self._one = torch.ones((), device=self.device, dtype=torch.float32)
        self._eye = {}

    def lr_at(self, k):
        return self.lr0 / (1.0 + self.lr_decay * k)

    def _mix(self, b):
        if b not in self._eye:
            self._eye[b] = torch.eye(b, device=self.device, dtype=torch.float32).contiguous()
        return self._eye[b]

    def _total(self, content, style):
        enc, dec = self.net.encoder, self.net.decoder
        with torch.no_grad():
            targets = [ops.chan_stats(t, EPS) for t in enc(style)]
            fc = enc(content, last_only=True)
            t = AdaINFn.apply(fc, targets[3][0], targets[3][1], self._mix(fc.shape[0]), 1.0, EPS)
        out = dec(t)
        losses = []

        def tap(i, x):
            x, l = StatsLossFn.apply(x, targets[i][0], targets[i][1], self.sw, EPS)
            losses.append(l)
            return x
        f4 = enc(out, tap_fn=tap, last_only=True)
        total = self.cw * A.MSELossFn.apply(f4, t)
        for l in losses:
            total = total + l
        return total

    def _batches(self, content, style):
        content = content.to(self.device, torch.float32).contiguous()
        style = style.to(self.device, torch.float32).contiguous()
        if content.dim() != 4 or style.dim() != 4 or content.shape[0] != style.shape[0]:
            raise ValueError(f"content {tuple(content.shape)} and style {tuple(style.shape)}: "
                             "[b, 3, h, w] batches of one size expected")
        return content, style

    def step(self, content_batch, style_batch) -> torch.Tensor:
        content, style = self._batches(content_batch, style_batch)
        self.flat_grad.zero_()
        self.slabs.prep()
        ops.ARENA.begin(self.device)
        try:
            total = self._total(content, style)
            total.backward(self._one)
        finally:
            ops.ARENA.end()
        self.opt.lr = self.lr_at(self.k)
        self.opt.step()
        self.k += 1
        return total.detach()

    @torch.no_grad()
    def evaluate(self, content_batch, style_batch) -> torch.Tensor:
        """The loss of the batches without a step."""
        content, style = self._batches(content_batch, style_batch)
        self.slabs.prep()
        return self._total(content, style)


class StyleFolder:
    """Style batches [b, 3, IMSIZE, IMSIZE] from a directory of images: every image once per
    cycle, each cycle shuffled with the seed; endless."""

    def __init__(self, path, batch_size, seed=0, imsize=None):
        self.path = path
        self.names = sorted(f for f in os.listdir(path) if f.lower().endswith(IMAGE_EXTS))
        if not self.names:
            raise FileNotFoundError(f"no style images under {path}")
        self.batch_size, self.imsize = int(batch_size), imsize
        self.rng = random.Random(seed)
        self.queue = []

    def next(self, b=None):
        out = []
        for _ in range(b or self.batch_size):
            if not self.queue:
                self.queue = list(self.names)
                self.rng.shuffle(self.queue)
            out.append(img_utils.image_loader(os.path.join(self.path, self.queue.pop()),
                                              self.imsize))
        return torch.cat(out).contiguous()


class SyntheticStyles:
    """StyleFolder's interface over seeded synthetic images (weights.synthetic_image)."""

    def __init__(self, n, batch_size, seed=0, imsize=None):
        self.n, self.batch_size, self.seed = max(1, int(n)), int(batch_size), seed
        self.size = imsize or constants.IMSIZE
        self.i = 0

    def next(self, b=None):
        b = b or self.batch_size
        out = [W.synthetic_image(self.seed * 100003 + 7919 + (self.i + j) % self.n,
                                 (1, 3, self.size, self.size)) for j in range(b)]
        self.i = (self.i + b) % self.n
        return torch.from_numpy(np.concatenate(out)).to(constants.DEVICE)


def train(net: AdaINNet, styles, name="nsp", epochs=1, loaders=None, style_weight=10.0,
          content_weight=1.0, lr=1e-4, log_every=20):
    """Train the decoder: a checkpoint data/models/adain_{name}_epoch{E}.pth per epoch; an
    epoch whose file exists is loaded and skipped.  styles: StyleFolder / SyntheticStyles;
    loaders: (test, train) content loaders (dataset.get_coco_loader by default)."""
    from . import dataset
    trainer = AdaINTrainer(net, style_weight, content_weight, lr)
    if callable(loaders):
        loaders = loaders(None)
    _, train_loader = loaders or dataset.get_coco_loader(test_split=0.10, test_limit=20,
                                                         batch_size=styles.batch_size)
    it = 0
    for epoch in range(epochs):
        ckpt = net.checkpoint_path(name, epoch)
        if os.path.isfile(ckpt):
            net.load(ckpt)
            continue
        LOGGER.info("Starting epoch %d", epoch)
        for batch in train_loader:
            batch = batch.squeeze(1) if batch.dim() == 5 else batch
            total = trainer.step(batch, styles.next(batch.shape[0]))
            if it % log_every == 0:
                LOGGER.info("Epoch: %d\tBatch Loss: %.4f", epoch, float(total))
            it += 1
        LOGGER.info("Saved %s", net.save(name, epoch))
    return trainer
