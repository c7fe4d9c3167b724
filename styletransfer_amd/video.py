"""video_st per-frame path on libstx (BASELINE.json config 5).

Reference: `VideoTransformNet.process_video` (stransfer/network.py:1071-1158): every
decoded frame is conditioned like an image (`dataset.iterate_on_video_batches`,
stransfer/dataset.py:280-310 -> `img_utils.image_loader_transform`: centre crop,
resize to IMSIZE, ImageNet normalisation), concatenated with the previous stylised
frame along channels (`torch.cat([frame, old], dim=1)`, the first frame with
itself) and run through the 6-channel ImageTransformNet; the output becomes the
next frame's `old`.  `get_temporal_loss` (:885-903) is ||dy|| / (||dx|| + 1).

`gatys_video` is the optimisation-based counterpart (Ruder, Dosovitskiy & Brox 2016):
the fused Gatys iteration per frame, started from the previous result warped along the
optical flow and tied to it by a consistency-masked loss.

`FrameEngine` makes one frame one hipGraph replay: the frame is copied into
channels 0-2 of a static [1, 6, H, W] input whose channels 3-5 hold the previous
output, the ITN forward runs on the HIP kernels, the output is copied back into
channels 3-5, and the temporal-loss norms of the step are reduced on the device
(the reference computes them only in training; here they are the per-frame
"temporal loss" of BASELINE config 5).
"""
from __future__ import annotations

import os
from typing import Iterator

import numpy as np
import torch

from . import color, constants, img_utils, ops

VIDEO_EXTS = (".mp4", ".avi", ".mov", ".mkv", ".gif", ".webm")
FRAME_EXTS = (".png", ".jpg", ".jpeg", ".bmp")


def mjpeg_avi(source):
    """video_io.read_mjpeg_avi(source) if source names an .avi file it accepts (Motion-JPEG:
    read without a codec library), else None (other video files go through imageio)."""
    if not (isinstance(source, str) and source.lower().endswith(".avi")
            and os.path.isfile(source)):
        return None
    from . import video_io
    try:
        return video_io.read_mjpeg_avi(source)
    except ValueError:
        return None


def iterate_raw_frames(source, max_frames=90 * 24) -> Iterator[np.ndarray]:
    """Decoded frames of a video as HxWx3 uint8 arrays (the sources of iterate_frames)."""
    from PIL import Image
    if isinstance(source, np.ndarray):
        frames = iter(source)
    elif isinstance(source, str) and source.endswith(".npy"):
        frames = iter(np.load(source, allow_pickle=False, mmap_mode="r"))
    elif isinstance(source, str) and os.path.isdir(source):
        def key(name):
            stem = os.path.splitext(name)[0]
            digits = "".join(ch for ch in stem if ch.isdigit())
            return (int(digits) if digits else -1, name)
        names = sorted((n for n in os.listdir(source) if n.lower().endswith(FRAME_EXTS)), key=key)
        frames = (np.asarray(Image.open(os.path.join(source, n)).convert("RGB")) for n in names)
    elif mjpeg_avi(source) is not None:
        import io
        frames = (np.asarray(Image.open(io.BytesIO(b)).convert("RGB"))
                  for b in mjpeg_avi(source)[3])
    elif isinstance(source, str) and source.lower().endswith(VIDEO_EXTS):
        try:
            import imageio
        except ImportError as e:
            raise RuntimeError(f"decoding {source} needs imageio (not installed); pass a "
                               "directory of frames or a .npy frame array instead") from e
        reader = imageio.get_reader(source)

        def gen():
            try:
                while True:
                    yield np.asarray(reader.get_next_data())
            except IndexError:
                return
        frames = gen()
    else:
        raise ValueError(f"unsupported video source {source!r}")
    for i, f in enumerate(frames):
        if i >= max_frames:
            break
        f = np.ascontiguousarray(f, dtype=np.uint8)
        if f.ndim == 3 and f.shape[2] == 4:
            f = np.ascontiguousarray(f[:, :, :3])  # RGBA frame: .convert("RGB") drops alpha
        elif f.ndim == 2:
            f = np.repeat(f[:, :, None], 3, axis=2)  # grayscale: PIL "L" -> "RGB" copies
        yield f


def iterate_frames(source, max_frames=90 * 24, imsize=None) -> Iterator[torch.Tensor]:
    """Conditioned frames [1, 3, IMSIZE, IMSIZE] of a video (stransfer/dataset.py:280-310),
    through the host-side PIL transforms (img_utils.image_loader_transform).

    `source`: a video file (decoded with imageio when it is installed, as the
    reference does), a directory of frame images (sorted by the integer in their
    name, then by name), a `.npy` array [T, H, W, 3] uint8 (loaded with
    allow_pickle=False), or an in-memory uint8 array of that shape."""
    from PIL import Image
    for f in iterate_raw_frames(source, max_frames):
        yield img_utils.image_loader_transform(Image.fromarray(f), imsize)


class FrameEngine:
    """One stylised frame = one hipGraph replay of the VideoTransformNet forward.

    raw_hw=(H, W): frames arrive as decoded HxWx3 uint8 (`step_raw`) and the graph
    also holds their conditioning (centre crop, Pillow-exact resize to the engine's
    size, normalisation: img_utils.FixedConditioner) written straight into the
    frame channels of the 6-channel input -- the per-frame path of
    process_video (stransfer/network.py:1117-1131) with no host-side resize.

    preserve_color=True: `out` is the luminance merge of the stylised frame onto the
    input frame (color.merge_luminance: the frame keeps its colours), one launch in the
    place of the output copy.  `prev` still receives the un-merged network output, so
    the recurrence -- every later frame's network input -- is what it is without it."""

    def __init__(self, net, shape, device=None, graph=True, raw_hw=None, preserve_color=False):
        self.net = net
        self.preserve_color = bool(preserve_color)
        self.dev = torch.device(device or constants.DEVICE)
        n, c, h, w = shape
        assert c == 3 and n == 1, shape  # the reference converts one video (batch 1)
        self.x6 = torch.zeros((n, 6, h, w), device=self.dev, dtype=torch.float32)
        self.frame = self.x6[:, :3]
        self.prev = self.x6[:, 3:]
        self.prev_frame = torch.zeros((n, 3, h, w), device=self.dev, dtype=torch.float32)
        self.out = None
        # device scalars: temporal loss (weight 1), ||y_t - y_{t-1}||, ||x_t - x_{t-1}||
        self.scal = torch.zeros(4, device=self.dev, dtype=torch.float32)
        self.graph = None
        self.use_graph = graph
        self.started = False
        self.cond = None
        if raw_hw is not None:
            assert h == w, "frames are conditioned to IMSIZE x IMSIZE"
            self.cond = img_utils.ImageConditioner(h, self.dev).fixed(*raw_hw, out=self.frame)

    def _forward(self):
        if self.cond is not None:
            self.cond.run()                # uint8 frame -> normalised frame channels
        with torch.no_grad():
            y = self.net(self.x6)
        if self.out is None:
            self.out = torch.empty_like(y)
        # temporal-loss terms of this step (stransfer/network.py:885-903): one fused
        # pass, [loss(w=1), ||y - y_prev||, ||x - x_prev||]
        ops.temporal_loss(y, self.prev, self.frame, self.prev_frame, 1.0,
                          out=self.scal[:3])
        if self.preserve_color:
            color.merge_luminance(y, self.frame, out=self.out)
        else:
            self.out.copy_(y)
        self.prev.copy_(y)                 # next step's "old stylised" channels
        self.prev_frame.copy_(self.frame)

    def step(self, frame: torch.Tensor) -> torch.Tensor:
        """Stylise one conditioned frame [n, 3, H, W]; returns the (static) output."""
        if self.cond is not None:
            raise RuntimeError("FrameEngine(raw_hw=...) takes uint8 frames: use step_raw")
        self.frame.copy_(frame)
        if not self.started:
            self.prev.copy_(frame)         # first frame: old = the frame itself
            self.prev_frame.copy_(frame)
            self.started = True
        return self._run()

    def step_raw(self, frame_u8) -> torch.Tensor:
        """Stylise one decoded HxWx3 uint8 frame (host array or device tensor)."""
        if self.cond is None:
            raise RuntimeError("FrameEngine without raw_hw takes conditioned frames: use step")
        self.cond.load(frame_u8)
        if not self.started:
            self.cond.run()                # first frame: old = the frame itself
            self.prev.copy_(self.frame)
            self.prev_frame.copy_(self.frame)
            self.started = True
        return self._run()

    def _run(self):
        if self.graph is not None:
            self.graph.replay()
        elif self.use_graph and self.out is not None:
            # the first frame ran eagerly (allocations, prepped-weight caches); capture
            # records without executing, then replay runs this frame
            self.graph = torch.cuda.CUDAGraph()
            with ops.graph_capture(self.graph):
                self._forward()
            self.graph.replay()
        else:
            self._forward()
        return self.out

    def temporal_loss(self, temporal_weight=1.0) -> float:
        """||y_t - y_{t-1}|| / (||x_t - x_{t-1}|| + 1) * w of the last step."""
        return float(self.scal[0]) * temporal_weight


class MjpegSink:
    """Stylised frames [1, 3, h, w] (normalised fp32, on the GPU) -> an MJPEG AVI file: the
    JPEG encoder's fp32 front end reads the frame where it lies, the int16 coefficients cross
    to the host and are Huffman-coded on the encoder's background thread while the GPU works
    on the next frame; no fp32 copy to the host, no PNG."""

    def __init__(self, path, fps=24.0, quality=90, subsampling="4:2:0", device=None):
        from . import jpeg
        if subsampling not in jpeg.SAMPLINGS:
            raise ValueError(f"subsampling {subsampling!r}: 4:4:4, 4:2:2 or 4:2:0")
        self.path, self.fps = path, fps
        self.quality, self.subsampling = int(quality), subsampling
        self.enc = jpeg.JpegBatchEncoder(device)
        self.writer = None
        self.inflight = 0
        self.frames = 0

    def _drain(self, keep):
        while self.inflight > keep:
            for data in self.enc.collect():
                self.writer.write(data)
            self.inflight -= 1

    def write(self, y: torch.Tensor):
        if self.writer is None:
            from . import video_io
            self.writer = video_io.MjpegAviWriter(self.path, self.fps, y.shape[-2], y.shape[-1])
        # (the encoder has read y when submit returns control of the stream: the kernels are
        # enqueued before the engine's next replay overwrites the static output)
        self.enc.submit([y], self.quality, self.subsampling)
        self.inflight += 1
        self.frames += 1
        self._drain(1)

    def close(self):
        try:
            if self.writer is not None:
                self._drain(0)
        finally:
            self.enc.close()
            if self.writer is not None:
                self.writer.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def iterate_device_frames(source, device=None, max_frames=90 * 24):
    """The frames of an MJPEG .avi as uint8 [h, w, 3] DEVICE tensors: Huffman-decoded on the
    host, the pixel stages on the GPU (jpeg.JpegBatchDecoder: Pillow's pixels); a frame the
    host decoder does not take is decoded by PIL and rides along as raw pixels."""
    from . import jpeg
    avi = mjpeg_avi(source)
    if avi is None:
        raise ValueError(f"{source!r}: not a Motion-JPEG .avi file")
    dec = jpeg.JpegBatchDecoder(device)
    for i, data in enumerate(avi[3]):
        if i >= max_frames:
            break
        rgb, shapes = dec.decode([data])
        yield rgb.view(shapes[0][0], shapes[0][1], 3)


def process_video(net, video_path, style_name="nsp", working_dir="workdir/", out_dir="results/",
                  fps=24.0, graph=True, max_frames=90 * 24, preserve_color=False,
                  format="png", quality=90, subsampling="4:2:0") -> str:
    """VideoTransformNet.process_video (stransfer/network.py:1071-1158) on FrameEngine.
    preserve_color: every written frame keeps its input frame's colours.

    format "png" (the default): frames 0.png, 1.png, ... in working_dir, muxed to an .mp4 when
    imageio is installed.  format "mjpeg": the frames go from the engine's output through the
    GPU JPEG encoder (quality, subsampling) into out_dir/video_st_<style>.avi (MjpegSink); no
    PNG, no frames in working_dir; returns that path.  A Motion-JPEG .avi as video_path is
    read without imageio, and decoded on the GPU when the engine runs on one."""
    if format not in ("png", "mjpeg"):
        raise ValueError(f"format {format!r}: 'png' or 'mjpeg'")
    mjpeg = format == "mjpeg"
    working_dir = os.path.join(constants.PROJECT_ROOT_PATH, working_dir)
    out_dir = os.path.join(constants.PROJECT_ROOT_PATH, out_dir)
    if not mjpeg:
        import shutil
        shutil.rmtree(working_dir, ignore_errors=True)
        os.makedirs(working_dir, exist_ok=True)
    os.makedirs(out_dir, exist_ok=True)
    eng = None
    S = constants.IMSIZE
    sink = None
    if mjpeg:
        sink = MjpegSink(os.path.join(out_dir, f"video_st_{style_name}.avi"), fps, quality,
                         subsampling, constants.DEVICE)
    if mjpeg_avi(video_path) is not None and torch.device(constants.DEVICE).type == "cuda":
        frames = iterate_device_frames(video_path, constants.DEVICE, max_frames)
    else:
        frames = iterate_raw_frames(video_path, max_frames)
    try:
        for i, frame in enumerate(frames):
            # decoded uint8 frames go to the GPU as they are; crop, resize and normalisation
            # run inside the per-frame graph (bit-identical to image_loader_transform)
            if eng is None or eng.cond.h != frame.shape[0] or eng.cond.w != frame.shape[1]:
                if eng is not None:  # a clip whose frame size changes: a new engine, as the
                    prev = eng.prev.clone()  # reference, but keep the recurrence going
                eng2 = FrameEngine(net, (1, 3, S, S), constants.DEVICE, graph=graph,
                                   raw_hw=tuple(frame.shape[:2]), preserve_color=preserve_color)
                if eng is not None:
                    eng2.prev.copy_(prev)
                    eng2.prev_frame.copy_(eng.prev_frame)
                    eng2.started = True
                eng = eng2
            y = eng.step_raw(frame)
            if mjpeg:
                sink.write(y)
            else:
                img_utils.imshow(y[0], path=os.path.join(working_dir, f"{i}.png"))
    finally:
        if sink is not None:
            sink.close()
    if mjpeg:
        return sink.path
    final = os.path.join(out_dir, f"video_st_{style_name}.mp4")
    try:
        import imageio
    except ImportError:
        return working_dir  # frames only: no encoder in this image
    from PIL import Image
    writer = imageio.get_writer(final, fps=fps)
    names = sorted(os.listdir(working_dir), key=lambda x: int(x.split(".")[0]))
    for nm in names:
        writer.append_data(np.array(Image.open(os.path.join(working_dir, nm))))
    writer.close()
    return final


# --------------------------------------------------- temporally consistent Gatys video
DEFAULT_TEMPORAL_WEIGHT = 200.0  # Ruder et al.: temporal 200 to content 1


MAX_LONG_TERM, MAX_OFFSET = 4, 16  # offsets of one long-term loss, and the farthest of them


def check_offsets(offsets):
    """The offsets of a long-term loss as a tuple of ints; ValueError names the rule broken."""
    try:
        ks = tuple(int(k) for k in offsets)
        if any(k != o for k, o in zip(ks, offsets)):
            raise TypeError
    except TypeError:
        raise ValueError(f"long-term offsets {offsets!r}: a sequence of integers expected") \
            from None
    if not 1 <= len(ks) <= MAX_LONG_TERM:
        raise ValueError(f"long-term offsets {ks}: 1 to {MAX_LONG_TERM} entries expected")
    if ks[0] != 1:
        raise ValueError(f"long-term offsets {ks}: the first must be 1 (the previous frame)")
    if any(b <= a for a, b in zip(ks, ks[1:])):
        raise ValueError(f"long-term offsets {ks}: strictly increasing expected")
    if ks[-1] > MAX_OFFSET:
        raise ValueError(f"long-term offsets {ks}: each at most {MAX_OFFSET}")
    return ks


def _flow_keys(k):
    return ("forward", "backward") if k == 1 else (f"forward_{k}", f"backward_{k}")


def _flow_array(z, path, key, k, n_frames, size):
    """z[key] checked as the flows of offset k of a clip of n_frames frames."""
    a = z[key]
    if a.dtype != np.float32:
        raise ValueError(f"{path}: '{key}' is {a.dtype}, float32 expected")
    if a.ndim != 4 or a.shape[1:] != (2, size, size):
        raise ValueError(f"{path}: '{key}' has shape {a.shape}, expected "
                         f"[T-{k}, 2, {size}, {size}] (flows at the working resolution)")
    if a.shape[0] != max(n_frames - k, 0):
        raise ValueError(f"{path}: '{key}' holds {a.shape[0]} flows, the clip's "
                         f"{n_frames} frames need {max(n_frames - k, 0)}")
    bad = int(a.size - np.isfinite(a).sum())
    if bad:
        raise ValueError(f"{path}: '{key}' holds {bad} non-finite values "
                         f"({bad / a.size:.2%} of it)")
    return np.ascontiguousarray(a)


def load_flows(path, n_frames, size):
    """(forward, backward) of an .npz: float32 arrays [n_frames - 1, 2, size, size] at the
    working resolution -- the flows between the conditioned frames (after centre crop and
    resize), channel 0 the column displacement, channel 1 the row displacement, in pixels.
    forward[t-1] maps frame t-1 onto frame t, backward[t-1] frame t onto frame t-1.
    ValueError names what is wrong with a file that does not fit."""
    with np.load(path, allow_pickle=False) as z:
        out = []
        for key in ("forward", "backward"):
            if key not in z.files:
                raise ValueError(f"{path}: no '{key}' array (found {sorted(z.files)})")
            out.append(_flow_array(z, path, key, 1, n_frames, size))
    return out[0], out[1]


def load_long_flows(path, n_frames, size, offsets):
    """{k: (forward_k, backward_k)} of an .npz for the offsets of a long-term loss: key 1 is
    load_flows' pair, key k > 1 the arrays 'forward_k' and 'backward_k', float32
    [n_frames - k, 2, size, size]: forward_k[t-k] maps frame t-k onto frame t, backward_k[t-k]
    frame t onto frame t-k.  ValueError names what is wrong with a file that does not fit."""
    out = {}
    with np.load(path, allow_pickle=False) as z:
        for k in check_offsets(offsets):
            pair = []
            for key in _flow_keys(k):
                if key not in z.files:
                    hint = "" if k == 1 else (f" for offset {k}: `--flow auto --save-flows` with "
                                              "these --long-term offsets writes it")
                    raise ValueError(f"{path}: no '{key}' array{hint} (found {sorted(z.files)})")
                pair.append(_flow_array(z, path, key, k, n_frames, size))
            out[k] = tuple(pair)
    return out


def save_flows(path, forward, backward, longer=None):
    """Write the .npz that load_flows reads: float32 'forward' and 'backward', each
    [T-1, 2, S, S].  longer: {k: (forward_k, backward_k)}, k > 1, each [T-k, 2, S, S], written
    as 'forward_k' and 'backward_k' (load_long_flows reads them)."""
    arrays = {}
    for k, (fk, bk) in sorted({1: (forward, backward), **(longer or {})}.items()):
        f, b = (np.ascontiguousarray(a, dtype=np.float32) for a in (fk, bk))
        if f.shape != b.shape or f.ndim != 4 or f.shape[1] != 2:
            raise ValueError(f"flows [T-{k}, 2, h, w] of one shape expected (got {f.shape}, "
                             f"{b.shape})")
        if longer and (int(k) != k or not 1 <= k <= MAX_OFFSET):
            raise ValueError(f"offset {k!r}: an integer in 1..{MAX_OFFSET} expected")
        arrays.update(zip(_flow_keys(int(k)), (f, b)))
    with open(path, "wb") as fh:  # (a file object: numpy appends no second .npz to the name)
        np.savez(fh, **arrays)


class FlowEstimator:
    """Dense optical flow between two conditioned frames on the GPU: coarse-to-fine
    Horn-Schunck with warping, relaxed by Jacobi iterations (include/stx.h).

    pair(prev, cur) -> (fwd, bwd), static [1, 2, h, w] tensors in this project's conventions
    (channel 0 = dx, 1 = dy, in pixels; bwd maps cur onto prev): both directions run as one
    batch of two.  Every level's buffers and the resample tables are made here; pair
    allocates nothing, synchronises nothing and can be captured (ops.graph_capture).  The
    estimator holds no graph: whoever captures pair owns the graph.

    pairs=P: buffers for P frame pairs, batch 2 P.  pairs_flow([(a_0, b_0), ...]) takes 1..P
    pairs and estimates them all in one sequence of launches (every kernel takes a batch;
    samples are independent, so a pair's flows are pair(a_q, b_q)'s bit for bit); a shorter
    list uses the leading part of the batch.  It returns static views [(fwd_q, bwd_q)]."""

    def __init__(self, h, w, device=None, alpha=15.0, warps=5, iters=40, min_side=16,
                 mean=None, std=None, pairs=1):
        if warps < 1 or iters < 1:
            raise ValueError(f"warps {warps}, iters {iters}: at least 1 each")
        if pairs < 1:
            raise ValueError(f"pairs {pairs}: at least 1")
        self.dev = torch.device(device or constants.DEVICE)
        self.alpha, self.warps, self.iters = float(alpha), int(warps), int(iters)
        self.mean, self.std = mean, std
        self.pairs = int(pairs)
        self.levels = ops.flow_pyramid(h, w, min_side)
        z = lambda *s: torch.zeros(s, device=self.dev, dtype=torch.float32)
        nb = 2 * self.pairs
        # per level: luma [A | B], pair q in samples 2q, 2q+1 = [(prev, cur) | (cur, prev)],
        # two flow buffers, coefficients
        self.grey = [z(2, nb, hl, wl) for hl, wl in self.levels]
        self.uv = [(z(nb, 2, hl, wl), z(nb, 2, hl, wl)) for hl, wl in self.levels]
        self.coef = [z(nb, 3, hl, wl) for hl, wl in self.levels]
        # level 0 starts in the buffer from which `warps` swaps end in uv[0][0]
        self.flow = self.uv[0][0]
        self.views = [(self.flow[2 * q:2 * q + 1], self.flow[2 * q + 1:2 * q + 2])
                      for q in range(self.pairs)]
        self.fwd, self.bwd = self.views[0]
        blank = z(1, 3, h, w)
        self.pairs_flow([(blank, blank)] * self.pairs)  # uploads the tables, sizes the scratch
        torch.cuda.synchronize(self.dev)

    def pair(self, prev, cur):
        return self.pairs_flow([(prev, cur)])[0]

    def pairs_flow(self, pairs):
        m = len(pairs)
        if not 1 <= m <= self.pairs:
            raise ValueError(f"pairs_flow: {m} pairs, this estimator takes 1..{self.pairs}")
        nb, whole = 2 * m, m == self.pairs
        g0 = self.grey[0]
        for q, (prev, cur) in enumerate(pairs):
            for img, a_slot, b_slot in ((prev, 2 * q, 2 * q + 1), (cur, 2 * q + 1, 2 * q)):
                ops.flow_luma(img, self.mean, self.std, out=g0[0, a_slot:a_slot + 1])
                ops.flow_luma(img, self.mean, self.std, out=g0[1, b_slot:b_slot + 1])
        for l in range(1, len(self.levels)):
            if whole:
                ops.resample2d(self.grey[l - 1], self.levels[l], "triangle", out=self.grey[l])
            else:  # the leading samples of A and of B are two contiguous runs
                for s in (0, 1):
                    ops.resample2d(self.grey[l - 1][s, :nb], self.levels[l], "triangle",
                                   out=self.grey[l][s, :nb])
        top = len(self.levels) - 1
        for l in range(top, -1, -1):
            hl, wl = self.levels[l]
            # `warps` swaps must end in buffer 0 (level 0: the static output)
            src = self.warps % 2
            uv = [u[:nb] for u in self.uv[l]]
            coef, a, b = self.coef[l][:nb], self.grey[l][0, :nb], self.grey[l][1, :nb]
            if l == top:
                uv[src].zero_()
            else:
                hc, wc = self.levels[l + 1]
                ops.resample2d(self.uv[l + 1][0][:nb], (hl, wl), "triangle", out=uv[src])
                ops.flow_scale(uv[src], np.float32(wl) / np.float32(wc),
                               np.float32(hl) / np.float32(hc))
            for _ in range(self.warps):
                ops.flow_linearize(a, b, uv[src], out=coef)
                ops.flow_jacobi(coef, uv[src], out=uv[src ^ 1], alpha=self.alpha,
                                iters=self.iters)
                src ^= 1
        return self.views[:m]


def estimate_flows(frames, device=None, offsets=(1,), **params):
    """(forward, backward) of a clip's conditioned frames [1, 3, S, S]: float32 arrays
    [T-1, 2, S, S], what load_flows returns (FlowEstimator; params: its keywords).
    offsets other than (1,): {k: (forward_k, backward_k)}, each [T-k, 2, S, S], what
    load_long_flows returns -- per frame one pairs_flow call over its offsets, the flows
    that gatys_video(..., "auto", long_term=offsets) estimates."""
    dev = torch.device(device or constants.DEVICE)
    offsets = check_offsets(offsets)
    est, past = None, []  # past: the last max(offsets) frames, nearest first
    found = {k: ([], []) for k in offsets}
    for frame in frames:
        frame = frame.to(dev, torch.float32).contiguous()
        if est is None:
            est = FlowEstimator(frame.shape[-2], frame.shape[-1], dev, pairs=len(offsets),
                                **params)
        ks = [k for k in offsets if k <= len(past)]
        if ks:
            for k, (f, b) in zip(ks, est.pairs_flow([(past[k - 1], frame) for k in ks])):
                found[k][0].append(f[0].cpu().numpy())
                found[k][1].append(b[0].cpu().numpy())
        past = [frame] + past[:offsets[-1] - 1]
    if est is None:
        raise ValueError("estimate_flows: no frames")
    shape = (0, 2) + tuple(past[0].shape[-2:])
    stack = lambda a: np.stack(a) if a else np.zeros(shape, np.float32)
    out = {k: (stack(f), stack(b)) for k, (f, b) in found.items()}
    return out[1] if offsets == (1,) else out


def _gatys_video_long(feat, frames, flows, steps, first_steps, temporal_weight, optimizer,
                      offsets, kw, lr):
    """gatys_video with the long-term loss over `offsets` (see there)."""
    from . import vgg as V
    dev = feat.device
    static, auto = flows == "static", flows == "auto"
    if not (static or auto):
        if not isinstance(flows, dict):  # (forward, backward): the offset-1 flows
            flows = {1: tuple(flows)}
        missing = [k for k in offsets if k not in flows]
        if missing:
            raise ValueError(f"long_term {offsets}: no flows given for offsets {missing}")
    K = offsets[-1]
    est = eng = results = seen = omega = init = cmask = zero = which = None
    for t, frame in enumerate(frames):
        frame = frame.to(dev, torch.float32).contiguous()
        if t == 0:
            n, _, h, w = frame.shape
            # rings of the last K results (for auto also of the frames): frame t in slot t % K
            results = [torch.empty_like(frame) for _ in range(K)]
            seen = [torch.empty_like(frame) for _ in range(K)] if auto else None
            omega, init = torch.empty_like(frame), torch.empty_like(frame)
            cmask = torch.zeros((n, h, w), device=dev, dtype=torch.float32)
            zero = torch.zeros((n, 2, h, w), device=dev, dtype=torch.float32)
            which = torch.empty((n, h, w), device=dev, dtype=torch.uint8)
            omega.copy_(frame)  # frame 0: an all-zero mask, the term is exactly 0
            if optimizer == "adam":
                eng = V.GatysEngine(feat, None, frame, lr=lr,
                                    temporal=(omega, cmask, temporal_weight), **kw)
            else:
                eng = V.GatysLBFGS(feat, None, frame, **kw)
            eng.run(first_steps)
        else:
            ks = [k for k in offsets if t - k >= 0]
            if static:
                pairs = [(zero, zero)] * len(ks)
            elif auto:
                if est is None:
                    est = FlowEstimator(h, w, dev, pairs=len(offsets))
                pairs = est.pairs_flow([(seen[(t - k) % K], frame) for k in ks])
            else:
                pairs = []
                for k in ks:
                    if t - k >= len(flows[k][0]):
                        raise ValueError(f"frame {t}: only {len(flows[k][0])} flows of offset "
                                         f"{k} given")
                    pairs.append(tuple(torch.as_tensor(f[t - k]).to(dev, torch.float32)
                                       .reshape(zero.shape).contiguous() for f in flows[k]))
            ops.flow_compose([results[(t - k) % K] for k in ks], [f for f, _ in pairs],
                             [b for _, b in pairs], frame, ref=omega, cmask=cmask, init=init,
                             which=which)
            if optimizer == "adam":
                eng.retarget(frame, init=init, temporal_ref=omega, temporal_mask=cmask)
                if eng.graph is None:
                    eng.run(steps)
                else:
                    for _ in range(steps):
                        eng.graph.replay()
            else:
                eng = V.GatysLBFGS(feat, None, frame, init=init,
                                   temporal=(omega, cmask, temporal_weight), **kw)
                eng.run(steps)
        results[t % K].copy_(eng.x.detach())
        if auto:
            seen[t % K].copy_(frame)
        yield results[t % K].clone()


def gatys_video(feat, frames, style_image, flows, steps, first_steps=None,
                temporal_weight=DEFAULT_TEMPORAL_WEIGHT, optimizer="adam", style_weight=100_000,
                content_weight=1, style_layer_weights=None, lr=1e-3,
                long_term=None) -> Iterator[torch.Tensor]:
    """Stylised frames [1, 3, h, w] of a clip, one Gatys optimisation per frame (Ruder,
    Dosovitskiy & Brox 2016, short-term consistency).  frames: conditioned frames, as
    iterate_frames yields them; flows: "static" (a fixed camera: zero flow both ways), "auto"
    (FlowEstimator.pair(frame t-1, frame t) before each frame t >= 1: the flows that
    estimate_flows returns, bit for bit) or (forward, backward), each [T-1, 2, h, w]
    (load_flows).  Frame 0 runs first_steps
    (default steps) from the content frame.  Frame t >= 1 starts from the previous result
    warped along backward[t-1] (the frame itself where the warp leaves the image) and adds

        temporal_weight / (3 h w) * sum c (x - warp)^2,   c = ops.flow_consistency,

    to the Gatys loss.  optimizer "adam": one engine, captured once and moved from frame to
    frame (GatysEngine.retarget), steps = iterations; "lbfgs": a GatysLBFGS per frame,
    steps = outer steps.

    long_term: None, or offsets such as (1, 2, 4) (strictly increasing from 1, at most 4, each
    <= 16; check_offsets): Ruder et al.'s long-term loss (eq. 9, 10).  Frame t is tied to
    the results t-k, each farther one only where every nearer one is inconsistent.  With 0/1
    masks and one weight that sum is the same masked loss on a composed reference and mask,
    which one ops.flow_compose per frame builds over the offsets with t - k >= 0 (DESIGN.md
    3.9): the engine, its graph and retarget are the short-term ones.  flows is then "static",
    "auto" (one FlowEstimator.pairs_flow per frame over (frame t-k, frame t)) or a dict
    {k: (forward_k, backward_k)} (load_long_flows): forward_k[t-k] maps frame t-k onto t."""
    from . import vgg as V
    if long_term is not None:
        long_term = check_offsets(long_term)
    if optimizer not in ("adam", "lbfgs"):
        raise ValueError(f"optimizer {optimizer!r}: 'adam' or 'lbfgs'")
    dev = feat.device
    if isinstance(flows, str) and flows not in ("static", "auto"):
        raise ValueError(f"flows {flows!r}: 'static', 'auto' or (forward, backward)")
    static, auto = flows == "static", flows == "auto"
    est = last = None
    first_steps = steps if first_steps is None else first_steps
    targets = feat.style_targets(style_image.to(dev, torch.float32))
    kw = dict(style_weight=style_weight, content_weight=content_weight, targets=targets,
              style_layer_weights=style_layer_weights)
    if long_term is not None:
        yield from _gatys_video_long(feat, frames, flows, steps, first_steps, temporal_weight,
                                     optimizer, long_term, kw, lr)
        return
    eng = prev = omega = init = cmask = zero = None
    for t, frame in enumerate(frames):
        frame = frame.to(dev, torch.float32).contiguous()
        if t == 0:
            n, _, h, w = frame.shape
            prev, omega, init = (torch.empty_like(frame) for _ in range(3))
            cmask = torch.zeros((n, h, w), device=dev, dtype=torch.float32)
            zero = torch.zeros((n, 2, h, w), device=dev, dtype=torch.float32)
            omega.copy_(frame)  # frame 0: an all-zero mask, the term is exactly 0
            if optimizer == "adam":
                eng = V.GatysEngine(feat, None, frame, lr=lr,
                                    temporal=(omega, cmask, temporal_weight), **kw)
                eng.run(first_steps)
            else:
                eng = V.GatysLBFGS(feat, None, frame, **kw)
                eng.run(first_steps)
        else:
            if static:
                fwd = bwd = zero
            elif auto:
                # launched eagerly: the host is a frame's iterations ahead of the device, and
                # a replayed capture of the estimator measured slower here
                if est is None:
                    est = FlowEstimator(h, w, dev)
                fwd, bwd = est.pair(last, frame)
            else:
                if t - 1 >= len(flows[0]):
                    raise ValueError(f"frame {t}: only {len(flows[0])} flows given")
                fwd, bwd = (torch.as_tensor(f[t - 1]).to(dev, torch.float32)
                            .reshape(zero.shape).contiguous() for f in flows)
            ops.flow_consistency(fwd, bwd, out=cmask)
            ops.flow_warp(prev, bwd, out=omega)
            ops.flow_warp(prev, bwd, fill=frame, out=init)
            if optimizer == "adam":
                eng.retarget(frame, init=init, temporal_ref=omega, temporal_mask=cmask)
                if eng.graph is None:
                    eng.run(steps)
                else:
                    for _ in range(steps):
                        eng.graph.replay()
            else:
                eng = V.GatysLBFGS(feat, None, frame, init=init,
                                   temporal=(omega, cmask, temporal_weight), **kw)
                eng.run(steps)
        prev.copy_(eng.x.detach())
        if auto:
            if last is None:
                last = torch.empty_like(frame)
            last.copy_(frame)
        yield prev.clone()
