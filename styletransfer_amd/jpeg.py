"""JPEG decode split between host and GPU (csrc/jpeg_host.cpp, csrc/jpeg.hip).

The host parses the markers and Huffman-decodes the scan into quantised DCT coefficients
(`entropy_decode`, no GPU needed: loader workers run it); the GPU dequantises, runs
libjpeg's integer IDCT, upsamples the chroma and converts to RGB (`JpegBatchDecoder`), into
the packed HxWx3 uint8 layout `img_utils.ImageConditioner` reads.  The pixels equal
Pillow's bit for bit.  A file the host decoder reports as unsupported (progressive, CMYK,
..., not a JPEG at all) or corrupt is decoded with PIL and rides along as raw pixels.

A batch crosses from a worker to the training process as ONE uint8 tensor (`pack`):

    int64 [1 + B * REC]   B, then per image a record of REC int64s (see _REC_FIELDS)
    payloads, 16-byte aligned:
        coefficients: int16 blocks (component after component, block raster over the
                      MCU-padded grid, natural order) then ncomp uint16[64] tables
        raw:          h * w * 3 pixels

The encode is the mirror (`JpegBatchEncoder`, `encode_image`): the GPU converts to YCbCr,
downsamples, runs libjpeg's integer forward DCT and quantises; the int16 coefficients cross
to the host through pinned memory and `entropy_encode` Huffman-codes them into a baseline
JFIF file -- Pillow's bytes (optimize=False) for the same pixels, quality and subsampling.
"""
from __future__ import annotations

import ctypes as C
import os
import queue
import threading

import numpy as np
import torch

from . import _native as N

OK, UNSUPPORTED, CORRUPT, BAD_ARGS = range(4)
STATUS_NAMES = {OK: "ok", UNSUPPORTED: "unsupported", CORRUPT: "corrupt", BAD_ARGS: "bad arguments"}

# per-image record of a packed batch (int64 each)
_REC_FIELDS = ("raw", "h", "w", "ncomp", "hmax", "vmax", "bw0", "bw1", "bw2", "bh0", "bh1", "bh2",
               "offset", "coef_bytes")
REC = len(_REC_FIELDS)


class JpegError(ValueError):
    """`entropy_decode` of a stream this decoder does not take; .status says which."""

    def __init__(self, status):
        super().__init__(f"JPEG entropy decode: {STATUS_NAMES.get(status, status)}")
        self.status = status


class JpegInfo:
    """What `info` reports: status and, when OK, the frame geometry."""

    def __init__(self, d: N.JpegDesc):
        self.status = int(d.status)
        self.h, self.w, self.ncomp = int(d.h), int(d.w), int(d.ncomp)
        n = self.ncomp if self.status == OK else 0
        self.sampling = [(int(d.hs[c]), int(d.vs[c])) for c in range(n)]   # (h, v) per component
        self.blocks = [(int(d.bw[c]), int(d.bh[c])) for c in range(n)]     # padded (bw, bh)
        self.restart_interval = int(d.restart_interval)
        self.coef_bytes = int(d.coef_bytes)

    @property
    def ok(self):
        return self.status == OK

    def __repr__(self):
        return (f"JpegInfo({STATUS_NAMES.get(self.status)}, {self.h}x{self.w}x{self.ncomp}, "
                f"sampling={self.sampling}, blocks={self.blocks})")


class JpegCoefs:
    """One entropy-decoded image: `coef` int16 (all components' blocks, natural order),
    `qtab` uint16 [ncomp, 64], and the geometry the device stage needs."""

    def __init__(self, inf: JpegInfo, coef: np.ndarray, qtab: np.ndarray):
        self.h, self.w, self.ncomp = inf.h, inf.w, inf.ncomp
        self.sampling, self.blocks = inf.sampling, inf.blocks
        self.coef, self.qtab = coef, qtab

    def component(self, c: int) -> np.ndarray:
        """Component c's coefficients as [bh, bw, 8, 8]."""
        o = sum(bw * bh * 64 for bw, bh in self.blocks[:c])
        bw, bh = self.blocks[c]
        return self.coef[o:o + bw * bh * 64].reshape(bh, bw, 8, 8)


def _buf(data):
    if isinstance(data, (bytes, bytearray, memoryview)):
        a = np.frombuffer(data, np.uint8)
    else:
        a = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    return a, a.ctypes.data if a.size else None


def info(data) -> JpegInfo:
    """Walk the markers of JPEG bytes: geometry and whether this decoder takes the file."""
    a, p = _buf(data)
    d = N.JpegDesc()
    N.lib().stx_jpeg_info(p, a.size, C.byref(d))
    return JpegInfo(d)


def try_entropy_decode(data):
    """(status, JpegCoefs or None): the loader's form, no exception for a fallback file."""
    a, p = _buf(data)
    L = N.lib()
    d = N.JpegDesc()
    st = L.stx_jpeg_info(p, a.size, C.byref(d))
    if st != OK:
        return st, None
    inf = JpegInfo(d)
    coef = np.empty(inf.coef_bytes // 2, np.int16)
    qtab = np.empty((inf.ncomp, 64), np.uint16)
    st = L.stx_jpeg_entropy_decode(p, a.size, coef.ctypes.data, coef.nbytes, qtab.ctypes.data)
    if st != OK:
        return st, None
    return OK, JpegCoefs(inf, coef, qtab)


def entropy_decode(data) -> JpegCoefs:
    """Huffman-decode JPEG bytes on the CPU; raises JpegError (unsupported / corrupt)."""
    st, co = try_entropy_decode(data)
    if st != OK:
        raise JpegError(st)
    return co


def _pil_rgb(src) -> np.ndarray:
    import io

    from PIL import Image
    img = Image.open(io.BytesIO(bytes(src)) if not isinstance(src, (str, os.PathLike)) else src)
    if img.mode != "RGB":
        img = img.convert("RGB")
    return np.asarray(img, dtype=np.uint8)


def load_item(src):
    """A file path or encoded bytes -> JpegCoefs, or (fallback) the PIL-decoded HxWx3 array."""
    if isinstance(src, (str, os.PathLike)):
        with open(src, "rb") as f:
            src = f.read()
    st, co = try_entropy_decode(src)
    return co if st == OK else _pil_rgb(src)


def _align16(n):
    return (n + 15) & ~15


def pack(items) -> torch.Tensor:
    """JpegCoefs / HxWx3 uint8 arrays -> one uint8 tensor (layout in the module docstring)."""
    B = len(items)
    head = _align16(8 * (1 + B * REC))
    recs = np.zeros((B, REC), np.int64)
    off = head
    for i, it in enumerate(items):
        if isinstance(it, JpegCoefs):
            (hmax, vmax) = it.sampling[0]
            bws = [b[0] for b in it.blocks] + [0, 0]
            bhs = [b[1] for b in it.blocks] + [0, 0]
            recs[i] = (0, it.h, it.w, it.ncomp, hmax, vmax, *bws[:3], *bhs[:3], off,
                       it.coef.nbytes)
            off = _align16(off + it.coef.nbytes + it.qtab.nbytes)
        else:
            a = np.asarray(it)
            if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8:
                raise ValueError(f"item {i}: JpegCoefs or an HxWx3 uint8 array expected")
            recs[i, :3] = (1, a.shape[0], a.shape[1])
            recs[i, 12] = off
            off = _align16(off + a.nbytes)
    packed = torch.empty(off, dtype=torch.uint8)
    pk = packed.numpy()
    hv = pk[:8 * (1 + B * REC)].view(np.int64)
    hv[0] = B
    hv[1:] = recs.reshape(-1)
    for it, r in zip(items, recs):
        o = int(r[12])
        if isinstance(it, JpegCoefs):
            n = it.coef.nbytes
            pk[o:o + n] = it.coef.view(np.uint8)
            pk[o + n:o + n + it.qtab.nbytes] = it.qtab.reshape(-1).view(np.uint8)
        else:
            a = np.ascontiguousarray(it)
            pk[o:o + a.nbytes] = a.reshape(-1)
    return packed


def records(packed: torch.Tensor) -> np.ndarray:
    """The int64 [B, REC] records of a packed HOST batch, checked against its size."""
    pk = packed.numpy()
    if pk.size < 8:
        raise ValueError("packed JPEG batch: no header")
    B = int(pk[:8].view(np.int64)[0])
    if B < 0 or 8 * (1 + B * REC) > pk.size:
        raise ValueError("packed JPEG batch: bad image count")
    recs = pk[8:8 * (1 + B * REC)].view(np.int64).reshape(B, REC).copy()
    for r in recs:
        raw, h, w, ncomp = (int(v) for v in r[:4])
        if not (1 <= h <= 65535 and 1 <= w <= 65535):
            raise ValueError("packed JPEG batch: bad image size")
        if raw:
            need = h * w * 3
        else:
            if ncomp not in (1, 3):
                raise ValueError("packed JPEG batch: bad component count")
            need = sum(int(r[6 + c]) * int(r[9 + c]) for c in range(ncomp)) * 128
            if need != int(r[13]):
                raise ValueError("packed JPEG batch: coefficient bytes do not match the grid")
            need += ncomp * 128
        if r[12] < 0 or r[12] % 16 or int(r[12]) + need > pk.size:
            raise ValueError("packed JPEG batch: payload out of range")
    return recs


def plan(recs: np.ndarray):
    """Records -> (stx_jpeg_job array, shapes [(h, w)], rgb bytes, workspace bytes): images
    one after another in the rgb buffer (the order ImageConditioner._plan assumes)."""
    B = len(recs)
    jobs = (N.JpegJob * max(B, 1))()
    shapes, rgb_off, tmp_off = [], 0, 0
    for i, r in enumerate(recs):
        raw, h, w, ncomp, hmax, vmax = (int(v) for v in r[:6])
        j = jobs[i]
        j.rgb_offset, j.coef_offset, j.h, j.w, j.raw = rgb_off, int(r[12]), h, w, raw
        if not raw:
            j.qtab_offset = int(r[12]) + int(r[13])
            j.tmp_offset, j.ncomp, j.hmax, j.vmax = tmp_off, ncomp, hmax, vmax
            for c in range(ncomp):
                j.bw[c], j.bh[c] = int(r[6 + c]), int(r[9 + c])
                tmp_off += j.bw[c] * j.bh[c] * 64
            tmp_off = _align16(tmp_off)
        shapes.append((h, w))
        rgb_off += h * w * 3
    return jobs, shapes, rgb_off, tmp_off


class JpegBatchDecoder:
    """The device stage: packed coefficients -> packed RGB, all images in one call."""

    def __init__(self, device=None):
        from . import constants
        self.device = torch.device(device) if device is not None else constants.DEVICE
        if self.device.type != "cuda":
            raise N.NativeError("JpegBatchDecoder needs a GPU (the IDCT and colour stage are HIP "
                                "kernels; use PIL on the host)")

    def launch(self, dpacked: torch.Tensor, jobs, njobs: int, rgb: torch.Tensor,
               tmp: torch.Tensor):
        """Enqueue the kernels on the current stream (device buffers, host jobs)."""
        N.check(N.lib().stx_jpeg_decode_batch(
            jobs, njobs, dpacked.data_ptr(), rgb.data_ptr(), tmp.data_ptr(), tmp.numel(),
            torch.cuda.current_stream(self.device).cuda_stream), "stx_jpeg_decode_batch")

    def decode_packed(self, packed: torch.Tensor):
        """A packed HOST batch (`pack`) -> (packed uint8 RGB device tensor, [(h, w)]).
        Upload and kernels are enqueued on the current stream; nothing synchronises."""
        jobs, shapes, rgb_bytes, tmp_bytes = plan(records(packed))
        if not shapes:
            raise ValueError("empty image batch")
        dev = self.device
        dp = packed.to(dev, non_blocking=True)
        rgb = torch.empty(rgb_bytes, dtype=torch.uint8, device=dev)
        tmp = torch.empty(max(tmp_bytes, 16), dtype=torch.uint8, device=dev)
        self.launch(dp, jobs, len(shapes), rgb, tmp)
        return rgb, shapes

    def decode(self, items):
        """items: file paths, encoded bytes, JpegCoefs or decoded HxWx3 uint8 arrays ->
        (packed uint8 device tensor of the images one after another, [(h, w)])."""
        items = [it if isinstance(it, (JpegCoefs, np.ndarray)) else load_item(it) for it in items]
        packed = pack(items)
        if torch.cuda.is_available():
            packed = packed.pin_memory()
        return self.decode_packed(packed)


def decode_image(path_or_bytes, device=None) -> torch.Tensor:
    """One image file (path or bytes) -> uint8 [H, W, 3] on the device, Pillow's pixels."""
    rgb, shapes = JpegBatchDecoder(device).decode([path_or_bytes])
    h, w = shapes[0]
    return rgb.view(h, w, 3)


# ------------------------------------------------------------------------------ encode
SAMPLINGS = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2),
             "444": (1, 1), "422": (2, 1), "420": (2, 2)}


def quant_tables(quality: int) -> np.ndarray:
    """uint16 [2, 64] (luma, chroma; natural order): libjpeg's tables of a quality."""
    q = np.empty((2, 64), np.uint16)
    st = N.lib().stx_jpeg_quant_tables(int(quality), q.ctypes.data)
    if st != OK:
        raise JpegError(st)
    return q


def grid(h, w, ncomp, hmax, vmax):
    """[(bw, bh)] per component: the MCU-padded block grids."""
    mx, my = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    return [(mx * (hmax if c == 0 else 1), my * (vmax if c == 0 else 1)) for c in range(ncomp)]


def encode_bound(h, w, ncomp, hmax, vmax) -> int:
    return int(N.lib().stx_jpeg_encode_bound(h, w, ncomp, hmax, vmax))


def try_entropy_encode(coef, h, w, ncomp, hmax, vmax, qtab, out: np.ndarray | None = None):
    """(status, bytes or None).  coef: int16 array in `entropy_decode`'s layout; qtab: uint16
    [ncomp, 64]; out: a reusable uint8 buffer of at least `encode_bound` bytes."""
    coef = np.ascontiguousarray(coef, dtype=np.int16).reshape(-1)
    qtab = np.ascontiguousarray(qtab, dtype=np.uint16).reshape(-1)
    if qtab.size < 64 * ncomp:
        return BAD_ARGS, None
    if out is None:
        out = np.empty(encode_bound(h, w, ncomp, hmax, vmax), np.uint8)
    n = C.c_size_t(0)
    st = N.lib().stx_jpeg_entropy_encode(coef.ctypes.data, coef.nbytes, h, w, ncomp, hmax, vmax,
                                         qtab.ctypes.data, out.ctypes.data if out.size else None,
                                         out.size, C.byref(n))
    if st != OK:
        return st, None
    return OK, out[:n.value].tobytes()


def entropy_encode(coef, h, w, ncomp, hmax, vmax, qtab) -> bytes:
    """Huffman-code quantised coefficients into a baseline JFIF file on the CPU."""
    st, data = try_entropy_encode(coef, h, w, ncomp, hmax, vmax, qtab)
    if st != OK:
        raise JpegError(st)
    return data


def reencode(co: JpegCoefs) -> bytes:
    """`entropy_decode`'s result back to a file (standard Huffman tables)."""
    hmax, vmax = co.sampling[0]
    return entropy_encode(co.coef, co.h, co.w, co.ncomp, hmax, vmax, co.qtab)


class _EncPlan:
    """One batch laid out: the jobs, per frame (h, w, ncomp, hmax, vmax, coefficient range),
    and the sizes of the three device buffers."""

    def __init__(self, frames, sampling, mean, std):
        self.n = len(frames)
        self.jobs = (N.JpegEncJob * max(self.n, 1))()
        self.meta, self.srcs = [], []
        src_off, coef_off, tmp_off = 0, 256, 0  # the two tables lead the coefficient buffer
        for i, f in enumerate(frames):
            fp32 = f.dtype == torch.float32
            if fp32:
                if f.ndim == 4 and f.shape[0] == 1:
                    f = f[0]
                if f.ndim != 3 or f.shape[0] != 3:
                    raise ValueError(f"frame {i}: a normalised float frame is [3, h, w]")
                h, w, ncomp = int(f.shape[1]), int(f.shape[2]), 3
            elif f.dtype == torch.uint8 and (f.ndim == 2 or (f.ndim == 3 and f.shape[2] == 3)):
                h, w, ncomp = int(f.shape[0]), int(f.shape[1]), 1 if f.ndim == 2 else 3
            else:
                raise ValueError(f"frame {i}: uint8 [h, w, 3] / [h, w] or float32 [3, h, w] "
                                 f"expected, got {f.dtype} {tuple(f.shape)}")
            if not (1 <= h <= 65535 and 1 <= w <= 65535):
                raise ValueError(f"frame {i}: {h}x{w} is outside JPEG's 1..65535")
            hmax, vmax = sampling if ncomp == 3 else (1, 1)
            j = self.jobs[i]
            j.src_offset, j.coef_offset, j.qtab_offset, j.tmp_offset = src_off, coef_off, 0, tmp_off
            j.h, j.w, j.ncomp, j.fp32, j.hmax, j.vmax = h, w, ncomp, int(fp32), hmax, vmax
            nblocks = 0
            for c, (bw, bh) in enumerate(grid(h, w, ncomp, hmax, vmax)):
                j.bw[c], j.bh[c] = bw, bh
                nblocks += bw * bh
            for c in range(3):
                j.mean[c], j.std_[c] = mean[c], std[c]
            self.meta.append((h, w, ncomp, hmax, vmax, coef_off, nblocks * 128))
            self.srcs.append((src_off, f.contiguous()))
            src_off = _align16(src_off + f.numel() * f.element_size())
            coef_off = _align16(coef_off + nblocks * 128)
            tmp_off = _align16(tmp_off + nblocks * 64)
        self.src_bytes, self.coef_bytes, self.tmp_bytes = src_off, coef_off, max(tmp_off, 16)


class JpegBatchEncoder:
    """Device images -> JPEG files.  `encode(frames)` runs the two kernels over the whole
    batch, copies the coefficients to pinned memory and Huffman-codes them on the host.
    `submit(frames)` / `collect()` pipeline it: the entropy stage of one batch runs on a
    background thread (the ctypes call releases the GIL) while the GPU works on the next; two
    pinned buffers with an event each, results in submission order; `close()` joins the
    thread.

    frames: a list of device tensors -- uint8 [h, w, 3] (RGB) or [h, w] (grey), or float32
    [3, h, w] / [1, 3, h, w] normalised with mean / std (default: ImageNet's, what
    `img_utils.to_pil` undoes).  The float path's byte is min(int(v * 255), 255) of the
    de-normalised, clamped v: `to_pil`'s byte, except that a value whose v * 255 reaches 256
    saturates here where `to_pil`'s float -> uint8 cast wraps."""

    def __init__(self, device=None, mean=None, std=None):
        from . import constants
        self.device = torch.device(device) if device is not None else constants.DEVICE
        if self.device.type != "cuda":
            raise N.NativeError("JpegBatchEncoder needs a GPU (the colour stage and the forward "
                                "DCT are HIP kernels; use PIL on the host)")
        self.mean = [float(np.float32(v)) for v in (mean or constants.IMAGENET_MEAN)]
        self.std = [float(np.float32(v)) for v in (std or constants.IMAGENET_STD)]
        self._qtabs = {}                    # quality -> (host uint16 [2, 64], device bytes)
        self._dev = {}                      # name -> growing device byte buffer
        self._pinned = [None, None]
        self._events = [torch.cuda.Event(), torch.cuda.Event()]
        self._busy = [None, None]           # slot -> threading.Event of the batch using it
        self._slot = 0
        self._out = np.empty(0, np.uint8)
        self._thread = None
        self._todo = queue.Queue()
        self._done = queue.Queue()
        self._pending = 0

    # ---- buffers
    def _buffer(self, name, nbytes):
        b = self._dev.get(name)
        if b is None or b.numel() < nbytes:
            b = self._dev[name] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return b

    def _pin(self, slot, nbytes):
        b = self._pinned[slot]
        if b is None or b.numel() < nbytes:
            b = self._pinned[slot] = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        return b

    def _tables(self, quality):
        t = self._qtabs.get(quality)
        if t is None:
            q = quant_tables(quality)
            t = self._qtabs[quality] = (q, torch.from_numpy(q.view(np.uint8).reshape(-1).copy())
                                        .to(self.device))
        return t

    # ---- the two stages
    def _launch(self, frames, quality, subsampling, slot):
        """Kernels and the device -> pinned copy of one batch on the current stream; the
        slot's event is recorded behind them."""
        if subsampling not in SAMPLINGS:
            raise ValueError(f"subsampling {subsampling!r}: one of {sorted(SAMPLINGS)}")
        if isinstance(frames, torch.Tensor):
            frames = [frames]
        frames = list(frames)
        if not frames:
            raise ValueError("empty image batch")
        for i, f in enumerate(frames):
            if not isinstance(f, torch.Tensor) or f.device.type != "cuda" or \
                    self.device.index not in (None, f.device.index):
                raise ValueError(f"frame {i}: a tensor on {self.device} expected")
        plan = _EncPlan(frames, SAMPLINGS[subsampling], self.mean, self.std)
        qhost, qdev = self._tables(int(quality))
        if plan.n == 1 and plan.srcs[0][1].data_ptr() % 16 == 0:
            src = plan.srcs[0][1]           # one frame is read where it lies
        else:
            src = self._buffer("src", plan.src_bytes)
            for off, f in plan.srcs:
                flat = f.reshape(-1).view(torch.uint8)
                src[off:off + flat.numel()].copy_(flat)
        coef = self._buffer("coef", plan.coef_bytes)
        tmp = self._buffer("tmp", plan.tmp_bytes)
        coef[:256].copy_(qdev)
        N.check(N.lib().stx_jpeg_encode_batch(
            plan.jobs, plan.n, src.data_ptr(), coef.data_ptr(), tmp.data_ptr(), plan.tmp_bytes,
            torch.cuda.current_stream(self.device).cuda_stream), "stx_jpeg_encode_batch")
        host = self._pin(slot, plan.coef_bytes)
        host[:plan.coef_bytes].copy_(coef[:plan.coef_bytes], non_blocking=True)
        self._events[slot].record(torch.cuda.current_stream(self.device))
        return plan, qhost, host

    def _entropy(self, plan, qhost, host, slot):
        self._events[slot].synchronize()
        pk = host.numpy()
        out = []
        for h, w, ncomp, hmax, vmax, off, nbytes in plan.meta:
            need = encode_bound(h, w, ncomp, hmax, vmax)
            if self._out.size < need:
                self._out = np.empty(need, np.uint8)
            qt = qhost if ncomp == 1 else qhost[[0, 1, 1]]
            st, data = try_entropy_encode(pk[off:off + nbytes].view(np.int16), h, w, ncomp, hmax,
                                          vmax, qt, self._out)
            if st != OK:
                raise JpegError(st)
            out.append(data)
        return out

    def encode(self, frames, quality=90, subsampling="4:2:0") -> list:
        """The JPEG bytes of every frame, in order (synchronises on the copy)."""
        if self._pending:
            raise RuntimeError("encode while submitted batches are outstanding: collect first")
        plan, qhost, host = self._launch(frames, quality, subsampling, 0)
        return self._entropy(plan, qhost, host, 0)

    # ---- pipelined form
    def _worker(self):
        while True:
            item = self._todo.get()
            if item is None:
                return
            plan, qhost, host, slot, free = item
            try:
                res = self._entropy(plan, qhost, host, slot)
            except Exception as e:  # handed to collect()
                res = e
            free.set()
            self._done.put(res)

    def submit(self, frames, quality=90, subsampling="4:2:0"):
        """Enqueue one batch; its files come out of the matching `collect()`."""
        if self._thread is None:
            self._thread = threading.Thread(target=self._worker, name="jpeg-entropy", daemon=True)
            self._thread.start()
        slot = self._slot
        if self._busy[slot] is not None:
            self._busy[slot].wait()         # the batch two back still reads this pinned buffer
        plan, qhost, host = self._launch(frames, quality, subsampling, slot)
        free = self._busy[slot] = threading.Event()
        self._slot ^= 1
        self._pending += 1
        self._todo.put((plan, qhost, host, slot, free))

    def collect(self) -> list:
        """The files of the oldest submitted batch (blocks until its entropy stage is done)."""
        if not self._pending:
            raise RuntimeError("collect without a submitted batch")
        res = self._done.get()
        self._pending -= 1
        if isinstance(res, Exception):
            raise res
        return res

    def close(self):
        if self._thread is not None:
            self._todo.put(None)
            self._thread.join()
            self._thread = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def encode_image(t: torch.Tensor, quality=90, subsampling="4:2:0", device=None) -> bytes:
    """One device image (uint8 [h, w, 3] / [h, w], or normalised float32 [3, h, w]) -> the
    bytes of a baseline JPEG file, Pillow's for the same pixels."""
    return JpegBatchEncoder(device if device is not None else t.device).encode(
        [t], quality, subsampling)[0]
