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
"""
from __future__ import annotations

import ctypes as C
import os

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
