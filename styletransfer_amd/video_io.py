"""Motion-JPEG in an AVI container, written and read without a codec library: an AVI file is
a RIFF tree whose `movi` list holds one chunk per frame, and an MJPEG frame is a baseline
JPEG file -- what `jpeg.JpegBatchEncoder` writes and `jpeg.JpegBatchDecoder` reads.

    RIFF 'AVI '
      LIST 'hdrl'   avih (main header)
                    LIST 'strl'   strh ('vids', 'MJPG', dwRate / dwScale = fps)
                                  strf (BITMAPINFOHEADER: 24 bits, 'MJPG')
      LIST 'movi'   '00dc' chunks, each padded to an even length
      idx1          one (ckid, flags, offset from 'movi', size) entry per frame

Files stay below 1 GiB (one RIFF; the OpenDML extension is not written or read)."""
from __future__ import annotations

import struct
from fractions import Fraction

RIFF_LIMIT = 1 << 30
_AVIF_HASINDEX, _AVIIF_KEYFRAME = 0x10, 0x10
_HEADER_BYTES = 12 + 12 + 8 + 56 + 12 + 8 + 56 + 8 + 40 + 12  # up to and including 'movi'

# ITU T.81 Annex K.3, the typical Huffman tables: (class << 4 | id, counts of lengths 1..16,
# symbols).  An "AVI1" frame leaves its DHT segment out and means these.
_STD_HUFFMAN = (
    (0x00, (0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12))),
    (0x10, (0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D),
     (0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61,
      0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52,
      0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25,
      0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45,
      0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64,
      0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83,
      0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
      0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6,
      0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3,
      0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8,
      0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA)),
    (0x01, (0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12))),
    (0x11, (0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77),
     (0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61,
      0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33,
      0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18,
      0x19, 0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44,
      0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63,
      0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A,
      0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
      0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4,
      0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA,
      0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7,
      0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA)),
)


def standard_dht() -> bytes:
    """One DHT segment holding the four standard tables."""
    body = b"".join(bytes([tc]) + bytes(counts) + bytes(syms)
                    for tc, counts, syms in _STD_HUFFMAN)
    return b"\xff\xc4" + struct.pack(">H", 2 + len(body)) + body


def with_dht(frame: bytes) -> bytes:
    """The frame itself if it carries a DHT segment before its scan; otherwise (the
    abbreviated "AVI1" form) the frame with the standard tables inserted before SOS, so that
    any JPEG decoder takes it.  Bytes that do not walk as JPEG markers come back unchanged."""
    if frame[:2] != b"\xff\xd8":
        return frame
    p, n = 2, len(frame)
    while p + 4 <= n and frame[p] == 0xFF:
        m = frame[p + 1]
        if m == 0xFF:
            p += 1
            continue
        if m == 0xC4:
            return frame
        if m == 0xDA:
            return frame[:p] + standard_dht() + frame[p:]
        if m == 0x01 or 0xD0 <= m <= 0xD8:
            p += 2
            continue
        p += 2 + struct.unpack_from(">H", frame, p + 2)[0]
    return frame


class MjpegAviWriter:
    """Write JPEG files as the frames of an MJPEG AVI: `write(jpeg_bytes)` per frame, then
    `close()` (which writes the index and patches the totals).  fps is stored as the
    fraction dwRate / dwScale.  A frame that would take the file past `limit` (1 GiB: one
    RIFF) raises ValueError before anything of it is written."""

    def __init__(self, path, fps, h, w, limit=RIFF_LIMIT):
        fr = Fraction(fps).limit_denominator(100000)
        if fr <= 0:
            raise ValueError(f"fps {fps!r}: a positive rate expected")
        if not (1 <= h <= 65535 and 1 <= w <= 65535):
            raise ValueError(f"frame size {h}x{w}: 1..65535 expected")
        self.path, self.h, self.w, self.limit = path, int(h), int(w), int(limit)
        self.rate, self.scale = fr.numerator, fr.denominator
        self.index = []                     # (offset from the 'movi' fourcc, size)
        self.max_chunk = 0
        self.f = open(path, "wb")
        self._header()
        self.movi = self.f.tell() - 4       # position of the 'movi' fourcc
        self.pos = self.f.tell()

    def _header(self):
        n, big = len(self.index), self.max_chunk
        movi_bytes = 4 + sum(8 + s + (s & 1) for _, s in self.index)
        total = _HEADER_BYTES - 16 + movi_bytes + 8 + 16 * n  # the RIFF payload after 'AVI '
        usec = round(1_000_000 * self.scale / self.rate)
        per_sec = int(sum(s for _, s in self.index) * self.rate / (self.scale * max(n, 1)))
        f = self.f
        f.seek(0)
        f.write(struct.pack("<4sI4s", b"RIFF", 4 + total, b"AVI "))
        f.write(struct.pack("<4sI4s", b"LIST", 4 + 8 + 56 + 12 + 8 + 56 + 8 + 40, b"hdrl"))
        f.write(struct.pack("<4sI14I", b"avih", 56, usec, per_sec, 0, _AVIF_HASINDEX, n, 0, 1,
                            big, self.w, self.h, 0, 0, 0, 0))
        f.write(struct.pack("<4sI4s", b"LIST", 4 + 8 + 56 + 8 + 40, b"strl"))
        f.write(struct.pack("<4sI4s4sIHHIIIIIIiI4H", b"strh", 56, b"vids", b"MJPG", 0, 0, 0, 0,
                            self.scale, self.rate, 0, n, big, -1, 0, 0, 0, self.w, self.h))
        f.write(struct.pack("<4sIIiiHH4sIiiII", b"strf", 40, 40, self.w, self.h, 1, 24, b"MJPG",
                            self.w * self.h * 3, 0, 0, 0, 0))
        f.write(struct.pack("<4sI4s", b"LIST", movi_bytes, b"movi"))

    def write(self, jpeg_bytes):
        if self.f is None:
            raise ValueError(f"{self.path}: write after close")
        data = bytes(jpeg_bytes)
        size = len(data)
        end = self.pos + 8 + size + (size & 1) + 8 + 16 * (len(self.index) + 1)
        if end > self.limit:
            raise ValueError(f"{self.path}: frame {len(self.index)} would take the file to {end} "
                             f"bytes, past the {self.limit}-byte limit of a plain AVI (OpenDML "
                             "is not written); split the clip")
        self.f.write(struct.pack("<4sI", b"00dc", size))
        self.f.write(data)
        if size & 1:
            self.f.write(b"\0")
        self.index.append((self.pos - self.movi, size))
        self.max_chunk = max(self.max_chunk, size)
        self.pos += 8 + size + (size & 1)

    def close(self):
        if self.f is None:
            return
        f = self.f
        f.seek(self.pos)
        f.write(struct.pack("<4sI", b"idx1", 16 * len(self.index)))
        for off, size in self.index:
            f.write(struct.pack("<4sIII", b"00dc", _AVIIF_KEYFRAME, off, size))
        self._header()
        f.close()
        self.f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _chunks(f, start, end):
    """(fourcc, payload offset, size) of the chunks in [start, end); LISTs are entered."""
    p = start
    while p + 8 <= end:
        f.seek(p)
        cc, size = struct.unpack("<4sI", f.read(8))
        if cc in (b"LIST", b"RIFF"):
            f.seek(p + 8)
            kind = f.read(4)
            yield kind, p + 12, max(size - 4, 0)
            if kind != b"movi":
                yield from _chunks(f, p + 12, min(p + 8 + size, end))
        else:
            yield cc, p + 8, size
        p += 8 + size + (size & 1)


def read_mjpeg_avi(path):
    """(fps, h, w, iterator of the frames' JPEG bytes) of an MJPEG AVI.  ValueError for a file
    that is no AVI or whose video stream is not MJPG (the message names its fourcc).  Frames
    in the abbreviated form without Huffman tables get the standard DHT segment (`with_dht`)."""
    import os
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        head = f.read(12)
        if len(head) < 12 or head[:4] != b"RIFF" or head[8:12] != b"AVI ":
            raise ValueError(f"{path}: not an AVI file")
        end = min(size, 8 + struct.unpack("<I", head[4:8])[0])
        fps = h = w = movi = None
        video = False
        for cc, off, n in _chunks(f, 12, end):
            f.seek(off)
            if cc == b"strh" and n >= 32:
                d = f.read(32)
                video = d[:4] == b"vids" and fps is None
                if video:
                    handler = d[4:8]
                    scale, rate = struct.unpack("<II", d[20:28])
                    fps = rate / scale if scale else 0.0
            elif cc == b"strf" and video and n >= 20 and h is None:
                d = f.read(20)
                w, h = struct.unpack("<ii", d[4:12])
                comp = d[16:20]
                if comp.upper() != b"MJPG":
                    shown = comp.decode("latin-1")
                    raise ValueError(f"{path}: the video stream is {shown!r} "
                                     f"(handler {handler.decode('latin-1')!r}), not MJPG; only "
                                     "Motion-JPEG AVI files are read")
                h = abs(h)
            elif cc == b"movi" and movi is None:
                movi = (off, n)
        if fps is None or h is None:
            raise ValueError(f"{path}: no video stream")
        if movi is None:
            raise ValueError(f"{path}: no 'movi' list")

    def frames():
        with open(path, "rb") as f:
            p, stop = movi[0], min(movi[0] + movi[1], size)
            while p + 8 <= stop:
                f.seek(p)
                cc, n = struct.unpack("<4sI", f.read(8))
                if cc == b"LIST":           # 'rec ' groups: step into them
                    p += 12
                    continue
                if cc[2:] in (b"dc", b"db") and cc[:2] == b"00" and n:
                    yield with_dht(f.read(n))
                p += 8 + n + (n & 1)

    return fps, h, w, frames()
