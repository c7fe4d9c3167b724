"""Plain numpy / pure-Python restatement of the whole baseline JPEG decode, written from
the formulas (ITU T.81 for the entropy coding; libjpeg's jidctint.c "islow" IDCT, its
"fancy" chroma upsampling and its fixed-point YCbCr -> RGB for the pixels), independent of
csrc/jpeg_host.cpp and csrc/jpeg.hip: its own marker walk, its own bit-by-bit Huffman
decoder, int64 arithmetic.  test_jpeg_host.py holds it against Pillow, pixel for pixel; the
C++ coefficients and the GPU pixels are then held against it and against Pillow.

Only what the tests feed it: SOF0/SOF1, 8 bits, one interleaved scan, 1 or 3 components
with 1x1 chroma and luma 1x1 / 2x1 / 2x2, restart intervals."""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48,
                   41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22,
                   15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
                   62, 63])


def _segments(data):
    """(marker, payload) up to and including SOS; then the offset of the scan data."""
    assert data[:2] == b"\xff\xd8"
    p, out = 2, []
    while True:
        assert data[p] == 0xFF
        while data[p + 1] == 0xFF:
            p += 1
        m = data[p + 1]
        p += 2
        n = (data[p] << 8) | data[p + 1]
        out.append((m, data[p + 2:p + n]))
        p += n
        if m == 0xDA:
            return out, p


def parse(data):
    """Frame header, tables and the scan's bytes."""
    segs, scan = _segments(data)
    J = {"q": {}, "dc": {}, "ac": {}, "restart": 0}
    for m, s in segs:
        if m in (0xC0, 0xC1):
            assert s[0] == 8
            J["h"], J["w"] = (s[1] << 8) | s[2], (s[3] << 8) | s[4]
            J["comps"] = [{"id": s[6 + 3 * c], "hs": s[7 + 3 * c] >> 4, "vs": s[7 + 3 * c] & 15,
                           "tq": s[8 + 3 * c]} for c in range(s[5])]
        elif m == 0xDB:
            o = 0
            while o < len(s):
                assert s[o] >> 4 == 0
                t = np.zeros(64, np.int64)
                t[ZIGZAG] = np.frombuffer(s[o + 1:o + 65], np.uint8)
                J["q"][s[o] & 15] = t
                o += 65
        elif m == 0xC4:
            o = 0
            while o < len(s):
                counts = list(s[o + 1:o + 17])
                syms = s[o + 17:o + 17 + sum(counts)]
                table, code, k = {}, 0, 0
                for ln in range(1, 17):
                    for _ in range(counts[ln - 1]):
                        table[(ln, code)] = syms[k]
                        code += 1
                        k += 1
                    code <<= 1
                J["ac" if s[o] >> 4 else "dc"][s[o] & 15] = table
                o += 17 + sum(counts)
        elif m == 0xDD:
            J["restart"] = (s[0] << 8) | s[1]
        elif m == 0xDA:
            assert s[0] == len(J["comps"])
            for c, comp in enumerate(J["comps"]):
                assert s[1 + 2 * c] == comp["id"]
                comp["td"], comp["ta"] = s[2 + 2 * c] >> 4, s[2 + 2 * c] & 15
    if len(J["comps"]) == 1:
        J["comps"][0]["hs"] = J["comps"][0]["vs"] = 1
    J["scan"] = data[scan:]
    return J


def _intervals(scan):
    """The scan split at its restart markers, un-stuffed, as strings of '0'/'1'."""
    out, cur, i = [], bytearray(), 0
    while i < len(scan):
        b = scan[i]
        if b != 0xFF:
            cur.append(b)
            i += 1
        elif scan[i + 1] == 0:
            cur.append(0xFF)
            i += 2
        elif 0xD0 <= scan[i + 1] <= 0xD7:
            out.append(cur)
            cur = bytearray()
            i += 2
        elif scan[i + 1] == 0xFF:
            i += 1
        else:
            break  # EOI (or any other marker) ends the scan
    out.append(cur)
    return ["".join(f"{b:08b}" for b in seg) for seg in out]


class _Bits:
    def __init__(self, s):
        self.s, self.p = s, 0

    def sym(self, table):
        code = 0
        for ln in range(1, 17):
            code = (code << 1) | (self.s[self.p + ln - 1] == "1")
            v = table.get((ln, code))
            if v is not None:
                self.p += ln
                return v
        raise ValueError("bad Huffman code")

    def value(self, n):
        if n == 0:
            return 0
        v = int(self.s[self.p:self.p + n], 2)
        self.p += n
        return v if v >= (1 << (n - 1)) else v - (1 << n) + 1


def decode_coefs(data):
    """-> (J, [per component int64 [bh, bw, 64] natural-order quantised coefficients],
    [per component int64[64] quantisation table])."""
    J = parse(data)
    comps = J["comps"]
    hmax, vmax = max(c["hs"] for c in comps), max(c["vs"] for c in comps)
    mx, my = -(-J["w"] // (8 * hmax)), -(-J["h"] // (8 * vmax))
    J["hmax"], J["vmax"] = hmax, vmax
    coefs = [np.zeros((my * c["vs"], mx * c["hs"], 64), np.int64) for c in comps]
    ivs = _intervals(J["scan"])
    ri = J["restart"] or mx * my
    mcu = 0
    for seg in ivs:
        if mcu >= mx * my:
            break
        bits, pred = _Bits(seg), [0] * len(comps)
        for _ in range(min(ri, mx * my - mcu)):
            y, x = divmod(mcu, mx)
            for c, comp in enumerate(comps):
                dc, ac = J["dc"][comp["td"]], J["ac"][comp["ta"]]
                for by in range(comp["vs"]):
                    for bx in range(comp["hs"]):
                        blk = coefs[c][y * comp["vs"] + by, x * comp["hs"] + bx]
                        pred[c] += bits.value(bits.sym(dc))
                        blk[0] = pred[c]
                        k = 1
                        while k < 64:
                            rs = bits.sym(ac)
                            r, s = rs >> 4, rs & 15
                            if s == 0:
                                if r != 15:
                                    break
                                k += 16
                                continue
                            k += r
                            blk[ZIGZAG[k]] = bits.value(s)
                            k += 1
            mcu += 1
    assert mcu == mx * my
    return J, coefs, [J["q"][c["tq"]] for c in comps]


def _fix(x, bits=13):
    return int(round(x * (1 << bits)))


def _pass(d, shift):
    """jidctint.c's 8-point butterfly along the LAST axis of d [..., 8] (int64)."""
    z2, z3 = d[..., 2], d[..., 6]
    z1 = (z2 + z3) * _fix(0.541196100)
    tmp2 = z1 - z3 * _fix(1.847759065)
    tmp3 = z1 + z2 * _fix(0.765366865)
    tmp0 = (d[..., 0] + d[..., 4]) << 13
    tmp1 = (d[..., 0] - d[..., 4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = d[..., 7], d[..., 5], d[..., 3], d[..., 1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * _fix(1.175875602)
    tmp0 = tmp0 * _fix(0.298631336)
    tmp1 = tmp1 * _fix(2.053119869)
    tmp2 = tmp2 * _fix(3.072711026)
    tmp3 = tmp3 * _fix(1.501321110)
    z1 = z1 * -_fix(0.899976223)
    z2 = z2 * -_fix(2.562915447)
    z3 = z3 * -_fix(1.961570560) + z5
    z4 = z4 * -_fix(0.390180644) + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    out = np.stack([tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0,
                    tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3], -1)
    return (out + (1 << (shift - 1))) >> shift


def idct_plane(coef, q):
    """[bh, bw, 64] quantised coefficients, q[64] -> uint8 plane [8 bh, 8 bw]."""
    bh, bw = coef.shape[:2]
    d = (coef * q).reshape(bh, bw, 8, 8)                       # [.., row, col]
    d = _pass(d.swapaxes(-1, -2), 11).swapaxes(-1, -2)         # columns: along the row index
    d = _pass(d, 18)                                           # rows
    d = np.clip(d + 128, 0, 255)
    return d.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def _h2v1(p):
    """[ch, cw] -> [ch, 2 cw]."""
    p = p.astype(np.int64)
    left = np.concatenate([p[:, :1], p[:, :-1]], 1)
    right = np.concatenate([p[:, 1:], p[:, -1:]], 1)
    even, odd = (3 * p + left + 1) >> 2, (3 * p + right + 2) >> 2
    even[:, 0], odd[:, -1] = p[:, 0], p[:, -1]
    return np.stack([even, odd], 2).reshape(p.shape[0], -1)


def _h2v2(p):
    """[ch, cw] -> [2 ch, 2 cw]."""
    p = p.astype(np.int64)
    up = np.concatenate([p[:1], p[:-1]], 0)
    down = np.concatenate([p[1:], p[-1:]], 0)
    rows = []
    for s in (3 * p + up, 3 * p + down):
        left = np.concatenate([s[:, :1], s[:, :-1]], 1)
        right = np.concatenate([s[:, 1:], s[:, -1:]], 1)
        even, odd = (3 * s + left + 8) >> 4, (3 * s + right + 7) >> 4
        even[:, 0], odd[:, -1] = (4 * s[:, 0] + 8) >> 4, (4 * s[:, -1] + 7) >> 4
        rows.append(np.stack([even, odd], 2).reshape(p.shape[0], -1))
    return np.stack(rows, 1).reshape(2 * p.shape[0], -1)


def pixels(J, coefs, qtabs):
    """Coefficients -> HxWx3 uint8, the way libjpeg (islow, fancy upsampling) does it."""
    h, w = J["h"], J["w"]
    planes = [idct_plane(c, q) for c, q in zip(coefs, qtabs)]
    y = planes[0][:h, :w].astype(np.int64)
    if len(planes) == 1:
        return np.repeat(y[:, :, None], 3, 2).astype(np.uint8)
    hmax, vmax = J["hmax"], J["vmax"]
    cw, ch = -(-w // hmax), -(-h // vmax)
    ch_planes = []
    for p in planes[1:]:
        p = p[:ch, :cw]  # the edge replication works on the real size, not the padded one
        if (hmax, vmax) == (2, 1):
            p = _h2v1(p)
        elif (hmax, vmax) == (2, 2):
            p = _h2v2(p)
        else:
            assert (hmax, vmax) == (1, 1)
        ch_planes.append(p[:h, :w].astype(np.int64) - 128)
    cb, cr = ch_planes
    F = lambda x: int(round(x * 65536))  # noqa: E731
    r = y + ((F(1.402) * cr + 32768) >> 16)
    g = y + ((-F(0.34414) * cb - F(0.71414) * cr + 32768) >> 16)
    b = y + ((F(1.772) * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], 2), 0, 255).astype(np.uint8)


def decode(data):
    """JPEG bytes -> HxWx3 uint8."""
    return pixels(*decode_coefs(data))


# ------------------------------------------------------------------ the shared case matrix
SIZES = [(1, 1), (8, 9), (16, 16), (17, 33), (37, 53), (64, 48)]   # (h, w)


def image(h, w, seed, noise=False):
    rng = np.random.default_rng(seed)
    if noise:
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    base = np.stack([np.sin(x / 5.0) * 90 + np.cos(y / 7.0) * 60 + 128,
                     np.sin((x + y) / 9.0) * 110 + 128, (x * y / 3.0) % 255], 2)
    return np.clip(base + rng.normal(0, 10, (h, w, 3)), 0, 255).astype(np.uint8)


def encode(arr, grey=False, **kw):
    import io

    from PIL import Image
    img = Image.fromarray(arr)
    if grey:
        img = img.convert("L")
    f = io.BytesIO()
    img.save(f, "JPEG", **kw)
    return f.getvalue()


def pil_decode(data):
    import io

    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"), dtype=np.uint8)


def cases():
    """[(name, JPEG bytes)]: the matrix every JPEG test runs -- sizes x subsampling
    (4:4:4 / 4:2:2 / 4:2:0 / greyscale), the qualities, restart intervals, optimised
    tables, saturating noise, one 480x640, and the two photographs under data/."""
    import os
    out = []
    for i, (h, w) in enumerate(SIZES):
        a = image(h, w, 10 + i)
        for ss in (0, 1, 2):
            out.append((f"{h}x{w}-ss{ss}-q90", encode(a, quality=90, subsampling=ss)))
        out.append((f"{h}x{w}-grey-q90", encode(a, grey=True, quality=90)))
    a = image(37, 53, 31)
    for q in (50, 100):
        for ss in (0, 1, 2):
            out.append((f"37x53-ss{ss}-q{q}", encode(a, quality=q, subsampling=ss)))
        out.append((f"37x53-grey-q{q}", encode(a, grey=True, quality=q)))
    for ss in (0, 1, 2):
        out.append((f"37x53-ss{ss}-restart3",
                    encode(a, quality=90, subsampling=ss, restart_marker_blocks=3)))
        out.append((f"37x53-ss{ss}-optimize", encode(a, quality=90, subsampling=ss, optimize=True)))
    out.append(("37x53-grey-restart3", encode(a, grey=True, quality=90, restart_marker_blocks=3)))
    n = image(64, 48, 32, noise=True)
    for ss in (0, 1, 2):
        out.append((f"noise64x48-ss{ss}-q100", encode(n, quality=100, subsampling=ss)))
    out.append(("480x640-ss2-q90", encode(image(480, 640, 33), quality=90)))
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for f in ("data/dancing.jpg", "data/styles/picasso.jpg"):
        with open(os.path.join(repo, f), "rb") as fh:
            out.append((os.path.basename(f), fh.read()))
    return out
