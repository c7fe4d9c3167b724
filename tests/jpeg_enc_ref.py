"""Plain numpy restatement of the pixel stages of the baseline JPEG encode, written from the
rules include/stx.h states for stx_jpeg_encode_batch (libjpeg's fixed-point RGB -> YCbCr, its
h2v1 / h2v2 downsampling with alternating bias, edge replication, jfdctint.c's "islow"
forward DCT, its quantisation and its dummy blocks), independent of csrc/jpeg.hip: int64
arithmetic on whole planes.  test_jpeg_enc_host.py holds it against the coefficients in
Pillow's streams (read with jpeg_ref.decode_coefs); the C++ entropy coder and the GPU
kernels are then held against it and against Pillow's bytes."""
import numpy as np

import jpeg_ref

SAMPLINGS = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}
PIL_SUBSAMPLING = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}

K_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55,
                   14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                   18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                   49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
K_CHROMA = np.array([17, 18, 24, 47] + [99] * 4 + [18, 21, 26, 66] + [99] * 4
                    + [24, 26, 56] + [99] * 5 + [47, 66] + [99] * 6 + [99] * 32)


def quant_tables(quality):
    """libjpeg's jpeg_set_quality: int64 [2, 64], natural order."""
    q = min(max(int(quality), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return np.stack([np.clip((t * scale + 50) // 100, 1, 255) for t in (K_LUMA, K_CHROMA)])


def ycc(rgb):
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + 8388608 + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + 8388608 + 32767) >> 16
    return y, cb, cr


def _pad_to(p, rows, cols):
    """Replicate the last row / column of p out to [rows, cols]."""
    return np.pad(p, ((0, rows - p.shape[0]), (0, cols - p.shape[1])), mode="edge")


def planes(img, hmax, vmax):
    """HxWx3 (or HxW) uint8 -> per component (sample plane over its REAL block extent,
    (rb_h, rb_w)).  Full-resolution columns are replicated from column w-1 and rows only up
    to a whole row group; after downsampling the last row is replicated down."""
    h, w = img.shape[:2]
    comps = [img.astype(np.int64)] if img.ndim == 2 else list(ycc(img))
    out = []
    for c, p in enumerate(comps):
        hs, vs = (hmax, vmax) if c == 0 else (1, 1)
        cw, chh = -(-w * hs // hmax), -(-h * vs // vmax)
        rbw, rbh = -(-cw // 8), -(-chh // 8)
        fx, fy = hmax // hs, vmax // vs                     # downsampling factors
        p = _pad_to(p, -(-h // fy) * fy, rbw * 8 * fx)
        if fx == 2 and fy == 2:
            bias = np.tile([1, 2], p.shape[1] // 4 + 1)[:p.shape[1] // 2]
            p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
        elif fx == 2:
            bias = np.tile([0, 1], p.shape[1] // 4 + 1)[:p.shape[1] // 2]
            p = (p[:, 0::2] + p[:, 1::2] + bias) >> 1
        else:
            assert (fx, fy) == (1, 1)
        out.append((_pad_to(p, rbh * 8, rbw * 8), (rbh, rbw)))
    return out


def _fix(x):
    return int(round(x * 8192))


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fpass(d, first):
    """jfdctint.c's 8-point butterfly along the LAST axis of d [..., 8] (int64)."""
    t0, t7, t1, t6 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7], d[..., 1] + d[..., 6], \
        d[..., 1] - d[..., 6]
    t2, t5, t3, t4 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5], d[..., 3] + d[..., 4], \
        d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    sh = 11 if first else 15
    o = [None] * 8
    if first:
        o[0], o[4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        o[0], o[4] = _descale(t10 + t11, 2), _descale(t10 - t11, 2)
    z1 = (t12 + t13) * _fix(0.541196100)
    o[2] = _descale(z1 + t13 * _fix(0.765366865), sh)
    o[6] = _descale(z1 - t12 * _fix(1.847759065), sh)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * _fix(1.175875602)
    t4, t5, t6, t7 = t4 * _fix(0.298631336), t5 * _fix(2.053119869), t6 * _fix(3.072711026), \
        t7 * _fix(1.501321110)
    z1, z2 = z1 * -_fix(0.899976223), z2 * -_fix(2.562915447)
    z3, z4 = z3 * -_fix(1.961570560) + z5, z4 * -_fix(0.390180644) + z5
    o[7], o[5] = _descale(t4 + z1 + z3, sh), _descale(t5 + z2 + z4, sh)
    o[3], o[1] = _descale(t6 + z2 + z3, sh), _descale(t7 + z1 + z4, sh)
    return np.stack(o, -1)


def fdct_quant(plane, q):
    """Sample plane [8 bh, 8 bw], q int64[64] -> quantised coefficients [bh, bw, 64]."""
    bh, bw = plane.shape[0] // 8, plane.shape[1] // 8
    d = plane.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3) - 128      # [.., row, col]
    d = _fpass(d, True)                                              # rows
    d = _fpass(d.swapaxes(-1, -2), False).swapaxes(-1, -2)           # columns
    d = d.reshape(bh, bw, 64)
    a = (np.abs(d) + 4 * q) // (8 * q)
    return np.where(d < 0, -a, a)


def coefficients(img, qtabs, hmax=1, vmax=1):
    """HxWx3 / HxW uint8 and int64 [2, 64] tables -> per component int64 [bh, bw, 64] over
    the MCU-padded grid (dummy blocks filled by libjpeg's rule), and the real extents."""
    h, w = img.shape[:2]
    mx, my = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    out, real = [], []
    for c, (p, (rbh, rbw)) in enumerate(planes(img, hmax, vmax)):
        hs, vs = (hmax, vmax) if c == 0 else (1, 1)
        co = np.zeros((my * vs, mx * hs, 64), np.int64)
        co[:rbh, :rbw] = fdct_quant(p, qtabs[1 if c else 0])
        # dummy blocks: zero AC, the DC of the previous block of the component in MCU order
        for y in range(my):
            for x in range(mx):
                prev = None
                for by in range(vs):
                    for bx in range(hs):
                        yy, xx = y * vs + by, x * hs + bx
                        if yy >= rbh or xx >= rbw:
                            co[yy, xx, 0] = prev
                        prev = co[yy, xx, 0]
        out.append(co)
        real.append((rbh, rbw))
    return out, real


def flat_coefs(coefs):
    """Per-component [bh, bw, 64] -> the int16 array the entropy coder reads."""
    return np.concatenate([c.reshape(-1) for c in coefs]).astype(np.int16)


# ------------------------------------------------------------------ the shared case matrix
SIZES = [(1, 1), (7, 9), (8, 8), (9, 17), (16, 16), (17, 33), (24, 40), (33, 47), (48, 64),
         (50, 100), (120, 72)]                                        # (h, w)
QUALITIES = [20, 50, 90, 100]
GREY_SIZES = [(1, 1), (9, 17), (24, 40), (50, 100)]


def pil_jpeg(arr, quality, sampling=None):
    """Pillow's baseline encode of an HxWx3 (sampling given) or HxW uint8 array."""
    if arr.ndim == 2:
        return jpeg_ref.encode(arr, quality=quality)
    return jpeg_ref.encode(arr, quality=quality, subsampling=PIL_SUBSAMPLING[sampling])


def color_cases():
    """[(name, HxWx3 uint8, sampling, quality)]: 11 sizes x 3 samplings x 4 qualities x
    (gradient, noise) = 264."""
    out = []
    for i, (h, w) in enumerate(SIZES):
        for noise in (False, True):
            a = jpeg_ref.image(h, w, 100 + i, noise=noise)
            for ss in SAMPLINGS:
                for q in QUALITIES:
                    out.append((f"{h}x{w}-{'noise' if noise else 'grad'}-{ss}-q{q}", a, ss, q))
    return out


def grey_cases():
    return [(f"{h}x{w}-grey-q{q}", jpeg_ref.image(h, w, 200 + i)[:, :, 1].copy(), q)
            for i, (h, w) in enumerate(GREY_SIZES) for q in (50, 90)]


def photo_cases():
    import os

    from PIL import Image
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = []
    for f in ("data/dancing.jpg", "data/styles/picasso.jpg"):
        a = np.asarray(Image.open(os.path.join(repo, f)).convert("RGB"), dtype=np.uint8)
        for ss in SAMPLINGS:
            out.append((f"{os.path.basename(f)}-{ss}", a, ss, 90))
    return out
