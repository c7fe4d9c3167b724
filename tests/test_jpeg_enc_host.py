"""The host half of the GPU JPEG encode and the MJPEG AVI container, no GPU needed: the
numpy restatement of the pixel stages (jpeg_enc_ref) reproduces the coefficients in Pillow's
streams, the C++ entropy coder (csrc/jpeg_host.cpp) turns coefficients into Pillow's bytes,
refuses what it cannot code without touching memory past `cap`, and video_io writes and
reads AVI files an independent RIFF walk agrees with."""
import ctypes as C
import struct

import numpy as np
import pytest

import jpeg_enc_ref as E
import jpeg_ref as R


@pytest.fixture(scope="module")
def colour():
    """[(name, array, sampling, quality, Pillow's bytes)]: the 264 colour cases."""
    return [(n, a, ss, q, E.pil_jpeg(a, q, ss)) for n, a, ss, q in E.color_cases()]


@pytest.fixture(scope="module")
def grey():
    return [(n, a, q, E.pil_jpeg(a, q)) for n, a, q in E.grey_cases()]


@pytest.fixture(scope="module")
def photos():
    return [(n, a, ss, q, E.pil_jpeg(a, q, ss)) for n, a, ss, q in E.photo_cases()]


def _check_coefs(name, arr, hmax, vmax, data):
    """The reference's coefficients against the ones in Pillow's stream `data`."""
    J, want, qt = R.decode_coefs(data)
    assert (J["hmax"], J["vmax"]) == (hmax, vmax), name
    got, real = E.coefficients(arr, np.stack([qt[0], qt[-1]]), hmax, vmax)
    for c, (g, w_, (rbh, rbw)) in enumerate(zip(got, want, real)):
        assert g.shape == w_.shape, (name, c)
        assert np.array_equal(g[:rbh, :rbw], w_[:rbh, :rbw]), (name, c, "real blocks")
        assert np.array_equal(g, w_), (name, c, "dummy blocks")
    return got, qt


def test_reference_coefficients_equal_pillow(colour, grey):
    assert len(colour) == 264
    dummies = 0
    for name, a, ss, q, data in colour:
        hmax, vmax = E.SAMPLINGS[ss]
        got, _ = _check_coefs(name, a, hmax, vmax, data)
        h, w = a.shape[:2]
        dummies += got[0].shape[0] * got[0].shape[1] - (-(-h // 8)) * (-(-w // 8))
    assert dummies > 100  # the dummy-block rule was exercised
    for name, a, q, data in grey:
        _check_coefs(name, a, 1, 1, data)


def test_reference_coefficients_equal_pillow_photos(photos):
    for name, a, ss, q, data in photos:
        _check_coefs(name, a, *E.SAMPLINGS[ss], data)


@pytest.mark.parametrize("q", [1, 20, 50, 75, 90, 95, 100])
def test_quant_tables_equal_pillow(q):
    from styletransfer_amd import jpeg
    _, _, qt = R.decode_coefs(E.pil_jpeg(R.image(16, 16, 5), q, "4:2:0"))
    got = jpeg.quant_tables(q)
    assert got.dtype == np.uint16 and got.shape == (2, 64)
    assert np.array_equal(got[0], qt[0]) and np.array_equal(got[1], qt[1])
    assert np.array_equal(got, E.quant_tables(q))


def test_round_trip_of_pillow_streams():
    """entropy_encode(entropy_decode(data)) == data: the header layout and the Huffman stage
    are Pillow's (optimize=False, no restart markers), for the four layouts."""
    from styletransfer_amd import jpeg
    n = 0
    for i, (h, w) in enumerate([(1, 1), (8, 8), (24, 40), (50, 100), (37, 53)]):
        for noise in (False, True):
            a = R.image(h, w, 40 + i, noise=noise)
            for q in (20, 90, 100):
                streams = [E.pil_jpeg(a, q, ss) for ss in E.SAMPLINGS]
                streams.append(E.pil_jpeg(a[:, :, 0].copy(), q))
                for data in streams:
                    assert jpeg.reencode(jpeg.entropy_decode(data)) == data, (h, w, noise, q, n)
                    n += 1
    assert n == 120


def test_reference_coefficients_encode_to_pillow_bytes(colour, grey, photos):
    from styletransfer_amd import jpeg
    for name, a, ss, q, data in colour + photos:
        hmax, vmax = E.SAMPLINGS[ss]
        qt = E.quant_tables(q)
        coefs, _ = E.coefficients(a, qt, hmax, vmax)
        got = jpeg.entropy_encode(E.flat_coefs(coefs), a.shape[0], a.shape[1], 3, hmax, vmax,
                                  qt[[0, 1, 1]])
        assert got == data, name
    for name, a, q, data in grey:
        qt = E.quant_tables(q)
        coefs, _ = E.coefficients(a, qt)
        got = jpeg.entropy_encode(E.flat_coefs(coefs), a.shape[0], a.shape[1], 1, 1, 1, qt[:1])
        assert got == data, name


def _raw_encode(coef, h, w, ncomp, hmax, vmax, qtab, cap, coef_bytes=None):
    """The C entry point on a buffer with 64 canary bytes behind `cap`."""
    from styletransfer_amd import _native as N
    buf = np.full(cap + 64, 0xA5, np.uint8)
    n = C.c_size_t(12345)
    coef = np.ascontiguousarray(coef, np.int16)
    qtab = np.ascontiguousarray(qtab, np.uint16)
    st = N.lib().stx_jpeg_entropy_encode(
        coef.ctypes.data, coef.nbytes if coef_bytes is None else coef_bytes, h, w, ncomp, hmax,
        vmax, qtab.ctypes.data, buf.ctypes.data, cap, C.byref(n))
    assert np.all(buf[cap:] == 0xA5), "wrote past cap"
    return st, n.value, buf[:cap]


def test_refusals():
    from styletransfer_amd import jpeg
    a = R.image(24, 40, 7, noise=True)
    qt = E.quant_tables(90)
    coefs, _ = E.coefficients(a, qt, 2, 2)
    flat, q3 = E.flat_coefs(coefs), qt[[0, 1, 1]].astype(np.uint16)
    want = E.pil_jpeg(a, 90, "4:2:0")
    bound = jpeg.encode_bound(24, 40, 3, 2, 2)
    assert bound >= len(want)
    st, n, out = _raw_encode(flat, 24, 40, 3, 2, 2, q3, bound)
    assert st == jpeg.OK and out[:n].tobytes() == want
    st, n, out = _raw_encode(flat, 24, 40, 3, 2, 2, q3, len(want))      # exactly enough
    assert st == jpeg.OK and out[:n].tobytes() == want
    # short cap: in the header, in the scan, one byte short
    for cap in (0, 1, 19, 300, 622, 640, len(want) - 2, len(want) - 1):
        st, n, _ = _raw_encode(flat, 24, 40, 3, 2, 2, q3, cap)
        assert (st, n) == (jpeg.BAD_ARGS, 0), cap
    # short coefficient array
    st, n, _ = _raw_encode(flat, 24, 40, 3, 2, 2, q3, bound, coef_bytes=flat.nbytes - 2)
    assert (st, n) == (jpeg.BAD_ARGS, 0)
    # out-of-range DC difference / AC value: hostile arrays never index outside a table
    for pos, val in ((0, 2048), (0, -2048), (64, 32767), (1, 1024), (5, -1024), (63, -32768)):
        bad = flat.copy()
        bad[pos] = val
        st, n, _ = _raw_encode(bad, 24, 40, 3, 2, 2, q3, bound)
        assert (st, n) == (jpeg.BAD_ARGS, 0), (pos, val)
    for pos, val in ((0, 1023), (1, 1023), (5, -1023)):                  # the limits pass
        ok = np.zeros_like(flat)
        ok[pos] = val
        st, n, out = _raw_encode(ok, 24, 40, 3, 2, 2, q3, bound)
        assert st == jpeg.OK and n > 600
        back = jpeg.entropy_decode(out[:n].tobytes())
        assert np.array_equal(back.coef, ok), (pos, val)
    rng = np.random.default_rng(3)
    for _ in range(20):
        hostile = rng.integers(-32768, 32768, flat.size).astype(np.int16)
        st, n, _ = _raw_encode(hostile, 24, 40, 3, 2, 2, q3, bound)
        assert (st, n) == (jpeg.BAD_ARGS, 0)
    # samplings the encoder does not write; unequal chroma tables; a zero table entry
    for ncomp, hm, vm in ((3, 1, 2), (3, 4, 1), (3, 2, 4), (1, 2, 2), (2, 1, 1), (4, 1, 1),
                          (3, 0, 0)):
        assert jpeg.encode_bound(24, 40, ncomp, hm, vm) == 0
        st, n, _ = _raw_encode(flat, 24, 40, ncomp, hm, vm, q3, bound)
        assert (st, n) == (jpeg.BAD_ARGS, 0), (ncomp, hm, vm)
    for h, w in ((0, 40), (24, 0), (65536, 8)):
        st, n, _ = _raw_encode(flat, h, w, 3, 2, 2, q3, bound)
        assert (st, n) == (jpeg.BAD_ARGS, 0)
    q_bad = q3.copy()
    q_bad[2, 5] += 1
    assert _raw_encode(flat, 24, 40, 3, 2, 2, q_bad, bound)[0] == jpeg.BAD_ARGS
    q_bad = q3.copy()
    q_bad[0, 0] = 0
    assert _raw_encode(flat, 24, 40, 3, 2, 2, q_bad, bound)[0] == jpeg.BAD_ARGS
    with pytest.raises(jpeg.JpegError):
        jpeg.entropy_encode(flat[:-1], 24, 40, 3, 2, 2, q3)


def test_enc_job_mirror_matches_the_library():
    from styletransfer_amd import _native as N
    out = (C.c_longlong * 2)()
    assert N.lib().stx_jpeg_enc_layout(None, 0) == 2
    assert N.lib().stx_jpeg_enc_layout(C.cast(out, C.c_void_p), 2) == 2
    assert N.JpegEncJob._fields_[-1][0] == "std_"
    assert (C.sizeof(N.JpegEncJob), N.JpegEncJob.std_.offset) == (out[0], out[1])
    assert N.lib().stx_jpeg_layout(None, 0) == 4       # the decoder's query keeps its count
    assert C.sizeof(N.JpegEncJob) * N.STX_JPEG_CHUNK <= 4096  # passed by value to the kernels


# ------------------------------------------------------------------------------ AVI
def _riff_walk(data):
    """An independent walk of an AVI file: {'chunks': [(path, fourcc, offset, size)]} with
    every size and padding rule checked on the way."""
    assert data[:4] == b"RIFF" and data[8:12] == b"AVI "
    assert struct.unpack_from("<I", data, 4)[0] == len(data) - 8, "RIFF size"
    found = []

    def walk(p, end, path):
        while p < end:
            assert p + 8 <= end, "chunk header cut"
            cc, n = data[p:p + 4], struct.unpack_from("<I", data, p + 4)[0]
            assert p + 8 + n <= end, (cc, "chunk runs past its parent")
            if cc == b"LIST":
                kind = data[p + 8:p + 12]
                found.append((path, b"LIST:" + kind, p, n))
                walk(p + 12, p + 8 + n, path + (kind,))
            else:
                found.append((path, cc, p, n))
            p += 8 + n + (n & 1)
            assert p % 2 == 0, "chunks start on even offsets"
        assert p == end, "padding runs past the parent"

    walk(12, len(data), ())
    return found


def _frames():
    small = [E.pil_jpeg(R.image(24, 40, 60 + i, noise=bool(i & 1)), 90, "4:2:0") for i in range(3)]
    other = [E.pil_jpeg(R.image(24, 40, 70 + i), 20, "4:4:4") for i in range(2)]
    frames = [small[0], other[0], small[1], other[1], small[2]]
    assert {len(f) & 1 for f in frames} == {0, 1}, "both paddings are exercised"
    return frames


def test_avi_writer_against_an_independent_walk(tmp_path):
    from styletransfer_amd import video_io
    frames = _frames()
    path = str(tmp_path / "clip.avi")
    with video_io.MjpegAviWriter(path, 29.97, 24, 40) as wr:
        for f in frames:
            wr.write(f)
    data = open(path, "rb").read()
    found = _riff_walk(data)
    by = {}
    for pth, cc, off, n in found:
        by.setdefault(cc, []).append((pth, off, n))
    assert [pth for pth, _, _ in by[b"avih"]] == [(b"hdrl",)]
    assert [pth for pth, _, _ in by[b"strh"]] == [(b"hdrl", b"strl")]
    assert [pth for pth, _, _ in by[b"strf"]] == [(b"hdrl", b"strl")]
    _, off, n = by[b"avih"][0]
    avih = struct.unpack_from("<14I", data, off + 8)
    assert n == 56 and avih[4] == 5 and avih[6] == 1 and (avih[8], avih[9]) == (40, 24)
    assert avih[3] & 0x10 and avih[0] == round(1e6 * 100 / 2997)
    _, off, n = by[b"strh"][0]
    assert n == 56 and data[off + 8:off + 16] == b"vidsMJPG"
    scale, rate, _, length = struct.unpack_from("<4I", data, off + 8 + 20)
    assert (rate, scale, length) == (2997, 100, 5)
    _, off, n = by[b"strf"][0]
    size, w, h, planes, bits = struct.unpack_from("<IiiHH", data, off + 8)
    assert (n, size, w, h, planes, bits) == (40, 40, 40, 24, 1, 24)
    assert data[off + 8 + 16:off + 8 + 20] == b"MJPG"
    movies = [(off, n) for pth, off, n in by[b"00dc"] if pth == (b"movi",)]
    assert [data[o + 8:o + 8 + n] for o, n in movies] == frames
    (_, movi_off, _), = by[b"LIST:movi"]
    (_, off, n), = by[b"idx1"]
    assert n == 16 * 5
    for i, (o, sz) in enumerate(movies):
        ckid, flags, rel, size = struct.unpack_from("<4sIII", data, off + 8 + 16 * i)
        assert ckid == b"00dc" and flags & 0x10 and size == sz
        assert movi_off + 8 + rel == o, "idx1 offsets count from the 'movi' fourcc"
        assert data[o:o + 4] == b"00dc"
    fps, h, w, it = video_io.read_mjpeg_avi(path)
    assert (h, w) == (24, 40) and abs(fps - 29.97) < 1e-9
    assert list(it) == frames


def test_avi_reader_inserts_missing_dht_and_refuses_other_codecs(tmp_path):
    from styletransfer_amd import video_io
    frames = _frames()

    def strip_dht(f):
        out, p = bytearray(f[:2]), 2
        while f[p + 1] != 0xDA:
            n = 2 + struct.unpack_from(">H", f, p + 2)[0]
            if f[p + 1] != 0xC4:
                out += f[p:p + n]
            p += n
        return bytes(out + f[p:])

    bare = [strip_dht(f) for f in frames]
    assert all(b"\xff\xc4" not in b[:b.index(b"\xff\xda")] for b in bare)
    from styletransfer_amd import jpeg
    # (libjpeg-turbo assumes the standard tables by itself; this project's decoder does not)
    assert jpeg.try_entropy_decode(bare[0])[0] == jpeg.CORRUPT
    path = str(tmp_path / "avi1.avi")
    with video_io.MjpegAviWriter(path, 24, 24, 40) as wr:
        for b in bare:
            wr.write(b)
    fps, h, w, it = video_io.read_mjpeg_avi(path)
    assert fps == 24.0
    got = list(it)
    assert len(got) == 5
    for g, f in zip(got, frames):
        assert np.array_equal(R.pil_decode(g), R.pil_decode(f))
        assert np.array_equal(jpeg.entropy_decode(g).coef, jpeg.entropy_decode(f).coef)
        assert np.array_equal(R.decode(g), R.pil_decode(f))  # the inserted tables are the standard ones
    # the same container with another codec in strh / strf
    data = bytearray(open(path, "rb").read())
    for tag in (b"vidsMJPG",):
        i = data.index(tag)
        data[i + 4:i + 8] = b"H264"
    i = data.index(b"strf")
    data[i + 8 + 16:i + 8 + 20] = b"H264"
    other = str(tmp_path / "h264.avi")
    open(other, "wb").write(bytes(data))
    with pytest.raises(ValueError, match="H264"):
        video_io.read_mjpeg_avi(other)
    open(other, "wb").write(b"RIFF\x04\0\0\0WAVE")
    with pytest.raises(ValueError, match="not an AVI"):
        video_io.read_mjpeg_avi(other)


def test_avi_size_guard(tmp_path):
    from styletransfer_amd import video_io
    frames = _frames()
    path = str(tmp_path / "small.avi")
    limit = 224 + 8 + len(frames[0]) + (len(frames[0]) & 1) + 8 + 16 + 50
    wr = video_io.MjpegAviWriter(path, 24, 24, 40, limit=limit)
    wr.write(frames[0])
    with pytest.raises(ValueError, match="limit"):
        wr.write(frames[1])
    wr.close()
    assert video_io.RIFF_LIMIT == 1 << 30
    data = open(path, "rb").read()
    assert len(data) <= limit
    _riff_walk(data)
    assert list(video_io.read_mjpeg_avi(path)[3]) == frames[:1]


def test_iterate_raw_frames_reads_mjpeg_avi(tmp_path):
    from styletransfer_amd import video, video_io
    frames = _frames()
    path = str(tmp_path / "in.avi")
    with video_io.MjpegAviWriter(path, 24, 24, 40) as wr:
        for f in frames:
            wr.write(f)
    got = list(video.iterate_raw_frames(path))
    assert len(got) == 5
    for g, f in zip(got, frames):
        assert g.dtype == np.uint8 and np.array_equal(g, R.pil_decode(f))
