"""The host half of the GPU JPEG decode (csrc/jpeg_host.cpp, styletransfer_amd/jpeg.py), no
GPU needed: the numpy restatement (jpeg_ref) reproduces Pillow pixel for pixel, the C++
entropy decoder reproduces jpeg_ref's coefficients and tables exactly, unsupported and
damaged streams are reported and never overrun a buffer, and the loader's collate
round-trips a mixed batch."""
import ctypes as C
import io

import numpy as np
import pytest
from PIL import Image

import jpeg_ref as R


@pytest.fixture(scope="module")
def matrix():
    """[(name, bytes, jpeg_ref's (J, coefs, qtabs))], decoded once for the module."""
    return [(name, data, R.decode_coefs(data)) for name, data in R.cases()]


def test_reference_decode_equals_pil(matrix):
    """jpeg_ref.pixels (islow IDCT, fancy upsampling, fixed-point colour) == Pillow, every
    pixel of every case: the formulas the HIP kernels restate are libjpeg's."""
    assert len(matrix) >= 40
    for name, data, ref in matrix:
        got, want = R.pixels(*ref), R.pil_decode(data)
        assert got.shape == want.shape, name
        assert np.array_equal(got, want), (name, int(np.abs(got.astype(int) - want).max()))


def test_entropy_decode_equals_reference(matrix):
    from styletransfer_amd import jpeg
    for name, data, (J, coefs, qtabs) in matrix:
        co = jpeg.entropy_decode(data)
        assert (co.h, co.w, co.ncomp) == (J["h"], J["w"], len(coefs)), name
        assert co.coef.dtype == np.int16 and co.qtab.dtype == np.uint16
        assert co.coef.size == sum(c.size for c in coefs), name
        for c, (want, q) in enumerate(zip(coefs, qtabs)):
            bh, bw = want.shape[:2]
            assert co.blocks[c] == (bw, bh), name
            assert np.array_equal(co.component(c).reshape(bh, bw, 64), want), (name, c)
            assert np.array_equal(co.qtab[c], q), (name, c)


def test_info_fields(matrix):
    from styletransfer_amd import jpeg
    for name, data, (J, coefs, _) in matrix:
        inf = jpeg.info(data)
        assert inf.ok and inf.status == jpeg.OK, name
        assert (inf.h, inf.w, inf.ncomp) == (J["h"], J["w"], len(coefs)), name
        assert inf.sampling == [(c["hs"], c["vs"]) for c in J["comps"]], name
        hmax, vmax = inf.sampling[0]
        mx, my = -(-inf.w // (8 * hmax)), -(-inf.h // (8 * vmax))
        assert inf.blocks == [(mx * hs, my * vs) for hs, vs in inf.sampling], name
        assert inf.coef_bytes == sum(bw * bh for bw, bh in inf.blocks) * 128, name
        assert inf.restart_interval == J["restart"], name
    by_name = {n: d for n, d, _ in matrix}
    assert jpeg.info(by_name["37x53-ss2-restart3"]).restart_interval > 0
    assert jpeg.info(by_name["17x33-ss1-q90"]).sampling == [(2, 1), (1, 1), (1, 1)]
    assert jpeg.info(by_name["17x33-ss2-q90"]).blocks == [(6, 4), (3, 2), (3, 2)]
    assert jpeg.info(by_name["1x1-grey-q90"]).blocks == [(1, 1)]


def _save(img, fmt="JPEG", **kw):
    f = io.BytesIO()
    img.save(f, fmt, **kw)
    return f.getvalue()


def test_unsupported_streams():
    from styletransfer_amd import jpeg
    rgb = Image.fromarray(R.image(37, 53, 5))
    # a sampling outside the three: 4:2:2's luma factors 2x1 patched to 1x2 in the SOF0 header
    ss1 = bytearray(_save(rgb, subsampling=1))
    sof = ss1.index(b"\xff\xc0")
    assert ss1[sof + 11] == 0x21
    ss1[sof + 11] = 0x12
    for what, data in [("progressive", _save(rgb, progressive=True)),
                       ("cmyk", _save(rgb.convert("CMYK"))),
                       ("png", _save(rgb, "PNG")),
                       ("1x2 luma", bytes(ss1)),
                       ("no image", b"\x00\x01\x02\x03")]:
        assert jpeg.info(data).status == jpeg.UNSUPPORTED, what
        st, co = jpeg.try_entropy_decode(data)
        assert st == jpeg.UNSUPPORTED and co is None, what
        with pytest.raises(jpeg.JpegError) as e:
            jpeg.entropy_decode(data)
        assert e.value.status == jpeg.UNSUPPORTED
        # ... and the batch decoder's loader decodes such a file with PIL instead
        if what in ("progressive", "cmyk", "png"):
            item = jpeg.load_item(data)
            assert isinstance(item, np.ndarray), what
            assert np.array_equal(item, R.pil_decode(data)), what


CANARY = 64


def _guarded_decode(data, coef_bytes, ncomp):
    """stx_jpeg_entropy_decode into a buffer with canary bytes behind coef and qtab; the
    input is an exact-size copy, so a read past len would at least leave the array."""
    from styletransfer_amd import _native as N
    src = np.frombuffer(bytes(data), np.uint8).copy()
    coef = np.full(coef_bytes + CANARY, 0xA5, np.uint8)
    qtab = np.full(ncomp * 128 + CANARY, 0x5A, np.uint8)
    st = N.lib().stx_jpeg_entropy_decode(src.ctypes.data, src.size, coef.ctypes.data, coef_bytes,
                                         qtab.ctypes.data)
    assert np.all(coef[coef_bytes:] == 0xA5) and np.all(qtab[ncomp * 128:] == 0x5A)
    return st, coef[:coef_bytes].view(np.int16)


@pytest.mark.parametrize("case", ["37x53-ss2-q90", "37x53-ss1-restart3"])
def test_truncated_streams_are_corrupt(matrix, case):
    """One stream cut at every 7th byte length: CORRUPT (never a padded 'clean' decode of
    less than the whole scan), no crash, canaries intact."""
    from styletransfer_amd import jpeg
    data = {n: d for n, d, _ in matrix}[case]
    inf = jpeg.info(data)
    full_st, full = _guarded_decode(data, inf.coef_bytes, inf.ncomp)
    assert full_st == jpeg.OK
    for n in range(0, len(data), 7):
        cut = data[:n]
        st, _ = _guarded_decode(cut, inf.coef_bytes, inf.ncomp)
        assert st == jpeg.CORRUPT, (n, st)   # PIL raises on a truncated file: no zero padding
        assert jpeg.info(cut).status in (jpeg.OK, jpeg.CORRUPT), n
    # a buffer one block short is refused before anything is written
    st, _ = _guarded_decode(data, inf.coef_bytes - 128, inf.ncomp)
    assert st == jpeg.BAD_ARGS


@pytest.mark.parametrize("case", ["37x53-ss2-q90", "37x53-ss0-restart3", "37x53-ss1-optimize"])
def test_flipped_scan_bytes(matrix, case):
    """Single bytes of the scan flipped: CORRUPT or a clean decode, never a crash or a
    write past the buffer."""
    from styletransfer_amd import jpeg
    data = {n: d for n, d, _ in matrix}[case]
    inf = jpeg.info(data)
    sos = data.index(b"\xff\xda")
    scan = sos + 2 + ((data[sos + 2] << 8) | data[sos + 3])  # the entropy-coded bytes
    rng = np.random.default_rng(7)
    seen = set()
    for pos in range(scan, len(data)):
        b = bytearray(data)
        b[pos] ^= int(rng.integers(1, 256))
        st, _ = _guarded_decode(bytes(b), inf.coef_bytes, inf.ncomp)
        assert st in (jpeg.OK, jpeg.CORRUPT), (pos, st)
        seen.add(st)
    assert jpeg.OK in seen and jpeg.CORRUPT in seen


def test_jpeg_layout_matches_mirrors():
    """stx_jpeg_layout: (size, last-member offset) of the two JPEG structs == the ctypes
    mirrors (the older structs stay with stx_abi_layout)."""
    from styletransfer_amd import _native as N
    mirrors = [(N.JpegDesc, "coef_bytes"), (N.JpegJob, "bh")]
    count = N.lib().stx_jpeg_layout(None, 0)
    assert count == 2 * len(mirrors)
    out = (C.c_longlong * count)()
    assert N.lib().stx_jpeg_layout(C.cast(out, C.c_void_p), count) == count
    for i, (S, last) in enumerate(mirrors):
        assert S._fields_[-1][0] == last
        assert (C.sizeof(S), getattr(S, last).offset) == (out[2 * i], out[2 * i + 1]), S
    assert C.sizeof(N.JpegJob) * N.STX_JPEG_CHUNK <= 4096  # passed to the kernels by value


def test_collate_round_trips_a_mixed_batch(matrix, tmp_path):
    """CocoDataset(decode="coefs") + _coef_collate: coefficients, tables and raw pixels
    come back out of the one packed tensor exactly, at the offsets the job plan uses."""
    from styletransfer_amd import dataset, jpeg
    by_name = {n: d for n, d, _ in matrix}
    rgb = Image.fromarray(R.image(24, 40, 3))
    files = {"a.jpg": by_name["37x53-ss2-q90"], "b.jpg": by_name["17x33-grey-q90"],
             "c.jpg": _save(rgb, progressive=True), "d.png": _save(rgb, "PNG"),
             "e.jpg": by_name["37x53-ss1-restart3"], "f.jpg": by_name["16x16-ss0-q90"]}
    for n, d in files.items():
        (tmp_path / n).write_bytes(d)
    ds = dataset.CocoDataset(path=str(tmp_path), decode="coefs")
    assert ds.images == sorted(files)
    items = [ds[i] for i in range(len(ds))]
    kinds = [isinstance(it, jpeg.JpegCoefs) for it in items]
    assert kinds == [True, True, False, False, True, True]
    packed = dataset._coef_collate(items)
    assert packed.dtype.is_floating_point is False and packed.dim() == 1
    recs = jpeg.records(packed)
    jobs, shapes, rgb_bytes, tmp_bytes = jpeg.plan(recs)
    assert shapes == [(37, 53), (17, 33), (24, 40), (24, 40), (37, 53), (16, 16)]
    assert rgb_bytes == sum(h * w * 3 for h, w in shapes)
    pk, rgb_off, tmp_end = packed.numpy(), 0, 0
    for name, it, j, (h, w) in zip(ds.images, items, jobs, shapes):
        assert (j.h, j.w, j.rgb_offset) == (h, w, rgb_off)
        rgb_off += h * w * 3
        assert j.coef_offset % 16 == 0
        if isinstance(it, jpeg.JpegCoefs):
            assert not j.raw and j.ncomp == it.ncomp and (j.hmax, j.vmax) == it.sampling[0]
            assert [(j.bw[c], j.bh[c]) for c in range(it.ncomp)] == it.blocks
            n = it.coef.nbytes
            assert np.array_equal(pk[j.coef_offset:j.coef_offset + n].view(np.int16), it.coef)
            assert j.qtab_offset == j.coef_offset + n
            assert np.array_equal(pk[j.qtab_offset:j.qtab_offset + it.ncomp * 128]
                                  .view(np.uint16).reshape(-1, 64), it.qtab)
            assert j.tmp_offset % 16 == 0 and j.tmp_offset >= tmp_end
            tmp_end = j.tmp_offset + sum(bw * bh for bw, bh in it.blocks) * 64
        else:
            assert j.raw
            assert np.array_equal(pk[j.coef_offset:j.coef_offset + h * w * 3].reshape(h, w, 3),
                                  it)
            assert np.array_equal(it, R.pil_decode(files[name]))
    assert tmp_end <= tmp_bytes
    # a damaged header is refused on the host, before any offset reaches a kernel
    bad = packed.clone()
    bad.numpy()[8 * (1 + 12):8 * (1 + 13)].view(np.int64)[0] = packed.numel()  # image 0's offset
    with pytest.raises(ValueError):
        jpeg.records(bad)


def test_gpu_decode_is_opt_in():
    """The switch defaults to off everywhere, and asks for the GPU path it extends."""
    import inspect

    from styletransfer_amd import dataset
    sig = inspect.signature(dataset.get_coco_loader)
    assert sig.parameters["gpu_decode"].default is False
    assert inspect.signature(dataset.CocoDataset.__init__).parameters["decode"].default is None
    with pytest.raises(ValueError):
        dataset.CocoDataset(images=[], path=".", decode="pixels")


def test_cli_switch():
    """fast_st train / train-multi carry --gpu-decode; it selects the COCO loader with the
    switch on and refuses --synthetic, and without it static_train keeps its default."""
    import click
    from click.testing import CliRunner

    from styletransfer_amd.clis import fast_st as cli
    for cmd in ("train", "train-multi"):
        out = CliRunner().invoke(cli.fast_st, [cmd, "--help"])
        assert out.exit_code == 0 and "--gpu-decode" in out.output, cmd
    assert cli._loaders(4, 0, False) is None
    assert callable(cli._loaders(4, 8, False)) and callable(cli._loaders(4, 0, True))
    with pytest.raises(click.UsageError):
        cli._loaders(4, 8, True)
