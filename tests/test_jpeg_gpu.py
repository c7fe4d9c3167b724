"""The device half of the JPEG decode (csrc/jpeg.hip through styletransfer_amd/jpeg.py) on
the GPU: dequantisation + IDCT + range limit, fancy chroma upsampling and YCbCr -> RGB give
Pillow's pixels bit for bit -- image by image, as one mixed batch in one call, and through
get_coco_loader(gpu_decode=True).  The yardstick is PIL's decode of the same bytes on the
machine the test runs on; tolerance: none (integer arithmetic, every pixel equal)."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def matrix():
    """[(name, bytes, PIL's HxWx3 decode)], built once."""
    return [(name, data, R.pil_decode(data)) for name, data in R.cases()]


def _save(img, fmt="JPEG", **kw):
    f = io.BytesIO()
    img.save(f, fmt, **kw)
    return f.getvalue()


def _diff(got, want):
    d = np.abs(got.astype(int) - want.astype(int))
    return int(d.max()), int((d > 0).sum())


def test_decode_image_equals_pil(dev, matrix):
    from styletransfer_amd import jpeg
    bad = []
    for name, data, want in matrix:
        got = jpeg.decode_image(data, dev)
        assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == want.shape, name
        got = got.cpu().numpy()
        if not np.array_equal(got, want):
            bad.append((name,) + _diff(got, want))
    assert not bad, bad


def test_decode_image_from_a_path(dev, matrix, tmp_path):
    from styletransfer_amd import jpeg
    name, data, want = next(m for m in matrix if m[0] == "dancing.jpg")
    p = tmp_path / "x.jpg"
    p.write_bytes(data)
    assert np.array_equal(jpeg.decode_image(str(p), dev).cpu().numpy(), want)


def test_mixed_batch_in_one_call(dev, matrix):
    """The whole matrix plus a progressive file (decoded by PIL, riding raw) in one
    decode(): every image lands at its own offset with its own pixels, and the bytes
    between images are exactly the images (nothing written out of place)."""
    from styletransfer_amd import _native as N
    from styletransfer_amd import jpeg
    prog = _save(Image.fromarray(R.image(45, 70, 77)), progressive=True)
    assert jpeg.info(prog).status == jpeg.UNSUPPORTED
    items = [d for _, d, _ in matrix]
    wants = [w for _, _, w in matrix]
    k = len(items) // 2
    items.insert(k, prog)
    wants.insert(k, R.pil_decode(prog))
    assert len(items) > N.STX_JPEG_CHUNK  # more than one launch's worth of jobs
    rgb, shapes = jpeg.JpegBatchDecoder(dev).decode(items)
    assert shapes == [w.shape[:2] for w in wants]
    assert rgb.numel() == sum(w.size for w in wants)
    host, o, bad = rgb.cpu().numpy(), 0, []
    for i, w in enumerate(wants):
        got = host[o:o + w.size].reshape(w.shape)
        o += w.size
        if not np.array_equal(got, w):
            bad.append((i,) + _diff(got, w))
    assert not bad, bad


def test_inconsistent_jobs_are_refused(dev, matrix):
    """The entry point checks every job against its own geometry and the workspace before
    it launches: a wrong grid or a short workspace is an error, not a launch."""
    from styletransfer_amd import _native as N
    from styletransfer_amd import jpeg
    data = next(d for n, d, _ in matrix if n == "37x53-ss2-q90")
    packed = jpeg.pack([jpeg.entropy_decode(data)])
    jobs, shapes, rgb_bytes, tmp_bytes = jpeg.plan(jpeg.records(packed))
    dec = jpeg.JpegBatchDecoder(dev)
    dp = packed.to(dev)
    rgb = torch.zeros(rgb_bytes, dtype=torch.uint8, device=dev)
    tmp = torch.empty(tmp_bytes, dtype=torch.uint8, device=dev)
    with pytest.raises(N.NativeError):
        dec.launch(dp, jobs, 1, rgb, tmp[:tmp_bytes - 16])
    jobs[0].bw[0] += 2
    with pytest.raises(N.NativeError):
        dec.launch(dp, jobs, 1, rgb, tmp)
    jobs[0].bw[0] -= 2
    jobs[0].hmax = 1
    with pytest.raises(N.NativeError):
        dec.launch(dp, jobs, 1, rgb, tmp)
    torch.cuda.synchronize()
    assert int(rgb.max()) == 0  # nothing ran


def _img(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """test_gpu_conditioned_coco_loader's folder, plus a greyscale JPEG, a progressive JPEG
    and a PNG (the last two take the PIL path and ride raw)."""
    d = tmp_path_factory.mktemp("coco")
    for i, (h, w) in enumerate([(480, 640), (427, 640), (640, 480), (300, 300), (256, 400),
                                (612, 612), (375, 500), (500, 333)]):
        Image.fromarray(_img(h, w, 100 + i)).save(d / f"{i:03d}.jpg", quality=90)
    Image.fromarray(R.image(333, 500, 1)).convert("L").save(d / "008.jpg", quality=90)
    Image.fromarray(R.image(480, 360, 2)).save(d / "009.jpg", quality=85, progressive=True)
    Image.fromarray(R.image(300, 420, 3)).save(d / "010.png")
    Image.fromarray(R.image(400, 400, 4)).save(d / "011.jpg", quality=75, subsampling=1)
    return str(d)


def test_gpu_decode_coco_loader_equals_pil_loader(dev, folder):
    """get_coco_loader(gpu_decode=True) == the PIL loader, batch by batch."""
    from styletransfer_amd import dataset
    g_test, g_train = dataset.get_coco_loader(batch_size=4, test_split=0.25, path=folder,
                                              gpu_conditioning=True, gpu_decode=True,
                                              num_workers=2)
    c_test, c_train = dataset.get_coco_loader(batch_size=4, test_split=0.25, path=folder,
                                              gpu_conditioning=False)
    got, want = list(g_test) + list(g_train), list(c_test) + list(c_train)
    assert len(got) == len(want) == 4
    for a, b in zip(got, want):
        assert a.is_cuda and a.shape == b.shape
        assert torch.equal(a.cpu(), b.cpu())


def test_pipelined_loader_batches_repeat(dev, folder):
    """Successive batches share the side stream and the allocator's buffers (depth 2: batch
    k + 2 is decoded while batch k is consumed): two passes over the pipelined loader give
    the same batches, and each equals the loader that uploads PIL-decoded pixels."""
    from styletransfer_amd import dataset
    kw = dict(batch_size=3, test_split=0.25, path=folder, gpu_conditioning=True, num_workers=0)
    _, g_train = dataset.get_coco_loader(gpu_decode=True, **kw)
    _, p_train = dataset.get_coco_loader(**kw)
    first = [b.clone() for b in g_train]
    second = [b.clone() for b in g_train]
    want = [b.clone() for b in p_train]
    assert len(first) == len(second) == len(want) == 3
    for a, b, c in zip(first, second, want):
        assert torch.equal(a, c) and torch.equal(b, c)
