"""The device half of the JPEG encode (csrc/jpeg.hip stx_jpeg_encode_batch, jpeg.py
JpegBatchEncoder) and the video paths built on it: the files equal Pillow's byte for byte
(quality, subsampling, optimize=False) for the same pixels."""
import ctypes as C
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_enc_ref as E
import jpeg_ref as R

pytestmark = pytest.mark.gpu

MEAN = np.array([0.485, 0.456, 0.406], np.float32).reshape(3, 1, 1)
STD = np.array([0.229, 0.224, 0.225], np.float32).reshape(3, 1, 1)


@pytest.fixture(scope="module")
def colour():
    return [(n, a, ss, q, E.pil_jpeg(a, q, ss)) for n, a, ss, q in E.color_cases()]


@pytest.fixture(scope="module")
def extra():
    """Greyscale and the two photographs."""
    out = [(n, a, "4:2:0", q, E.pil_jpeg(a, q)) for n, a, q in E.grey_cases()]
    return out + [(n, a, ss, q, E.pil_jpeg(a, q, ss)) for n, a, ss, q in E.photo_cases()]


def test_encode_image_equals_pillow(dev, colour, extra):
    """1x1; 8x8 at 4:2:0 (a chroma block half replicated rows); 24x40 (the bottom rule and
    right-edge dummy blocks); 50x100 (both kinds of dummy blocks); every sampling, four
    qualities, gradient and noise; grey; two photographs."""
    from styletransfer_amd import jpeg
    assert len(colour) == 264
    bad = []
    for name, a, ss, q, want in colour + extra:
        got = jpeg.encode_image(torch.from_numpy(a).to(dev), q, ss)
        if got != want:
            bad.append(name)
    assert not bad, (len(bad), bad[:10])


def test_one_mixed_batch_crosses_the_chunk_and_stays_in_bounds(dev, colour, extra):
    from styletransfer_amd import _native as N
    from styletransfer_amd import jpeg
    picks = [c for c in colour if c[3] == 90][::2] + [e for e in extra if e[3] == 90][:8]
    assert len(picks) >= 40 > N.STX_JPEG_CHUNK
    assert {c[2] for c in picks} == {"4:4:4", "4:2:2", "4:2:0"}
    assert {c[1].ndim for c in picks} == {2, 3}
    enc = jpeg.JpegBatchEncoder(dev)
    # encode() takes one sampling per call: the mixed batch goes through the C entry point
    plans = [jpeg._EncPlan([torch.from_numpy(a).to(dev)], jpeg.SAMPLINGS[ss], enc.mean, enc.std)
             for _, a, ss, _, _ in picks]
    jobs = (N.JpegEncJob * len(picks))()
    src_off, coef_off, tmp_off, srcs, meta = 0, 256, 0, [], []
    for i, p in enumerate(plans):
        C.memmove(C.byref(jobs[i]), C.byref(p.jobs[0]), C.sizeof(N.JpegEncJob))
        jobs[i].src_offset, jobs[i].coef_offset, jobs[i].tmp_offset = src_off, coef_off, tmp_off
        h, w, ncomp, hmax, vmax, _, nbytes = p.meta[0]
        meta.append((h, w, ncomp, hmax, vmax, coef_off, nbytes))
        srcs.append((src_off, p.srcs[0][1]))
        src_off = jpeg._align16(src_off + p.srcs[0][1].numel())
        coef_off = jpeg._align16(coef_off + nbytes)
        tmp_off = jpeg._align16(tmp_off + nbytes // 2)
    PAD = 4096
    src = torch.zeros(src_off + 16, dtype=torch.uint8, device=dev)
    for off, t in srcs:
        src[off:off + t.numel()] = t.reshape(-1)
    coef = torch.full((coef_off + PAD,), 0xA5, dtype=torch.uint8, device=dev)
    tmp = torch.full((tmp_off + PAD,), 0xA5, dtype=torch.uint8, device=dev)
    qhost, qdev = enc._tables(90)
    coef[:256] = qdev
    N.check(N.lib().stx_jpeg_encode_batch(jobs, len(picks), src.data_ptr(), coef.data_ptr(),
                                          tmp.data_ptr(), tmp_off,
                                          torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize(dev)
    assert bool((coef[coef_off:] == 0xA5).all()) and bool((tmp[tmp_off:] == 0xA5).all())
    host = coef.cpu().numpy()
    for (name, a, ss, q, want), (h, w, ncomp, hmax, vmax, off, nbytes) in zip(picks, meta):
        got = jpeg.entropy_encode(host[off:off + nbytes].view(np.int16), h, w, ncomp, hmax, vmax,
                                  qhost if ncomp == 1 else qhost[[0, 1, 1]])
        assert got == want, name
    # the workspace check: one byte short is refused before anything is launched
    rc = N.lib().stx_jpeg_encode_batch(jobs, len(picks), src.data_ptr(), coef.data_ptr(),
                                       tmp.data_ptr(), tmp_off - 1,
                                       torch.cuda.current_stream(dev).cuda_stream)
    assert rc != 0
    # and the batch interface: same-sampling frames of mixed sizes, past one chunk
    same = [c for c in colour if c[2] == "4:2:0" and c[3] == 50][:22] * 2
    files = enc.encode([torch.from_numpy(c[1]).to(dev) for c in same], 50, "4:2:0")
    assert len(files) == 44 and files == [c[4] for c in same]
    enc.close()


def _normalised(a):
    """HxWx3 uint8 -> the float32 [3, h, w] tensor whose to_pil bytes are a's (checked)."""
    from styletransfer_amd import img_utils
    t = torch.from_numpy(((a.transpose(2, 0, 1).astype(np.float32) / 255 - MEAN) / STD))
    return t, np.asarray(img_utils.to_pil(t))


def test_fp32_front_end(dev):
    from styletransfer_amd import jpeg
    for i, (h, w) in enumerate([(1, 1), (24, 40), (50, 100), (33, 47)]):
        t, back = _normalised(R.image(h, w, 300 + i, noise=bool(i & 1)))
        for ss in E.SAMPLINGS:
            want = E.pil_jpeg(back, 90, ss)              # Image.save(to_pil(t))
            assert jpeg.encode_image(t.to(dev), 90, ss) == want, (h, w, ss)
            assert jpeg.encode_image(t.to(dev)[None], 90, ss) == want
    # out of range: far above 1 saturates at 255 (to_pil wraps there), below 0 gives 0, NaN 0
    t, _ = _normalised(R.image(24, 40, 310))
    t = t.clone()
    t[:, :8] = 50.0
    t[:, 8:12] = -50.0
    t[0, 12, :5] = 1e30
    t[1, 13, :5] = float("nan")
    v = np.clip(t.numpy() * STD + MEAN, 0, 255)          # two float32 roundings
    v = np.where(np.isnan(v), np.float32(0), v)
    rule = np.minimum((v * np.float32(255)).astype(np.int64), 255).astype(np.uint8)
    assert rule[:, :8].min() == 255 and rule[:, 8:12].max() == 0
    want = E.pil_jpeg(np.ascontiguousarray(rule.transpose(1, 2, 0)), 90, "4:2:0")
    assert jpeg.encode_image(t.to(dev), 90, "4:2:0") == want


def test_submit_collect_equals_encode(dev):
    from styletransfer_amd import jpeg
    frames = [R.image(40, 56, 400 + i, noise=i == 3) for i in range(8)]
    want = [E.pil_jpeg(a, 90, "4:2:0") for a in frames]
    dframes = [torch.from_numpy(a).to(dev) for a in frames]
    with jpeg.JpegBatchEncoder(dev) as enc:
        assert enc.encode(dframes) == want
        got = []
        for i, f in enumerate(dframes):       # at most two batches in flight
            enc.submit([f])
            if i >= 1:
                got += enc.collect()
        got += enc.collect()
        assert got == want
        with pytest.raises(RuntimeError):
            enc.collect()
        for f in dframes[:3]:                  # three outstanding: the third waits for slot 0
            enc.submit([f, f])
        assert [enc.collect() for _ in range(3)] == [[w, w] for w in want[:3]]
    assert enc._thread is None


@pytest.fixture(scope="module")
def video_net():
    """A VideoTransformNet with synthetic weights whose last convolution is scaled down, so
    that the stylised frames stay inside [0, 1] after de-normalisation: there the encoder's
    bytes and to_pil's are the same by the stated rule (the saturating case is
    test_fp32_front_end's)."""
    from styletransfer_amd import network
    from styletransfer_amd import weights as W
    sd = {k: torch.from_numpy(v) for k, v in W.itn_synthetic(777, in_channels=6)}
    sd["22.weight"] = sd["22.weight"] * 0.1
    sd["22.bias"] = sd["22.bias"] * 0.1
    net = network.VideoTransformNet(torch.rand([3, 64, 64]))
    net.load_state_dict(sd)
    return net


def _clip(n=6, h=40, w=48):
    rng = np.random.default_rng(11)
    base = rng.integers(0, 256, (h, w + 4 * n, 3), dtype=np.uint8)
    return np.stack([base[:, 4 * t:4 * t + w] for t in range(n)])   # a panning clip


def test_process_video_mjpeg_and_avi_input(dev, tmp_path, monkeypatch, video_net):
    from styletransfer_amd import constants, img_utils, jpeg, video, video_io
    monkeypatch.setattr(constants, "IMSIZE", 64)
    arr = _clip()
    src = tmp_path / "clip.npy"
    np.save(src, arr)
    wd, out = str(tmp_path / "wd") + "/", str(tmp_path / "out") + "/"
    # the default path: PNG frames, the bytes of the PIL-conditioned recurrence
    ret = video.process_video(video_net, str(src), working_dir=wd, out_dir=out)
    assert ret == wd
    eng = video.FrameEngine(video_net, (1, 3, 64, 64), dev, graph=False)
    pngs = []
    for i, f in enumerate(video.iterate_frames(arr, imsize=64)):
        y = eng.step(f)[0].cpu()
        v = (y * torch.from_numpy(STD) + torch.from_numpy(MEAN)).clamp(0, 255) * 255
        assert float(v.max()) < 256, "the fixture keeps the frames in to_pil's exact range"
        b = io.BytesIO()
        img_utils.to_pil(y).save(b, "PNG")
        pngs.append(open(os.path.join(wd, f"{i}.png"), "rb").read())
        assert pngs[-1] == b.getvalue(), i
    assert sorted(os.listdir(wd)) == sorted(f"{i}.png" for i in range(6))
    # mjpeg: one .avi, no PNG, no working_dir frames
    wd2 = str(tmp_path / "wd2") + "/"
    avi = video.process_video(video_net, str(src), "nsp", wd2, out, fps=12.5, format="mjpeg")
    assert avi == os.path.join(out, "video_st_nsp.avi") and not os.path.exists(wd2)
    assert os.listdir(out) == ["video_st_nsp.avi"]
    fps, h, w, it = video_io.read_mjpeg_avi(avi)
    frames = list(it)
    assert (fps, h, w, len(frames)) == (12.5, 64, 64, 6)
    for i, (f, png) in enumerate(zip(frames, pngs)):
        a = np.asarray(Image.open(io.BytesIO(png)).convert("RGB"))
        assert f == E.pil_jpeg(a, 90, "4:2:0"), i
    avi2 = video.process_video(video_net, str(src), "q50", wd2, out, format="mjpeg", quality=50,
                               subsampling="4:4:4")
    for i, (f, png) in enumerate(zip(video_io.read_mjpeg_avi(avi2)[3], pngs)):
        a = np.asarray(Image.open(io.BytesIO(png)).convert("RGB"))
        assert f == E.pil_jpeg(a, 50, "4:4:4"), i
    with pytest.raises(ValueError):
        video.process_video(video_net, str(src), working_dir=wd2, out_dir=out, format="webm")
    # that AVI as the input: device-decoded frames are PIL's, and the transfer of the .avi
    # equals the transfer of the .npy of those decoded frames
    decoded = np.stack([R.pil_decode(f) for f in frames])
    got = [t.cpu().numpy() for t in video.iterate_device_frames(avi, dev)]
    assert len(got) == 6 and all(np.array_equal(g, d) for g, d in zip(got, decoded))
    assert all(np.array_equal(g, d) for g, d in zip(video.iterate_raw_frames(avi), decoded))
    np.save(tmp_path / "decoded.npy", decoded)
    a1 = video.process_video(video_net, avi, "from_avi", wd2, out, format="mjpeg")
    a2 = video.process_video(video_net, str(tmp_path / "decoded.npy"), "from_npy", wd2, out,
                             format="mjpeg")
    assert list(video_io.read_mjpeg_avi(a1)[3]) == list(video_io.read_mjpeg_avi(a2)[3])
    wd3 = str(tmp_path / "wd3") + "/"
    video.process_video(video_net, avi, working_dir=wd3, out_dir=out)
    video.process_video(video_net, str(tmp_path / "decoded.npy"), working_dir=wd2, out_dir=out)
    for i in range(6):
        assert open(wd3 + f"{i}.png", "rb").read() == open(wd2 + f"{i}.png", "rb").read(), i
    assert jpeg.info(frames[0]).sampling[0] == (2, 2)
