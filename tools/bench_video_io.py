"""Measurements of the video output path: results to one JSON file.

    python tools/bench_video_io.py cpu                     # host entropy coder vs Pillow
    python tools/bench_video_io.py gpu                     # stx_jpeg_encode_batch by HIP events
    python tools/bench_video_io.py e2e [--parent DIR]      # process_video / gatys_video fps

cpu (no GPU needed, one thread): stx_jpeg_entropy_encode ms per frame at 256x256, 512x512 and
1920x1080 against Pillow's save as JPEG (same quality and subsampling) and as PNG.
gpu: the two kernels of one frame, back-to-back calls between two events, several rounds
(median, min, max), with the bytes read and written.
e2e: frames per second of video.process_video on a synthetic clip with PNG output, MJPEG
output (pipelined and synchronous) and no output, and of video.gatys_video likewise.  With
--parent DIR (a built checkout of the parent commit) the PNG figure is measured alternately
in that tree and in this one, each run a fresh process, and the scatter is reported.

--out FILE merges the section into FILE (default profiles/video_io_bench.json)."""
import argparse
import io
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(256, 256), (512, 512), (1080, 1920)]


def frame(h, w, seed=0):
    """A photograph-like frame: smooth structure plus mild noise."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    base = np.stack([np.sin(x / 37) * 80 + np.cos(y / 23) * 60 + 128,
                     np.sin((x + y) / 51) * 100 + 128, np.cos(x / 17) * np.sin(y / 29) * 90 + 128], 2)
    return np.clip(base + rng.normal(0, 6, (h, w, 3)), 0, 255).astype(np.uint8)


def med_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "reps": reps}


def bench_cpu(args):
    import torch
    from PIL import Image
    from styletransfer_amd import jpeg
    torch.set_num_threads(1)
    out = {}
    for h, w in SIZES:
        a = frame(h, w)
        img = Image.fromarray(a)

        def save(fmt, **kw):
            b = io.BytesIO()
            img.save(b, fmt, **kw)
            return b.getvalue()

        data = save("JPEG", quality=90, subsampling=2)
        co = jpeg.entropy_decode(data)
        buf = np.empty(jpeg.encode_bound(h, w, 3, 2, 2), np.uint8)
        st, again = jpeg.try_entropy_encode(co.coef, h, w, 3, 2, 2, co.qtab, buf)
        assert st == jpeg.OK and again == data
        reps = 30 if h < 1000 else 8
        out[f"{h}x{w}"] = {
            "jpeg_bytes": len(data),
            "stx_jpeg_entropy_encode": med_ms(
                lambda: jpeg.try_entropy_encode(co.coef, h, w, 3, 2, 2, co.qtab, buf), reps),
            "pillow_jpeg_q90_420": med_ms(lambda: save("JPEG", quality=90, subsampling=2), reps),
            "pillow_png": med_ms(lambda: save("PNG"), max(reps // 4, 3)),
        }
    return out


def bench_gpu(args):
    import torch
    from styletransfer_amd import _native as N
    from styletransfer_amd import jpeg
    dev = torch.device("cuda", 0)
    enc = jpeg.JpegBatchEncoder(dev)
    out = {"device": torch.cuda.get_device_name(0)}
    for h, w in SIZES:
        a = torch.from_numpy(frame(h, w)).to(dev)
        f32 = torch.randn(3, h, w, device=dev)
        for name, src in (("uint8", a), ("fp32", f32)):
            plan = jpeg._EncPlan([src], (2, 2), enc.mean, enc.std)
            coef = torch.empty(plan.coef_bytes, dtype=torch.uint8, device=dev)
            tmp = torch.empty(plan.tmp_bytes, dtype=torch.uint8, device=dev)
            coef[:256] = enc._tables(90)[1]
            st = torch.cuda.current_stream(dev).cuda_stream

            def call():
                N.check(N.lib().stx_jpeg_encode_batch(plan.jobs, 1, src.data_ptr(), coef.data_ptr(),
                                                      tmp.data_ptr(), plan.tmp_bytes, st))
            for _ in range(10):
                call()
            torch.cuda.synchronize()
            rounds, calls = [], 50
            for _ in range(7):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls):
                    call()
                e1.record()
                e1.synchronize()
                rounds.append(e0.elapsed_time(e1) * 1e3 / calls)
            out[f"{h}x{w}-{name}"] = {
                "us_per_frame_median": statistics.median(rounds), "us_min": min(rounds),
                "us_max": max(rounds), "rounds": len(rounds), "calls_per_round": calls,
                "bytes_in": src.numel() * src.element_size(),
                "bytes_planes": plan.tmp_bytes, "bytes_out": plan.coef_bytes - 256}
        # the whole encode of one frame, host stage included
        y = f32[None]
        for mode in ("encode", "submit_collect"):
            def run(n=20):
                if mode == "encode":
                    for _ in range(n):
                        enc.encode([y])
                else:
                    enc.submit([y])
                    for _ in range(n - 1):
                        enc.submit([y])
                        enc.collect()
                    enc.collect()
            run(5)
            torch.cuda.synchronize()
            ts = []
            for _ in range(5):
                t = time.perf_counter()
                run()
                ts.append((time.perf_counter() - t) * 1e3 / 20)
            out[f"{h}x{w}-fp32-{mode}"] = {"ms_per_frame_median": statistics.median(ts),
                                           "ms_min": min(ts), "ms_max": max(ts)}
    enc.close()
    return out


def _video_net():
    import torch
    from styletransfer_amd import network
    from styletransfer_amd import weights as W
    sd = {k: torch.from_numpy(v) for k, v in W.itn_synthetic(777, in_channels=6)}
    net = network.VideoTransformNet(torch.rand([3, 64, 64]))
    net.load_state_dict(sd)
    return net


def _clip(n, h=360, w=640):
    base = frame(h, w + 4 * n)
    return np.stack([base[:, 4 * t:4 * t + w] for t in range(n)])


def e2e_png(args):
    """One fresh-process measurement of process_video with PNG output (any tree that has
    video.process_video: run with cwd = the tree)."""
    import tempfile

    import torch
    from styletransfer_amd import video
    net, clip = _video_net(), _clip(args.frames)
    with tempfile.TemporaryDirectory() as d:
        video.process_video(net, clip[:4], working_dir=d + "/w0/", out_dir=d + "/o/")   # warm
        torch.cuda.synchronize()
        t = time.perf_counter()
        video.process_video(net, clip, working_dir=d + "/w/", out_dir=d + "/o/")
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
    print(json.dumps({"png_fps": args.frames / dt}))


def bench_e2e(args):
    import tempfile

    import torch
    from styletransfer_amd import constants, img_utils, video
    from styletransfer_amd import vgg as V
    out = {"frames": args.frames, "imsize": constants.IMSIZE}
    net, clip = _video_net(), _clip(args.frames)

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return args.frames / (time.perf_counter() - t)

    with tempfile.TemporaryDirectory() as d:
        def png():
            video.process_video(net, clip, working_dir=d + "/w/", out_dir=d + "/o/")

        def mjpeg():
            video.process_video(net, clip, "b", d + "/w2/", d + "/o/", format="mjpeg")

        def mjpeg_sync():
            eng = video.FrameEngine(net, (1, 3, constants.IMSIZE, constants.IMSIZE),
                                    constants.DEVICE, raw_hw=clip.shape[1:3])
            from styletransfer_amd import jpeg, video_io
            enc = jpeg.JpegBatchEncoder(constants.DEVICE)
            with video_io.MjpegAviWriter(d + "/sync.avi", 24, constants.IMSIZE,
                                         constants.IMSIZE) as wr:
                for f in clip:
                    wr.write(enc.encode([eng.step_raw(f)])[0])

        def none():
            eng = video.FrameEngine(net, (1, 3, constants.IMSIZE, constants.IMSIZE),
                                    constants.DEVICE, raw_hw=clip.shape[1:3])
            for f in clip:
                eng.step_raw(f)

        for name, fn in (("png", png), ("mjpeg", mjpeg), ("mjpeg_sync", mjpeg_sync),
                         ("none", none)):
            fn()
            out[f"convert_video_{name}_fps"] = [timed(fn) for _ in range(3)]

        # gatys_video: a short clip at the working size, few steps per frame
        feat = V.VGGFeatures(V.load_vgg19_weights(), torch.device(constants.DEVICE))
        if args.gatys_frames:
            gframes = list(video.iterate_frames(clip[:args.gatys_frames]))
            style = gframes[0]

            def gatys(sink):
                n = 0
                for y in video.gatys_video(feat, gframes, style, "static", args.gatys_steps):
                    if sink == "png":
                        img_utils.imshow(y[0], path=f"{d}/g{n}.png")
                    elif sink is not None:
                        sink.write(y)
                    n += 1
                if sink not in (None, "png"):
                    sink.close()
            for name in ("png", "mjpeg", "none"):
                def fn():
                    gatys(video.MjpegSink(d + "/g.avi", device=constants.DEVICE)
                          if name == "mjpeg" else (None if name == "none" else "png"))
                fn()
                out[f"gatys_video_{name}_fps"] = [
                    v * args.gatys_frames / args.frames for v in (timed(fn) for _ in range(2))]
            out["gatys_frames"], out["gatys_steps"] = args.gatys_frames, args.gatys_steps

    if args.parent:
        runs = {"parent": [], "branch": []}
        for _ in range(args.ab_rounds):
            for name, tree in (("parent", args.parent), ("branch", REPO)):
                env = dict(os.environ, PYTHONPATH=tree)
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "e2e-png",
                                    "--frames", str(args.frames)], cwd=tree, env=env,
                                   capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    raise RuntimeError(f"{name}: {r.stderr[-2000:]}")
                runs[name].append(json.loads(r.stdout.strip().splitlines()[-1])["png_fps"])
        out["png_fps_parent_vs_branch"] = {
            **runs, "parent_median": statistics.median(runs["parent"]),
            "branch_median": statistics.median(runs["branch"]),
            "parent_spread": max(runs["parent"]) - min(runs["parent"]),
            "branch_spread": max(runs["branch"]) - min(runs["branch"])}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("section", choices=["cpu", "gpu", "e2e", "e2e-png"])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "video_io_bench.json"))
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--gatys-frames", type=int, default=4)
    ap.add_argument("--gatys-steps", type=int, default=20)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--ab-rounds", type=int, default=3)
    args = ap.parse_args()
    if args.section == "e2e-png":
        sys.path.insert(0, os.getcwd())
        return e2e_png(args)
    sys.path.insert(0, REPO)
    res = {"cpu": bench_cpu, "gpu": bench_gpu, "e2e": bench_e2e}[args.section](args)
    doc = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            doc = json.load(f)
    doc[args.section] = res
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
