"""What does region-guided Gatys transfer cost over the plain one?

One GPU, one process, everything graph-replayed (device time, no launch gaps):

  kernels  ops.guided_style_loss at R = 1 (all-ones weights) against ops.style_loss on the
           same z at (1,64,512,512) and (1,256,128,128) -- both on the split path (z_amax
           given); a graph of --calls back-to-back calls of each, alternating, us per call.
           Also ops.guided_gram_bwd at R = 1, 2 against ops.gram_bwd (fp32 1x1 MFMA conv).
  engine   one replayed GuidedGatysEngine iteration at --size^2 with R = 1 and R = 2
           against one GatysEngine iteration, ms per iteration.

Each figure is timed over windows of --steps replays (after --warmup) with a device
synchronise around each window; --rounds rounds alternate the candidates and show the
spread ((max - min) / median).  Prints one JSON line, with the box's calibration (fp16
GEMM rate and copy bandwidth, as bench.py's `box` block) taken first in the same process.

    python tools/bench_guided.py [--size 512] [--steps 200] [--warmup 20] [--rounds 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from styletransfer_amd import ops  # noqa: E402
from styletransfer_amd import vgg as V  # noqa: E402
from styletransfer_amd import weights as W  # noqa: E402


def graph_of(fn, calls):
    """A captured graph of `calls` back-to-back fn() (after two eager calls)."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with ops.graph_capture(g):
        for _ in range(calls):
            fn()
    return g


def window(replay, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        replay()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def compare(cands, steps, warmup, rounds, unit):
    """cands: name -> replay callable.  Alternating windows; medians and spreads."""
    for r in cands.values():
        window(r, warmup)
    t = {k: [] for k in cands}
    for _ in range(rounds):
        for k, r in cands.items():
            t[k].append(window(r, steps) * unit)
    med = {k: statistics.median(v) for k, v in t.items()}
    return {"median": {k: round(v, 3) for k, v in med.items()},
            "spread": {k: round((max(v) - min(v)) / med[k], 4) for k, v in t.items()}}


def box_calibration(dev):
    """The box's own speed, as bench.py's `box` block measures it: a fixed fp16 GEMM
    (8192^3, torch.matmul, TF/s) and a 1 GiB device-to-device copy (read + write, GB/s),
    HIP events, best of 3 x 10."""
    def avg_ms(fn, reps=10):
        fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps
    n = 8192
    x = torch.randn(n, n, device=dev, dtype=torch.float16)
    y = torch.randn(n, n, device=dev, dtype=torch.float16)
    o = torch.empty(n, n, device=dev, dtype=torch.float16)
    mm = min(avg_ms(lambda: torch.matmul(x, y, out=o)) for _ in range(3))
    del x, y, o
    src = torch.ones(1 << 28, device=dev, dtype=torch.float32)
    dst = torch.empty_like(src)
    cp = min(avg_ms(lambda: dst.copy_(src)) for _ in range(3))
    nbytes = 2 * src.numel() * 4
    del src, dst
    return {"fp16_gemm_tflops": round(2.0 * n ** 3 / (mm * 1e-3) / 1e12, 1),
            "hbm_copy_gbs": round(nbytes / (cp * 1e-3) / 1e9, 1)}


def kernel_bench(shape, dev, a):
    b, c, h, w = shape
    hw = h * w
    z = torch.randn(shape, device=dev, generator=torch.Generator(dev).manual_seed(1))
    za = ops.amax(z)
    T = torch.zeros(1, c, c, device=dev)
    cp = ops.coef_pitch(c)
    out = {}
    cands = {}
    coef0 = torch.empty(b, cp, cp, device=dev)
    loss0 = torch.empty((), device=dev)
    cands["style_loss"] = graph_of(
        lambda: ops.style_loss(z, T[0], coef=coef0, loss=loss0, z_amax=za), a.calls).replay
    keep = []
    for R in (1, 2):
        wts = torch.ones(R, hw, device=dev)
        Tr = torch.zeros(R, c, c, device=dev)
        coef = torch.empty(b, R, cp, cp, device=dev)
        lr = torch.empty(R, device=dev)
        keep.append((wts, Tr, coef, lr))
        cands[f"guided_R{R}"] = graph_of(
            lambda wts=wts, Tr=Tr, coef=coef, lr=lr, R=R: ops.guided_style_loss(
                z, wts, Tr, [1.0] * R, z_amax=za, w_max=1.0, coef=coef, loss_r=lr), a.calls).replay
    r = compare(cands, a.steps // 4 + 1, a.warmup // 4 + 1, a.rounds, 1e6 / a.calls)
    r["ratio_R1_over_style_loss"] = round(r["median"]["guided_R1"] / r["median"]["style_loss"], 4)
    out["forward_us"] = r
    # backward: coef of the R = 1 / 2 forwards above; the plain one is stx_gram_bwd
    dz = torch.empty_like(z)
    cands = {"gram_bwd": graph_of(lambda: ops.gram_bwd(coef0, z, dz=dz), a.calls).replay}
    for R, (wts, Tr, coef, lr) in zip((1, 2), keep):
        ca = ops.amax(coef)
        cands[f"guided_R{R}"] = graph_of(
            lambda wts=wts, coef=coef, ca=ca: ops.guided_gram_bwd(
                coef, z, wts, dz=dz, z_amax=za, coef_amax=ca), a.calls).replay
    out["backward_us"] = compare(cands, a.steps // 4 + 1, a.warmup // 4 + 1, a.rounds,
                                 1e6 / a.calls)
    return out


def engine_bench(dev, a):
    H = a.size
    feat = V.VGGFeatures(W.vgg19_synthetic(1234, 5), dev)
    img = lambda seed: torch.from_numpy(W.synthetic_image(seed, (1, 3, H, H)))  # noqa: E731
    content, s0, s1 = img(12), img(11), img(13)
    left = torch.zeros(H, H)
    left[:, :H // 2] = 1
    engines = {
        "gatys": V.GatysEngine(feat, s0, content),
        "guided_R1": V.GuidedGatysEngine(feat, [s0], content, torch.ones(1, H, H)),
        "guided_R2": V.GuidedGatysEngine(feat, [s0, s1], content, torch.stack([left, 1 - left])),
    }
    for e in engines.values():
        e.capture(warmup=2)
    r = compare({k: e.graph.replay for k, e in engines.items()}, a.steps, a.warmup, a.rounds, 1e3)
    for k in ("guided_R1", "guided_R2"):
        r[f"ratio_{k}_over_gatys"] = round(r["median"][k] / r["median"]["gatys"], 4)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20, help="kernel calls per captured graph")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_guided: needs a GPU (there is no CPU path to time)")
    dev = torch.device("cuda", 0)
    res = {"steps": a.steps, "rounds": a.rounds, "calls_per_graph": a.calls,
           "box": box_calibration(dev), "kernels": {}}
    for shape in ((1, 64, 512, 512), (1, 256, 128, 128)):
        res["kernels"]["x".join(map(str, shape))] = kernel_bench(shape, dev, a)
    res["engine_ms"] = engine_bench(dev, a)
    res["size"] = a.size
    print(json.dumps(res))


if __name__ == "__main__":
    main()
