"""What do the AdaIN kernels cost, against the InstanceNorm forward at the same shape?

Per kernel: stx_chan_stats, stx_adain, stx_stats_loss, stx_stats_loss_bwd and the yardstick
stx_instnorm_fwd (the same traffic as stx_adain: read x, write y; twice what the two
statistics kernels read) at the training taps (B = 8 at 256^2: 64 x 256^2, 128 x 128^2,
256 x 64^2, 512 x 32^2) and at the 512^2 conversion shape (B = 1: 512 x 64^2).  Each
candidate is a captured graph of --calls back-to-back calls, the candidates alternate inside
each of --rounds rounds of windows of --steps replays with a device synchronise around each
window; medians in us per call and each candidate's spread ((max - min) / median).

End to end: images/s of AdaINNet.forward at 512^2 (style statistics given) and eager steps/s
of AdaINTrainer.step at B = 8, 256^2.

Prints one JSON line, with the box's calibration (bench.py's `box` block) taken first.

    python tools/bench_adain.py [--calls 20] [--steps 20] [--warmup 5] [--rounds 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_guided import box_calibration, compare, graph_of  # noqa: E402
from styletransfer_amd import _native as N  # noqa: E402
from styletransfer_amd import adain as M  # noqa: E402
from styletransfer_amd import ops  # noqa: E402
from styletransfer_amd import weights as W  # noqa: E402

TRAIN_TAPS = [(8, 64, 256), (8, 128, 128), (8, 256, 64), (8, 512, 32)]
CONVERT_TAPS = [(1, 512, 64)]


def kernel_bench(shape, dev, a):
    n, c, side = shape
    g = torch.Generator(dev).manual_seed(1)
    x = torch.randn(n, c, side, side, device=dev, generator=g)
    y = torch.empty_like(x)
    dx = torch.empty_like(x)
    gamma, beta = torch.ones(c, device=dev), torch.zeros(c, device=dev)
    smean, sstd = torch.randn(n, c, device=dev, generator=g), torch.rand(n, c, device=dev,
                                                                        generator=g) + 0.5
    mix = torch.eye(n, device=dev)
    tm, ts = smean.clone(), sstd.clone()
    out = torch.empty(3, device=dev)
    am = torch.zeros(N.STX_AMAX_SLOTS, device=dev)
    _, mean, std = ops.stats_loss(x, tm, ts)
    cands = {
        "instnorm_fwd": lambda: ops.instnorm_fwd(x, gamma, beta, out=y, out_amax=am),
        "chan_stats": lambda: ops.chan_stats(x),
        "adain": lambda: ops.adain(x, smean, sstd, mix, 1.0, out=y, out_amax=am),
        "stats_loss": lambda: ops.stats_loss(x, tm, ts, out=out),
        "stats_loss_bwd": lambda: ops.stats_loss_bwd(x, mean, std, tm, ts, dx=dx, out_amax=am),
        "stats_loss_bwd_acc": lambda: ops.stats_loss_bwd(x, mean, std, tm, ts, dx=dx,
                                                         accumulate=True, out_amax=am),
    }
    graphs = {k: graph_of(f, a.calls).replay for k, f in cands.items()}
    r = compare(graphs, a.steps, a.warmup, a.rounds, 1e6 / a.calls)
    base = r["median"]["instnorm_fwd"]
    r["ratio_to_instnorm_fwd"] = {k: round(v / base, 3) for k, v in r["median"].items()}
    r["mbytes_x"] = round(x.numel() * 4 / 1e6, 2)
    return r


def rate(fn, steps, warmup, rounds):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        t.append(steps / (time.perf_counter() - t0))
    med = statistics.median(t)
    return {"median_per_s": round(med, 2), "spread": round((max(t) - min(t)) / med, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20, help="calls per captured graph")
    ap.add_argument("--steps", type=int, default=20, help="graph replays per window")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--e2e-steps", type=int, default=10)
    ap.add_argument("--no-box", action="store_true", help="skip the box calibration")
    ap.add_argument("--no-e2e", action="store_true", help="kernels only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_adain: needs a GPU (there is no CPU path to time)")
    dev = torch.device("cuda", 0)
    res = {"calls": a.calls, "steps": a.steps, "rounds": a.rounds,
           "box": None if a.no_box else box_calibration(dev), "unit": "us per call",
           "train_taps": {}, "convert_taps": {}}
    for key, shapes in (("train_taps", TRAIN_TAPS), ("convert_taps", CONVERT_TAPS)):
        for s in shapes:
            res[key]["%dx%dx%d^2" % s] = kernel_bench(s, dev, a)
    if not a.no_e2e:
        net = M.AdaINNet(decoder_seed=11)
        img = torch.from_numpy(W.synthetic_image(1, (1, 3, 512, 512))).to(dev)
        stats = net.style_stats(torch.from_numpy(W.synthetic_image(2, (1, 3, 512, 512))).to(dev))
        res["convert_512_images_per_s"] = rate(lambda: net.convert(img, stats), a.e2e_steps, 2,
                                               a.rounds)
        tr = M.AdaINTrainer(net)
        cb = torch.from_numpy(W.synthetic_image(3, (8, 3, 256, 256))).to(dev)
        sb = torch.from_numpy(W.synthetic_image(4, (8, 3, 256, 256))).to(dev)
        res["train_b8_256_steps_per_s"] = rate(lambda: tr.step(cb, sb), a.e2e_steps, 2, a.rounds)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
