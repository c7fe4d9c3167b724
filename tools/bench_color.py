"""What do the colour-control kernels cost, and what does --preserve-color add to a frame?

One GPU, one process, everything graph-replayed (device time, no launch gaps):

  stats    ops.color_stats of one image at 512^2 and 1080^2 against torch's copy_ of the
           same tensor (the calibration copy: it reads the same 12 h w bytes and writes
           them too); a graph of --calls back-to-back calls of each, alternating, us per
           call, and the bytes each moves per second.
  affine   ops.color_affine without base (the recolouring / luminance image: reads x,
           writes out) and with base and clamp (the luminance merge: reads x and base)
           against copy_ of the same tensor, same sizes.
  engine   one replayed video.FrameEngine frame at --size^2 with and without
           preserve_color (the merge takes the place of the output copy), ms per frame.

Each figure is timed over windows of --steps replays (after --warmup) with a device
synchronise around each window; --rounds rounds alternate the candidates and show the
spread ((max - min) / median).  Prints one JSON line, with the box's calibration (fp16
GEMM rate and copy bandwidth, as bench.py's `box` block) taken first in the same process.

    python tools/bench_color.py [--size 256] [--steps 200] [--warmup 20] [--rounds 5]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_guided import box_calibration, compare, graph_of  # noqa: E402
from styletransfer_amd import network, ops, video  # noqa: E402
from styletransfer_amd import weights as W  # noqa: E402

SIZES = ((512, 512), (1080, 1080))


def _rates(r, moved):
    """GB/s of each candidate from its median us per call and the bytes it moves."""
    r["gbs"] = {k: round(moved[k] / (v * 1e-6) / 1e9, 1) for k, v in r["median"].items()}
    return r


def stats_bench(dev, a):
    out = {}
    for h, w in SIZES:
        x = torch.randn(1, 3, h, w, device=dev, generator=torch.Generator(dev).manual_seed(1))
        st = torch.empty(1, 9, device=dev, dtype=torch.float64)
        dst = torch.empty_like(x)
        cands = {"color_stats": graph_of(lambda: ops.color_stats(x, out=st), a.calls).replay,
                 "copy": graph_of(lambda: dst.copy_(x), a.calls).replay}
        r = compare(cands, a.steps // 4 + 1, a.warmup // 4 + 1, a.rounds, 1e6 / a.calls)
        out[f"{h}x{w}"] = _rates(r, {"color_stats": 12 * h * w, "copy": 24 * h * w})
    return out


def affine_bench(dev, a):
    from styletransfer_amd import color
    M, (lo, hi) = color.merge_matrix(), color.gamut_bounds()
    out = {}
    for h, w in SIZES:
        g = torch.Generator(dev).manual_seed(2)
        x = torch.randn(1, 3, h, w, device=dev, generator=g)
        base = torch.randn(1, 3, h, w, device=dev, generator=g)
        dst = torch.empty_like(x)
        cands = {
            "affine": graph_of(lambda: ops.color_affine(x, M, b=lo, out=dst), a.calls).replay,
            "affine_base_clamp": graph_of(
                lambda: ops.color_affine(x, M, None, base=base, lo=lo, hi=hi, out=dst),
                a.calls).replay,
            "copy": graph_of(lambda: dst.copy_(x), a.calls).replay,
        }
        r = compare(cands, a.steps // 4 + 1, a.warmup // 4 + 1, a.rounds, 1e6 / a.calls)
        n = 12 * h * w
        out[f"{h}x{w}"] = _rates(r, {"affine": 2 * n, "affine_base_clamp": 3 * n, "copy": 2 * n})
    return out


def engine_bench(dev, a):
    """The flag is tried only where FrameEngine has it, so the same tool times the plain
    replay of a tree from before the switch."""
    H = a.size
    sd = {k: torch.from_numpy(v) for k, v in W.itn_synthetic(777, in_channels=6)}
    frames = [torch.from_numpy(W.synthetic_image(900 + t, (1, 3, H, H))).to(dev)
              for t in range(3)]
    engines = {}
    for name, kw in (("plain", {}), ("preserve_color", {"preserve_color": True})):
        net = network.VideoTransformNet(torch.rand([3, 64, 64]))
        net.load_state_dict(sd)
        try:
            eng = video.FrameEngine(net, (1, 3, H, H), dev, graph=True, **kw)
        except TypeError:
            continue
        for f in frames:
            eng.step(f)
        engines[name] = eng
    r = compare({k: e.graph.replay for k, e in engines.items()}, a.steps, a.warmup, a.rounds,
                1e3)
    if "preserve_color" in engines:
        r["extra_us"] = round(1e3 * (r["median"]["preserve_color"] - r["median"]["plain"]), 2)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20, help="kernel calls per captured graph")
    ap.add_argument("--engine-only", action="store_true",
                    help="only the FrameEngine replay (also runs on a tree without the kernels)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_color: needs a GPU (there is no CPU path to time)")
    dev = torch.device("cuda", 0)
    res = {"steps": a.steps, "rounds": a.rounds, "calls_per_graph": a.calls, "size": a.size,
           "box": box_calibration(dev)}
    if not a.engine_only:
        res["stats_us"] = stats_bench(dev, a)
        res["affine_us"] = affine_bench(dev, a)
    res["engine_ms"] = engine_bench(dev, a)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
