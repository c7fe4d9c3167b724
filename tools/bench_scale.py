"""What does scale control cost: the resampler, a level transition, a whole pyramid?

One GPU, one process:

  resample  ops.resample2d at 3x512^2 -> 3x1024^2, 3x1024^2 -> 3x512^2 and 3x256^2 ->
            3x512^2, both filters, against torch's copy_ of a tensor that moves the same
            bytes (reads in + out floats in all: a copy of (in + out) / 2 floats); graphs of
            --calls back-to-back calls, alternating windows, us per call and the ratio.
  levels    per size of --sizes: one level transition of scale.coarse_to_fine (three
            resamples, the style targets, the content target, the engine and its capture;
            wall time, device synchronised) against that level's replayed iteration, and
            how many iterations the transition is worth.
  engine    GatysEngine at 512^2 built directly and the 512^2 level as coarse_to_fine
            builds it (resampled inputs, init): replayed iterations alternated, their
            spread -- it is the same engine, so a difference is a finding.
  pyramid   wall time of coarse_to_fine over --sizes with --iters iterations per level
            against a single-scale run of --iters iterations at the top size.

Prints one JSON line, with the box's calibration taken first in the same process.

    python tools/bench_scale.py [--sizes 256,512,1024] [--iters 100] [--steps 100]
                                [--warmup 10] [--rounds 5] [--calls 20]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_guided import box_calibration, compare, graph_of  # noqa: E402
from styletransfer_amd import ops, scale  # noqa: E402
from styletransfer_amd import vgg as V  # noqa: E402
from styletransfer_amd import weights as W  # noqa: E402

RESAMPLES = ((512, 1024), (1024, 512), (256, 512))


def resample_bench(dev, a):
    out = {}
    for n_in, n_out in RESAMPLES:
        x = torch.randn(1, 3, n_in, n_in, device=dev,
                        generator=torch.Generator(dev).manual_seed(1))
        y = torch.empty(1, 3, n_out, n_out, device=dev)
        moved = 4 * (x.numel() + y.numel())
        src = torch.randn(moved // 8, device=dev)
        dst = torch.empty_like(src)
        cands = {f: graph_of(lambda f=f: ops.resample2d(x, n_out, f, out=y), a.calls).replay
                 for f in ("triangle", "cubic")}
        cands["copy"] = graph_of(lambda: dst.copy_(src), a.calls).replay
        r = compare(cands, a.steps // 4 + 1, a.warmup // 4 + 1, a.rounds, 1e6 / a.calls)
        r["bytes"] = moved
        r["gbs"] = {k: round(moved / (v * 1e-6) / 1e9, 1) for k, v in r["median"].items()}
        r["x_copy"] = {k: round(v / r["median"]["copy"], 2) for k, v in r["median"].items()}
        out[f"{n_in}->{n_out}"] = r
    return out


def _wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def _images(dev, top):
    return (torch.from_numpy(W.synthetic_image(11, (1, 3, top, top))).to(dev),
            torch.from_numpy(W.synthetic_image(12, (1, 3, top, top))).to(dev))


def _level(feat, style, content, prev, size):
    """One level as scale.coarse_to_fine sets it up, captured."""
    x = ops.resample2d(prev, size)
    eng = V.GatysEngine(feat, scale._at(style, size), scale._at(content, size), init=x)
    return eng.capture(warmup=1)


def levels_bench(dev, feat, sizes, a):
    style, content = _images(dev, sizes[-1])
    out = {}
    for size in sizes:
        prev = ops.resample2d(content, max(size // 2, 32))
        _level(feat, style, content, prev, size)  # tables, workspaces, allocator blocks
        ms = sorted(_wall(lambda: _level(feat, style, content, prev, size))[0]
                    for _ in range(3))
        eng = _level(feat, style, content, prev, size)
        it = compare({"iteration": eng.graph.replay}, a.steps, a.warmup, a.rounds, 1e3)
        out[str(size)] = {"transition_ms": round(ms[1], 3),
                          "iteration_ms": it["median"]["iteration"],
                          "iteration_spread": it["spread"]["iteration"],
                          "iterations_per_s": round(1e3 / it["median"]["iteration"], 1),
                          "transition_in_iterations":
                              round(ms[1] / it["median"]["iteration"], 1)}
        scale._release(eng)
    return out


def engine_bench(dev, feat, a, size=512):
    style, content = _images(dev, 2 * size)
    s, c = ops.resample2d(style, size), ops.resample2d(content, size)
    plain = V.GatysEngine(feat, s.clone(), c.clone()).capture(warmup=1)
    level = _level(feat, style, content, ops.resample2d(content, size // 2), size)
    r = compare({"plain": plain.graph.replay, "level": level.graph.replay}, a.steps, a.warmup,
                a.rounds, 1e3)
    r["level_over_plain"] = round(r["median"]["level"] / r["median"]["plain"], 4)
    return r


def pyramid_bench(dev, feat, sizes, a):
    style, content = _images(dev, sizes[-1])
    scale.coarse_to_fine(feat, style, content, sizes, 2)  # tables, workspaces
    multi = [_wall(lambda: scale.coarse_to_fine(feat, style, content, sizes, a.iters))[0]
             for _ in range(3)]
    single = [_wall(lambda: scale.coarse_to_fine(feat, style, content, sizes[-1:], a.iters))[0]
              for _ in range(3)]
    return {"iters_per_level": a.iters, "sizes": sizes,
            "pyramid_ms": round(sorted(multi)[1], 2), "single_top_ms": round(sorted(single)[1], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512,1024")
    ap.add_argument("--iters", type=int, default=100, help="iterations per pyramid level")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20, help="kernel calls per captured graph")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_scale: needs a GPU (there is no CPU path to time)")
    dev = torch.device("cuda", 0)
    sizes = scale.check_sizes([int(s) for s in a.sizes.split(",")])
    feat = V.VGGFeatures(V.load_vgg19_weights(), dev)
    res = {"steps": a.steps, "rounds": a.rounds, "calls_per_graph": a.calls,
           "box": box_calibration(dev)}
    res["resample_us"] = resample_bench(dev, a)
    res["levels"] = levels_bench(dev, feat, sizes, a)
    res["engine_512_ms"] = engine_bench(dev, feat, a)
    res["pyramid"] = pyramid_bench(dev, feat, sizes, a)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
