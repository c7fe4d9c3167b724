"""What does temporally consistent Gatys video cost per frame, and what does the temporal
term add to an iteration?

One GPU, one process, --size^2 (512), --frames synthetic frames (one texture seen through a
window that moves by (2, 1) px per frame, exact flows), --steps Adam iterations per frame:

  clip       video.gatys_video over the clip: frames/s over the frames after the first (the
             first also captures the graph), host clock around a device synchronise.
  setup      what a frame costs before its first iteration: ops.flow_consistency, the two
             ops.flow_warp (the reference of the term, the filled init) and
             GatysEngine.retarget (the content target's four convs, five copies, three
             clears), device events around the sequence, us.
  iteration  one replayed iteration of an engine with the temporal term and of one without,
             alternating windows of --window replays between device events, us, and their
             difference.
  term       ops.masked_mse alone (accumulating gradient, add_to) in a graph of --calls calls
             against copy_ of the image (reads and writes 12 h w bytes each), us per call and
             the GB/s of the bytes each moves: the term reads x, ref and the gradient, writes
             the gradient, over 3 channels, and reads the mask: 52 h w bytes.

--long-term 1,2,4 adds the long-term loss (--flow auto: the clip's flows are
estimated instead of given):

  clip       also with long_term, in runs alternating with the short-term ones.
  long_setup one ops.flow_compose at count 1 and at every offset, against the 3 and 3 J
             launches of the existing ops that it replaces (a flow_consistency and two
             flow_warp per offset): captured graphs of --calls set-ups, alternating windows
             between device events, us per set-up; and the same four launched eagerly.
  long_iteration  a replayed iteration of an engine on the composed (ref, mask) and of one on
             the short-term pair, alternating windows: the graph is the same.

Prints one JSON line, with the box's calibration (bench.py's `box` block) taken first.

    python tools/bench_gatys_video.py [--size 512] [--frames 8] [--steps 50]
                                      [--long-term 1,2,4] [--flow exact|auto]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_guided import box_calibration, compare, graph_of  # noqa: E402
from styletransfer_amd import ops, video  # noqa: E402
from styletransfer_amd import vgg as V  # noqa: E402
from styletransfer_amd import weights as W  # noqa: E402

DX, DY = 2, 1


def make_clip(size, frames):
    tex = W.synthetic_image(81, (1, 3, size + DY * frames, size + DX * frames))
    clip = [torch.from_numpy(np.ascontiguousarray(
        tex[:, :, DY * t:DY * t + size, DX * t:DX * t + size])) for t in range(frames)]
    bwd = np.zeros((frames - 1, 2, size, size), np.float32)
    bwd[:, 0], bwd[:, 1] = DX, DY
    return clip, (-bwd, bwd)


def long_flows(size, frames, offsets):
    """The clip's exact flows over k frames, {k: (forward_k, backward_k)}."""
    out = {}
    for k in offsets:
        bwd = np.zeros((max(frames - k, 0), 2, size, size), np.float32)
        bwd[:, 0], bwd[:, 1] = DX * k, DY * k
        out[k] = (-bwd, bwd)
    return out


def events_compare(cands, steps, rounds, unit):
    """cands: name -> callable.  Alternating windows of `steps` calls between device events;
    medians and spreads in us / unit."""
    t = {k: [] for k in cands}
    for fn in cands.values():
        fn()
    for _ in range(rounds):
        for k, fn in cands.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(steps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            t[k].append(e0.elapsed_time(e1) * 1e3 / (steps * unit))
    med = {k: statistics.median(v) for k, v in t.items()}
    return {"median": {k: round(v, 3) for k, v in med.items()},
            "spread": {k: round((max(v) - min(v)) / med[k], 4) for k, v in t.items()}}


def events_us(fn, reps):
    """Median device time of fn() between two events, us."""
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return round(statistics.median(out), 2), round((max(out) - min(out)) / statistics.median(out), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--window", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20, help="kernel calls per captured graph")
    ap.add_argument("--temporal-weight", type=float, default=video.DEFAULT_TEMPORAL_WEIGHT)
    ap.add_argument("--long-term", default=None, metavar="1,K,...",
                    help="offsets of the long-term loss: adds its clip rate, set-up and iteration")
    ap.add_argument("--flow", choices=("exact", "auto"), default="exact",
                    help="the clip runs' flows: the clip's exact ones, or estimated per frame")
    a = ap.parse_args()
    offsets = None if a.long_term is None else \
        video.check_offsets([int(v) for v in a.long_term.split(",")])
    if not torch.cuda.is_available():
        sys.exit("bench_gatys_video: needs a GPU (there is no CPU path to time)")
    dev = torch.device("cuda", 0)
    S = a.size
    res = {"size": S, "frames": a.frames, "steps": a.steps, "box": box_calibration(dev)}
    feat = V.VGGFeatures(W.vgg19_synthetic(1234, 5), dev)
    style = torch.from_numpy(W.synthetic_image(11, (1, 3, S, S))).to(dev)
    clip, flows = make_clip(S, a.frames)
    clip = [f.to(dev) for f in clip]

    # ---- the clip
    def run_clip(long_term=None):
        fl = "auto" if a.flow == "auto" else flows if long_term is None else \
            long_flows(S, a.frames, long_term)
        it = video.gatys_video(feat, clip, style, fl, steps=a.steps,
                               temporal_weight=a.temporal_weight, long_term=long_term)
        next(it)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = sum(1 for _ in it)
        torch.cuda.synchronize()
        return n / (time.perf_counter() - t0)
    run_clip()  # warm-up: allocations, prepared weights
    res["flow"] = a.flow
    if offsets is None:
        fps = [run_clip() for _ in range(3)]
    else:
        run_clip(offsets)
        fps, fps_long = [], []
        for _ in range(3):  # alternating runs
            fps.append(run_clip())
            fps_long.append(run_clip(offsets))
        res["clip_fps_long_term"] = {"offsets": list(offsets),
                                     "median": round(statistics.median(fps_long), 3),
                                     "runs": [round(v, 3) for v in fps_long]}
    res["clip_fps"] = {"median": round(statistics.median(fps), 3),
                       "runs": [round(v, 3) for v in fps]}

    # ---- set-up of a frame, and the iteration with and without the term
    fwd, bwd = (torch.from_numpy(f[0:1]).to(dev) for f in flows)
    prev = clip[0].clone()
    omega, init = torch.empty_like(prev), torch.empty_like(prev)
    cmask = torch.zeros(1, S, S, device=dev)
    targets = feat.style_targets(style)
    with_t = V.GatysEngine(feat, None, clip[0], targets=targets,
                           temporal=(prev, cmask, a.temporal_weight))
    without = V.GatysEngine(feat, None, clip[0], targets=targets)
    with_t.run(3)
    without.run(3)

    def setup():
        ops.flow_consistency(fwd, bwd, out=cmask)
        ops.flow_warp(prev, bwd, out=omega)
        ops.flow_warp(prev, bwd, fill=clip[1], out=init)
        with_t.retarget(clip[1], init=init, temporal_ref=omega, temporal_mask=cmask)

    def kernels_only():
        ops.flow_consistency(fwd, bwd, out=cmask)
        ops.flow_warp(prev, bwd, out=omega)
        ops.flow_warp(prev, bwd, fill=clip[1], out=init)
    setup()
    res["setup_us"] = dict(zip(("median", "spread"), events_us(setup, 20)))
    res["setup_flow_kernels_us"] = dict(zip(("median", "spread"), events_us(kernels_only, 20)))
    res["consistency_share"] = round(float(cmask.mean()), 4)

    def window(eng):
        def run():
            for _ in range(a.window):
                eng.graph.replay()
        return run
    for e in (with_t, without):
        window(e)()
    t = {"with_term": [], "without": []}
    for _ in range(a.rounds):
        for k, e in (("with_term", with_t), ("without", without)):
            t[k].append(events_us(window(e), 1)[0] / a.window)
    med = {k: statistics.median(v) for k, v in t.items()}
    res["iteration_us"] = {
        "median": {k: round(v, 2) for k, v in med.items()},
        "spread": {k: round((max(v) - min(v)) / med[k], 4) for k, v in t.items()},
        "term_us": round(med["with_term"] - med["without"], 2),
        "term_share": round((med["with_term"] - med["without"]) / med["with_term"], 4)}

    if offsets is not None:
        # ---- one compose against the launches it replaces, and the iteration on its outputs
        J = len(offsets)
        lf = long_flows(S, a.frames, offsets)
        fwds = [torch.from_numpy(lf[k][0][0:1]).to(dev) for k in offsets]
        bwds = [torch.from_numpy(lf[k][1][0:1]).to(dev) for k in offsets]
        prevs = [clip[q % len(clip)].clone() for q in range(J)]
        refs = [torch.empty_like(prev) for _ in range(J)]
        inits = [torch.empty_like(prev) for _ in range(J)]
        masks = [torch.zeros(1, S, S, device=dev) for _ in range(J)]
        which = torch.empty(1, S, S, device=dev, dtype=torch.uint8)
        fill = clip[1]

        def compose(count):
            return lambda: ops.flow_compose(prevs[:count], fwds[:count], bwds[:count], fill,
                                            ref=refs[0], cmask=masks[0], init=inits[0], which=which)

        def existing(count):
            def run():
                for q in range(count):
                    ops.flow_consistency(fwds[q], bwds[q], out=masks[q])
                    ops.flow_warp(prevs[q], bwds[q], out=refs[q])
                    ops.flow_warp(prevs[q], bwds[q], fill=fill, out=inits[q])
            return run
        fns = {"compose_1": compose(1), "ops_3_launches": existing(1),
               f"compose_{J}": compose(J), f"ops_{3 * J}_launches": existing(J)}
        graphs = {k: graph_of(fn, a.calls) for k, fn in fns.items()}
        res["long_setup_us"] = {
            "captured": events_compare({k: g.replay for k, g in graphs.items()}, 20, a.rounds,
                                       a.calls),
            "eager": events_compare(fns, 20, a.rounds, 1)}
        compose(J)()
        res["long_setup_us"]["settled_at_first_offset"] = round(float((which == 0).float().mean()), 4)
        long_e = V.GatysEngine(feat, None, clip[0], targets=targets,
                               temporal=(refs[0], masks[0], a.temporal_weight))
        long_e.run(3)
        engines = {"long_term": long_e, "short_term": with_t}
        res["long_iteration_us"] = events_compare({k: window(e) for k, e in engines.items()}, 1,
                                                  a.rounds, a.window)

    # ---- the term's kernel alone against a copy
    x, ref, grad = (torch.randn(1, 3, S, S, device=dev) for _ in range(3))
    mask = (torch.rand(1, S, S, device=dev) > 0.1).float()
    out, tot, dst = torch.zeros(1, device=dev), torch.zeros((), device=dev), torch.empty_like(x)
    cands = {"masked_mse": graph_of(lambda: ops.masked_mse(
                 x, ref, mask, 1e-3, out=out, add_to=tot, grad=grad, accumulate=True), a.calls).replay,
             "copy": graph_of(lambda: dst.copy_(x), a.calls).replay}
    r = compare(cands, 50, 10, a.rounds, 1e6 / a.calls)
    moved = {"masked_mse": 52 * S * S, "copy": 24 * S * S}
    r["gbs"] = {k: round(moved[k] / (v * 1e-6) / 1e9, 1) for k, v in r["median"].items()}
    res["term_us"] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
