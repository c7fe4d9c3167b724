"""What does estimating the optical flow of a frame pair cost, and what does fusing Jacobi
iterations into one launch buy?

One GPU, one process; the batch is 2 (both directions of a pair), --sizes squares:

  jacobi     ops.flow_jacobi, --iters iterations, in a captured graph of --calls calls, for
             fuse = 1, 2, 4, MAXFUSE and the library's choice (0): alternating windows, us per
             iteration (median, spread).
  pieces     ops.flow_luma (n = 2) and ops.flow_linearize alone, captured likewise, us per call.
  pair       video.FlowEstimator.pair at the default parameters: eager (host clock around a
             device synchronise: the launches' host cost included) and as one captured graph
             replayed, us per frame pair; and the number of kernel launches of a pair.

  pairs      with --pairs P > 1: FlowEstimator(pairs=P).pairs_flow over P frame pairs (one
             sequence of launches, batch 2 P) against P pair calls of a one-pair estimator,
             eager and replayed, alternating windows, us per P pairs.

Prints one JSON line, with the box's calibration (bench.py's `box` block) taken first.

    python tools/bench_flow.py [--sizes 512,32] [--iters 40] [--pairs 3]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_guided import box_calibration, compare, graph_of  # noqa: E402
from styletransfer_amd import _native as N  # noqa: E402
from styletransfer_amd import ops, video  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512,32")
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--calls", type=int, default=10, help="calls per captured graph")
    ap.add_argument("--steps", type=int, default=20, help="replays per window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-box", action="store_true", help="skip the box calibration")
    ap.add_argument("--pairs", type=int, default=1,
                    help="also time pairs_flow over this many pairs against as many pair calls")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_flow: needs a GPU (there is no CPU path to time)")
    dev = torch.device("cuda", 0)
    res = {"iters": a.iters, "box": None if a.no_box else box_calibration(dev), "sizes": {}}
    for S in (int(s) for s in a.sizes.split(",")):
        r = {}
        coef = torch.empty(2, 3, S, S, device=dev).uniform_(-40, 40)
        uv, out = torch.randn(2, 2, S, S, device=dev), torch.empty(2, 2, S, S, device=dev)
        fuses = sorted({0, 1, 2, 4, N.STX_FLOW_JACOBI_MAXFUSE})
        cands = {f"fuse{f}": graph_of(lambda f=f: ops.flow_jacobi(coef, uv, out=out, iters=a.iters,
                                                                 fuse=f), a.calls).replay
                 for f in fuses}
        r["jacobi_us_per_iteration"] = compare(cands, a.steps, 5, a.rounds,
                                               1e6 / (a.calls * a.iters))
        img = torch.randn(2, 3, S, S, device=dev)
        grey = torch.empty(2, S, S, device=dev)
        grey_b = torch.rand(2, S, S, device=dev) * 255
        cands = {"luma": graph_of(lambda: ops.flow_luma(img, out=grey), a.calls).replay,
                 "linearize": graph_of(lambda: ops.flow_linearize(grey, grey_b, uv, out=coef),
                                       a.calls).replay}
        r["pieces_us"] = compare(cands, a.steps, 5, a.rounds, 1e6 / a.calls)
        if S >= 32:
            est = video.FlowEstimator(S, S, dev)
            p, c = torch.randn(1, 3, S, S, device=dev), torch.randn(1, 3, S, S, device=dev)
            g = graph_of(lambda: est.pair(p, c), 1)
            r["pair_us"] = compare({"eager": lambda: est.pair(p, c), "replayed": g.replay},
                                   a.steps, 3, a.rounds, 1e6)
            r["levels"] = est.levels
            per = lambda hw: 1 if max(hw) <= 32 else -(-est.iters // N.STX_FLOW_JACOBI_MAXFUSE)
            r["pair_launches"] = 4 + 2 * (len(est.levels) - 1) + 3 * (len(est.levels) - 1) + 1 + \
                sum(est.warps * (1 + per(hw)) for hw in est.levels)
            if a.pairs > 1:
                batched = video.FlowEstimator(S, S, dev, pairs=a.pairs)
                frames = [torch.randn(1, 3, S, S, device=dev) for _ in range(a.pairs)]
                many = lambda: batched.pairs_flow([(f, c) for f in frames])

                def separate():
                    for f in frames:
                        est.pair(f, c)
                gm, gs = graph_of(many, 1), graph_of(separate, 1)
                r["pairs_us"] = compare({"batched_eager": many, "separate_eager": separate,
                                         "batched_replayed": gm.replay,
                                         "separate_replayed": gs.replay}, a.steps, 3, a.rounds, 1e6)
                r["pairs"] = a.pairs
        res["sizes"][str(S)] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
