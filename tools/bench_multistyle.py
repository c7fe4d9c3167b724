"""What does a multi-style training step cost over the single-style one?

One GPU, B=8 at 256^2, graph-replayed steps (train_step): the single-style FastStTrainer
and MultiStyleTrainer (S styles) alternate in ONE process, each timed over windows of
--steps replays (after --warmup) with a device synchronise around each window; --rounds
rounds show the spread.  Prints one JSON line: ms/step per round for both, the medians,
their ratio and each trainer's spread (max - min over the median).

--count-launches also counts the device kernels of one eager forward/backward of each
trainer (torch.profiler; a run of its own, not a timed one).

    python tools/bench_multistyle.py [--styles 4] [--steps 200] [--warmup 20] [--rounds 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from styletransfer_amd import network  # noqa: E402
from styletransfer_amd import weights as W  # noqa: E402
from styletransfer_amd.train import FastStTrainer, MultiStyleTrainer  # noqa: E402


def window(trainer, batches, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        trainer.train_step(batches[i % len(batches)])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def count_kernels(trainer, batch):
    from torch.profiler import ProfilerActivity, profile
    trainer.step(batch)  # sizes every workspace
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        if hasattr(trainer, "set_styles"):
            trainer.set_styles(batch.shape[0], advance=False)
        trainer._fwd_bwd(batch)
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
               and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--styles", type=int, default=4)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--count-launches", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_multistyle: needs a GPU (there is no CPU path to time)")
    dev = torch.device("cuda", 0)
    B, H, S = a.batch, a.size, a.styles
    styles = [torch.from_numpy(W.synthetic_image(41 + i, (1, 3, H, H))).to(dev) for i in range(S)]
    batches = [torch.from_numpy(W.synthetic_image(50 + i, (B, 3, H, H))).to(dev) for i in range(4)]
    sd = {k: torch.from_numpy(v) for k, v in W.itn_synthetic(4321)}
    single = network.ImageTransformNet(styles[0], B)
    single.load_state_dict(sd)
    multi = network.MultiStyleTransformNet(styles, B)
    shapes = {k: v.dim() for k, v in multi.state_dict().items()}
    multi.load_state_dict({k: v.expand(S, -1).contiguous() if shapes[k] == 2 else v
                           for k, v in sd.items()})  # every style starts from the same rows
    trainers = {"single": FastStTrainer(single, styles[0]), "multi": MultiStyleTrainer(multi, styles)}
    if a.count_launches:
        print(json.dumps({"kernels_per_fwd_bwd": {k: count_kernels(t, batches[0])
                                                   for k, t in trainers.items()}}))
        return
    for t in trainers.values():
        window(t, batches, a.warmup)  # the capture's eager step, then replays
    ms = {k: [] for k in trainers}
    for _ in range(a.rounds):
        for k, t in trainers.items():  # alternate inside each round
            ms[k].append(window(t, batches, a.steps))
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(json.dumps({
        "batch": B, "size": H, "styles": S, "steps": a.steps, "rounds": a.rounds,
        "ms_per_step": {k: [round(x, 4) for x in v] for k, v in ms.items()},
        "median_ms": {k: round(v, 4) for k, v in med.items()},
        "ratio_multi_over_single": round(med["multi"] / med["single"], 4),
        "spread": {k: round((max(v) - min(v)) / med[k], 4) for k, v in ms.items()},
    }))


if __name__ == "__main__":
    main()
