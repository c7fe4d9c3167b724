"""What does moving the JPEG pixel stages to the GPU buy the fast_st loader?

One run, the loader leg's workload (dataset.write_synthetic_jpegs: 640x480, quality 90):

  worker   images/s of ONE loader worker, measured in this process on one thread, for a
           batch of --batch images at a time, item by item and then the collate, exactly
           what a DataLoader worker executes:
             pil      CocoDataset(decode_only=True) + _pack_collate   (today's path)
             entropy  CocoDataset(decode="coefs")   + _coef_collate   (--gpu-decode)
           The two alternate for --rounds rounds over the same files; the median round and
           the spread ((max - min) / median) are reported.
  gpu      the device stage for one batch of --batch entropy-decoded images, resident in
           HBM: stx_jpeg_decode_batch (IDCT + upsampling + colour) alone, the conditioning
           that follows it alone, and both; HIP events around --steps calls after --warmup.
  loader   bench.py's loader leg (get_coco_loader over --loader-files files at batch
           --batch: a warm-up epoch, then --loader-epochs timed epochs of conditioned
           batches in HBM) with gpu_decode off and on, alternating, for each worker count
           of --loader-workers; images/s and, as bench.py reports it, images/s per worker
           (the loader's rate over its worker count: what the whole pipeline -- workers,
           shared memory, the pin thread, the consumer -- delivers per CPU spent on a
           worker, not what one worker can decode).
  cpus_for_8_ranks   bench.py's formula, 8 x (per-rank fast_st images/s / images per worker
           + 1), for the in-process worker rates and for each loader run, with --step-rate
           (images/s per rank; measure it in the same session with bench.py and pass it in).

Prints one JSON line; --out writes it to a file as well.  The pixels are checked against
PIL before anything is timed.

    python tools/bench_jpeg.py [--files 64] [--batch 8] [--rounds 5] [--step-rate 1930]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from styletransfer_amd import dataset, img_utils, jpeg  # noqa: E402


def _worker_pass(ds, collate, batch):
    n = len(ds) - len(ds) % batch
    t = time.perf_counter()
    for i in range(0, n, batch):
        collate([ds[j] for j in range(i, i + batch)])
    return n / (time.perf_counter() - t)


def worker_rates(path, batch, rounds):
    cands = {"pil": (dataset.CocoDataset(path=path, decode_only=True), dataset._pack_collate),
             "entropy": (dataset.CocoDataset(path=path, decode="coefs"), dataset._coef_collate)}
    for ds, col in cands.values():  # page cache, library load
        _worker_pass(ds, col, batch)
    runs = {k: [] for k in cands}
    for _ in range(rounds):
        for k, (ds, col) in cands.items():
            runs[k].append(_worker_pass(ds, col, batch))
    out = {}
    for k, v in runs.items():
        med = statistics.median(v)
        out[k] = {"images_per_s": round(med, 1), "spread": round((max(v) - min(v)) / med, 3)}
    out["entropy_over_pil"] = round(out["entropy"]["images_per_s"] / out["pil"]["images_per_s"], 3)
    return out


def _loader_pass(path, batch, workers, gpu_decode, epochs):
    _, train = dataset.get_coco_loader(batch_size=batch, test_split=0.0, path=path,
                                       gpu_conditioning=True, gpu_decode=gpu_decode,
                                       num_workers=workers)
    for _ in train:  # warm-up epoch: workers started, pinned/host caches filled
        pass
    torch.cuda.synchronize()
    t, count = time.perf_counter(), 0
    for _ in range(epochs):
        for b in train:
            count += b.shape[0]
    torch.cuda.synchronize()
    rate = count / (time.perf_counter() - t)
    del train
    return rate


def loader_rates(path, batch, workers_list, epochs, rounds, step_rate):
    out = {}
    for w in workers_list:
        runs = {"pil": [], "entropy": []}
        for _ in range(rounds):
            for k in runs:
                runs[k].append(_loader_pass(path, batch, w, k == "entropy", epochs))
        r = {}
        for k, v in runs.items():
            med = statistics.median(v)
            r[k] = {"images_per_s": round(med, 1), "per_worker": round(med / w, 1),
                    "spread": round((max(v) - min(v)) / med, 3),
                    "runs": [round(x, 1) for x in v]}
            if step_rate:
                r[k]["cpus_for_8_ranks"] = round(8 * (step_rate / (med / w) + 1), 1)
        r["entropy_over_pil"] = round(r["entropy"]["images_per_s"] / r["pil"]["images_per_s"], 3)
        out[f"workers{w}"] = r
    return out


def _events(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def gpu_stage(path, batch, steps, warmup, rounds):
    dev = torch.device("cuda", 0)
    ds = dataset.CocoDataset(path=path, decode="coefs")
    items = [ds[i] for i in range(batch)]
    packed = dataset._coef_collate(items).pin_memory()
    dec, cond = jpeg.JpegBatchDecoder(dev), img_utils.ImageConditioner(device=dev)
    jobs, shapes, rgb_bytes, jtmp_bytes = jpeg.plan(jpeg.records(packed))
    metas, coef, max_rows, tmp_bytes, src_bytes = cond._plan(shapes)
    dp = packed.to(dev)
    rgb = torch.empty(rgb_bytes, dtype=torch.uint8, device=dev)
    jtmp = torch.empty(max(jtmp_bytes, 16), dtype=torch.uint8, device=dev)
    meta = torch.frombuffer(bytearray(bytes(metas)), dtype=torch.uint8).to(dev)
    cf = torch.from_numpy(coef).to(dev)
    tmp = torch.empty(max(tmp_bytes, 16), dtype=torch.uint8, device=dev)
    out = torch.empty((batch, 3, cond.size, cond.size), dtype=torch.float32, device=dev)

    def decode():
        dec.launch(dp, jobs, batch, rgb, jtmp)

    def condition():
        cond._launch(rgb, meta, batch, max_rows, cf, out, tmp)

    def both():
        decode()
        condition()

    def upload():
        dp.copy_(packed, non_blocking=True)

    decode()
    torch.cuda.synchronize()
    want = np.concatenate([np.asarray(dataset.CocoDataset(path=path, decode_only=True)[i])
                           .reshape(-1) for i in range(batch)])
    if not np.array_equal(rgb.cpu().numpy(), want):
        raise SystemExit("GPU decode != PIL decode: not timing a wrong result")
    cands = {"decode": decode, "condition": condition, "decode+condition": both,
             "upload": upload}
    runs = {k: [] for k in cands}
    for _ in range(rounds):
        for k, fn in cands.items():
            runs[k].append(_events(fn, steps, warmup))
    res = {k: {"ms_per_batch": round(statistics.median(v), 4),
               "spread": round((max(v) - min(v)) / statistics.median(v), 3)}
           for k, v in runs.items()}
    res["batch"] = batch
    res["coef_mb"] = round(packed.numel() / 1e6, 3)
    res["rgb_mb"] = round(rgb_bytes / 1e6, 3)
    res["note"] = ("HIP events around back-to-back calls on resident buffers; decode = "
                   "stx_jpeg_decode_batch (2 launches), condition = stx_image_condition (2 "
                   "launches), upload = the pinned packed coefficient batch host -> device")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--step-rate", type=float, default=None,
                    help="fast_st images/s per rank (bench.py's fast_st value), for cpus_for_8_ranks")
    ap.add_argument("--loader-files", type=int, default=256)
    ap.add_argument("--loader-epochs", type=int, default=3)
    ap.add_argument("--loader-rounds", type=int, default=3)
    ap.add_argument("--loader-workers", default="2,4,15",
                    help="worker counts of the loader runs, comma separated ('' skips them)")
    ap.add_argument("--no-gpu", action="store_true", help="worker rates only")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.set_num_threads(1)
    res = {"metric": "fast_st loader: one worker's images/s with PIL decode vs entropy-only decode",
           "workload": f"{a.files} write_synthetic_jpegs files, 640x480, quality 90"}
    with tempfile.TemporaryDirectory() as d:
        dataset.write_synthetic_jpegs(d, a.files)
        res["jpeg_kb"] = round(sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))
                               / a.files / 1024, 1)
        res["worker"] = worker_rates(d, a.batch, a.rounds)
        if not a.no_gpu:
            if not torch.cuda.is_available():
                raise SystemExit("bench_jpeg: the GPU stage needs a GPU (--no-gpu: worker rates "
                                 "only)")
            res["gpu"] = gpu_stage(d, a.batch, a.steps, a.warmup, a.rounds)
            wl = [int(w) for w in a.loader_workers.split(",") if w.strip()]
            if wl:
                dataset.write_synthetic_jpegs(d, a.loader_files, seed=7)
                res["loader"] = loader_rates(d, a.batch, wl, a.loader_epochs, a.loader_rounds,
                                             a.step_rate)
                res["loader"]["usable_cpus"] = dataset.usable_cpus()
    if a.step_rate:
        res["step_rate"] = a.step_rate
        res["cpus_for_8_ranks"] = {
            k: round(8 * (a.step_rate / res["worker"][k]["images_per_s"] + 1), 1)
            for k in ("pil", "entropy")}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
