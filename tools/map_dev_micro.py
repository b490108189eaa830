"""Dev tool: the COCO metric at validation-epoch scale, list evaluator against device evaluator.

A synthetic epoch is built once and kept on the device: --images (5000) images x 300 live detections
(max_det 300, every slot live), 80 classes, about 7 ground truths per image (Poisson), detections
jittered around the ground truths with beta-distributed scores quantised to 1/1024 (ties across
images) over a floor of random boxes; fed in batches of 32.  Both evaluators see the same tensors:
  list    yms.metrics.MeanAveragePrecision: update() on the per-image slices (seven .cpu() copies a
          batch), compute() with the host accumulation
  device  yms.metrics.CocoEvaluator: update() on the padded batch, compute() with the device accumulation
Each repetition times one whole epoch (reset, every update, compute) between device events and on the
wall clock (the clock stops after compute(), which ends in a host read); the two alternate, after one
untimed warm-up epoch each.  Prints the times per repetition, their spread, and whether the two
evaluators' tables and summaries agree on this workload.
--crowd F (default 0: the workload above, untouched) marks a fraction F of the ground truths crowd and gives
every one an annotation area u * w*h, u ~ U(0.3, 1), drawn from a generator of their own; both evaluators
then take them (iscrowd / area keys, gt_crowd / gt_area), i.e. the matching runs its crowd-aware kernels.
After those repetitions the device evaluator is timed --reps more times in two parts with a synchronise between
them: reset + every update (the match kernel), and compute() (device accumulate, summary, host read).
--tree DIR imports yms from another checkout's DIR/yolo-ms_amd (an A/B run of this script against another build).
Usage: python tools/map_dev_micro.py [--images 5000] [--reps 3] [--batch 32] [--crowd 0.15] [--tree DIR]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "yolo-ms_amd")]
import numpy as np
import torch

MAX_DET, NC = 300, 80
KEYS = ("map", "map_50", "map_75", "map_small", "map_medium", "map_large",
        "mar_1", "mar_10", "mar_100", "mar_small", "mar_medium", "mar_large")


def epoch(n_images, seed=0):
    """-> boxes [N, 300, 4], scores [N, 300], labels [N, 300] and per-image ground-truth dicts (numpy)"""
    rng = np.random.default_rng(seed)
    boxes = np.zeros((n_images, MAX_DET, 4), np.float32)
    scores = np.zeros((n_images, MAX_DET), np.float32)
    labels = np.zeros((n_images, MAX_DET), np.int32)
    targets = []
    for i in range(n_images):
        k = int(rng.poisson(7))
        ctr = rng.uniform(40, 600, (k, 2))
        wh = np.exp(rng.uniform(np.log(8), np.log(300), (k, 2)))
        gb = np.concatenate([ctr - wh / 2, ctr + wh / 2], 1).astype(np.float32)
        gl = rng.integers(0, NC, k)
        targets.append({"boxes": gb.reshape(-1, 4), "labels": gl.astype(np.int64)})
        near = min(MAX_DET, 30 * k)
        b = np.sort(rng.uniform(0, 640, (MAX_DET, 4)).astype(np.float32).reshape(MAX_DET, 2, 2), axis=1).reshape(MAX_DET, 4)
        lab = rng.integers(0, NC, MAX_DET)
        sc = rng.random(MAX_DET) * 0.3
        if near:
            src = rng.integers(0, k, near)
            b[:near] = gb[src] + rng.normal(0, 0.08, (near, 4)) * np.tile(wh[src], 2)
            lab[:near] = np.where(rng.random(near) < 0.85, gl[src], lab[:near])
            sc[:near] = rng.beta(2, 5, near) + 0.001
        b[:, 2:] = np.maximum(b[:, 2:], b[:, :2] + 1)
        boxes[i], labels[i] = b, lab
        scores[i] = np.maximum(np.round(sc * 1024) / 1024, 1.0 / 1024)
    return boxes, scores, labels, targets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--crowd", type=float, default=0.0)
    ap.add_argument("--tree", default=None)
    a = ap.parse_args()
    if a.tree:
        sys.path[:0] = [os.path.abspath(a.tree), os.path.join(os.path.abspath(a.tree), "yolo-ms_amd")]
    if not torch.cuda.is_available():
        sys.exit("map_dev_micro: needs a ROCm GPU (no CPU fallback)")
    from yms.metrics import CocoEvaluator, MeanAveragePrecision
    import yms.metrics
    print(f"# yms build {'with' if hasattr(yms.metrics, 'coco_results') else 'without'} iscrowd / area support"
          f"{' (--tree)' if a.tree else ''}", flush=True)
    N, B = a.images, a.batch
    boxes, scores, labels, targets = epoch(N)
    if a.crowd > 0:
        rng = np.random.default_rng(1)
        for t in targets:
            k, b = len(t["labels"]), t["boxes"]
            t["iscrowd"] = (rng.random(k) < a.crowd).astype(np.uint8)
            t["area"] = (rng.uniform(0.3, 1.0, k) * (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])).astype(np.float32)
    db, ds, dl = (torch.from_numpy(x).cuda() for x in (boxes, scores, labels))
    counts = torch.full((N,), MAX_DET, dtype=torch.int32, device="cuda")
    dev_batches, list_batches = [], []
    for i in range(0, N, B):
        j = min(i + B, N)
        gts = CocoEvaluator.pad_targets(targets[i:j], "cuda", flags=True) if a.crowd > 0 \
            else CocoEvaluator.pad_targets(targets[i:j], "cuda")
        dev_batches.append(((db[i:j], ds[i:j], dl[i:j], counts[i:j]), gts))
        list_batches.append(([{"boxes": db[k], "scores": ds[k], "labels": dl[k]} for k in range(i, j)],
                             [{k2: torch.from_numpy(v).cuda() for k2, v in t.items()} for t in targets[i:j]]))
    ev, metric = CocoEvaluator(NC, capacity_images=max(1024, N)), MeanAveragePrecision()

    def run_device():
        ev.reset()
        for dets, gts in dev_batches:
            ev.update(dets, *gts)
        return ev.compute()

    def run_list():
        metric.reset()
        for preds, tg in list_batches:
            metric.update(preds, tg)
        return metric.compute()

    def timed(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.record()
        out = fn()
        e.record()
        e.synchronize()
        return out, s.elapsed_time(e), (time.perf_counter() - t0) * 1e3

    n_gt = sum(len(t["labels"]) for t in targets)
    if a.crowd > 0:
        print(f"# crowd path: {sum(int(t['iscrowd'].sum()) for t in targets)} crowd ground truths, area = u * w*h", flush=True)
    print(f"# {N} images x {MAX_DET} detections = {N * MAX_DET} rows, {NC} classes, {n_gt} ground truths "
          f"({n_gt / N:.2f} per image), {len(dev_batches)} updates of {B}; one warm-up epoch each, then {a.reps} "
          f"alternating repetitions of reset + updates + compute", flush=True)
    out_d, out_l = run_device(), run_list()                    # warm-up, and the results to compare
    same = all(np.array_equal(x, y) for x, y in zip(ev.tables(), metric.tables()))
    worst = max(abs(out_d[k].item() - out_l[k].item()) for k in KEYS)
    print(f"# tables (precision, recall, npig) identical: {same}; largest summary difference {worst:.3g}; "
          f"map {out_d['map'].item():.6f} map_50 {out_d['map_50'].item():.6f} mar_100 {out_d['mar_100'].item():.6f}",
          flush=True)
    t = {"list": [], "device": []}
    for r in range(a.reps):
        for label, fn in (("list", run_list), ("device", run_device)):
            _, ev_ms, wall_ms = timed(fn)
            t[label].append(wall_ms)
            print(f"rep {r} {label:6s} events {ev_ms:10.2f} ms  wall {wall_ms:10.2f} ms", flush=True)
    for label, v in t.items():
        print(f"# {label:6s} wall: median {np.median(v):.2f} ms, spread (max - min) {max(v) - min(v):.2f} ms")
    print(f"# list / device (median wall): {np.median(t['list']) / np.median(t['device']):.1f}x")

    def updates():
        ev.reset()
        for dets, gts in dev_batches:
            ev.update(dets, *gts)

    parts = {"updates": [], "compute": []}
    for r in range(a.reps):
        for label, fn in (("updates", updates), ("compute", ev.compute)):
            _, ev_ms, wall_ms = timed(fn)
            parts[label].append(wall_ms)
        print(f"rep {r} device in parts: updates {parts['updates'][-1]:8.2f} ms  compute {parts['compute'][-1]:8.2f} ms "
              f"(wall)", flush=True)
    for label, v in parts.items():
        print(f"# device {label:7s} wall: median {np.median(v):.2f} ms, min {min(v):.2f} max {max(v):.2f}")


if __name__ == "__main__":
    main()
