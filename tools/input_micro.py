"""Dev tool: what the input side delivers with the recipe's augmentation on -- B=64 outputs of 640x640,
Mosaic 1 / MixUp 1 (eight sources per output), the full augmentation config -- over a synthetic
COCO directory generated here with PIL (640x480 quality-90 JPEGs, 7 boxes each; nothing is
downloaded).  Two paths run alternately in one process, a window of --batches batches each per round:
  parent   COCODataset(mosaic=True) in a DataLoader with --workers workers (at most 12), the batch
           collated by collate_to_gpu in the main process: every source decoded, every box on the host
  cached   CachedCOCODataset over a DeviceImageCache holding every image, plans sampled in
           --cached-workers workers, collate_cached in the main process: two launches, no decode
A window starts with a fresh iterator over the loader's persistent workers (nothing prefetched) and
ends with a device synchronise; the other path's workers are idle meanwhile.  Printed per window:
batches/s, and per batch the main process's milliseconds inside the collate (wall), waiting for the
workers, and of CPU time.  Before the rounds: the host's PIL decode rate (one core) and the cached
collate's host half alone (batch_tables).  The DataLoader workers are started before the GPU is
opened, so no worker inherits it.
Usage: python tools/input_micro.py [--rounds 3] [--batches 36] [--images 256] [--workers 12]"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "yolo-ms_amd")]
import numpy as np
import torch

from yms import cache as C
from yms import data as D

AUG = {"hsv_h": 0.015, "hsv_s": 0.7, "hsv_v": 0.4, "degrees": 20.0, "translate": 0.1, "scale": 0.5,
       "shear": 8.0, "perspective": 0.08, "flipud": 0.5, "fliplr": 0.5, "mosaic": 1.0, "mixup": 1.0}
SRC = (480, 640)


def make_coco(root, n, boxes_per_image):
    """n smooth random 640x480 JPEGs (a 15x20 random field upsampled, plus grain) with random boxes."""
    from PIL import Image
    rng = np.random.default_rng(0)
    images, anns = [], []
    h, w = SRC
    for i in range(n):
        field = Image.fromarray(rng.integers(0, 256, (15, 20, 3), dtype=np.uint8)).resize((w, h), Image.BICUBIC)
        im = np.clip(np.asarray(field, np.int16) + rng.integers(-12, 13, (h, w, 3)), 0, 255).astype(np.uint8)
        fn = f"{i:06d}.jpg"
        Image.fromarray(im).save(os.path.join(root, fn), quality=90)
        images.append({"id": i + 1, "file_name": fn, "height": h, "width": w})
        for _ in range(boxes_per_image):
            x, y = rng.uniform(0, w - 40), rng.uniform(0, h - 40)
            bw, bh = rng.uniform(8, w - x), rng.uniform(8, h - y)
            anns.append({"id": len(anns) + 1, "image_id": i + 1, "category_id": int(rng.integers(1, 81)),
                         "bbox": [x, y, bw, bh], "area": bw * bh, "iscrowd": 0})
    path = os.path.join(root, "ann.json")
    with open(path, "w") as f:
        json.dump({"images": images, "annotations": anns,
                   "categories": [{"id": k, "name": str(k)} for k in range(1, 81)]}, f)
    return path


def identity(batch):
    return batch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batches", type=int, default=36, help="batches per timed window")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--boxes", type=int, default=7)
    ap.add_argument("--workers", type=int, default=12)
    ap.add_argument("--cached-workers", type=int, default=8)
    a = ap.parse_args()
    B, S, K = a.batch, a.size, a.batches
    with tempfile.TemporaryDirectory() as root:
        t0 = time.perf_counter()
        ann = make_coco(root, a.images, a.boxes)
        print(f"# {a.images} JPEGs of {SRC[1]}x{SRC[0]} written in {time.perf_counter() - t0:.1f} s", flush=True)
        args = (root, ann, AUG, True, (S, S), 80)
        ds = D.COCODataset(*args, seed=0, mosaic=True)
        resident = torch.zeros(len(ds), dtype=torch.uint8).share_memory_()
        cd = C.CachedCOCODataset(*args, seed=0, mosaic=True, resident=resident)

        t0 = time.perf_counter()
        for i in range(min(64, len(ds))):
            ds._load(i)
        decode_ms = (time.perf_counter() - t0) * 1e3 / min(64, len(ds))

        def loader(dataset, workers):
            sampler = torch.utils.data.RandomSampler(dataset, replacement=True, num_samples=K * B)
            return torch.utils.data.DataLoader(dataset, batch_size=B, sampler=sampler, num_workers=workers,
                                               collate_fn=identity, persistent_workers=workers > 0)

        loaders = {"parent": loader(ds, max(0, min(12, a.workers))), "cached": loader(cd, max(0, a.cached_workers))}
        for ld in loaders.values():             # start the persistent workers now, before the GPU is opened
            iter(ld)
        if not torch.cuda.is_available():
            sys.exit("input_micro: needs a ROCm GPU (no CPU fallback)")
        cache = C.DeviceImageCache.for_dataset(cd, a.images * SRC[0] * SRC[1] * 3 + (1 << 20), "cuda",
                                               chunk_bytes=1 << 28, resident=resident)
        assert cache.fill(ds) == len(ds) and cache.num_resident == len(ds)
        torch.cuda.synchronize()
        collates = {"parent": lambda b: D.collate_to_gpu(b, (S, S), "cuda", torch.bfloat16),
                    "cached": lambda b: C.collate_cached(b, cache, (S, S), "cuda", torch.bfloat16)}
        print(f"# PIL decode + convert + np.array, one core: {decode_ms:.2f} ms per image", flush=True)

        def window(name):
            collate = collates[name]
            torch.cuda.synchronize()
            host = wait = 0.0
            c0, t0 = time.process_time(), time.perf_counter()
            it = iter(loaders[name])
            for _ in range(K):
                w0 = time.perf_counter()
                batch = next(it)
                h0 = time.perf_counter()
                collate(batch)
                h1 = time.perf_counter()
                wait += h0 - w0
                host += h1 - h0
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            return K / dt, host * 1e3 / K, wait * 1e3 / K, (time.process_time() - c0) * 1e3 / K

        for name in loaders:                    # warm-up: code objects, pinned blocks, allocator
            window(name)
        probe = [cd[int(i)] for i in np.random.default_rng(1).integers(0, len(cd), B)]
        assert all(not images for _, _, images in probe)
        for _ in range(2):
            t0 = time.perf_counter()
            C.batch_tables(probe, cache, (S, S))
            tables_ms = (time.perf_counter() - t0) * 1e3
        x, t = collates["cached"](probe)
        kept = int((t[:, 0] >= 0).sum())
        print(f"# cached collate's host half (batch_tables, {B} MixUp samples): {tables_ms:.2f} ms; "
              f"targets {tuple(t.shape)} padded, {kept} boxes kept", flush=True)

        print(f"# B={B} {S}x{S} bf16, mosaic 1 / mixup 1, {K} batches per window, parent workers "
              f"{loaders['parent'].num_workers}, cached workers {loaders['cached'].num_workers}")
        for r in range(a.rounds):
            for name in loaders:
                bps, host, wait, cpu = window(name)
                print(f"round {r} {name:7s} {bps:7.2f} batches/s {bps * B:8.0f} img/s   main process per batch: "
                      f"collate {host:7.2f} ms, wait {wait:7.2f} ms, cpu {cpu:7.2f} ms", flush=True)
        del loaders


if __name__ == "__main__":
    main()
