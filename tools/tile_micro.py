"""Dev tool: what tiled inference costs -- YOLOv8-s, bf16, tile 640, nc=80, four 2048 x 2048 images,
overlap 0.2, the full view on: 16 windows + 1 = 17 slots per image, 68 tile inputs run as three chunks
of 32 (the last padded with blanks).  Cases run alternately in one process, each timed between device
events in windows of at least 50 calls after a warm-up:
  draw        the three mosaic_normalize launches that draw all inputs from the originals
  fwd         the three eval forwards at batch 32 (random weights: the time does not depend on them)
  merge       yms_tile_merge without bounds (edge=None); bytes = rows read + rows written, and the rate
              beside yms_copy (the runtime's device-to-device copy) moving the same bytes
  merge_edge  the same with edge=32: score units re-read their row's box and test it
  copy        yms_copy of the merged tensor
  detect      ops.detect on the merged tensor (17 * 8400 rows per image), conf 0.001, IoU 0.65, multi-label
The merge and detect cases read synthetic predictions (a floor of uniform [0, 0.2) scores on random
boxes plus a few hundred confident boxes per tile); a random-weight head would make every pair a
candidate.  The buffers (384 MB per merge) are read again call after call and partly stay in the
256 MB Infinity Cache: the rates are cache-assisted, and comparable with each other only.
Usage: python tools/tile_micro.py [--rounds 3] [--images 4] [--calls 100]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "yolo-ms_amd")]
import numpy as np
import torch

from yms import _lib as L
from yms import data as D
from yms import ops, set_compute_dtype, tiles

H0 = W0 = 2048
TILE, OVERLAP, BATCH = 640, 0.2, 32
CONF, IOU, MAX_DET, MAX_NMS = 0.001, 0.65, 300, 30000


def synthetic_pred(T, A, nc, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    p = torch.empty((T, A, 4 + nc), device="cuda")
    p[..., :2] = torch.rand((T, A, 2), device="cuda", generator=g) * TILE
    p[..., 2:4] = torch.rand((T, A, 2), device="cuda", generator=g) * 96 + 4
    p[..., 4:] = torch.rand((T, A, nc), device="cuda", generator=g) * 0.2
    rows = torch.randint(0, A, (T, 300), device="cuda", generator=g)
    cls = torch.randint(0, nc, (T, 300), device="cuda", generator=g)
    p[torch.arange(T, device="cuda")[:, None], rows, 4 + cls] = torch.rand((T, 300), device="cuda", generator=g) * 0.7 + 0.25
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--images", type=int, default=4)
    ap.add_argument("--calls", type=int, default=100, help="timed calls per window (at least 50)")
    ap.add_argument("--variant", default="s")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tile_micro: needs a ROCm GPU (no CPU fallback)")
    from yolov8.yolov8 import YOLOv8
    B, nc, calls = a.images, 80, max(50, a.calls)
    torch.manual_seed(0)
    model = YOLOv8(a.variant, nc).cuda().eval()
    model.head.stride = torch.tensor([8.0, 16.0, 32.0])
    set_compute_dtype(model, torch.bfloat16)
    rng = np.random.default_rng(0)
    images = D.to_device([rng.integers(0, 256, (H0, W0, 3), dtype=np.uint8) for _ in range(B)], "cuda")
    shapes = [(H0, W0)] * B

    def table(edge):
        plans = tiles.tile_plans(shapes, TILE, OVERLAP, 1.0, True, edge)
        host = tiles.slot_table(plans)
        return plans, host, torch.from_numpy(host.reshape(-1).view(np.uint8)).pin_memory().to("cuda")

    plans, host, tab = table(None)
    _, _, tab_edge = table(32)
    S = host.shape[1]
    inputs = [(im, sl.plan) for im, slots in zip(images, plans) for sl in slots]
    T = len(inputs)
    inputs += [(images[0], tiles._blank_plan(TILE, D.MOSAIC_FILL, shapes[0]))] * (-T % BATCH)
    chunks = [inputs[k:k + BATCH] for k in range(0, len(inputs), BATCH)]

    def draw():
        return [D.mosaic_normalize([[im] for im, _ in c], [p for _, p in c], (TILE, TILE), dtype=torch.bfloat16)
                for c in chunks]

    xs = draw()

    def fwd():
        with torch.no_grad():
            for x in xs:
                model(x)

    with torch.no_grad():
        A = int(model(xs[0]).shape[1])
    pred = synthetic_pred(len(inputs), A, nc)
    merged = tiles.merge_slots(pred, tab, B, S)
    merged_edge = tiles.merge_slots(pred, tab_edge, B, S)
    cut = float((merged_edge[..., 4] == -1).float().mean()) - float((merged[..., 4] == -1).float().mean())
    ident = D.Frames([(1.0, 1.0, 0.0, 0.0, W0, H0)] * B, "cuda")
    kw = dict(multi_label=True, max_det=MAX_DET, max_nms=MAX_NMS)
    bytes_moved = 2 * merged.numel() * 4
    dst = torch.empty_like(merged)
    st = L.stream_ptr()
    det = ops.detect(merged, CONF, IOU, frames=ident, **kw)

    cases = [("draw", draw), ("fwd", fwd),
             ("merge", lambda: tiles.merge_slots(pred, tab, B, S)),
             ("merge_edge", lambda: tiles.merge_slots(pred, tab_edge, B, S)),
             ("copy", lambda: L.call("yms_copy", dst.data_ptr(), merged.data_ptr(), bytes_moved // 2, st)),
             ("detect", lambda: ops.detect(merged, CONF, IOU, frames=ident, **kw))]

    def timed(fn, k):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(k):
            fn()
        e.record()
        e.synchronize()
        return s.elapsed_time(e) / k

    for _, fn in cases:
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    print(f"# YOLOv8-{a.variant} bf16 nc={nc} tile {TILE} overlap {OVERLAP} full view: {B} images of {H0}x{W0} -> "
          f"{S} slots each, {T} tile inputs in {len(chunks)} chunks of {BATCH}, {A} rows per tile, {S * A} merged rows "
          f"per image; merge moves {bytes_moved / 1e6:.1f} MB (read + write); edge=32 suppresses {100 * cut:.1f} % of "
          f"the rows; candidates per image at conf {CONF}: {int(det.candidates.min())}..{int(det.candidates.max())} "
          f"(max_nms {MAX_NMS}); {calls} calls per window")
    for r in range(a.rounds):
        for label, fn in cases:
            ms = timed(fn, calls)
            extra = f"  {bytes_moved / ms / 1e6:7.0f} GB/s" if label in ("merge", "merge_edge", "copy") else ""
            print(f"round {r} {label:10s} {ms:8.4f} ms/call{extra}", flush=True)


if __name__ == "__main__":
    main()
