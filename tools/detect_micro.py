"""Dev tool: the COCO-protocol detect in isolation -- B=32, A=8400, nc=80 on tests/test_nms_gpu.py-style
clustered input (20 objects x 30 jittered boxes per image over a floor of uniform [0, 0.2) scores).
Four cases run alternately in one process, each timed between device events in windows of at least
50 calls after a warm-up:
  nms_idx     ops.batched_nms_indices(conf 0.25)                      (a) the post-process as it was
  det_best    ops.detect(conf 0.25, best-class, max_nms 30000)        (a) the same NMS + the new stages
  det_coco    ops.detect(conf 0.001, multi_label, max_nms 30000, max_det 300)   (b)
  cand_coco   yms_det_candidates alone at conf 0.001, multi_label     (c) against its streaming bound:
              B * A * (4 + nc) * 4 bytes per pass over pred (90 MB here); an image whose candidates fit
              max_nms is read by 2 passes (count, write), an overflowing one by 5 (count, two more
              histograms, rank, write)
Prints ms per call per case and round, and for cand_coco the share of the HBM bound.
Usage: python tools/detect_micro.py [--rounds 3] [--batch 32] [--calls 400]"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "yolo-ms_amd")]
import numpy as np
import torch

from yms import _lib as L
from yms import ops

HBM_GBS = 8000.0


def clustered(B, nc, K=20, J=30, A=8400, seed=0):
    rng = np.random.default_rng(seed)
    pred = np.zeros((B, A, 4 + nc), np.float32)
    pred[..., 4:] = rng.uniform(0, 0.2, (B, A, nc)).astype(np.float32)
    for b in range(B):
        for _ in range(K):
            cx, cy = rng.uniform(40, 600, 2)
            w, h = rng.uniform(20, 200, 2)
            lab = rng.integers(0, nc)
            for _ in range(J):
                a = rng.integers(0, A)
                pred[b, a, :4] = [cx + rng.normal(0, 4), cy + rng.normal(0, 4), w * rng.uniform(0.8, 1.2),
                                  h * rng.uniform(0.8, 1.2)]
                pred[b, a, 4 + lab] = rng.beta(2, 5) + 0.25
        bg = pred[b, :, 2] == 0
        pred[b, bg, :2] = rng.uniform(0, 640, (bg.sum(), 2))
        pred[b, bg, 2:4] = rng.uniform(4, 100, (bg.sum(), 2))
    return pred


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--calls", type=int, default=400, help="timed calls per window (at least 50)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("detect_micro: needs a ROCm GPU (no CPU fallback)")
    B, A, nc, K = a.batch, 8400, 80, 30000
    calls = max(50, a.calls)
    d = torch.from_numpy(clustered(B, nc, A=A)).cuda()
    i32 = dict(dtype=torch.int32, device="cuda")
    cb, cs = torch.empty((B, K, 4), device="cuda"), torch.empty((B, K), device="cuda")
    cl, ca = torch.empty((B, K), **i32), torch.empty((B, K), **i32)
    cc, ct = torch.empty(B, **i32), torch.empty(B, **i32)
    wsb = L.lib().yms_det_ws_bytes(B, A, nc, K)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    st = L.stream_ptr()

    def cand():
        L.call("yms_det_candidates", B, A, nc, d.data_ptr(), ctypes.c_float(0.001), 1, None, K, cb.data_ptr(),
               cs.data_ptr(), cl.data_ptr(), ca.data_ptr(), cc.data_ptr(), ct.data_ptr(), ws.data_ptr(), wsb, st)

    cases = [("nms_idx", lambda: ops.batched_nms_indices(d, 0.25, 0.45)),
             ("det_best", lambda: ops.detect(d, 0.25, 0.45, max_nms=K)),
             ("det_coco", lambda: ops.detect(d, 0.001, 0.45, multi_label=True, max_nms=K, max_det=300)),
             ("cand_coco", cand)]

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
    over = int((ct > K).sum())
    passes = (2 * (B - over) + 5 * over) / B
    pass_mb = B * A * (4 + nc) * 4 / 1e6
    bound_ms = passes * pass_mb / HBM_GBS
    print(f"# B={B} A={A} nc={nc} max_nms={K}: candidates at conf 0.001 per image {int(ct.min())}..{int(ct.max())}, "
          f"{over} of {B} images overflow -> {passes:.2f} passes of {pass_mb:.1f} MB, HBM bound {bound_ms:.4f} ms "
          f"at {HBM_GBS:.0f} GB/s; {calls} calls per window")
    for r in range(a.rounds):
        for label, fn in cases:
            ms = timed(fn, calls)
            extra = f"  {100 * bound_ms / ms:5.1f}% of the HBM bound" if label == "cand_coco" else ""
            print(f"round {r} {label:9s} {ms:8.4f} ms/call{extra}", flush=True)


if __name__ == "__main__":
    main()
