"""Dev tool: the detection losses in isolation -- yms_tal_loss (task-aligned assigner, opt-in),
yms_dsl_loss (dynamic soft-label assigner + QFL + GIoU, YOLO-MS's own, opt-in) and yms_det_loss (the
reference's ComputeLoss) alternated in one process on the same head maps: B=64,
640x640 (8400 anchors), nc=80, bf16 NHWC maps with channel stride 144, value + gradient, 8 and 40
GTs per image.  Maps, gradients, targets and workspaces are allocated once; the timed work is the
launches only, between device events, in windows of at least 0.5 s after a warm-up.  Prints ms per
call, the algorithmic bytes (maps read once + gradient written once) and the bytes/s achieved.
Usage: python tools/loss_micro.py [--rounds 3] [--batch 64] [--size 640] [--gts 8 40] [--losses tal dsl det]"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "yolo-ms_amd")]
import torch

from yms import _lib as L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--nc", type=int, default=80)
    ap.add_argument("--gts", type=int, nargs="+", default=[8, 40])
    ap.add_argument("--losses", nargs="+", default=["tal", "dsl", "det"], choices=["tal", "dsl", "det"])
    ap.add_argument("--window", type=float, default=0.5, help="least seconds per timed window")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("loss_micro: needs a ROCm GPU (no CPU fallback)")
    B, S, nc = a.batch, a.size, a.nc
    dev, dt = "cuda", torch.bfloat16
    C = 64 + nc
    ld = (C + 7) // 8 * 8
    strides = (8.0, 16.0, 32.0)
    hs = [S // int(s) for s in strides]
    A = sum(h * h for h in hs)
    g = torch.Generator().manual_seed(0)
    maps, grads = [], []
    for h in hs:
        m = torch.randn(B, h, h, ld, generator=g) * 1.5
        for side in range(4):                   # boxes of ~2 strides per side, as a part-trained head's
            m[..., side * 16 + 1:side * 16 + 4] += 3.0
        m[..., 64:] -= 3.0                      # mostly-background class scores
        maps.append(m.to(dev, dt))
        grads.append(torch.zeros(B, h, h, ld, dtype=dt, device=dev))
    n = len(maps)
    mp = (ctypes.c_void_p * n)(*[m.data_ptr() for m in maps])
    gp = (ctypes.c_void_p * n)(*[t.data_ptr() for t in grads])
    hsa = (ctypes.c_int * n)(*hs)
    sta = (ctypes.c_float * n)(*strides)
    lam = (ctypes.c_float * 3)(7.5, 0.5, 1.5)
    gains = (ctypes.c_float * 3)(2.0, 1.0, 0.0)
    out = torch.empty(5, dtype=torch.float32, device=dev)
    st = L.stream_ptr()
    code = L.dtype_code(dt)
    fS = ctypes.c_float(float(S))
    nbytes = 2 * B * A * C * 2                  # maps read + gradient written, bf16

    def targets(per_img):
        wh = torch.rand(B * per_img, 2, generator=g) * 0.4 + 0.05
        c = torch.rand(B * per_img, 2, generator=g) * (1 - wh) + wh / 2
        img = torch.arange(B).repeat_interleave(per_img).float()[:, None]
        cls = torch.randint(0, nc, (B * per_img, 1), generator=g).float()
        return torch.cat([img, cls, c, wh], 1).to(dev).contiguous()

    cases = []
    for per_img in a.gts:
        tg = targets(per_img)
        M = tg.shape[0]
        wt = torch.empty(L.lib().yms_tal_loss_ws_bytes(B, A, nc, M), dtype=torch.uint8, device=dev)
        wd = torch.empty(L.lib().yms_det_loss_ws_bytes(B, A, nc, M), dtype=torch.uint8, device=dev)
        wq = torch.empty(L.lib().yms_dsl_loss_ws_bytes(B, A, nc, M), dtype=torch.uint8, device=dev)
        cases.append((f"tal gt{per_img}", lambda tg=tg, M=M, wt=wt: L.call(
            "yms_tal_loss", code, B, nc, n, mp, gp, hsa, hsa, sta, ld, tg.data_ptr(), M, fS, fS, 10,
            ctypes.c_float(0.5), ctypes.c_float(6.0), lam, wt.data_ptr(), wt.numel(), out.data_ptr(), None, None, st)))
        cases.append((f"dsl gt{per_img}", lambda tg=tg, M=M, wq=wq: L.call(
            "yms_dsl_loss", code, B, nc, n, mp, gp, hsa, hsa, sta, ld, tg.data_ptr(), M, fS, fS, 13,
            ctypes.c_float(3.0), ctypes.c_float(3.0), ctypes.c_float(2.0), gains, wq.data_ptr(), wq.numel(),
            out.data_ptr(), None, None, None, st)))
        cases.append((f"det gt{per_img}", lambda tg=tg, M=M, wd=wd: L.call(
            "yms_det_loss", code, B, nc, n, mp, gp, hsa, hsa, sta, ld, tg.data_ptr(), M, fS, fS, 3, None, lam,
            wd.data_ptr(), wd.numel(), out.data_ptr(), st)))

    def timed(fn, k):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(k):
            fn()
        e.record()
        e.synchronize()
        return s.elapsed_time(e) / k            # ms per call

    cases = [(label, fn) for label, fn in cases if label.split()[0] in a.losses]
    iters = {}
    for label, fn in cases:                     # warm-up, then size the window from a short timed run
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        iters[label] = max(10, int(a.window * 1e3 / timed(fn, 10)) + 1)
    print(f"# B={B} {S}x{S} nc={nc} bf16 ld={ld} anchors={A}: algorithmic {nbytes / 1e6:.1f} MB per call "
          f"(maps read + gradient written); iterations per window {iters}")
    for r in range(a.rounds):
        for label, fn in cases:
            ms = timed(fn, iters[label])
            print(f"round {r} {label:10s} {ms:8.4f} ms/call {nbytes / (ms * 1e-3) / 1e9:8.1f} GB/s", flush=True)


if __name__ == "__main__":
    main()
