"""Dev tool: the SPPF pool chain in isolation -- yms_sppf_pool_fwd / yms_sppf_pool_bwd over a 4-slot
concat buffer (ld = 4c), bf16, timed between device events in windows of at least 0.2 s after a
warm-up.  Blocks of route 0 (one launch per pool; argmax + gather per pool in the backward) and
route 1 (one launch per direction, planes in LDS) alternate in one process (yms_sppf_route_set).
Cases: the training line's plane (64, 20, 20, 256) forward and backward, and the inference line's
(32, 20, 20, 256) forward.  Prints us per call and the GB/s of the chain's algorithmic bytes
(forward: 1 slot read + 3 written; backward: 3 value + 4 gradient slots read, 3 written).
Usage: python tools/sppf_micro.py [--rounds 3]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "yolo-ms_amd")]
import torch

from yms import _lib as L

CASES = [("fwd", 64, 20, 20, 256), ("bwd", 64, 20, 20, 256), ("fwd", 32, 20, 20, 256)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.2, help="least seconds per timed window")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sppf_micro: needs a ROCm GPU (no CPU fallback)")
    code, st = L.dtype_code(torch.bfloat16), L.stream_ptr()
    g = torch.Generator().manual_seed(0)
    runs = []
    for kind, n, h, w, c in CASES:
        ld = 4 * c
        buf = torch.randn(n, h, w, ld, generator=g).to(torch.bfloat16).cuda()
        L.call("yms_sppf_pool_fwd", code, n, h, w, c, buf.data_ptr(), ld, 0, st)
        gb = torch.randn(n, h, w, ld, generator=g).to(torch.bfloat16).cuda()
        ws = torch.empty(L.lib().yms_sppf_ws_bytes(n, h, w, c), dtype=torch.uint8, device="cuda")
        slot = n * h * w * c * 2
        if kind == "fwd":
            def launch(k, n=n, h=h, w=w, c=c, ld=ld, buf=buf):
                for _ in range(k):
                    L.call("yms_sppf_pool_fwd", code, n, h, w, c, buf.data_ptr(), ld, 0, st)
            nbytes = 4 * slot
        else:
            # the gradient buffer is accumulated in place call after call: the values grow (bf16
            # saturates to inf), the work per call does not depend on them
            def launch(k, n=n, h=h, w=w, c=c, ld=ld, buf=buf, gb=gb, ws=ws):
                for _ in range(k):
                    L.call("yms_sppf_pool_bwd", code, n, h, w, c, buf.data_ptr(), ld, 0, gb.data_ptr(), ld, 0,
                           ws.data_ptr(), st)
            nbytes = 10 * slot
        fits = L.lib().yms_sppf_fused_fits(code, h, w, c)
        runs.append((f"{kind} ({n}, {h}, {w}, {c})", launch, nbytes, fits))

    def timed(launch, k):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        launch(k)
        e.record()
        e.synchronize()
        return s.elapsed_time(e) * 1e3 / k          # us per call

    prev = L.lib().yms_sppf_route_set(-1)
    iters = {}
    for label, launch, _, _ in runs:
        for route in (0, 1):
            L.lib().yms_sppf_route_set(route)
            launch(10)
            torch.cuda.synchronize()
            iters[label, route] = max(20, int(a.window * 1e6 / timed(launch, 20)) + 1)
    print("# SPPF pool chain, bf16, ld = 4c; route 0 = one launch per pool (backward: argmax + gather per pool), "
          "route 1 = one launch per direction")
    for r in range(a.rounds):
        for label, launch, nbytes, fits in runs:
            for route in (0, 1):
                L.lib().yms_sppf_route_set(route)
                us = timed(launch, iters[label, route])
                print(f"round {r} {label:24s} route {route} (fused fits: {fits}) {us:8.2f} us/call "
                      f"{nbytes / us / 1e3:8.1f} GB/s", flush=True)
    L.lib().yms_sppf_route_set(prev)


if __name__ == "__main__":
    main()
