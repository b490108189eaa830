"""Fine-tuning measurements on the GPU (bench.py's training workload under freeze patterns; bench.py itself
is not touched).

  step   one process = one tree (--root: this one, or a checkout of another commit with its library built)
         and one model; every configuration gets its own model, the timed rounds interleave them:
         forward + ComputeLoss + backward + SGD-nesterov over the trainable parameters, B=64, 640^2, bf16.
         Configurations: <pattern>[+ne]; pattern none | bb (["backbone"]) | bbneck (["backbone", "neck"]);
         +ne = yms.finetune's norm_eval on the frozen part ("none+ne": every BN module in eval mode, nothing
         frozen).  A tree without yms.finetune (the parent) runs the patterns without +ne: requires_grad is
         flipped as the reference's freeze_layers does.
  micro  yms_bn_frozen_act_bwd against the three-pass route (reduce, finalize without coefficients, apply
         with a zeroed table) on the step's layer shapes, bf16, SiLU, in place, interleaved rounds; the
         operands rotate through enough buffer sets to exceed the 256 MB memory-side cache.

One JSON line per measurement on stdout."""
import argparse
import json
import os
import statistics
import sys
import time

PATTERNS = {"none": [], "bb": ["backbone"], "bbneck": ["backbone", "neck"]}
MICRO_SHAPES = [(409600, 64), (102400, 128), (25600, 256), (409600, 320), (25600, 80)]
HBM_PEAK = 8.0e12          # bytes / s (MI355X_MICROARCH)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["step", "micro"])
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--tag", default="this")
    ap.add_argument("--version", default="s")
    ap.add_argument("--configs", default="none,bb,bbneck,bb+ne,bbneck+ne,none+ne")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--nc", type=int, default=80)
    ap.add_argument("--gts", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10, help="timed steps (micro: launches) per round")
    ap.add_argument("--warmup", type=int, default=6)
    return ap.parse_args()


def step_mode(a):
    import torch
    sys.path[:0] = [a.root]
    import bench                                     # the tree's own: synth_targets, make_sgd
    from yms import set_compute_dtype
    from yolov8.tools.loss import ComputeLoss
    from yolov8.yolov8 import YOLOv8

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.cuda.set_stream(torch.cuda.Stream(device=dev, priority=-1))       # as bench.py --priority 1
    x = torch.randn(a.batch, 3, a.size, a.size, device=dev, generator=torch.Generator(device=dev).manual_seed(1234))
    tg = bench.synth_targets(a.batch, a.nc, a.gts, 4321, dev)
    steps = {}
    for cfg in a.configs.split(","):
        pat, _, ne = cfg.partition("+")
        torch.manual_seed(0)
        m = YOLOv8(a.version, a.nc).to(dev)
        m.head.stride = torch.tensor([8.0, 16.0, 32.0])
        set_compute_dtype(m, torch.bfloat16)
        m.train()
        if ne:
            from yms import finetune
            if PATTERNS[pat]:
                finetune.freeze(m, PATTERNS[pat], norm_eval=True)
            else:
                finetune.norm_eval(m)
        else:
            for name, p in m.named_parameters():
                if any(s in name for s in PATTERNS[pat]):
                    p.requires_grad = False
        opt = bench.make_sgd([p for p in m.parameters() if p.requires_grad])
        crit = ComputeLoss(m.head, a.nc, dev, (a.size, a.size))

        def step(m=m, opt=opt, crit=crit):
            opt.zero_grad(set_to_none=True)
            crit.loss_tensor(m(x), tg)[0].backward()
            opt.step()

        for _ in range(a.warmup):
            step()
        steps[cfg] = step
    torch.cuda.synchronize()
    for r in range(a.rounds):
        for cfg, step in steps.items():
            step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                step()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) / a.steps * 1e3
            print(json.dumps({"kind": "step", "tree": a.tag, "version": a.version, "config": cfg, "round": r,
                              "ms_per_step": round(ms, 3)}), flush=True)


def micro_mode(a):
    import torch
    sys.path[:0] = [a.root, os.path.join(a.root, "yolo-ms_amd")]
    from yms import _lib as L

    st, BF = L.stream_ptr(), L.BF16
    for npix, c in MICRO_SHAPES:
        per_set = 2 * npix * c * 2
        nsets = max(2, min(16, -(-600_000_000 // per_set)))
        zs = [torch.randn(npix, c, device="cuda").to(torch.bfloat16) for _ in range(nsets)]
        gs = [torch.randn(npix, c, device="cuda").to(torch.bfloat16) for _ in range(nsets)]
        sc, sh = torch.rand(c, device="cuda") + 0.5, torch.randn(c, device="cuda") * 0.2
        mi = torch.cat([torch.randn(c, device="cuda") * 0.1, torch.rand(c, device="cuda") + 0.5])
        rows = L.lib().yms_bn_bwd_rows(npix, c)
        ws = torch.empty(rows * 2 * c, device="cuda")
        zero = torch.zeros(2 * c, device="cuda")
        cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
        dg, db = torch.empty(c, device="cuda"), torch.empty(c, device="cuda")
        P = lambda t: t.data_ptr()

        def one(z, g, sums):
            L.call("yms_bn_frozen_act_bwd", BF, npix, c, P(z), c, 0, P(g), c, 0, P(sc), P(sh), P(mi), 1, P(z), c, 0,
                   None, 0, 0, 0, P(ws), P(cnt), P(dg) if sums else None, P(db) if sums else None, st)

        def three(z, g, sums):
            L.call("yms_bn_act_bwd_reduce", BF, npix, c, P(z), c, 0, P(g), c, 0, P(sc), P(sh), P(mi), 1, P(ws), st)
            L.call("yms_bn_act_bwd_finalize", c, P(ws), rows, npix, P(dg) if sums else None, P(db) if sums else None,
                   None, st)
            L.call("yms_bn_act_bwd_apply", BF, npix, c, P(z), c, 0, P(g), c, 0, P(sc), P(sh), P(mi), P(zero), 1, P(z),
                   c, 0, None, 0, 0, 0, st)

        routes = {"one_pass+sums": (one, True), "three_pass+sums": (three, True), "one_pass": (one, False),
                  "three_pass": (three, False)}
        times = {k: [] for k in routes}
        k = 0
        for r in range(a.rounds + 1):                  # round 0 warms up
            for name, (fn, sums) in routes.items():
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(a.steps):
                    fn(zs[k % nsets], gs[k % nsets], sums)
                    k += 1
                e.record()
                torch.cuda.synchronize()
                if r:
                    times[name].append(s.elapsed_time(e) / a.steps * 1e3)
        nb = 3 * npix * c * 2                            # 2 * es read + es written per element
        for name, ts in times.items():
            us = statistics.median(ts)
            print(json.dumps({"kind": "micro", "route": name, "npix": npix, "c": c, "us": round(us, 2),
                              "us_min": round(min(ts), 2), "us_max": round(max(ts), 2),
                              "algorithmic_GBps": round(nb / us / 1e3, 1),
                              "hbm_peak_share": round(nb / (us * 1e-6) / HBM_PEAK, 3), "buffer_sets": nsets}), flush=True)
        del zs, gs


if __name__ == "__main__":
    args = parse()
    (step_mode if args.mode == "step" else micro_mode)(args)
