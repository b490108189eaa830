"""Dev tool: the optimizer step in isolation, torch's fused optimizers against yms.optim, on the parameter
sets of YOLOv8-s and YOLO-MS-L with the gradients as views of one flat arena (as the backward leaves them).

Per pair the two arms alternate in one process (REPS rounds each); a round is a device-event time over
enough step() calls to fill about 1 s / REPS after a warm-up, so it contains the host's share of a step,
as a training loop pays it.  Printed: us per step (median and min..max over the rounds), launches per step
(yms: counted by the optimizer; torch: not counted here, 5 multi_tensor_apply per SGD step in
profiles/r06final2_stats_train_summary.txt) and the achieved bytes/s from the algorithmic bytes: 20 B
(SGD) / 28 B (Adam, AdamW) per parameter element, + 8 B per EMA element (parameters and float buffers).
"yms launches only" is the yms arm's yms_optim_step(_ext) call without step()'s host work, for reading how
much of a step is the host's.  The "adamw+ema(exp)+schedule" pair is the YOLO-MS recipe's step: yms
evaluates the warm-up / cosine schedule on the device, the torch arm pays a LambdaLR step per iteration.
--ab-lib adds "ab launches only" to the SGD / Adam pairs: another build's yms_optim_step on the same
table, alternating with this build's, for comparing the kernels of two commits in one process.

    python tools/optim_micro.py [--models s,ms-l] [--out profiles/optim_micro.txt] [--ab-lib other/libyms.so]
"""
import argparse
import copy
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "yolo-ms_amd")]
import torch  # noqa: E402

from yms import _lib as L  # noqa: E402
from yms import optim as O  # noqa: E402
from yolov8.yolov8 import YOLOv8  # noqa: E402

REPS = 5
DECAY = 0.9999
# (label, kind, with_ema, recipe): recipe = exp-momentum EMA and a warm-up + cosine schedule that is mid-cosine
VARIANTS = [("sgd     ", "sgd", False, False), ("sgd +ema", "sgd", True, False), ("adam    ", "adam", False, False),
            ("adam+ema", "adam", True, False), ("adamw   ", "adamw", False, False),
            ("adamw+ema(exp)+schedule", "adamw", True, True)]
SCHEDULE = [O.Segment(0, 1000, 1e-5, 1.0), O.Segment(0, 10 ** 7, 1.0, 0.05, shape="cosine")]


def flat_grads(params, seed):
    arena = torch.randn(sum(p.numel() for p in params), device="cuda",
                        generator=torch.Generator(device="cuda").manual_seed(seed)) * 1e-3
    off = 0
    for p in params:
        p.grad = arena[off:off + p.numel()].view(p.shape)
        off += p.numel()
    return arena


class TorchEma:
    """ModelEMA's update with torch's multi-tensor ops (the decay is fixed: the schedule costs nothing)."""

    def __init__(self, model):
        self.src = [t for t in model.state_dict(keep_vars=True).values() if t.is_floating_point()]
        self.ema = [t.detach().clone() for t in self.src]

    @torch.no_grad()
    def update(self):
        torch._foreach_mul_(self.ema, DECAY)
        torch._foreach_add_(self.ema, [t.detach() for t in self.src], alpha=1.0 - DECAY)


def arms(version, kind, with_ema, recipe=False, ab_lib=None):
    """-> {arm name: (step fn, launches fn, algorithmic bytes)} on two copies of the model."""
    torch.manual_seed(0)
    base = YOLOv8(version, 80).cuda()
    out = {}
    for name in ("torch", "yms"):
        m = copy.deepcopy(base)
        params = [p for p in m.parameters() if p.requires_grad]
        keep = flat_grads(params, 1)
        n = sum(p.numel() for p in params)
        ne = sum(t.numel() for t in m.state_dict().values() if t.is_floating_point()) if with_ema else 0
        nbytes = n * (20 if kind == "sgd" else 28) + 8 * ne
        if name == "torch":
            if kind == "sgd":
                opt = torch.optim.SGD(params, lr=0.01, momentum=0.937, nesterov=True, weight_decay=5e-4, fused=True)
            elif kind == "adam":
                opt = torch.optim.Adam(params, lr=1e-3, weight_decay=5e-4, fused=True)
            else:
                opt = torch.optim.AdamW(params, lr=1e-3, weight_decay=0.05, fused=True)
            ema = TorchEma(m) if with_ema else None
            sch = torch.optim.lr_scheduler.LambdaLR(opt, lambda n: O.schedule_factor(SCHEDULE, n)) if recipe else None

            def step(opt=opt, ema=ema, sch=sch):
                opt.step()
                if ema is not None:
                    ema.update()
                if sch is not None:
                    sch.step()
            launches = lambda: "-"
        else:
            if kind == "sgd":
                opt = O.SGD(params, lr=0.01, momentum=0.937, nesterov=True, weight_decay=5e-4)
            elif kind == "adam":
                opt = O.Adam(params, lr=1e-3, weight_decay=5e-4)
            else:
                opt = O.AdamW(params, lr=1e-3, weight_decay=0.05, schedule=SCHEDULE if recipe else None)
            if with_ema:
                opt.attach_ema(m, decay=DECAY, tau=2000, **(dict(rule="exp_momentum") if recipe else {}))
            step = opt.step
            launches = lambda opt=opt: opt.last_launches
        out[name] = (step, launches, nbytes, (m, keep, opt), len(params), n)
    # the yms arm's two launches alone, without step()'s host work (table lookup, version bumps)
    opt.step()
    (table, nchunks, _, _), gbase = opt._step_table()
    args = (opt._KIND, table.data_ptr(), nchunks, gbase, opt._hyper.data_ptr(), opt._counters.data_ptr(), None, 0)
    if opt._use_ext():
        ext = opt._ext.data_ptr() if recipe else None
        raw = lambda: L.call("yms_optim_step_ext", *args[:5], ext, args[5], opt._sched.data_ptr(), None, 0, L.stream_ptr())
    else:
        raw = lambda: L.call("yms_optim_step", *args, L.stream_ptr())
    out["yms launches only"] = (raw, lambda: 2, nbytes, None, len(params), n)
    if ab_lib is not None and not opt._use_ext():
        fn = ab_lib.yms_optim_step
        fn.restype, fn.argtypes = L._SIGS["yms_optim_step"]
        out["ab launches only"] = (lambda: L.check(fn(*args, L.stream_ptr()), "ab yms_optim_step"), lambda: 2, nbytes,
                                   None, len(params), n)
    return out


def timed(step, n):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        step()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / n          # us per step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="s,ms-l")
    ap.add_argument("--out", default=None)
    ap.add_argument("--ab-lib", default=None)
    a = ap.parse_args()
    ab_lib = ctypes.CDLL(os.path.abspath(a.ab_lib)) if a.ab_lib else None
    assert torch.cuda.is_available(), "optim_micro needs a ROCm GPU"
    lines = [f"optimizer step, torch fused vs yms.optim, {torch.cuda.get_device_name(0)}, torch {torch.__version__}; "
             f"{REPS} alternating rounds per arm, us per step() (device events around the loop)"]
    print(lines[0], flush=True)
    for version in a.models.split(","):
        for label, kind, with_ema, recipe in VARIANTS:
            pair = arms(version, kind, with_ema, recipe, ab_lib)
            for step, *_ in pair.values():
                for _ in range(10):
                    step()
            torch.cuda.synchronize()
            count = {k: max(10, int(1e6 / REPS / max(timed(v[0], 20), 1.0))) for k, v in pair.items()}
            us = {k: [] for k in pair}
            for _ in range(REPS):
                for k, v in pair.items():
                    us[k].append(timed(v[0], count[k]))
            med = {k: statistics.median(v) for k, v in us.items()}
            spread = max(us["torch"]) - min(us["torch"])
            _, _, nbytes, _, ntens, nelem = pair["yms"]
            head = len(lines)
            lines.append(f"{version:5s} {label} {ntens:4d} tensors {nelem / 1e6:6.2f} M elements")
            for k, v in pair.items():
                lines.append(f"    {k:17s} {med[k]:8.1f} us/step  (min {min(us[k]):7.1f} max {max(us[k]):7.1f}, {count[k]} steps/round)"
                             f"  launches/step {v[1]()!s:>2s}  {v[2] / med[k] / 1e3:7.0f} GB/s")
            verdict = "no slower" if med["yms"] <= med["torch"] + spread else "SLOWER"
            lines.append(f"    yms / torch = {med['yms'] / med['torch']:.3f}  (torch spread {spread:.1f} us): yms is {verdict}")
            for ln in lines[head:]:
                print(ln, flush=True)
            del pair
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
