"""Main-stream time of the detection head inside a training step (dev tool).

Wraps the head's steps in the plan's schedule -- the HeadGroup, or with YMS_HEAD_GROUP=0 the ops of
model.head's convolutions -- between HIP events on the main stream, in the forward and in the
backward, and prints the median span over the timed steps.  It splices a stand-in for those steps
into plan.sched of the model's cached plan: a measuring aid for this process only.  The spans are
main-stream elapsed times: in the backward the side stream's weight gradients run beside them, as in
the step.
    YMS_HEAD_GROUP=0 python tools/head_span.py            # ungrouped
    YMS_HEAD_GROUP=2 python tools/head_span.py            # grouped forward + backward"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "yolo-ms_amd")]


class Span:
    """Stands in plan.sched for the head's steps: runs them between two events per direction."""

    def __init__(self, steps):
        self.steps = steps
        self.bwd_ops = tuple(op for s in reversed(steps) for op in getattr(s, "bwd_ops", (s,)))
        self.ev = {"fwd": [], "bwd": []}

    def _timed(self, key, fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        self.ev[key].append((a, b))

    def fwd(self, rt):
        self._timed("fwd", lambda: [s.fwd(rt) for s in self.steps])

    def bwd(self, rt):
        self._timed("bwd", lambda: [s.bwd(rt) for s in reversed(self.steps)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--version", default="s")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    from yms import set_compute_dtype
    from yms.plan import HeadGroup
    from yolov8.tools.loss import ComputeLoss
    from yolov8.yolov8 import YOLOv8
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = YOLOv8(a.version, 80).to(dev).train()
    set_compute_dtype(m, torch.bfloat16)
    x = torch.randn(a.batch, 3, a.size, a.size, device=dev)
    g = torch.Generator().manual_seed(1)
    tg = torch.cat([torch.randint(0, a.batch, (8 * a.batch, 1), generator=g).float(),
                    torch.randint(0, 80, (8 * a.batch, 1), generator=g).float(),
                    torch.rand(8 * a.batch, 2, generator=g) * 0.6 + 0.2, torch.rand(8 * a.batch, 2, generator=g) * 0.3 + 0.05],
                   1).to(dev)
    crit = ComputeLoss(m.head, 80, dev, (a.size, a.size))

    def step():
        for p in m.parameters():
            p.grad = None
        total, _ = crit.loss_tensor(m(x), tg)
        total.backward()

    step()
    plan = next(p for p in m.__dict__["_yms_plans"].values() if p.training)
    # the head's steps: the schedule entries (a HeadGroup, or the ungrouped ops) whose convolutions are
    # modules of model.head -- whatever their number (YMS_HEAD_FUSE=0 has 18 ops, not 15)
    head_convs = {id(c) for c in m.head.modules() if isinstance(c, torch.nn.Conv2d)}

    def in_head(s):
        ops = s.ops if isinstance(s, HeadGroup) else [s]
        convs = [c.conv for op in ops for c in getattr(op, "members", [op]) if hasattr(c, "conv")]
        return bool(convs) and all(id(c) in head_convs for c in convs)

    flags = [in_head(s) for s in plan.sched]
    nhead = flags.index(True)
    assert all(flags[nhead:]) and not any(flags[:nhead]), "the head's ops are expected at the end of the schedule"
    span = Span(plan.sched[nhead:])
    plan.sched[nhead:] = [span]
    for _ in range(a.warmup):
        step()
    span.ev = {"fwd": [], "bwd": []}
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(a.steps):
        step()
    t1.record()
    torch.cuda.synchronize()
    out = {"head_group": plan.opts.head_group, "ms_per_step_no_optimizer": round(t0.elapsed_time(t1) / a.steps, 3)}
    for k, evs in span.ev.items():
        out[f"head_{k}_us_median"] = round(statistics.median(s.elapsed_time(e) for s, e in evs) * 1e3, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
