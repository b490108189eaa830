"""CPU tier: data-parallel gradient buckets under a frozen backbone, over gloo with world_size 2.

The plan's backward walks only the steps that run (Plan.bwd_sched); the bucketer is driven exactly as
runner._PlanFn.backward drives it, without the kernels.  The buckets must tile the trainable parameters'
gradients and nothing else, every bucket must be reduced exactly once although the backbone's ops are
never visited, and finish() must join."""
import os

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_dist_cpu import _free_port


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from yms import finetune, runner
        from yms.dist import GradBucketer
        from yolov8.yolov8 import YOLOv8
        m = YOLOv8("n", 3).train()
        frozen = finetune.freeze(m, ["backbone"])
        plan = runner.get_plan(m, [torch.empty(2, 3, 64, 64, device="meta")], torch.bfloat16, True)
        params = plan.params()
        names = {id(p): n for n, p in m.named_parameters()}
        # the runner's flat gradient arena: trainable parameters in backward-completion order
        offs, total = {}, 0
        for i in plan.pgrad_order:
            if params[i].requires_grad:
                offs[i] = total
                total += params[i].numel()
        pg = torch.empty(total)
        views = [pg[offs[i]:offs[i] + p.numel()].view(p.shape) if i in offs else None for i, p in enumerate(params)]
        bk = GradBucketer(bucket_cap_mb=0.5)
        launched, visited = [], 0
        for it in range(2):                           # twice: the cached bucket layout
            pg.copy_(torch.arange(total, dtype=torch.float32) % 97 * (rank + 1))
            bk.begin(plan, pg, None, views)
            for step in plan.bwd_sched:
                for op in getattr(step, "bwd_ops", (step,)):
                    visited += 1
                    if bk.pending(op):
                        assert op.runs_bwd
                        bk.op_done(op)
            launched.append(bk.launched_buckets)
            outstanding = len(bk.works)
            bk.finish()
        exp = torch.arange(total, dtype=torch.float32) % 97 * (1 + world) / 2
        buckets = bk.buckets
        tiles = buckets[0][0] == 0 and buckets[-1][1] == total and all(a[1] == b[0] for a, b in zip(buckets, buckets[1:]))
        trainable = sum(p.numel() for n, p in m.named_parameters() if p.requires_grad)
        in_arena = {names[id(params[i])] for i in offs}
        q.put((rank, torch.allclose(pg, exp), launched, len(buckets), outstanding, tiles, total == trainable,
               not (in_arena & set(frozen)), visited, 2 * sum(len(getattr(s, "bwd_ops", (s,))) for s in plan.sched),
               len(bk.works)))
    finally:
        dist.destroy_process_group()


def test_frozen_backbone_buckets_gloo_world2():
    world = 2
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
    for rank, averaged, launched, nb, outstanding, tiles, only_trainable, none_frozen, visited, all_ops, left in res:
        assert averaged, rank                                   # every element reduced (once: a second SUM would double it)
        assert launched == [nb, nb] and nb >= 3 and outstanding == nb, (launched, nb, outstanding)
        assert tiles and only_trainable and none_frozen
        assert visited < all_ops                                # the backbone's ops were never visited
        assert left == 0                                        # finish() joined everything
