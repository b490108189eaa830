"""Reference and runner for the fine-tuning tests.

oracle_step: oracle.model_ref / oracle.ms_ref in fp64 on the CPU with the Conv blocks named in `eval_bn`
run with training=False (running statistics, buffers untouched) -- their conv_block is wrapped for the
duration of the call -- and only the parameters outside `frozen` requiring a gradient.
gpu_step: the same step(s) of the planned model under a freeze pattern, collecting maps, gradients and
buffers."""
import pytest
import torch

from oracle import model_ref as M
from oracle import ms_ref as MS
from yms import finetune, set_compute_dtype
from yolov8.yolov8 import YOLOv8

X_SEED = 3


def fixture(v, nc, size=(64, 64)):
    ms = v.startswith("ms-")
    sd = M.ordered_init((MS if ms else M).init_params(v, nc))
    x = torch.randn(2, 3, *size, generator=torch.Generator().manual_seed(X_SEED + nc))
    if ms:
        # eval-mode BN layers use the running statistics: as in a pretrained model they match the data
        # (oracle.ms_ref.calibrate).  With the closed-form buffers the MS stacks leave their training scale
        # and torch's own CPU fp32 run of this step misses fp64 by 9e-4 of a map's maximum, the whole gate.
        sd = MS.calibrate(sd, v, nc, x)
    return sd, x


def frozen_names(sd, patterns):
    return [k for k in sd if any(p in k for p in patterns) and "running" not in k and "num_batches" not in k]


def eval_blocks(sd, patterns, norm_eval, frozen):
    """The Conv blocks whose BN is in eval mode: norm_eval=True -> those whose gamma and beta are frozen
    (finetune.freeze), "all" -> every block, a list -> those names."""
    blocks = [k[:-len(".bn.weight")] for k in sd if k.endswith(".bn.weight")]
    if norm_eval == "all":
        return set(blocks)
    if isinstance(norm_eval, (list, tuple)):
        return set(norm_eval)
    if not norm_eval:
        return set()
    return {b for b in blocks if f"{b}.bn.weight" in frozen and f"{b}.bn.bias" in frozen}


def oracle_step(v, nc, sd, x, frozen=(), eval_bn=()):
    """-> (maps, {name: fp64 gradient}, {name: buffer after the step})."""
    ms = v.startswith("ms-")
    p = {}
    for k, t in sd.items():
        t = t.clone().double() if t.is_floating_point() else t.clone()
        if t.is_floating_point() and "running" not in k and k != "head.dfl.conv.weight" and k not in frozen:
            t.requires_grad_(True)
        p[k] = t
    with pytest.MonkeyPatch.context() as mp:
        for mod in (M, MS):
            real = mod.conv_block

            def wrapped(p_, name, x_, k, s, training, *a, _real=real, **kw):
                return _real(p_, name, x_, k, s, training and name not in eval_bn, *a, **kw)

            mp.setattr(mod, "conv_block", wrapped)
        outs = (MS if ms else M).forward(p, v, nc, x.double(), True)
    sum((o ** 2).mean() for o in outs).backward()
    grads = {k: t.grad for k, t in p.items() if t.is_floating_point() and t.grad is not None}
    bufs = {k: t.detach() for k, t in p.items() if "running" in k or "num_batches" in k}
    return [o.detach() for o in outs], grads, bufs


def apply_pattern(m, patterns, norm_eval):
    if patterns:
        finetune.freeze(m, patterns, norm_eval=norm_eval is True)
    if norm_eval == "all":
        finetune.norm_eval(m)
    elif isinstance(norm_eval, (list, tuple)):
        for name in norm_eval:                      # by hand, as a user would: no helper
            m.get_submodule(name).bn.eval()


def gpu_step(v, nc, sd, x, dtype, patterns=(), norm_eval=False, env=None, steps=1, opt=None):
    """-> dict(maps, grads {name: tensor | None}, before / after buffers, params, plan, model); env: switches
    set for the duration of the run; opt: callable(trainable parameters) -> optimizer, stepped after each
    backward."""
    with pytest.MonkeyPatch.context() as mp:
        for k, val in (env or {}).items():
            mp.setenv(k, str(val))
        m = YOLOv8(v, nc).cuda()
        m.load_state_dict(sd)
        set_compute_dtype(m, dtype)
        m.train()
        apply_pattern(m, list(patterns), norm_eval)
        before = {k: t.clone() for k, t in m.named_buffers()}
        o = opt([q for q in m.parameters() if q.requires_grad]) if opt is not None else None
        xg = x.cuda()
        for _ in range(steps):
            for q in m.parameters():
                q.grad = None
            outs = m(xg)
            sum((t.double() ** 2).mean() for t in outs).backward()
            if o is not None:
                o.step()
        torch.cuda.synchronize()
        plans = [pl for pl in m.__dict__["_yms_plans"].values() if pl.training]
        assert len(plans) == 1
        return dict(maps=[t.detach().clone() for t in outs],
                    grads={k: (q.grad.clone() if q.grad is not None else None) for k, q in m.named_parameters()},
                    before=before, after={k: t.clone() for k, t in m.named_buffers()},
                    params={k: q.detach().clone() for k, q in m.named_parameters()}, plan=plans[0], model=m)
