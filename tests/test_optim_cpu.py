"""CPU tier of yms.optim: the host-only table builder of csrc/optim.hip, the argument checks of its
entry points (no launch happens: the pointers are host dummies), the config reader and the
constructors' refusals."""
import ctypes

import pytest
import torch

from yms import _lib as L
from yms import optim as O
from yolov8.yolov8 import YOLOv8

C = 4096            # yms_optim_chunk_elems(), asserted below
PB, S0, S1, EB = 0x10000000, 0x20000000, 0x30000000, 0x40000000      # fake bases: only arithmetic is done on them


def _jobs():
    """(param, grad, state0, state1, ema, count, group, flags) for the issue's sizes, a job without a
    gradient and an EMA-only job; slots packed at 4-element granularity like yms.optim does."""
    rows, off, goff = [], 0, 4          # gradients at odd element offsets of an arena
    for i, n in enumerate((1, 3, C - 1, C, C + 1, 3 * C + 5)):
        fl = L.OPTIM_EMA if i % 2 else 0
        rows.append((PB + 4 * off, 4 * goff, off, off, off if fl else -1, n, i % 3, fl))
        off += (n + 3) // 4 * 4
        goff += n + 1
    rows.append((PB + 4 * off, 0, off, off, off, 700, 7, L.OPTIM_GRAD_NONE | L.OPTIM_EMA))      # frozen parameter
    off += 700
    rows.append((PB + 4 * off, 0, -1, -1, off, C + 9, 0, L.OPTIM_GRAD_NONE | L.OPTIM_EMA))      # EMA-only buffer
    rows.append((PB + 4 * (off + 2 * C), 0x7000_0004, 0, -1, -1, 5, 1, L.OPTIM_GRAD_ABS))       # absolute gradient
    return rows


def _arr(rows):
    return (L.OptimJob * len(rows))(*[L.OptimJob(*r) for r in rows])


def test_table_builder_covers_every_element_once():
    lib = L.lib()
    assert lib.yms_optim_chunk_elems() == C
    assert ctypes.sizeof(L.OptimChunk) == 48 and ctypes.sizeof(L.OptimJob) == 56
    rows = _jobs()
    arr = _arr(rows)
    want = sum(-(-r[5] // C) for r in rows)
    assert lib.yms_optim_table_chunks(len(rows), arr) == want
    nb = lib.yms_optim_table_bytes(len(rows), arr)
    assert nb == want * 48
    tab = (L.OptimChunk * want)()
    assert lib.yms_optim_table_build(len(rows), arr, S0, S1, EB, ctypes.addressof(tab), nb) == 0
    it = iter(tab)
    for (param, grad, s0, s1, ema, count, group, flags) in rows:
        done = 0
        while done < count:                   # the job's chunks follow each other and tile it exactly
            c = next(it)
            assert c.p == param + 4 * done
            assert c.n == min(C, count - done) and 1 <= c.n <= C      # never past the tensor's end
            assert (c.group, c.flags) == (group, flags)
            assert c.s0 == (None if s0 < 0 else S0 + 4 * (s0 + done))
            assert c.s1 == (None if s1 < 0 else S1 + 4 * (s1 + done))
            assert c.e == (None if ema < 0 else EB + 4 * (ema + done))
            if not flags & L.OPTIM_GRAD_NONE:
                assert c.g == grad + 4 * done
            done += c.n
        assert done == count
    assert next(it, None) is None
    # partial sums of the norm pass: one per chunk while few, a fixed 1024 then, <= 128 chunks per block always
    for n, g in ((1, 1), (1023, 1023), (1024, 1024), (5000, 1024), (131072, 1024), (131073, 1025), (1 << 22, 32768)):
        assert lib.yms_optim_norm_partials(n) == g
        assert -(-n // g) <= 128
    assert lib.yms_optim_norm_partials(0) == 0 and lib.yms_optim_norm_partials((1 << 22) + 1) == -1


def test_argument_validation():
    """One valid call per entry point with one argument broken -> YMS_ERR_INVALID before any launch."""
    lib = L.lib()
    buf = (ctypes.c_float * 64)()
    P = ctypes.addressof(buf)
    good = (PB, 16, 0, 0, 0, 100, 0, L.OPTIM_EMA)
    names = ("param", "grad", "state0", "state1", "ema", "count", "group", "flags")
    one = _arr([good])
    assert lib.yms_optim_table_chunks(1, one) == 1 and lib.yms_optim_table_bytes(1, one) == 48
    broken = dict(param_null=dict(param=None), count0=dict(count=0), count_neg=dict(count=-3), group_neg=dict(group=-1),
                  group8=dict(group=8), flag_unknown=dict(flags=8), none_and_abs=dict(flags=3),
                  grad_neg=dict(grad=-4), grad_unaligned=dict(grad=6), no_state=dict(state0=-1),
                  abs_null=dict(flags=L.OPTIM_GRAD_ABS, grad=0), ema_without_slot=dict(ema=-1), slot_bad=dict(state1=-2))
    tab = (L.OptimChunk * 4)()
    T = ctypes.addressof(tab)
    for label, change in broken.items():
        bad = _arr([tuple(change.get(k, v) for k, v in zip(names, good))])
        assert lib.yms_optim_table_chunks(1, bad) == -1, label
        assert lib.yms_optim_table_bytes(1, bad) == 0, label
        assert lib.yms_optim_table_build(1, bad, P, P, P, T, 192) == 1, label
    assert lib.yms_optim_table_chunks(-1, one) == -1 and lib.yms_optim_table_chunks(1, None) == -1
    assert lib.yms_optim_table_chunks(0, None) == 0

    def rows(name, good, **broken):
        fn = getattr(lib, name)
        for label, change in broken.items():
            assert set(change) <= set(good), (name, label)
            assert fn(*[change.get(k, v) for k, v in good.items()]) == 1, (name, label)

    rows("yms_optim_table_build", dict(njobs=1, jobs=one, s0=P, s1=P, ema=P, table=T, nbytes=48),
         njobs=dict(njobs=-1), jobs=dict(jobs=None), table=dict(table=None), small=dict(nbytes=47),
         s0_null=dict(s0=None), s1_null=dict(s1=None), ema_null=dict(ema=None))
    rows("yms_optim_grad_norm", dict(table=P, nchunks=2, base=P, partials=P, stream=None),
         table=dict(table=None), nchunks0=dict(nchunks=0), nchunks_neg=dict(nchunks=-2), partials=dict(partials=None))
    rows("yms_optim_step", dict(kind=L.OPTIM_ADAM, table=P, nchunks=2, base=P, hyper=P, counters=P, partials=P,
                                npartials=2, stream=None),
         kind=dict(kind=2), kind_neg=dict(kind=-1), table=dict(table=None), nchunks0=dict(nchunks=0),
         nchunks_neg=dict(nchunks=-1), nchunks_huge=dict(nchunks=1 << 31), hyper=dict(hyper=None),
         counters=dict(counters=None), partials_without_count=dict(npartials=0),
         count_without_partials=dict(partials=None), npartials_neg=dict(npartials=-1))
    rows("yms_optim_swap", dict(table=P, nchunks=2, stream=None), table=dict(table=None), nchunks0=dict(nchunks=0),
         nchunks_neg=dict(nchunks=-7))


def _cfg(**training):
    return {"training": dict({"learning_rate": 0.002, "weight_decay": 5e-4}, **training)}


def test_optimizer_config_reads_the_reference_keys():
    m = YOLOv8("n", 3)
    cls, groups, kw, ema = O.optimizer_config(m, _cfg(optimizer="SGD"))
    assert cls is O.SGD and ema is None
    assert kw == dict(lr=0.002, momentum=0.937, nesterov=True, weight_decay=5e-4, clip_grad_norm=None,
                      skip_nonfinite=False)
    assert [id(p) for p in groups] == [id(p) for p in m.parameters()]
    cls, groups, kw, ema = O.optimizer_config(m, _cfg(optimizer="adam"))
    assert cls is O.Adam and kw["betas"] == (0.9, 0.999) and kw["lr"] == 0.002 and kw["weight_decay"] == 5e-4
    cls, _, kw, ema = O.optimizer_config(m, _cfg(optimizer="adam", adam_betas=[0.8, 0.99], clip_grad_norm=10.0,
                                                 skip_nonfinite=True, ema={"tau": 500}))
    assert kw["betas"] == (0.8, 0.99) and kw["clip_grad_norm"] == 10.0 and kw["skip_nonfinite"] is True
    assert ema == {"decay": 0.9999, "tau": 500}
    _, _, kw, _ = O.optimizer_config(m, _cfg(optimizer="sgd", sgd_momentum=0.9, sgd_nesterov=False))
    assert kw["momentum"] == 0.9 and kw["nesterov"] is False
    for fn in (O.optimizer_config, O.build_optimizer):
        with pytest.raises(ValueError, match="Unsupported optimizer: lion"):
            fn(m, _cfg(optimizer="Lion"))


def test_no_decay_group_holds_bn_weights_and_biases():
    m = YOLOv8("n", 3)
    _, groups, _, _ = O.optimizer_config(m, _cfg(optimizer="sgd", no_decay_bn_bias=True))
    assert len(groups) == 2 and "weight_decay" not in groups[0] and groups[1]["weight_decay"] == 0.0
    nd = {id(p) for p in groups[1]["params"]}
    dc = {id(p) for p in groups[0]["params"]}
    assert not nd & dc and len(nd) + len(dc) == len(list(m.parameters()))
    bn = {id(p) for mod in m.modules() if isinstance(mod, torch.nn.BatchNorm2d) for p in mod.parameters(recurse=False)}
    assert bn and bn <= nd
    for name, p in m.named_parameters():
        assert (id(p) in nd) == (id(p) in bn or name.endswith(".bias")), name
    assert any(name.endswith(".bias") and id(p) not in bn for name, p in m.named_parameters())   # the head's conv biases


def test_constructors_refuse_what_the_kernel_lacks():
    p = [torch.nn.Parameter(torch.zeros(4))]
    for kw in (dict(dampening=0.1), dict(maximize=True), dict(foreach=True), dict(fused=True), dict(differentiable=True)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            O.SGD(p, lr=0.1, momentum=0.9, **kw)
    for kw in (dict(amsgrad=True), dict(maximize=True), dict(foreach=True), dict(fused=True), dict(capturable=True),
               dict(differentiable=True)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            O.Adam(p, **kw)
    nine = [{"params": [torch.nn.Parameter(torch.zeros(2))]} for _ in range(9)]
    with pytest.raises(ValueError, match="at most 8"):
        O.SGD(nine, lr=0.1)
    for cls, kw in ((O.SGD, dict(lr=0.1)), (O.Adam, {})):
        with pytest.raises(ValueError, match="ROCm"):
            cls(p, **kw)                      # CPU parameters: there is no CPU path
    with pytest.raises(ValueError, match="clip_grad_norm"):
        O.SGD(p, lr=0.1, clip_grad_norm=0.0)
