"""Optimizer step on the package's own kernels (csrc/optim.hip): SGD / Adam / AdamW, weight EMA,
gradient-norm clipping, a device-side non-finite skip and a per-iteration schedule evaluated on the
device, in two launches per step (three with clip or skip) whatever the number of tensors, with no host
sync and no per-step upload.

    opt = yms.optim.build_optimizer(model, cfg)        # for tools/utils.py:11-25 get_optimizer(model.parameters(), cfg)
    opt = yms.optim.SGD(model.parameters(), lr=0.01, momentum=0.937, nesterov=True, weight_decay=5e-4,
                        clip_grad_norm=10.0, skip_nonfinite=True)
    opt.attach_ema(model)                              # ModelEMA(decay=0.9999, tau=2000)
    opt.set_schedule([Segment(0, 1000, 1e-5, 1.0),     # linear warm-up, then a cosine to 5 %: no upload per step,
                      Segment(45000, 90000, 1.0, 0.05, shape="cosine")])   # and a captured step follows it
    ...
    loss.backward(); opt.step()
    with opt.ema_applied():
        validate(model)
    opt = yms.optim.yolo_ms_recipe(model, iters_per_epoch)   # AdamW + exp-momentum EMA + warm-up / cosine

The classes are ``torch.optim.Optimizer`` subclasses: ``param_groups``, ``zero_grad``, the torch LR
schedulers and ``yms.checkpoint`` work unchanged, and ``state_dict()`` is torch's format (a checkpoint
of ``torch.optim.SGD`` / ``Adam`` / ``AdamW`` loads here and the reverse).  One divergence: Adam's and
AdamW's ``'step'`` is a single optimizer-wide device count (torch counts per parameter), so every
``'step'`` of a loaded state must agree, and a parameter frozen for some steps reports the common count.

A torch scheduler changes ``param_groups`` every iteration, which costs an upload per step and cannot
reach a captured step without a host call.  ``set_schedule`` instead puts up to 8 ``Segment`` s on the
device once; every step multiplies each group's learning rate (or momentum / beta1) by the segments'
factors at the schedule index, the number of ``step()`` calls so far (updates + skipped steps), which the
kernel reads from its own counters.  ``schedule_factor`` is the same formula on the host.

The tensors reach the kernel as a cached device table of fixed-size chunks (``yms_optim_table_build``).
When every gradient is a view of one storage -- the backward's flat arena (runner.py) -- the table
holds gradient OFFSETS and the arena base is an argument: the table is keyed by (parameter pointers,
gradient offsets, gradient-present pattern), is rebuilt only on a miss, and is valid inside a captured
graph.  Gradients from other autograd paths are keyed by their addresses (not capturable).
Hyper-parameters live in a device array refreshed from ``param_groups`` when they change
(``sync_hyper()`` between graph replays), so a scheduler's new learning rate reaches a captured step.

The kernels write parameters through raw pointers; ``step`` and the EMA swap bump the written
tensors' version counters, which ``Plan.ensure_eval_cache`` keys the eval-time packed weights on.
"""
from __future__ import annotations

import contextlib
import ctypes
import math
from collections import OrderedDict, namedtuple

import torch
from torch.optim import Optimizer

from . import _lib as L

__all__ = ["SGD", "Adam", "AdamW", "Segment", "schedule_factor", "build_optimizer", "optimizer_config",
           "yolo_ms_recipe"]

_TABLES_MAX = 4
_HYPER_DOUBLES = ctypes.sizeof(L.OptimHyper) // 8
_STAGING_SLOTS = 4
_TARGETS = {"lr": L.OPTIM_SCHED_LR, "momentum": L.OPTIM_SCHED_MOMENTUM}
_SHAPES = {"linear": L.OPTIM_SCHED_LINEAR, "cosine": L.OPTIM_SCHED_COSINE}
_EMA_RULES = {"tau": L.OPTIM_EMA_TAU, "exp_momentum": L.OPTIM_EMA_EXPMOM}

Segment = namedtuple("Segment", "begin end start stop target shape groups", defaults=("lr", "linear", None))
Segment.__doc__ = """One piece of a schedule: a FACTOR on the groups' base value of `target` ("lr", or "momentum" =
SGD momentum / Adam beta1) that is `start` up to iteration `begin`, `stop` from iteration `end` on, and
moves between them on a "linear" or half-"cosine" `shape` inside.  `groups`: the parameter-group indices
it applies to (None = all).  Several segments on one target multiply.  A segment with end <= begin is
ignored."""


def _check_segment(s, ngroups=L.OPTIM_MAX_GROUPS):
    if s.target not in _TARGETS or s.shape not in _SHAPES:
        raise ValueError(f"yms.optim: a segment's target is one of {sorted(_TARGETS)} and its shape one of "
                         f"{sorted(_SHAPES)}, got {s.target!r} / {s.shape!r}")
    if s.groups is not None and not all(isinstance(g, int) and 0 <= g < ngroups for g in s.groups):
        raise ValueError(f"yms.optim: a segment's groups are indices below {ngroups}, got {s.groups!r}")


def schedule_factor(segments, n, group=0, target="lr"):
    """The factor on `group`'s base `target` at schedule index `n` (the number of ``step()`` calls made
    before): the product over the matching segments of  start (n <= begin) | stop (n >= end) | with
    u = (n - begin) / (end - begin):  start + (stop - start) u  (linear),
    stop + (start - stop)(1 + cos(pi u)) / 2  (cosine).  The kernel evaluates the same in fp64."""
    f = 1.0
    for s in segments or ():
        s = Segment(*s)
        _check_segment(s)
        if not s.end > s.begin or s.target != target or (s.groups is not None and group not in s.groups):
            continue
        if n <= s.begin:
            v = float(s.start)
        elif n >= s.end:
            v = float(s.stop)
        else:
            u = (n - s.begin) / (s.end - s.begin)
            v = s.start + (s.stop - s.start) * u if s.shape == "linear" else \
                s.stop + (s.start - s.stop) * (1.0 + math.cos(math.pi * u)) / 2.0
        f *= v
    return f


def _round4(n):
    return (n + 3) // 4 * 4


def _check_tensor(t, what):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
            and t.numel() > 0):
        raise ValueError(f"yms.optim: {what} must be a non-empty contiguous float32 ROCm tensor "
                         f"(got {tuple(t.shape)} {t.dtype} on {t.device}); there is no CPU path")


class _Fused(Optimizer):
    """Shared machinery; the subclasses give the kernel kind, the state keys and their hyper row."""
    _KIND = None
    _STATE_KEYS = ()
    _UNSUPPORTED = ()

    def __init__(self, params, defaults, clip_grad_norm, skip_nonfinite, schedule=None):
        if clip_grad_norm is not None and not float(clip_grad_norm) > 0.0:
            raise ValueError(f"yms.optim: clip_grad_norm must be positive, got {clip_grad_norm}")
        self._built = False
        super().__init__(params, defaults)
        self._check_groups()
        self.clip_grad_norm = None if clip_grad_norm is None else float(clip_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self._params = [p for g in self.param_groups for p in g["params"]]
        self._pgroup = [gi for gi, g in enumerate(self.param_groups) for _ in g["params"]]
        dev = self._params[0].device
        for p in self._params:
            _check_tensor(p, "every parameter")
            if p.device != dev:
                raise ValueError("yms.optim: all parameters must be on one device")
        self._dev = dev
        self._soff, off = [], 0
        for p in self._params:               # 16-B aligned slots
            self._soff.append(off)
            off += _round4(p.numel())
        self._bufs = [torch.zeros(off, dtype=torch.float32, device=dev) for _ in self._STATE_KEYS]
        self._install_state_views()
        self._counters = torch.zeros(4, dtype=torch.int32, device=dev)       # yms_optim_counters
        self._hyper = torch.zeros(_HYPER_DOUBLES, dtype=torch.float64, device=dev)
        self._hyper_last = None
        self._staging = []                   # pinned (host buffer, copy-done event) slots, used in turn
        self._staging_i = 0
        self._ema = None
        self._tables = {}
        self.table_builds = 0                # table cache misses (tests)
        self.last_launches = 0
        # yms_optim_ext (EMA rule + schedule) and the tick's read-out: fixed addresses, so a captured step keeps them
        self._ext = torch.zeros(ctypes.sizeof(L.OptimExt), dtype=torch.uint8, device=dev)
        self._sched = torch.zeros(L.OPTIM_MAX_GROUPS, 2, dtype=torch.float64, device=dev)
        self._segments = ()
        self._built = True
        if schedule is not None:
            self.set_schedule(schedule)

    # ---- construction ---------------------------------------------------------------------
    def add_param_group(self, param_group):
        if getattr(self, "_built", False):
            raise ValueError("yms.optim: parameter groups are fixed at construction (the state is one flat buffer)")
        super().add_param_group(param_group)

    def _check_groups(self):
        if len(self.param_groups) > L.OPTIM_MAX_GROUPS:
            raise ValueError(f"yms.optim: at most {L.OPTIM_MAX_GROUPS} parameter groups, got {len(self.param_groups)}")
        for g in self.param_groups:
            for k in self._UNSUPPORTED:
                if g.get(k):
                    raise ValueError(f"yms.optim: {k}={g[k]!r} is not implemented by the kernel")

    def _install_state_views(self):
        for p, off in zip(self._params, self._soff):
            st = self.state[p]
            for key, buf in zip(self._STATE_KEYS, self._bufs):
                st[key] = buf[off:off + p.numel()].view(p.shape)

    # ---- read-outs (device tensors, no sync) -------------------------------------------------
    @property
    def grad_norm(self):
        return self._counters[3:4].view(torch.float32)[0]

    @property
    def skipped_steps(self):
        return self._counters[2]

    def _counts(self):
        return self._counters.tolist()

    def _set_counts(self, step, ema_step, skipped):
        self._counters.copy_(torch.tensor([int(step), int(ema_step), int(skipped), 0], dtype=torch.int32))

    # ---- hyper-parameters ---------------------------------------------------------------------
    def _hyper_row(self, group):
        raise NotImplementedError

    def _hyper_values(self):
        ema = self._ema
        exp = ema is not None and ema["rule"] == "exp_momentum"       # its two numbers ride in the decay / tau slots
        v = [self.clip_grad_norm or 0.0, 1.0 if self.skip_nonfinite else 0.0,
             (ema["momentum"] if exp else ema["decay"]) if ema else 0.0,
             (ema["gamma"] if exp else ema["tau"]) if ema else 0.0]
        for g in self.param_groups:
            row = [float(x) for x in self._hyper_row(g)]
            v += row + [0.0] * (8 - len(row))
        return tuple(v + [0.0] * (_HYPER_DOUBLES - len(v)))

    def sync_hyper(self):
        """Refresh the device hyper-parameter array from ``param_groups`` (a no-op when nothing moved).
        ``step()`` calls it; a graph user calls it between replays, after ``scheduler.step()``."""
        vals = self._hyper_values()
        if vals == self._hyper_last:
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("yms.optim: the hyper-parameters differ from the device copy during stream capture; "
                               "call opt.sync_hyper() before capturing (and between replays)")
        if len(self._staging) < _STAGING_SLOTS:
            self._staging.append([torch.empty(_HYPER_DOUBLES, dtype=torch.float64, pin_memory=True), None])
        slot = self._staging[self._staging_i % len(self._staging)]
        self._staging_i += 1
        if slot[1] is not None:
            slot[1].synchronize()            # the copy that last read this slot (several uploads ago)
        slot[0].copy_(torch.tensor(vals, dtype=torch.float64))
        self._hyper.copy_(slot[0], non_blocking=True)
        slot[1] = torch.cuda.Event()
        slot[1].record(torch.cuda.current_stream(self._dev))
        self._hyper_last = vals

    # ---- the schedule and the EMA rule (yms_optim_ext) ---------------------------------------------
    def set_schedule(self, segments):
        """Put a schedule of up to 8 ``Segment`` s on the device (None or empty: remove it).  One
        upload, here; no step uploads anything for it, and a step captured after this call follows it
        through its replays.  The schedule is configuration, not state: its position is the saved
        ``step`` + ``skipped`` counts, the segments come from the code that builds the optimizer."""
        segs = tuple(Segment(*s) for s in (segments or ()))
        if len(segs) > L.OPTIM_MAX_SEGMENTS:
            raise ValueError(f"yms.optim: at most {L.OPTIM_MAX_SEGMENTS} schedule segments, got {len(segs)}")
        for s in segs:
            _check_segment(s, len(self.param_groups))
        old, self._segments = self._segments, segs
        try:
            self._upload_ext()
        except RuntimeError:
            self._segments = old
            raise

    def _ema_rule(self):
        return self._ema["rule"] if self._ema else "tau"

    def _upload_ext(self):
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("yms.optim: the schedule and the EMA rule are uploaded when they are set, which cannot "
                               "be captured; call set_schedule() / attach_ema() before capturing")
        ext = L.OptimExt(float(_EMA_RULES[self._ema_rule()]), float(len(self._segments)))
        for i, s in enumerate(self._segments):
            mask = (1 << L.OPTIM_MAX_GROUPS) - 1 if s.groups is None else sum(1 << g for g in set(s.groups))
            ext.seg[i] = L.OptimSegment(float(s.begin), float(s.end), float(s.start), float(s.stop),
                                        _TARGETS[s.target], _SHAPES[s.shape], mask, 0)
        self._ext.copy_(torch.frombuffer(bytearray(bytes(ext)), dtype=torch.uint8))

    def _use_ext(self):
        """The new entry point serves AdamW, the second EMA rule and schedules; everything else keeps
        calling yms_optim_step."""
        return self._KIND == L.OPTIM_ADAMW or bool(self._segments) or self._ema_rule() != "tau"

    @property
    def scheduled(self):
        """float64 [groups, 2] on the device: the learning rate and momentum (beta1) the last ``step()``
        ran at, written by its tick (no sync).  Only steps of an AdamW, a scheduled or an exp-momentum-EMA
        optimizer write it; for any other the values are ``param_groups``'."""
        if not self._use_ext():
            raise RuntimeError("yms.optim: no schedule is set; the step runs at the values in param_groups")
        return self._sched[:len(self.param_groups)]

    # ---- the device table ---------------------------------------------------------------------
    def _build_table(self, goffs, absolute):
        """goffs[i]: parameter i's gradient (byte offset from the arena base, or its address when
        `absolute`), None = no gradient this step.  -> (device table, chunks, partials, written)."""
        jobs, written = [], []
        ema = self._ema
        two = len(self._STATE_KEYS) > 1
        for i, p in enumerate(self._params):
            eoff = ema["poff"].get(i, -1) if ema else -1
            if goffs[i] is None and eoff < 0:
                continue
            fl = (L.OPTIM_EMA if eoff >= 0 else 0)
            if goffs[i] is None:
                fl |= L.OPTIM_GRAD_NONE
            else:
                written.append(p)
                if absolute:
                    fl |= L.OPTIM_GRAD_ABS
            jobs.append(L.OptimJob(p.data_ptr(), goffs[i] or 0, self._soff[i], self._soff[i] if two else -1, eoff,
                                   p.numel(), self._pgroup[i], fl))
        if ema:
            for t, off in ema["extra"]:
                jobs.append(L.OptimJob(t.data_ptr(), 0, -1, -1, off, t.numel(), 0, L.OPTIM_GRAD_NONE | L.OPTIM_EMA))
        if not jobs:
            return None, 0, None, written
        table, nchunks = self._upload_table(jobs)
        npart = L.lib().yms_optim_norm_partials(nchunks)
        if npart < 0:
            raise RuntimeError("yms.optim: too many elements for the norm reduction")
        partials = torch.empty(max(npart, 1), dtype=torch.float32, device=self._dev)
        return table, nchunks, partials, written

    def _upload_table(self, jobs):
        """Job list -> (device table, rows): built in host memory by the library, then one upload."""
        lib = L.lib()
        arr = (L.OptimJob * len(jobs))(*jobs)
        nb = lib.yms_optim_table_bytes(len(jobs), arr)
        nchunks = lib.yms_optim_table_chunks(len(jobs), arr)
        if nb == 0 or nchunks <= 0:
            raise RuntimeError("yms.optim: invalid job list")
        host = bytearray(nb)
        cbuf = (ctypes.c_char * nb).from_buffer(host)
        bp = [b.data_ptr() for b in self._bufs] + [None] * (2 - len(self._bufs))
        L.check(lib.yms_optim_table_build(len(jobs), arr, bp[0], bp[1],
                                          self._ema["buf"].data_ptr() if self._ema else None,
                                          ctypes.addressof(cbuf), nb), "yms_optim_table_build")
        del cbuf
        return torch.frombuffer(host, dtype=torch.uint8).to(self._dev), nchunks

    def _cached_table(self, key, goffs, absolute):
        ent = self._tables.get(key)
        if ent is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("yms.optim: the job table for these gradients is not on the device yet and an "
                                   "upload cannot be captured; run a warm-up step() with the same parameters and "
                                   "gradient layout before capturing")
            if len(self._tables) >= _TABLES_MAX:
                self._tables.clear()
            ent = self._tables[key] = self._build_table(goffs, absolute)
            self.table_builds += 1
        return ent

    def _check_grads(self):
        for p in self._params:
            g = p.grad
            if g is not None and (g.dtype != torch.float32 or g.is_sparse or not g.is_contiguous()
                                  or g.device != self._dev):
                raise RuntimeError("yms.optim: gradients must be contiguous float32 tensors on the parameters' device")

    def _step_table(self):
        """The table for the gradients present now and the arena base (None: absolute addresses).
        The per-step host work is one pointer per parameter and gradient; everything else (the checks,
        the job list, the upload) happens on a cache miss."""
        ptrs, first = [], None
        for p in self._params:
            g = p.grad
            if g is None:
                ptrs.append(None)
            else:
                if first is None:
                    first = g
                ptrs.append(g.data_ptr())
        if first is None:
            return (None, 0, None, ()), None
        pkey = tuple([p.data_ptr() for p in self._params])
        ekey = self._ema["key"]() if self._ema else None
        # one flat arena: every gradient lies inside the first one's storage
        st = first.untyped_storage()
        base = st.data_ptr()
        end = base + st.nbytes()
        if all(a is None or base <= a < end for a in ptrs):
            goffs = [None if a is None else a - base for a in ptrs]
            key = ("flat", pkey, tuple(goffs), ekey)
            absolute = False
        else:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("yms.optim: only gradients that are views of one flat arena can be captured")
            goffs, key, base, absolute = ptrs, ("abs", pkey, tuple(ptrs), ekey), None, True
        if key not in self._tables:
            self._check_grads()
        return self._cached_table(key, goffs, absolute), base

    # ---- step -----------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        (table, nchunks, partials, written), base = self._step_table()
        self.last_launches = 0
        if nchunks == 0 or not written:      # no gradient anywhere: nothing to do, as torch
            return loss
        self.sync_hyper()
        st = L.stream_ptr(self._dev)
        pp, npart = None, 0
        if self.clip_grad_norm is not None or self.skip_nonfinite:
            L.call("yms_optim_grad_norm", table.data_ptr(), nchunks, base, partials.data_ptr(), st)
            pp, npart = partials.data_ptr(), partials.numel()
            self.last_launches += 1
        if self._use_ext():
            ext = self._ext.data_ptr() if self._segments or self._ema_rule() != "tau" else None
            L.call("yms_optim_step_ext", self._KIND, table.data_ptr(), nchunks, base, self._hyper.data_ptr(), ext,
                   self._counters.data_ptr(), self._sched.data_ptr(), pp, npart, st)
        else:
            L.call("yms_optim_step", self._KIND, table.data_ptr(), nchunks, base, self._hyper.data_ptr(),
                   self._counters.data_ptr(), pp, npart, st)
        self.last_launches += 2              # the update and the counter tick
        torch.autograd.graph.increment_version(written)
        return loss

    # ---- EMA --------------------------------------------------------------------------------------
    def attach_ema(self, model, decay=0.9999, tau=2000, *, rule="tau", momentum=0.0002, gamma=2000):
        """Keep an exponential moving average of ``model``'s parameters and floating-point buffers,
        seeded from their current values and updated inside ``step()``.  The BN running statistics are
        written by the forward; their EMA follows them at each optimizer step.  At the k-th update:
        rule "tau" (YOLOv5 / ultralytics ModelEMA): e' = delta e + (1 - delta) p', delta = decay (1 - exp(-k / tau));
        rule "exp_momentum" (the RTMDet lineage's ExpMomentumEMA): e' = (1 - mu) e + mu p',
        mu = (1 - momentum) exp(-k / gamma) + momentum."""
        if rule not in _EMA_RULES:
            raise ValueError(f"yms.optim: the EMA rule is one of {sorted(_EMA_RULES)}, got {rule!r}")
        if rule == "exp_momentum" and not (0.0 <= momentum <= 1.0 and gamma > 0):
            raise ValueError(f"yms.optim: exp_momentum needs 0 <= momentum <= 1 and gamma > 0, got {momentum}, {gamma}")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("yms.optim: attach_ema() uploads and cannot be captured")
        from .checkpoint import _unwrap
        model = _unwrap(model)
        pidx = {id(p): i for i, p in enumerate(self._params)}
        entries, poff, extra, off = [], {}, [], 0
        for name, t in model.state_dict(keep_vars=True).items():
            if not t.is_floating_point():
                continue
            _check_tensor(t, f"EMA tensor {name}")
            entries.append((name, t, off))
            if id(t) in pidx:
                poff[pidx[id(t)]] = off
            else:
                extra.append((t, off))
            off += _round4(t.numel())
        buf = torch.empty(off, dtype=torch.float32, device=self._dev)
        self._ema = {"decay": float(decay), "tau": float(tau), "rule": rule, "momentum": float(momentum),
                     "gamma": float(gamma), "buf": buf, "entries": entries, "poff": poff,
                     "extra": extra, "model": model,
                     "key": lambda: tuple(t.data_ptr() for t, _ in extra)}
        self._upload_ext()
        self._tables.clear()
        self._seed_ema()
        c = self._counts()
        self._set_counts(c[0], 0, c[2])

    def _ema_view(self, t, off):
        return self._ema["buf"][off:off + t.numel()].view(t.shape)

    @torch.no_grad()
    def _seed_ema(self, names=None):
        for name, t, off in self._ema["entries"]:
            if names is None or name in names:
                self._ema_view(t, off).copy_(t)

    def _need_ema(self):
        if self._ema is None:
            raise RuntimeError("yms.optim: no EMA attached (call opt.attach_ema(model) first)")
        return self._ema

    def ema_state_dict(self):
        """The EMA weights under the model's state_dict keys (integer buffers from the live model)."""
        ema = self._need_ema()
        views = {name: self._ema_view(t, off) for name, t, off in ema["entries"]}
        return OrderedDict((k, (views[k] if k in views else v).detach().clone())
                           for k, v in ema["model"].state_dict().items())

    @torch.no_grad()
    def _swap(self):
        ema = self._need_ema()
        key = ("swap", tuple(t.data_ptr() for _, t, _ in ema["entries"]))
        ent = self._tables.get(key)
        if ent is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("yms.optim: the EMA swap table is not on the device yet; swap once before capturing")
            ent = self._tables[key] = self._upload_table(
                [L.OptimJob(t.data_ptr(), 0, -1, -1, off, t.numel(), 0, L.OPTIM_GRAD_NONE | L.OPTIM_EMA)
                 for _, t, off in ema["entries"]])
        L.call("yms_optim_swap", ent[0].data_ptr(), ent[1], L.stream_ptr(self._dev))
        torch.autograd.graph.increment_version([t for _, t, _ in ema["entries"]])

    @contextlib.contextmanager
    def ema_applied(self):
        """Run the block with the EMA values in the model's own tensors (validation, export): the
        tensors and the EMA slots exchange VALUES in place, in one launch each way, because the plan
        caches parameter pointers and tensors must not be re-homed."""
        self._swap()
        try:
            yield self
        finally:
            self._swap()

    # ---- state dict -------------------------------------------------------------------------------
    def _export_count(self, count):
        pass

    def state_dict(self):
        c = self._counts()
        self._export_count(c[0])
        sd = super().state_dict()
        y = {"format": 1, "step": c[0], "ema_step": c[1], "skipped": c[2]}
        if self._ema:
            y["ema_decay"], y["ema_tau"] = self._ema["decay"], self._ema["tau"]
            y["ema_rule"], y["ema_momentum"], y["ema_gamma"] = (self._ema[k] for k in ("rule", "momentum", "gamma"))
            y["ema"] = {name: self._ema_view(t, off) for name, t, off in self._ema["entries"]}
        sd["yms"] = y
        return sd

    def _loaded_count(self, states, yms):
        raise NotImplementedError

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        yms = state_dict.get("yms")
        states = list(state_dict["state"].values())
        step = self._loaded_count(states, yms)
        super().load_state_dict({"state": state_dict["state"], "param_groups": state_dict["param_groups"]})
        self._check_groups()
        for p, off in zip(self._params, self._soff):
            st = self.state.get(p, {})
            for key, buf in zip(self._STATE_KEYS, self._bufs):
                slot, v = buf[off:off + p.numel()], st.get(key)
                if v is None:
                    slot.zero_()
                else:
                    slot.copy_(v.reshape(-1))
        self._install_state_views()
        ema_step = 0
        if self._ema:
            have = yms.get("ema") if yms else None
            if have:
                for name, t, off in self._ema["entries"]:
                    if name in have:
                        self._ema_view(t, off).copy_(have[name])
                self._seed_ema({name for name, _, _ in self._ema["entries"]} - set(have))
                ema_step = int(yms.get("ema_step", 0))
            else:
                self._seed_ema()             # no EMA in the file: start it from the current weights
        self._set_counts(step, ema_step, int(yms.get("skipped", 0)) if yms else 0)
        self._hyper_last = None


class SGD(_Fused):
    """``torch.optim.SGD`` on one launch: d = g + wd p; b' = d on the first update, else mom b + d;
    p' = p - lr (d + mom b') with nesterov, else p - lr b'."""
    _KIND = L.OPTIM_SGD
    _STATE_KEYS = ("momentum_buffer",)
    _UNSUPPORTED = ("dampening", "maximize", "foreach", "fused", "differentiable")

    def __init__(self, params, lr, momentum=0, nesterov=False, weight_decay=0, *, clip_grad_norm=None,
                 skip_nonfinite=False, schedule=None, dampening=0, maximize=False, foreach=None, fused=None,
                 differentiable=False):
        if lr < 0 or momentum < 0 or weight_decay < 0:
            raise ValueError("yms.optim.SGD: lr, momentum and weight_decay must be non-negative")
        if nesterov and momentum <= 0:
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                        maximize=maximize, foreach=foreach, differentiable=differentiable, fused=fused)
        super().__init__(params, defaults, clip_grad_norm, skip_nonfinite, schedule)

    def _hyper_row(self, g):
        return (g["lr"], g["momentum"], 0.0, 0.0, g["weight_decay"], 1.0 if g["nesterov"] else 0.0)

    def _loaded_count(self, states, yms):
        if yms and "step" in yms:
            return int(yms["step"])
        # a torch.optim.SGD state has no count: with momentum buffers it is past its first update
        return 1 if any(s.get("momentum_buffer") is not None for s in states) else 0


class Adam(_Fused):
    """``torch.optim.Adam`` (L2 decay folded into the gradient; AdamW is its own class; no amsgrad) on one
    launch.  ``'step'`` in the state is the optimizer-wide device count (module docstring)."""
    _KIND = L.OPTIM_ADAM
    _STATE_KEYS = ("exp_avg", "exp_avg_sq")
    _UNSUPPORTED = ("amsgrad", "maximize", "foreach", "fused", "capturable", "differentiable",
                    "decoupled_weight_decay")
    _DECOUPLED = False

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, *, clip_grad_norm=None,
                 skip_nonfinite=False, schedule=None, amsgrad=False, maximize=False, foreach=None, fused=None,
                 capturable=False, differentiable=False):
        if lr < 0 or eps < 0 or weight_decay < 0 or not (0 <= betas[0] < 1 and 0 <= betas[1] < 1):
            raise ValueError(f"yms.optim.{type(self).__name__}: invalid lr / betas / eps / weight_decay")
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=amsgrad,
                        maximize=maximize, foreach=foreach, capturable=capturable, differentiable=differentiable,
                        fused=fused, decoupled_weight_decay=self._DECOUPLED)
        super().__init__(params, defaults, clip_grad_norm, skip_nonfinite, schedule)

    def _hyper_row(self, g):
        return (g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"], 0.0)

    def _export_count(self, count):
        for p in self._params:
            self.state[p]["step"] = torch.tensor(float(count), dtype=torch.float32)

    def _loaded_count(self, states, yms):
        steps = {float(s["step"]) for s in states if "step" in s}
        if len(steps) > 1:
            raise ValueError(f"yms.optim.Adam: one update count for all parameters, the state has {sorted(steps)}")
        return int(steps.pop()) if steps else 0


class AdamW(Adam):
    """``torch.optim.AdamW`` (no amsgrad) on one launch: the decay is decoupled, p1 = p (1 - lr wd) with the
    factor formed in fp64, then Adam's update of p1 from the (clipped) gradient alone, so clipping
    never scales the decay.  State keys, ``'step'`` and the state dict are Adam's; a
    ``torch.optim.AdamW`` checkpoint loads here and the reverse."""
    _KIND = L.OPTIM_ADAMW
    _UNSUPPORTED = tuple(k for k in Adam._UNSUPPORTED if k != "decoupled_weight_decay")
    _DECOUPLED = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, **kw):
        super().__init__(params, lr, betas, eps, weight_decay, **kw)


def _decay_groups(model, norms=(torch.nn.modules.batchnorm._NormBase,)):
    """[{decayed parameters}, {norm weights and every bias, weight_decay 0}]"""
    decay, no_decay = [], []
    for mod in model.modules():
        for pname, p in mod.named_parameters(recurse=False):
            (no_decay if isinstance(mod, norms) or pname == "bias" else decay).append(p)
    return [{"params": decay}, {"params": no_decay, "weight_decay": 0.0}]


def optimizer_config(model, cfg):
    """(class, parameter groups, constructor keywords, EMA keywords or None) for ``cfg['training']``: the
    keys and defaults of the reference's get_optimizer (tools/utils.py:11-25) plus ``optimizer: adamw``
    and the optional ``ema: {decay, tau}`` or ``ema: {rule: exp_momentum, momentum, gamma}``,
    ``clip_grad_norm``, ``skip_nonfinite``, ``no_decay_bn_bias`` and ``lr_schedule: {warmup_iters,
    warmup_start_factor, cosine_begin_iter, cosine_end_iter, min_lr_ratio}`` (a linear warm-up and a cosine
    to ``min_lr_ratio`` x the learning rate, as two segments under the ``schedule`` keyword)."""
    tr = cfg["training"]
    name = tr["optimizer"].lower()
    lr, wd = tr["learning_rate"], tr["weight_decay"]
    if name in ("adam", "adamw"):
        cls = Adam if name == "adam" else AdamW
        kw = dict(lr=lr, betas=tuple(tr.get("adam_betas", [0.9, 0.999])), weight_decay=wd)
    elif name == "sgd":
        cls, kw = SGD, dict(lr=lr, momentum=tr.get("sgd_momentum", 0.937), nesterov=tr.get("sgd_nesterov", True),
                            weight_decay=wd)
    else:
        raise ValueError(f"Unsupported optimizer: {name}")
    kw["clip_grad_norm"] = tr.get("clip_grad_norm")
    kw["skip_nonfinite"] = bool(tr.get("skip_nonfinite", False))
    sch = tr.get("lr_schedule")
    if sch:
        segs = []
        if sch.get("warmup_iters"):
            segs.append(Segment(0, sch["warmup_iters"], sch.get("warmup_start_factor", 1e-3), 1.0))
        if sch.get("cosine_end_iter"):
            segs.append(Segment(sch.get("cosine_begin_iter", 0), sch["cosine_end_iter"], 1.0,
                                sch.get("min_lr_ratio", 0.0), shape="cosine"))
        kw["schedule"] = segs
    if tr.get("no_decay_bn_bias"):
        # the YOLOv5 / v8 grouping: BN weights and every bias carry no weight decay
        groups = _decay_groups(model)
    else:
        groups = list(model.parameters())
    ema = tr.get("ema")
    if ema is not None and ema is not False:
        ema = dict(ema) if isinstance(ema, dict) else {}
        if ema.get("rule", "tau") == "exp_momentum":
            ema = {"rule": "exp_momentum", "momentum": ema.get("momentum", 0.0002), "gamma": ema.get("gamma", 2000)}
        elif ema.get("rule", "tau") == "tau":
            ema = {"decay": ema.get("decay", 0.9999), "tau": ema.get("tau", 2000)}
        else:
            raise ValueError(f"Unsupported EMA rule: {ema['rule']}")
    else:
        ema = None
    return cls, groups, kw, ema


def build_optimizer(model, cfg):
    """Drop-in for the reference's ``get_optimizer(model.parameters(), cfg)``, taking the model."""
    cls, groups, kw, ema = optimizer_config(model, cfg)
    opt = cls(groups, **kw)
    if ema is not None:
        opt.attach_ema(model, **ema)
    return opt


def yolo_ms_recipe_config(model, iters_per_epoch, epochs=300, batch_size=256):
    """``yolo_ms_recipe``'s (class, parameter groups, constructor keywords, EMA keywords), unbuilt."""
    norms = (torch.nn.modules.batchnorm._NormBase, torch.nn.GroupNorm, torch.nn.LayerNorm)
    kw = dict(lr=0.004 * batch_size / 256, betas=(0.9, 0.999), weight_decay=0.05,
              schedule=[Segment(0, 1000, 1e-5, 1.0),
                        Segment((epochs // 2) * iters_per_epoch, epochs * iters_per_epoch, 1.0, 0.05, shape="cosine")])
    return AdamW, _decay_groups(model, norms), kw, {"rule": "exp_momentum", "momentum": 0.0002, "gamma": 2000}


def yolo_ms_recipe(model, iters_per_epoch, epochs=300, batch_size=256):
    """The optimizer of YOLO-MS's training recipe (the RTMDet lineage's), built and with its EMA attached:
    AdamW at lr 0.004 for batch 256 (scaled linearly with ``batch_size``), weight decay 0.05 and none on
    norm weights and biases; per iteration, a linear warm-up of the learning rate from 1e-5 x over the first
    1000 iterations, flat, then a cosine to 0.05 x from epoch ``epochs // 2`` to ``epochs``; the
    exp-momentum EMA with momentum 0.0002 and gamma 2000.  The schedule runs on the device, so ``step()``
    uploads nothing and can be captured.

    These values are the published recipe's as this project's maintainers know them.  mmengine, mmdet and
    mmyolo are not available to this project's tests, so parity with their AdamW / ExpMomentumEMA /
    LinearLR / CosineAnnealingLR classes is UNPINNED; what the tests pin is the kernels against fp64
    restatements of the formulas in include/yms.h, torch.optim.AdamW and torch's LinearLR /
    CosineAnnealingLR.  Not included: the recipe's stage-two augmentation switch, SyncBN."""
    cls, groups, kw, ema = yolo_ms_recipe_config(model, iters_per_epoch, epochs, batch_size)
    opt = cls(groups, **kw)
    opt.attach_ema(model, **ema)
    return opt
