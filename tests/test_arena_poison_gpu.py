"""A plan's results do not depend on the initial contents of its arenas outside plan.zero_ranges /
plan.gzero_ranges.

Plan.new_arena, _PlanFn.backward and Plan.ensure_eval_cache take every byte the planned model touches
(activations, activation gradients, the flat parameter-gradient arena, every scratch region, the eval
cache) from torch.empty, and only the zero ranges are cleared.  The kernels move whole 16-byte channel
groups, so a step is right only if every group an op reads was written earlier in the step or lies in
a zeroed range.  A fresh process usually gets zero pages from the caching allocator, which hides a
violation; here the memory is filled on purpose.

arena_fill(byte) replaces the name `torch` inside yms.plan, yms.runner and yolov8.tools.loss by a proxy
whose `empty` allocates as usual and then fills the tensor's bytes with `byte` on the current stream
(the runner takes its stream pointer from that stream, so the fill is ordered before the plan's own
yms_zero calls); torch.zeros is left alone.  yms.ops (NMS) and yms.optim stay unpatched: the NMS
workspace holds integer work lists and tests/test_nms_gpu.py covers it, and the optimizer's partials
are NaN-prefilled in tests/test_optim_gpu.py.

Fills: 0x00 is the explicit baseline; 0xFF is NaN in bf16, f16 and f32; 0x7C is about 5e36, finite, in
bf16 and f32 (NaN in f16): fmaxf in the pooling kernels and comparisons swallow NaN, so a read of poison
that NaN hides shows up as a huge value.

Gate: every collected tensor of a poisoned run is torch.equal to the 0x00 run's.  No arithmetic
tolerance applies: either no poisoned byte reaches a result or one does.  Its premise -- two separate
runs of one configuration are bit-identical -- is a test of its own here
(test_two_zero_filled_runs_are_bit_identical).

Negative control: with exactly the op.z_padding ranges left out of Plan.new_arena (commit 3a9769c's
fix; every other zero range and all of gzero_ranges stay) the 0xFF run's gradients differ.

The slot tests at the end drive single entry points on operands that sit in a middle slot of a wider
buffer whose other slots hold NaN, into outputs prefilled with a sentinel: the result equals, bit for
bit, the same call with zero-filled neighbours, and nothing outside the output's channels is stored.

Scratch regions, from their consumers' code (they hold data only, so poison cannot become an address):
"stats" = fp32 moment rows + fp32 pixel counts, written by the conv of the same op before its finalize;
"bwd" / "bnr*" = fp32 partial rows, one per reduce block, written before the finalize sums them; "coef"
and "sib" = fp32 coefficient / dgamma, dbeta rows written by the finalize; "wgrad", "stemwg" and the
depthwise weight gradient's workspace = fp32 split slabs written by the GEMM before its reduce; "sppf" =
one arg-max BYTE per output (ky * 5 + kx), written by the first launch of yms_sppf_pool_bwd and only
COMPARED with a tap index by the second, never used as an offset; "cnt" = the arrival counters, the one
integer field, zeroed through gzero_ranges (and left at zero by the kernel).  The loss's workspace holds
integer work lists (kcnt, kidx, fg, cbits, nfg): each is written by an earlier kernel of the same call
for every entry a later kernel reads.
"""
import contextlib
import ctypes

import pytest
import torch

import hiputil as H
import test_step_routes_gpu as R
import yms.plan
import yms.runner
import yolov8.tools.loss
from yms import _lib as L
from yms import set_compute_dtype
from yms.plan import Plan
from yolov8.yolov8 import YOLOv8

pytestmark = pytest.mark.gpu

PATCHED = (yms.plan, yms.runner, yolov8.tools.loss)
ZERO, POISON = 0x00, (0xFF, 0x7C)
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32


class _TorchProxy:
    """`torch` with an `empty` that fills what it allocates (device tensors) with one byte value."""

    def __init__(self, byte):
        self._byte, self.fills = byte, 0

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *args, **kwargs):
        t = torch.empty(*args, **kwargs)
        if t.is_cuda and t.numel():
            t.view(-1).view(torch.uint8).fill_(self._byte)       # on the current stream
            self.fills += 1
        return t


@pytest.fixture
def arena_fill():
    @contextlib.contextmanager
    def fill(byte):
        proxy = _TorchProxy(byte)
        with pytest.MonkeyPatch.context() as mp:
            for mod in PATCHED:
                assert mod.torch is torch
                mp.setattr(mod, "torch", proxy)
            yield proxy
        assert all(mod.torch is torch for mod in PATCHED)
    return fill


def test_the_proxy_fills_only_torch_empty(arena_fill):
    with arena_fill(0x7C) as proxy:
        e = yms.plan.torch.empty((3, 5), dtype=BF16, device="cuda")
        z = yms.runner.torch.zeros(7, dtype=F32, device="cuda")
        s = yolov8.tools.loss.torch.empty((), dtype=F32, device="cuda")
        assert yms.plan.torch.float32 is F32 and proxy.fills == 2
    assert (e.view(torch.uint8) == 0x7C).all() and (z == 0).all() and s.item() > 1e36
    assert e.float().min().item() > 1e36 and torch.isfinite(e.float()).all()
    assert torch.full((2,), -1, dtype=torch.int16).view(BF16).isnan().all()       # 0xFF: NaN in every format
    assert torch.full((2,), -1, dtype=torch.int16).view(F16).isnan().all()
    assert torch.full((2,), -1, dtype=torch.int32).view(F32).isnan().all()
    assert torch.full((2,), 0x7C7C, dtype=torch.int16).view(F16).isnan().all()


# ---- training -----------------------------------------------------------------------------------------
N3 = ("n", 3, BF16)
TRAIN_CASES = [c + ({},) for c in R.CASES] + [("n", 17, F16, {})]                  # 81 -> 88 padding
# the switches that change which pass writes which buffer
TRAIN_CASES += [N3 + ({k: 0},) for k in ("YMS_HEAD_FUSE", "YMS_BNRED", "YMS_STEM", "YMS_GRAD_INPLACE", "YMS_HEAD_GROUP")]


def _case_id(c):
    v, nc, dtype, env = c
    return "-".join([v, str(nc), str(dtype).replace("torch.", "")] + [f"{k}={val}" for k, val in env.items()])


_TRAIN = {}


def _train(arena_fill, case, byte, steps=2, cache=True):
    """One run per (case, fill), a fresh model and plan each, shared by the tests and left unchanged."""
    v, nc, dtype, env = case
    key = (v, nc, dtype, tuple(env.items()), byte, steps)
    if not cache or key not in _TRAIN:
        with arena_fill(byte) as proxy:
            out, _, plan = R._run(v, nc, dtype, env, steps=steps)
        assert proxy.fills >= 4 * steps           # arena, gradient arena, parameter gradients, the loss's workspace
        if not cache:
            return out, plan
        _TRAIN[key] = (out, plan)
    return _TRAIN[key]


def _differing(got, base):
    assert got.keys() == base.keys()
    return [k for k in base if not torch.equal(got[k], base[k])]


def _check_options(plan, env):
    o = plan.opts
    want = {"YMS_HEAD_FUSE": o.head_fuse, "YMS_BNRED": o.bnred, "YMS_STEM": o.stem, "YMS_GRAD_INPLACE": o.grad_inplace,
            "YMS_HEAD_GROUP": o.head_group}
    for k, val in env.items():
        assert int(want[k]) == val, (k, want[k])


def test_two_zero_filled_runs_are_bit_identical(arena_fill):
    """The premise of the gate below; a failure here is non-reproducibility, not a read of poison."""
    a, _ = _train(arena_fill, N3 + ({},), ZERO)
    b, _ = _train(arena_fill, N3 + ({},), ZERO, cache=False)
    bad = _differing(b, a)
    assert not bad, f"{len(bad)} of {len(a)} tensors differ between two 0x00 runs, first {bad[:4]}"


@pytest.mark.parametrize("byte", POISON, ids=hex)
@pytest.mark.parametrize("case", TRAIN_CASES, ids=_case_id)
def test_training_step_ignores_arena_contents(arena_fill, case, byte):
    base, bplan = _train(arena_fill, case, ZERO)
    got, plan = _train(arena_fill, case, byte)
    _check_options(plan, case[3])
    assert plan is not bplan and plan.zero_ranges == bplan.zero_ranges and plan.gzero_ranges == bplan.gzero_ranges
    assert any(k.startswith("s1:grad:") for k in base) and any(k.startswith("s1:buf:") for k in base)
    assert all(torch.isfinite(t.float()).all() for t in base.values())
    bad = _differing(got, base)
    assert not bad, f"fill {byte:#04x}: {len(bad)} of {len(base)} tensors differ from the 0x00 run, first {bad[:6]}"


def test_gate_reports_unzeroed_z_padding(arena_fill, monkeypatch):
    """Negative control: without the z_padding ranges the input gradients read NaN padding of dz through
    zero weight rows.  One step, values only: every other zero range and the arrival counters stay."""
    case = N3 + ({},)
    base, bplan = _train(arena_fill, case, ZERO)
    real, skipped = Plan.new_arena, []

    def without_z_padding(self, device, stream):
        pad = [r for op in self.ops for r in op.z_padding(self.es)]
        keep = [r for r in self.zero_ranges if r not in pad]
        assert pad and len(keep) == len(self.zero_ranges) - len(pad) and keep == [(b.off, b.npix * b.ld * self.es)
                                                                                  for b in self.bufs if b.zero]
        skipped.append(len(pad))
        full, self.zero_ranges = self.zero_ranges, keep
        try:
            return real(self, device, stream)
        finally:
            self.zero_ranges = full

    monkeypatch.setattr(Plan, "new_arena", without_z_padding)
    got, plan = _train(arena_fill, case, 0xFF, steps=1, cache=False)
    monkeypatch.undo()
    assert skipped == [skipped[0]] and plan.gzero_ranges == bplan.gzero_ranges
    base0 = {k: t for k, t in base.items() if k.startswith("s0:")}
    bad = _differing(got, base0)
    print(f"without the z_padding ranges, 0xFF: {len(bad)} of {len(base0)} tensors differ, first {bad[:4]}")
    assert any(":grad:" in k for k in bad), "the gate did not notice the unzeroed padding"
    assert any(not torch.isfinite(got[k]).all() for k in bad)
    # the forward never reads the padding: maps, loss and buffers are untouched
    assert all(":grad:" in k for k in bad), [k for k in bad if ":grad:" not in k]


# ---- eval and decode ----------------------------------------------------------------------------------
EVAL_CASES = [(v, nc, dt) for v, nc in (("n", 3), ("n", 80), ("ms-xs", 80)) for dt in (BF16, F16, F32)]


def _eval(arena_fill, v, nc, dtype, byte):
    """The decode model called twice (the second call runs on the plan's cached, not re-zeroed arena)
    -> {name: tensor on the CPU} of both calls' raw head maps and decoded output."""
    sd, x = R._fixture(v, nc)
    out = {}
    with arena_fill(byte) as proxy:
        m = YOLOv8(v, nc).cuda()
        m.load_state_dict(sd)
        set_compute_dtype(m, dtype)
        m.eval()
        m.head.stride = torch.tensor([8.0, 16.0, 32.0])
        xg = x.cuda()
        for call in range(2):
            y = m(xg)
            (plan,) = m.__dict__["_yms_plans"].values()
            assert not plan.training and plan.kind[0] == "decode" and len(plan._infer_arenas) == 1
            (arena,) = plan._infer_arenas.values()
            if call:
                assert arena.data_ptr() == first, "the second call did not reuse the decode plan's arena"
            first = arena.data_ptr()
            out[f"c{call}:decoded"] = y.clone()
            for i, o in enumerate(plan.outputs):
                out[f"c{call}:map{i}"] = plan.act_tensor(arena, o, dtype).clone()
        torch.cuda.synchronize()
    assert proxy.fills >= 4                      # the arena, the eval cache, one decoded output per call
    A = sum(o.h * o.w for o in plan.outputs)
    assert out["c0:decoded"].shape == (2, A, 4 + nc) and len(plan.outputs) == 3
    return {k: t.cpu() for k, t in out.items()}


@pytest.mark.parametrize("v,nc,dtype", EVAL_CASES, ids=R._ids)
def test_eval_and_decode_ignore_arena_contents(arena_fill, v, nc, dtype):
    base = _eval(arena_fill, v, nc, dtype, ZERO)
    assert all(torch.isfinite(t.float()).all() for t in base.values())
    for k in [k for k in base if k.startswith("c0:")]:
        assert torch.equal(base[k], base["c1" + k[2:]]), k
    for byte in POISON:
        bad = _differing(_eval(arena_fill, v, nc, dtype, byte), base)
        assert not bad, f"fill {byte:#04x}: {bad} differ from the 0x00 run"


# ---- single entry points on middle slots of wider buffers ------------------------------------------------
# Every operand sits at channel offset 8 (inputs) / 16 (outputs) of a buffer 16 / 24 channels wider than
# it needs; the other slots hold NaN (inputs) or the sentinel (outputs).  Each case runs twice, with zero
# and with NaN neighbours: the outputs must be equal bit for bit, and untouched outside their channels.
NAN, SENT = float("nan"), 1.5
XOFF, YOFF = 8, 16


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _in(x, dtype, fill):
    return H.nhwc(x, dtype, ld=H.r8(x.shape[1]) + 16, off=XOFF, fill=fill)


def _out(n, h, w, c, dtype):
    return torch.full((n, h, w, H.r8(c) + 24), SENT, dtype=dtype, device="cuda")


def _rand(g, *shape):
    return torch.randn(*shape, generator=g)


def _same_and_inside(runs, c=None, off=YOFF, sent=SENT):
    """runs: the output tensors of the zero-neighbour and the NaN-neighbour call (lists, same order)."""
    zero, nan = runs
    assert len(zero) == len(nan) and zero
    for a, b in zip(zero, nan):
        assert a.shape == b.shape and torch.isfinite(a.float()).all() and torch.isfinite(b.float()).all()
        assert torch.equal(_bits(a), _bits(b)), "NaN in a neighbouring slot changed the result"
    if c is not None:
        for t in (zero[0], nan[0]):
            outside = torch.cat([t[..., :off], t[..., off + c:]], -1)
            assert (outside == sent).all(), "stored outside the output's channels"
            assert (t[..., off:off + c] != sent).any()


def _both(fn):
    out = [fn(0.0), fn(NAN)]
    torch.cuda.synchronize()
    return out


def test_slot_operands_have_nan_neighbours():
    x = _rand(torch.Generator().manual_seed(4), 2, 20, 3, 5)
    for dtype in (BF16, F32):
        z, p = _in(x, dtype, 0.0), _in(x, dtype, NAN)
        assert z.shape == p.shape == (2, 3, 5, 24 + 16)
        assert torch.equal(z[..., XOFF:XOFF + 24], p[..., XOFF:XOFF + 24]) and (p[..., XOFF + 20:XOFF + 24] == 0).all()
        assert torch.equal(H.nchw(p, 20, XOFF).cpu(), x.to(dtype).float())
        assert p[..., :XOFF].isnan().all() and p[..., XOFF + 24:].isnan().all() and not z.isnan().any()
        assert torch.equal(H.nhwc(x, dtype), H.nhwc(x, dtype, fill=0.0)) and not H.nhwc(x, dtype, off=8).isnan().any()


IGEMM, DIRECT = (2, 24, 9, 9, 40, 3, 1), (2, 32, 16, 32, 32, 3, 1)          # (n, cin, h, w, cout, k, stride)
S2_FIRST = (2, 32, 64, 64, 64, 3, 2)                                        # test_conv_direct_gpu.S2[0]
WG_ROUTES = {"tt": (IGEMM, {"YMS_WG_HALO": "0", "YMS_WG_RING": "0"}),
             "ring": ((2, 64, 40, 40, 128, 3, 1), {"YMS_WG_HALO": "0", "YMS_WG_RING": "2"}),     # test_conv_gpu.WGR[0]
             "halo": ((2, 32, 20, 20, 32, 3, 1), {"YMS_WG_HALO": "2"})}                          # test_conv_gpu.WGH[0]


def _conv_operands(shp, dtype, seed):
    n, cin, h, w, cout, k, s = shp
    g = torch.Generator().manual_seed(seed)
    sh = H.shape(n, h, w, cin, cout, k, s, dtype)
    x, wt = _rand(g, n, cin, h, w), _rand(g, cout, cin, k, k) / (cin * k * k) ** 0.5
    return sh, x, wt, _rand(g, n, cout, sh.ho, sh.wo), g


@pytest.mark.parametrize("res,stats", [(False, False), (True, False), (False, True)], ids=["epilogue", "residual", "stats"])
@pytest.mark.parametrize("shp,dt", [(IGEMM, "bf16"), (IGEMM, "f32"), (DIRECT, "bf16")], ids=["igemm-bf16", "igemm-f32", "direct-bf16"])
def test_conv_fwd_slot(shp, dt, res, stats):
    dtype = H.DT[dt]
    sh, x, wt, r, g = _conv_operands(shp, dtype, 5)
    sp = ctypes.pointer(sh)
    if shp is DIRECT:
        assert L.lib().yms_conv_direct_set(-1) == 1
    wp = H.pack(wt, sh, dtype, 0)
    sc, sf = (torch.rand(sh.cout, generator=g) + 0.5).cuda(), (_rand(g, sh.cout) * 0.1).cuda()
    rows, sld = L.lib().yms_conv_stats_rows(sp), L.lib().yms_conv_stats_ld(sp)

    def run(fill):
        xb, rb = _in(x, dtype, fill), _in(r, dtype, fill) if res else None
        y = _out(sh.n, sh.ho, sh.wo, sh.cout, dtype)
        st = H.stats_buffer(rows, sld) if stats else None
        L.call("yms_conv_fwd", sp, xb.data_ptr(), xb.shape[-1], XOFF, wp.data_ptr(), y.data_ptr(), y.shape[-1], YOFF,
               None if stats else sc.data_ptr(), None if stats else sf.data_ptr(), L.ACT_NONE if stats else L.ACT_SILU,
               L.ptr(rb), rb.shape[-1] if res else 0, XOFF if res else 0, L.ptr(st), L.stream_ptr())
        if not stats:
            return [y]
        mom, cnt = H.split_stats(st, rows, sld)
        return [y, mom[:, :, :sh.cout].contiguous(), cnt]

    _same_and_inside(_both(run), sh.cout)


@pytest.mark.parametrize("acc", [0, 1], ids=["store", "accumulate"])
@pytest.mark.parametrize("shp,dt", [(IGEMM, "bf16"), (IGEMM, "f32"), (DIRECT, "bf16"), (S2_FIRST, "bf16")],
                         ids=["igemm-bf16", "igemm-f32", "direct-s1-bf16", "direct-s2-bf16"])
def test_conv_dgrad_slot(shp, dt, acc):
    dtype = H.DT[dt]
    sh, _, wt, dz, _ = _conv_operands(shp, dtype, 6)
    sp = ctypes.pointer(sh)
    wpt = H.pack(wt, sh, dtype, 1)

    def run(fill):
        dzb = _in(dz, dtype, fill)
        dx = _out(sh.n, sh.h, sh.w, sh.cin, dtype)           # accumulate: onto the sentinel
        L.call("yms_conv_dgrad", sp, dzb.data_ptr(), dzb.shape[-1], XOFF, wpt.data_ptr(), dx.data_ptr(), dx.shape[-1],
               YOFF, acc, L.stream_ptr())
        return [dx]

    _same_and_inside(_both(run), sh.cin)


@pytest.mark.parametrize("acc", [0, 1], ids=["store", "accumulate"])
@pytest.mark.parametrize("route", list(WG_ROUTES))
def test_conv_wgrad_slot(route, acc, monkeypatch):
    shp, env = WG_ROUTES[route]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    dtype = torch.bfloat16
    sh, x, _, dz, _ = _conv_operands(shp, dtype, 7)
    sp = ctypes.pointer(sh)
    wsb = L.lib().yms_conv_wgrad_ws_bytes(sp)

    def run(fill):
        xb, dzb = _in(x, dtype, fill), _in(dz, dtype, fill)
        ws = torch.full((wsb // 4 + 1,), NAN, dtype=torch.float32, device="cuda")
        dw = torch.full((sh.cout, sh.cin, sh.k, sh.k), SENT, device="cuda")
        L.call("yms_conv_wgrad", sp, xb.data_ptr(), xb.shape[-1], XOFF, dzb.data_ptr(), dzb.shape[-1], XOFF,
               ws.data_ptr(), wsb, dw.data_ptr(), acc, L.stream_ptr())
        return [dw]

    runs = _both(run)
    _same_and_inside(runs)
    assert (runs[0][0] != SENT).all()                         # every weight's gradient was written


DW_TINY = [(1, 1, 1, 8, 3), (2, 2, 2, 16, 3)]                 # test_dwconv_edges_gpu.TINY[:2]: (n, h, w, c, k)


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("shp", DW_TINY)
def test_dwconv_slots(shp, dt):
    n, h, w, c, k = shp
    dtype = H.DT[dt]
    g = torch.Generator().manual_seed(8)
    x, dz, wt = _rand(g, n, c, h, w), _rand(g, n, c, h, w), (_rand(g, c, k, k) / k).cuda()
    sc, sf = (torch.rand(c, generator=g) + 0.5).cuda(), (_rand(g, c) * 0.1).cuda()
    ds = L.DwShape(n, h, w, c, k, L.dtype_code(dtype))
    sp = ctypes.pointer(ds)
    rows = L.lib().yms_dwconv_stats_rows(sp)

    def fwd(stats):
        def run(fill):
            xb, y = _in(x, dtype, fill), _out(n, h, w, c, dtype)
            st = H.stats_buffer(rows, H.r8(c)) if stats else None
            L.call("yms_dwconv_fwd", sp, xb.data_ptr(), xb.shape[-1], XOFF, wt.data_ptr(), y.data_ptr(), y.shape[-1], YOFF,
                   None if stats else sc.data_ptr(), None if stats else sf.data_ptr(), L.ACT_NONE if stats else L.ACT_SILU,
                   L.ptr(st), H.r8(c) if stats else 0, L.stream_ptr())
            return [y] + ([st] if stats else [])
        return run

    def dgrad(acc):
        def run(fill):
            dzb, dx = _in(dz, dtype, fill), _out(n, h, w, c, dtype)
            L.call("yms_dwconv_dgrad", sp, dzb.data_ptr(), dzb.shape[-1], XOFF, wt.data_ptr(), dx.data_ptr(), dx.shape[-1],
                   YOFF, acc, L.stream_ptr())
            return [dx]
        return run

    for run in (fwd(False), fwd(True), dgrad(0), dgrad(1)):
        _same_and_inside(_both(run), c)


EW = (2, 9, 9, 40)                                            # (n, h, w, c) of the per-pixel passes


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("res", [False, True], ids=["nores", "res"])
def test_affine_act_slot(res, dt):
    n, h, w, c = EW
    dtype = H.DT[dt]
    g = torch.Generator().manual_seed(9)
    z, r = _rand(g, n, c, h, w), _rand(g, n, c, h, w)
    sc, sf = (torch.rand(c, generator=g) + 0.5).cuda(), (_rand(g, c) * 0.1).cuda()

    def run(fill):
        zb, rb, y = _in(z, dtype, fill), _in(r, dtype, fill) if res else None, _out(n, h, w, c, dtype)
        L.call("yms_affine_act", L.dtype_code(dtype), n * h * w, c, zb.data_ptr(), zb.shape[-1], XOFF, sc.data_ptr(),
               sf.data_ptr(), L.ACT_SILU, L.ptr(rb), rb.shape[-1] if res else 0, XOFF if res else 0, y.data_ptr(),
               y.shape[-1], YOFF, L.stream_ptr())
        return [y]

    _same_and_inside(_both(run), c)


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("gres", [None, 0, 1], ids=["nores", "res-store", "res-accumulate"])
def test_bn_act_bwd_apply_slot(gres, dt):
    n, h, w, c = EW
    dtype = H.DT[dt]
    g = torch.Generator().manual_seed(10)
    z, gy = _rand(g, n, c, h, w), _rand(g, n, c, h, w)
    sc, sf = (torch.rand(c, generator=g) + 0.5).cuda(), (_rand(g, c) * 0.1).cuda()
    mi = torch.cat([_rand(g, c) * 0.1, torch.rand(c, generator=g) + 0.5]).cuda()
    coef = (_rand(g, 2 * c) * 0.1).cuda()

    def run(fill):
        zb, gb, dz = _in(z, dtype, fill), _in(gy, dtype, fill), _out(n, h, w, c, dtype)
        gr = _out(n, h, w, c, dtype) if gres is not None else None
        L.call("yms_bn_act_bwd_apply", L.dtype_code(dtype), n * h * w, c, zb.data_ptr(), zb.shape[-1], XOFF, gb.data_ptr(),
               gb.shape[-1], XOFF, sc.data_ptr(), sf.data_ptr(), mi.data_ptr(), coef.data_ptr(), L.ACT_SILU, dz.data_ptr(),
               dz.shape[-1], YOFF, L.ptr(gr), gr.shape[-1] if gr is not None else 0, YOFF if gr is not None else 0,
               gres or 0, L.stream_ptr())
        return [dz] + ([gr] if gr is not None else [])

    runs = _both(run)
    _same_and_inside(runs, c)
    if gres is not None:
        _same_and_inside([r[1:] for r in runs], c)


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_upsample2x_fwd_slot(dt):
    n, h, w, c = 2, 5, 7, 24
    dtype = H.DT[dt]
    x = _rand(torch.Generator().manual_seed(11), n, c, h, w)

    def run(fill):
        xb, y = _in(x, dtype, fill), _out(n, 2 * h, 2 * w, c, dtype)
        L.call("yms_upsample2x_fwd", L.dtype_code(dtype), n, h, w, c, xb.data_ptr(), xb.shape[-1], XOFF, y.data_ptr(),
               y.shape[-1], YOFF, L.stream_ptr())
        return [y]

    runs = _both(run)
    _same_and_inside(runs, c)
    assert torch.equal(H.nchw(runs[1][0], c, YOFF).cpu(), x.to(dtype).float().repeat_interleave(2, 2).repeat_interleave(2, 3))


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("acc", [0, 1], ids=["store", "accumulate"])
@pytest.mark.parametrize("two", [False, True], ids=["a", "a+b"])
def test_add_views_slot(two, acc, dt):
    n, h, w, c = 2, 5, 7, 24
    dtype = H.DT[dt]
    g = torch.Generator().manual_seed(12)
    a, b = _rand(g, n, c, h, w), _rand(g, n, c, h, w)

    def run(fill):
        ab, bb, y = _in(a, dtype, fill), _in(b, dtype, fill) if two else None, _out(n, h, w, c, dtype)
        L.call("yms_add_views", L.dtype_code(dtype), n * h * w, c, ab.data_ptr(), ab.shape[-1], XOFF, L.ptr(bb),
               bb.shape[-1] if two else 0, XOFF if two else 0, y.data_ptr(), y.shape[-1], YOFF, acc, L.stream_ptr())
        return [y]

    _same_and_inside(_both(run), c)


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("ld", [8, 16])
def test_pack_input_writes_zero_padding_up_to_ld(ld, dt):
    """yms.h: "channels padded with zeros up to ld" -- zeros in [c, ld), the sentinel past the last pixel."""
    n, c, h, w = 2, 3, 5, 7
    dtype = H.DT[dt]
    x = _rand(torch.Generator().manual_seed(13), n, c, h, w).cuda()
    buf = torch.full((n * h * w * ld + 64,), SENT, dtype=dtype, device="cuda")
    L.call("yms_pack_input", L.dtype_code(dtype), n, c, h, w, x.data_ptr(), buf.data_ptr(), ld, L.stream_ptr())
    torch.cuda.synchronize()
    y = buf[:n * h * w * ld].view(n, h, w, ld)
    assert torch.equal(y[..., :c].permute(0, 3, 1, 2), x.to(dtype))
    assert (y[..., c:] == 0).all() and (buf[n * h * w * ld:] == SENT).all()
