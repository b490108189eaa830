"""Depthwise conv kernels (csrc/dwconv.hip) at the edges the width / channel-block matrix of
test_dwconv_gpu.py leaves open: every operand a channel slice of a wider buffer whose slack is hostile
(large finite values beside the inputs, a fixed pattern beside the outputs that must survive bit for
bit), maps smaller than the halo, the widths / heights at the host selectors' switches, f16 with
k = 3, both `accumulate` values onto NaN prefills, a NaN workspace and a bit-identical second weight
gradient, the four eval epilogues, and the branch-sum kernels in all three dtypes.

Reference: torch's grouped convolution (groups = C) and its autograd on the CPU in float64, on operands
rounded to the dtype under test; the weights stay fp32 (the kernels take them unpacked)."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from hiputil import DT, check_moments, r8
from test_dwconv_gpu import TOL, _close          # forward 2e-5 / 1e-2 / 2e-3 of max|ref|, dgrad twice that
from yms import _lib as L

pytestmark = pytest.mark.gpu

# the weight-gradient tolerance of test_dwconv_gpu.test_dwconv_fwd_dgrad_wgrad (inline there), of max|ref|
WG_TOL = {"f32": 1e-4, "bf16": 2e-3, "f16": 5e-4}
# moments: the same file's check_moments bound
ST_TOL = {"f32": 1e-4, "bf16": 1e-3, "f16": 1e-3}
ALL_DT = ("f32", "bf16", "f16")

# (off, trail) of each operand's view: non-zero multiples of 8, no two operands of a call alike
VIEWS = dict(x=(8, 24), y=(16, 8), z=(24, 16), dz=(32, 40), dx=(40, 32))
# a second set (other offsets for x and the eval y, larger ld everywhere) for test_dwconv_second_view_set
VIEWS2 = dict(x=(24, 8), y=(40, 48), z=(8, 56), dz=(16, 24), dx=(56, 16))
GUARD = 777.0


# ---- view harness ---------------------------------------------------------------------------------
def in_view(t, dtype, view, g):
    """channel-last [..., c] values -> device buffer [..., off + c + trail] of dtype with t at
    [off, off + c) and random +-(1e4 .. 3e4) in the slack (finite in f16): a read at the wrong channel
    misses by orders of magnitude"""
    off, trail = view
    c = t.shape[-1]
    shape = tuple(t.shape[:-1]) + (off + c + trail,)
    buf = (torch.rand(shape, generator=g) * 2e4 + 1e4) * (torch.randint(0, 2, shape, generator=g) * 2 - 1)
    buf = buf.to(dtype)
    buf[..., off:off + c] = t.to(dtype)
    return buf.cuda()


def out_view(lead, c, dtype, view, body=float("nan")):
    """-> (device buffer, its host prefill): slack = a fixed non-zero pattern, the view itself = body
    (channel-last values, or NaN: a kernel that stores must not read it)"""
    off, trail = view
    ld = off + c + trail
    idx = torch.arange(math.prod(lead) * ld).view(*lead, ld)
    pre = ((idx % 251 + 1).float() * 0.25).to(dtype)
    pre[..., off:off + c] = body if isinstance(body, float) else body.to(dtype)
    return pre.cuda(), pre


def body_of(buf, pre, c, view):
    """the view's values (host, fp64) after checking that the slack still holds its prefill bit for bit"""
    off, _ = view
    h = buf.cpu()
    assert torch.equal(h[..., :off], pre[..., :off]), "leading slack written"
    assert torch.equal(h[..., off + c:], pre[..., off + c:]), "trailing slack written"
    got = h[..., off:off + c].double()
    assert torch.isfinite(got).all()
    return got


def cl(t):
    return t.permute(0, 2, 3, 1)          # NCHW -> channel-last


class Case:
    """operands (rounded to dtype) and fp64 references of one (shape, dtype), computed once"""

    def __init__(self, shp, dt, views=VIEWS):
        n, h, w, c, k = shp
        self.shp, self.dt, self.dtype, self.v = shp, dt, DT[dt], views
        g = self.g = torch.Generator().manual_seed(sum(shp) * 7 + len(dt))
        self.x = torch.randn(n, c, h, w, generator=g).to(self.dtype).double()
        self.wt = torch.randn(c, 1, k, k, generator=g) / k
        self.dz = torch.randn(n, c, h, w, generator=g).to(self.dtype).double()
        xg = self.x.clone().requires_grad_(True)
        wg = self.wt.double().requires_grad_(True)
        z = F.conv2d(xg, wg, None, 1, k // 2, 1, c)
        z.backward(self.dz)
        self.z, self.dx, self.dw = z.detach(), xg.grad, wg.grad
        self.sh = L.DwShape(n, h, w, c, k, L.dtype_code(self.dtype))
        self.sp = ctypes.pointer(self.sh)
        self.wd = self.wt.contiguous().cuda()
        self.xb = in_view(cl(self.x), self.dtype, views["x"], g)
        self.dzb = in_view(cl(self.dz), self.dtype, views["dz"], g)

    def fwd(self, view, scale=None, shift=None, act=L.ACT_NONE, stats=None, stats_ld=0):
        n, h, w, c, k = self.shp
        y, pre = out_view((n, h, w), c, self.dtype, view)
        L.call("yms_dwconv_fwd", self.sp, self.xb.data_ptr(), self.xb.shape[-1], self.v["x"][0], self.wd.data_ptr(),
               y.data_ptr(), y.shape[-1], view[0], L.ptr(scale), L.ptr(shift), act, L.ptr(stats), stats_ld,
               L.stream_ptr())
        return y, body_of(y, pre, c, view)


def check_eval(cs):
    c = cs.shp[3]
    sc = torch.rand(c, generator=cs.g) + 0.5
    sf = torch.randn(c, generator=cs.g) * 0.1
    scd, sfd = sc.cuda(), sf.cuda()
    _, got = cs.fwd(cs.v["y"], scd, sfd, L.ACT_SILU)
    _close(got, cl(F.silu(cs.z * sc.double().view(1, -1, 1, 1) + sf.double().view(1, -1, 1, 1))), TOL[cs.dt])


def check_train(cs):
    n, h, w, c, k = cs.shp
    rows = L.lib().yms_dwconv_stats_rows(cs.sp)
    ld = r8(c) + 16                                   # wider than the channels: the counts' address depends on it
    size = rows * (2 * ld + 1)
    buf = torch.full((size + 1,), float("nan"), dtype=torch.float32, device="cuda")
    buf[size] = GUARD                                 # the first float past the declared size
    y, got = cs.fwd(cs.v["z"], stats=buf, stats_ld=ld)
    _close(got, cl(cs.z), TOL[cs.dt])
    assert buf[size].item() == GUARD
    counts = buf[rows * 2 * ld:size]
    assert counts.sum().item() == n * h * w
    check_moments((buf[:rows * 2 * ld].view(rows, 2, ld), counts), cs.z, ST_TOL[cs.dt])
    return y, got


def check_dgrad(cs):
    n, h, w, c, k = cs.shp
    base = torch.randn(n, h, w, c, generator=cs.g).to(cs.dtype)
    for acc in (0, 1):
        vdx = cs.v["dx"]
        dx, pre = out_view((n, h, w), c, cs.dtype, vdx, base if acc else float("nan"))
        L.call("yms_dwconv_dgrad", cs.sp, cs.dzb.data_ptr(), cs.dzb.shape[-1], cs.v["dz"][0], cs.wd.data_ptr(),
               dx.data_ptr(), dx.shape[-1], vdx[0], acc, L.stream_ptr())
        _close(body_of(dx, pre, c, vdx), cl(cs.dx) + (base.double() if acc else 0), TOL[cs.dt] * 2)


def check_wgrad(cs):
    n, h, w, c, k = cs.shp
    wsb = L.lib().yms_dwconv_wgrad_ws_bytes(cs.sp)
    assert wsb > 0 and wsb % (k * k * c * 4) == 0
    ndw = c * k * k
    dw0 = torch.randn(ndw, generator=cs.g)

    def run(ws_fill, acc):
        ws = torch.full((wsb // 4 + 1,), float("nan"), device="cuda")
        if ws_fill is not None:
            ws[:-1] = ws_fill
        ws[-1] = GUARD
        dw = torch.full((ndw + 8,), GUARD, device="cuda")
        dw[:ndw] = dw0.cuda() if acc else float("nan")
        L.call("yms_dwconv_wgrad", cs.sp, cs.xb.data_ptr(), cs.xb.shape[-1], cs.v["x"][0], cs.dzb.data_ptr(), cs.dzb.shape[-1],
               cs.v["dz"][0], ws.data_ptr(), wsb, dw.data_ptr(), acc, L.stream_ptr())
        out = dw.cpu()
        assert ws[-1].item() == GUARD and (out[ndw:] == GUARD).all(), "wrote past the workspace / dw"
        return out[:ndw]

    first = run(None, 0)                               # NaN workspace, NaN dw: every row written, dw stored
    _close(first.double().view(c, 1, k, k), cs.dw, WG_TOL[cs.dt])
    second = run(torch.randn(wsb // 4, generator=cs.g).cuda() * 100, 0)
    assert torch.equal(first, second), "weight gradient depends on the workspace's prior contents"
    _close((run(None, 1).double() - dw0.double()).view(c, 1, k, k), cs.dw, WG_TOL[cs.dt])


def run_all_passes(shp, dt, views=VIEWS):
    cs = Case(shp, dt, views)
    check_eval(cs)
    check_train(cs)
    check_dgrad(cs)
    check_wgrad(cs)
    return cs


# ---- shapes (n, h, w, c, k); routing copied from the host selectors of dwconv.hip --------------------
# forward / dgrad: 16-bit k = 7 on maps <= 48 wide -> dwconv_mfma_kernel (NCB 2 for w <= 32, else 3);
#   otherwise the strip walker, TX = 32 if w % 32 == 0, 40 if w % 40 == 0, 20 if w <= 20, 40 if w <= 40,
#   else 32; 16-bit k = 3 takes 64-channel blocks (G 8) for C % 64 == 0, 56-channel blocks (G 7) for
#   C % 56 == 0 and C % 32 != 0, else 32-channel blocks (G 4, and always for fp32 and k >= 5).
# weight gradient: fp32 -> tile kernel (8 x 32 tiles); 16-bit k = 3 -> strip kernel (dwconv_wgrad3, G 4);
#   16-bit k >= 5 on maps <= 64 wide (k = 5: <= 96) -> MFMA with ceil(w / 32) column chunks, NB = 2 for one
#   chunk and 17 <= h <= 32; wider -> register-prefetch kernel (dwconv_wgrad2).
# tiny maps, every k: all of TX 20, one tile, ring rows mostly padding; 16-bit k = 7 -> MFMA forward (NCB 2)
# with 1-3 real rows in the 16-row unit; 16-bit k >= 5 -> MFMA weight gradient, one chunk, NB 1 (h = 20, w = 1: NB 2)
TINY = [(n, h, w, c, k) for k in (3, 5, 7, 9) for (n, h, w, c) in
        ((1, 1, 1, 8), (2, 2, 2, 16), (1, 3, 5, 24), (3, 1, 20, 8), (1, 20, 1, 8))]
# tiny maps, k = 3, 16-bit: 64-channel blocks (C 64), 56-channel blocks (C 56: one, C 112: two) on less than a tile
TINY += [(2, 4, 4, 64, 3), (1, 2, 2, 56, 3), (1, 2, 2, 112, 3)]
# width switches at h 13, n 2, C 24 (a partial 32-channel block; one and a half 16-channel MFMA groups):
WIDTHS = [
    (2, 13, 21, 24, 3), (2, 13, 21, 24, 9),   # w 21: first TX 40 width past TX 20; k 9 wgrad MFMA 1 chunk
    (2, 13, 41, 24, 3), (2, 13, 41, 24, 9),   # w 41: first TX 32 width past TX 40, 9-column last tile; wgrad MFMA 2 chunks
    (2, 13, 48, 24, 7),                       # last MFMA forward / dgrad width: three full 16-column blocks (NCB 3)
    (2, 13, 49, 24, 7),                       # first k 7 strip width (TX 32); wgrad MFMA 2 chunks
    (2, 13, 65, 24, 7), (2, 13, 65, 24, 9),   # w 65: wgrad MFMA -> register prefetch (TX 32), 1-column last tile
    (2, 13, 96, 24, 5),                       # last MFMA wgrad width of k 5: three full chunks (NCH 3); TX 32 strips
    (2, 13, 97, 24, 5),                       # first register-prefetch width of k 5, 1-column last tile
    (2, 13, 64, 24, 9),                       # last MFMA wgrad width of k 9: two full chunks
]
# height switches of the 16-row MFMA units at w 24 (TX 40 strips, one chunk), C 16, n 3: weight gradient
# NB = 1 / 2 / 2 / 1 at h 16 / 17 / 32 / 33 (k 5, 9); k 7 adds the MFMA forward / dgrad (NCB 2) with a 1-row last unit
HEIGHTS = [(3, h, 24, 16, k) for k in (5, 9, 7) for h in (16, 17, 32, 33)]
# f16, k = 3 (f32 and bf16 run these in test_dwconv_gpu.py): G 8 at TX 20 / 40 / 32, G 7 at TX 40 / 20,
# G 8 with C 192 at TX 40 (w 23), G 4 at TX 40 (w 80) and TX 32 (w 45); weight gradient: strip kernel at each TX
F16_K3 = [(2, 20, 20, 64, 3), (2, 40, 40, 128, 3), (2, 16, 64, 64, 3), (2, 24, 40, 112, 3), (1, 20, 20, 168, 3),
          (1, 9, 23, 192, 3), (2, 24, 80, 32, 3), (2, 11, 45, 24, 3)]

CASES = [(dt, sh) for sh in TINY + WIDTHS + HEIGHTS for dt in ALL_DT] + [("f16", sh) for sh in F16_K3]


@pytest.mark.parametrize("dt,shp", CASES)
def test_dwconv_edges_through_views(shp, dt):
    """eval forward, train forward + statistics, dgrad (store onto NaN / accumulate) and weight gradient
    (store onto NaN / accumulate, NaN workspace, bit-identical rerun) with every operand a view"""
    run_all_passes(shp, dt)


# the offsets varied: VIEWS2 (x at 24 instead of 8, the eval y at 40 instead of 16, every ld larger) on one shape
# per route -- TX 20 / G 8, TX 40 / G 7, TX 32 / G 4 (k 3: strip weight gradient at each TX); MFMA forward / dgrad
# NCB 3 and NCB 2; MFMA weight gradient with 2 chunks, NB 2, 3 chunks; register prefetch; a map inside the halo
# (fp32: the 32-channel strip walker and the tile weight gradient on the same shapes)
VIEWS2_SHAPES = [(2, 20, 20, 64, 3), (2, 24, 40, 112, 3), (2, 13, 41, 24, 3), (2, 13, 48, 24, 7), (3, 17, 24, 16, 7),
                 (2, 13, 96, 24, 5), (2, 13, 65, 24, 9), (1, 3, 5, 24, 9)]


@pytest.mark.parametrize("dt", ALL_DT)
@pytest.mark.parametrize("shp", VIEWS2_SHAPES)
def test_dwconv_second_view_set(shp, dt):
    """every pass again at other channel offsets and row strides: a result must not depend on them"""
    run_all_passes(shp, dt, VIEWS2)


# one multi-strip case, sized for 256 CUs.  (8, 88, 64, 256, 3), 16-bit: TX 32 / TY 8 -> 2 x 11 tiles per image.
# forward / dgrad (dw_strip_grid): G 8 -> 4 channel groups, base = 8 * 2 * 4 = 64 blocks per strip row, slots =
#   2 * 256 = 512; cost(tps) = rounds * (8 tps + 2): tps 11 -> 90, 6 -> 50, 4 -> 34, 3 -> 26 (4 strips, 256 blocks),
#   2 -> 18 (6 strips, 384 blocks, one round), 1 -> 2 * 10 = 20 (11 strips, 704 blocks, two rounds): tps = 2, six
#   strips per tile column, the last one a single tile.
# weight gradient (dw_wg3_grid): G 4 -> 8 channel groups, base = 128, slots = 512; cost(tps) = rounds *
#   (8 tps + 2 + 24): tps 11 -> 114, 6 -> 74, 4 -> 58, 3 -> 50 (4 strips, 512 blocks, one round), 2 -> 2 * 42 = 84,
#   1 -> 3 * 34: tps = 3, four strips, the last one 2 tiles; one workspace row per (image, tile column, strip).
MULTI_STRIP = (8, 88, 64, 256, 3)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_dwconv_multi_strip_through_views(dt):
    if torch.cuda.get_device_properties(0).multi_processor_count != 256:
        pytest.skip("the strip split is derived for 256 CUs")
    n, h, w, c, k = MULTI_STRIP
    sp = ctypes.pointer(L.DwShape(n, h, w, c, k, L.dtype_code(DT[dt])))
    assert L.lib().yms_dwconv_wgrad_ws_bytes(sp) == 8 * 2 * 4 * (9 * 256 * 4)
    run_all_passes(MULTI_STRIP, dt)


# ---- eval epilogues ---------------------------------------------------------------------------------
# strip kernel with a 9-column last tile (G 4), 64-channel blocks on less than a tile, and k = 7 on a
# 48-wide map (16-bit: the MFMA kernel, NCB 3; fp32: the strip walker)
@pytest.mark.parametrize("dt", ALL_DT)
@pytest.mark.parametrize("shp", [(2, 13, 41, 24, 3), (2, 4, 4, 64, 3), (2, 13, 48, 24, 7), (3, 17, 24, 16, 7)])
def test_dwconv_eval_epilogues(shp, dt):
    """scale + shift + SiLU | scale + shift | SiLU alone | nothing: scale / shift NULL is the identity,
    ACT_NONE applies no activation, and with everything off eval writes the train-mode z bit for bit"""
    cs = Case(shp, dt)
    c = shp[3]
    sc = torch.rand(c, generator=cs.g) + 0.5
    sf = torch.randn(c, generator=cs.g) * 0.1
    scd, sfd = sc.cuda(), sf.cuda()
    aff = cs.z * sc.double().view(1, -1, 1, 1) + sf.double().view(1, -1, 1, 1)
    for scale, shift, act, ref in ((scd, sfd, L.ACT_SILU, F.silu(aff)), (scd, sfd, L.ACT_NONE, aff),
                                   (None, None, L.ACT_SILU, F.silu(cs.z)), (None, None, L.ACT_NONE, cs.z)):
        _, got = cs.fwd(cs.v["y"], scale, shift, act)
        _close(got, cl(ref), TOL[dt])
    _, z_train = check_train(cs)
    assert torch.equal(got, z_train), "eval with no scale, shift or activation differs from the train-mode z"


# ---- branch-sum kernels -----------------------------------------------------------------------------
V_A, V_B, V_S = (8, 16), (16, 24), (24, 8)


@pytest.mark.parametrize("npix,c", [(3001, 24), (1, 8)])
@pytest.mark.parametrize("dt", ALL_DT)
def test_add_views_all_forms(dt, npix, c):
    """y (+)= a + b and y (+)= a (b = NULL: the branch-sum backward), every view with its own ld and
    offset, against the fp32 sum in the kernel's order (a + b) + y rounded once"""
    dtype = DT[dt]
    g = torch.Generator().manual_seed(npix + c)
    a = torch.randn(npix, c, generator=g).to(dtype)
    b = torch.randn(npix, c, generator=g).to(dtype)
    y0 = torch.randn(npix, c, generator=g).to(dtype)
    ab, bb = in_view(a, dtype, V_A, g), in_view(b, dtype, V_B, g)
    for with_b in (True, False):
        for acc in (0, 1):
            y, pre = out_view((npix,), c, dtype, V_S, y0 if acc else float("nan"))
            L.call("yms_add_views", L.dtype_code(dtype), npix, c, ab.data_ptr(), ab.shape[-1], V_A[0],
                   bb.data_ptr() if with_b else None, bb.shape[-1] if with_b else 0, V_B[0] if with_b else 0,
                   y.data_ptr(), y.shape[-1], V_S[0], acc, L.stream_ptr())
            e = a.float() + b.float() if with_b else a.float()
            if acc:
                e = e + y0.float()
            assert torch.equal(body_of(y, pre, c, V_S), e.to(dtype).double()), (with_b, acc)


@pytest.mark.parametrize("npix,c", [(3001, 24), (1, 8)])
@pytest.mark.parametrize("acc1,acc2", [(0, 0), (1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("dt", ALL_DT)
def test_add_grad2_all_forms(dt, acc1, acc2, npix, c):
    """ga (+)= g and gb (+)= g in one pass: fp32 sum rounded once, a stored addend never read"""
    dtype = DT[dt]
    gen = torch.Generator().manual_seed(npix + c + 2 * acc1 + acc2)
    g = torch.randn(npix, c, generator=gen).to(dtype)
    a0 = torch.randn(npix, c, generator=gen).to(dtype)
    b0 = torch.randn(npix, c, generator=gen).to(dtype)
    gv = in_view(g, dtype, V_S, gen)
    ga, pa = out_view((npix,), c, dtype, V_A, a0 if acc1 else float("nan"))
    gb, pb = out_view((npix,), c, dtype, V_B, b0 if acc2 else float("nan"))
    L.call("yms_add_grad2", L.dtype_code(dtype), npix, c, gv.data_ptr(), gv.shape[-1], V_S[0], ga.data_ptr(),
           ga.shape[-1], V_A[0], acc1, gb.data_ptr(), gb.shape[-1], V_B[0], acc2, L.stream_ptr())
    ea = (a0.float() + g.float() if acc1 else g.float()).to(dtype).double()
    eb = (b0.float() + g.float() if acc2 else g.float()).to(dtype).double()
    assert torch.equal(body_of(ga, pa, c, V_A), ea)
    assert torch.equal(body_of(gb, pb, c, V_B), eb)


# ---- the argument table's baselines ---------------------------------------------------------------------
def test_argument_table_baselines_are_valid():
    """every valid call that test_dwconv_args_cpu.py breaks one argument of returns YMS_OK on device
    memory (one zeroed 16 MiB buffer behind every pointer: the values do not matter here), so its rows
    are refused for the broken argument and not for the baseline"""
    import test_dwconv_args_cpu as A
    buf = torch.zeros(16 << 20, dtype=torch.uint8, device="cuda")
    for label, (name, good) in A.baselines(buf.data_ptr()).items():
        args = [L.stream_ptr() if k == "stream" else v for k, v in good.items()]
        assert getattr(L.lib(), name)(*args) == 0, label
    torch.cuda.synchronize()
