"""Layout, cast, upsample and BN-fold entry points of include/yms.h driven directly through the
C-ABI, at shapes the whole-model tests never reach: channel counts that are no multiple of 8 or 64
together with pixel counts that are no multiple of 64, views at a channel offset inside a wider
buffer, every dtype pair, and element counts past the 16384 x 256 grid cap.  Everything but
yms_bn_fold is a data movement or a single rounding, so the checks are exact (torch.equal); every
output buffer is pre-filled with NaN and the part outside the written view must keep its bits."""
import ctypes

import pytest
import torch

from hiputil import DT, r8
from yms import _lib as L

pytestmark = pytest.mark.gpu

DTS = ["bf16", "f16", "f32"]
NAN = float("nan")


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _randn(shape, seed, dtype=torch.float32):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dtype)


def _outside(buf, off, c):
    """the channels of an NHWC buffer that lie outside the view [off, off + c)"""
    return torch.cat([buf[..., :off], buf[..., off + c:]], -1)


UP_SHAPES = [(1, 1, 1, 8), (2, 5, 7, 20), (3, 4, 6, 3), (1, 20, 20, 64)]
OFFS = [(0, 0), (8, 0), (0, 8), (8, 8)]


@pytest.mark.parametrize("n,h,w,c", UP_SHAPES)
@pytest.mark.parametrize("dt", DTS)
def test_upsample2x_fwd_exact(n, h, w, c, dt):
    """Nearest x2: every output pixel (Y, X) is a copy of input pixel (Y // 2, X // 2), for source and
    destination views at channel offsets 0 / 8 of buffers wider than the view; the destination's other
    channels keep their NaN sentinel."""
    dtype, code = DT[dt], L.dtype_code(DT[dt])
    for xoff, yoff in OFFS:
        xld, yld = r8(xoff + c) + 8, r8(yoff + c) + 16
        x = _randn((n, h, w, xld), n * 100 + c + xoff).to(dtype).cuda()
        y = torch.full((n, 2 * h, 2 * w, yld), NAN, dtype=dtype, device="cuda")
        y0 = y.clone()
        L.call("yms_upsample2x_fwd", code, n, h, w, c, x.data_ptr(), xld, xoff, y.data_ptr(), yld, yoff,
               L.stream_ptr())
        torch.cuda.synchronize()
        ref = x[..., xoff:xoff + c].repeat_interleave(2, 1).repeat_interleave(2, 2)
        assert torch.equal(y[..., yoff:yoff + c], ref), (xoff, yoff)
        assert _same_bits(_outside(y, yoff, c), _outside(y0, yoff, c)), (xoff, yoff)


def _upsample_bwd_ref(gy, old, off_g, c, dtype):
    """fp32 sum in the kernel's order -- old value (or 0), then taps (0,0), (0,1), (1,0), (1,1) --
    rounded once to the dtype."""
    s = old.float() if old is not None else torch.zeros_like(gy[:, ::2, ::2, off_g:off_g + c], dtype=torch.float32)
    for dy in (0, 1):
        for dx in (0, 1):
            s = s + gy[:, dy::2, dx::2, off_g:off_g + c].float()
    return s.to(dtype)


def _upsample_bwd_case(n, h, w, c, dt, acc, goff, xoff, gld=None, on_device=False):
    dtype, code = DT[dt], L.dtype_code(DT[dt])
    gld, xld = gld or r8(goff + c) + 8, r8(xoff + c) + 16
    dev = "cuda" if on_device else "cpu"      # the big case draws its data and its reference on the device
    g = torch.Generator(device=dev).manual_seed(n + h + c + goff)
    gy = torch.randn((n, 2 * h, 2 * w, gld), generator=g, device=dev).to(dtype)
    gx = torch.full((n, h, w, xld), NAN, dtype=dtype, device=dev)
    old = None
    if acc:
        old = torch.randn((n, h, w, c), generator=g, device=dev).to(dtype)
        gx[..., xoff:xoff + c] = old
    gyd, gxd = gy.cuda(), gx.cuda()
    gx0 = gxd.clone()
    L.call("yms_upsample2x_bwd", code, n, h, w, c, gyd.data_ptr(), gld, goff, gxd.data_ptr(), xld, xoff, acc,
           L.stream_ptr())
    torch.cuda.synchronize()
    ref = _upsample_bwd_ref(gy, old, goff, c, dtype).cuda()
    assert torch.equal(gxd[..., xoff:xoff + c], ref), (acc, goff, xoff)
    assert _same_bits(_outside(gxd, xoff, c), _outside(gx0, xoff, c)), (acc, goff, xoff)


@pytest.mark.parametrize("n,h,w,c", UP_SHAPES)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("acc", [0, 1])
def test_upsample2x_bwd_exact(n, h, w, c, dt, acc):
    """gx (+)= the four taps of gy, exact: the reference adds in fp32 in the kernel's order (old value,
    then (0,0), (0,1), (1,0), (1,1)) on the CPU and rounds once, so no ulp allowance is needed.
    Without accumulate the destination view starts as NaN and must be overwritten; channels outside
    the view (and the masked c % 8 tail's neighbours) keep the NaN sentinel."""
    for goff, xoff in OFFS:
        _upsample_bwd_case(n, h, w, c, dt, acc, goff, xoff)


def test_upsample2x_bwd_past_grid_cap():
    """8 x 256 x 256 x 72 bf16 with accumulate: 8 * 256 * 256 * 9 = 4,718,592 eight-channel items, above
    the 16384 blocks x 256 threads the launch is capped at, so every thread takes a second trip
    through the grid-stride loop.  (8 x 128 x 128 x 72 has 1,179,648 items and stays below the cap.)
    Data and the fp32 reference (the same additions in the same order) are evaluated on the device."""
    _upsample_bwd_case(8, 256, 256, 72, "bf16", 1, 0, 8, gld=72, on_device=True)


@pytest.mark.parametrize("n,c,h,w,ld", [(2, 3, 5, 7, 8), (1, 5, 9, 13, 16), (2, 8, 4, 4, 8), (1, 12, 3, 3, 32)])
@pytest.mark.parametrize("dt", DTS)
def test_pack_input_exact(n, c, h, w, ld, dt):
    """NCHW fp32 -> NHWC dtype: channels [0, c) are the rounded input, channels [c, ld) are written as
    exact (+0) zeros (the one entry point whose contract writes the padding), nothing after the last
    pixel is touched."""
    dtype, code = DT[dt], L.dtype_code(DT[dt])
    x = _randn((n, c, h, w), n + c + h)
    npix = n * h * w
    flat = torch.full((npix * ld + 64,), NAN, dtype=dtype, device="cuda")
    flat0 = flat.clone()
    xd = x.cuda()
    L.call("yms_pack_input", code, n, c, h, w, xd.data_ptr(), flat.data_ptr(), ld, L.stream_ptr())
    torch.cuda.synchronize()
    y = flat[:npix * ld].view(n, h, w, ld)
    assert torch.equal(y[..., :c], x.permute(0, 2, 3, 1).to(dtype).cuda())
    assert (_bits(y[..., c:]) == 0).all()
    assert _same_bits(flat[npix * ld:], flat0[npix * ld:])


HW = [(5, 7), (8, 8), (9, 13), (1, 65)]
CS = [3, 64, 65, 130]
RUNNER_PAIRS = [("f32", "bf16"), ("f32", "f32"), ("bf16", "bf16"), ("f16", "f16")]


def _layout_shapes():
    for (h, w) in HW:
        for c in CS:
            for n in (1, 3):
                for ld, off in ((r8(c), 0), (r8(c) + 16, 8)):
                    yield n, h, w, c, ld, off


def _nchw_to_nhwc_case(dn, dv, n, h, w, c, ld, off, acc):
    tn, tv = DT[dn], DT[dv]
    x = _randn((n, c, h, w), n * 1000 + c * 10 + h + off).to(tn).cuda()
    y = torch.full((n, h, w, ld), NAN, dtype=tv, device="cuda")
    if acc:
        y[..., off:off + c] = _randn((n, h, w, c), c + h + 3).to(tv).cuda()
    y0 = y.clone()
    L.call("yms_nchw_to_nhwc", L.dtype_code(tn), L.dtype_code(tv), n, h, w, c, x.data_ptr(), y.data_ptr(), ld, off,
           acc, L.stream_ptr())
    torch.cuda.synchronize()
    ref = x.permute(0, 2, 3, 1).float()
    if acc:
        ref = y0[..., off:off + c].float() + ref
    key = (dn, dv, n, h, w, c, ld, off, acc)
    assert torch.equal(y[..., off:off + c], ref.to(tv)), key
    assert _same_bits(_outside(y, off, c), _outside(y0, off, c)), key


def _nhwc_to_nchw_case(dv, dn, n, h, w, c, ld, off):
    tn, tv = DT[dn], DT[dv]
    x = _randn((n, h, w, ld), n * 1000 + c * 10 + h + off).to(tv).cuda()     # random outside the view too
    count = n * c * h * w
    flat = torch.full((count + 64,), NAN, dtype=tn, device="cuda")
    flat0 = flat.clone()
    L.call("yms_nhwc_to_nchw", L.dtype_code(tv), L.dtype_code(tn), n, h, w, c, x.data_ptr(), ld, off,
           flat.data_ptr(), L.stream_ptr())
    torch.cuda.synchronize()
    ref = x[..., off:off + c].permute(0, 3, 1, 2).float().to(tn).contiguous()
    key = (dv, dn, n, h, w, c, ld, off)
    assert torch.equal(flat[:count].view(n, c, h, w), ref), key
    assert _same_bits(flat[count:], flat0[count:]), key


@pytest.mark.parametrize("dn,dv", RUNNER_PAIRS)
@pytest.mark.parametrize("acc", [0, 1])
def test_nchw_to_nhwc_exact(dn, dv, acc):
    """The 64 x 64 LDS transpose into an NHWC view, tail tiles in both directions (hw % 64 != 0 with
    c % 64 != 0): exact against (old.float() + x.float()).to(dtype) when accumulating, a rounded copy
    otherwise; the destination's channels outside the view keep their NaN."""
    for n, h, w, c, ld, off in _layout_shapes():
        _nchw_to_nhwc_case(dn, dv, n, h, w, c, ld, off, acc)


@pytest.mark.parametrize("dn,dv", RUNNER_PAIRS)
def test_nhwc_to_nchw_exact(dn, dv):
    """The transpose back: the NHWC view at (ld, off) -> contiguous NCHW, nothing past the last element."""
    for n, h, w, c, ld, off in _layout_shapes():
        _nhwc_to_nchw_case(dv, dn, n, h, w, c, ld, off)


@pytest.mark.parametrize("dn", DTS)
@pytest.mark.parametrize("dv", DTS)
def test_layout_all_dtype_pairs(dn, dv):
    """All nine (NCHW dtype, NHWC dtype) pairs on one ragged shape (3 x 9 x 13, 65 channels at offset 8)."""
    n, h, w, c = 3, 9, 13, 65
    ld, off = r8(c) + 16, 8
    for acc in (0, 1):
        _nchw_to_nhwc_case(dn, dv, n, h, w, c, ld, off, acc)
    _nhwc_to_nchw_case(dv, dn, n, h, w, c, ld, off)


def _cast_values(count):
    """fp32 values: randn at three scales, the exact halfway points of the bf16 and f16 roundings
    (ties to an even and to an odd neighbour), f16 subnormals and their halfway points, and values
    around the f16 overflow threshold (65520 is the tie that rounds to inf)."""
    g = torch.Generator().manual_seed(count)
    base = torch.randn(3 * 16, generator=g) * torch.tensor([1.0, 1e-6, 1e5]).repeat_interleave(16)
    bits = base[:16].view(torch.int32)
    half_bf16 = torch.cat([(bits & ~0xFFFF) | 0x8000, (bits & ~0x1FFFF) | 0x18000]).view(torch.float32)
    half_f16 = torch.cat([(bits & ~0x1FFF) | 0x1000, (bits & ~0x3FFF) | 0x3000]).view(torch.float32)
    sub = torch.tensor([2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -24, 2.5 * 2.0 ** -24, 1e-7, 3e-6, 6e-5, 6.1e-5,
                        2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, 2.0 ** -26, 0.0, -0.0])
    big = torch.tensor([65504.0, 65519.0, 65520.0, 65521.0, 65535.0, 65536.0, 1e5, 7e4, 3.3e38])
    pool = torch.cat([half_bf16, half_f16, sub, -sub, big, -big, base])      # 156 values: counts >= 255 see all
    return pool.repeat(-(-count // pool.numel()))[:count].clone()


@pytest.mark.parametrize("di", DTS)
@pytest.mark.parametrize("do", DTS)
@pytest.mark.parametrize("count", [1, 255, 257, 16384 * 256 + 3])
def test_cast_exact(di, do, count):
    """yms_cast: one round-to-nearest-even conversion through fp32, bit-for-bit against
    x.float().to(dtype) -- ties, f16 subnormals, overflow to inf, signed zeros -- for every dtype pair,
    one thread, one block +- 1 and a count past the grid cap; the guard tail is untouched."""
    ti, to = DT[di], DT[do]
    x = _cast_values(count).to(ti).cuda()
    y = torch.full((count + 64,), NAN, dtype=to, device="cuda")
    y0 = y.clone()
    L.call("yms_cast", L.dtype_code(ti), L.dtype_code(to), count, x.data_ptr(), y.data_ptr(), L.stream_ptr())
    torch.cuda.synchronize()
    ref = x.cpu().float().to(to).cuda()
    assert _same_bits(y[:count], ref)
    assert _same_bits(y[count:], y0[count:])


@pytest.mark.parametrize("c", [1, 8, 257, 1000])
def test_bn_fold(c):
    """Eval fold.  BN branch against fp64: scale = g / sqrt(rv + eps) within 1e-6 relative; shift =
    b - rm * scale within 1e-6 of |b| + |rm * scale| (the fp32 subtraction's own operands: where the
    two terms cancel, no fp32 evaluation can be 1e-6 relative to the difference).  Running variances
    go down to 1e-6, a thousand times below eps = 1e-3, so a fold without eps is off by ~30x there.
    Bias-only branch (gamma NULL): scale == 1 and shift == beta (or 0 with beta NULL), exactly."""
    g = torch.Generator().manual_seed(c)
    gam = torch.randn(c, generator=g)
    bet = torch.randn(c, generator=g)
    rm = torch.randn(c, generator=g) * 10
    rv = 10.0 ** (torch.rand(c, generator=g) * 7 - 6)
    rv[0] = 1e-6
    eps = 1e-3
    dev = [t.cuda() for t in (gam, bet, rm, rv)]

    def run(gp, bp, rmp, rvp):
        out = torch.full((2, c + 8), NAN, device="cuda")
        L.call("yms_bn_fold", c, gp, bp, rmp, rvp, ctypes.c_float(eps), out[0].data_ptr(), out[1].data_ptr(),
               L.stream_ptr())
        torch.cuda.synchronize()
        assert torch.isnan(out[:, c:]).all()
        return out[0, :c].cpu(), out[1, :c].cpu()

    sc, sh = run(*[t.data_ptr() for t in dev])
    sc64 = gam.double() / (rv.double() + float(torch.tensor(eps))).sqrt()
    sh64 = bet.double() - rm.double() * sc64
    e_sc = ((sc.double() - sc64).abs() / sc64.abs()).max().item()
    e_sh = ((sh.double() - sh64).abs() / (bet.double().abs() + (rm.double() * sc64).abs())).max().item()
    assert e_sc <= 1e-6 and e_sh <= 1e-6, (e_sc, e_sh)
    sc, sh = run(None, dev[1].data_ptr(), None, None)
    assert torch.equal(sc, torch.ones(c)) and torch.equal(sh, bet)
    sc, sh = run(None, None, None, None)
    assert torch.equal(sc, torch.ones(c)) and (_bits(sh) == 0).all()
