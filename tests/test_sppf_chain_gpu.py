"""The SPPF pool chain as one launch per direction (sppf_chain_fwd_kernel / sppf_chain_bwd_kernel,
planes in LDS) through yms_sppf_pool_fwd / yms_sppf_pool_bwd, against torch's CPU max_pool2d chained
three times and its backward, and bit for bit against the per-pool launches (yms_sppf_route_set(0)).

Values are multiples of 0.25 in [-1, 1] with both zeros, so nearly every window holds ties and the
first maximum in scan order decides the sign of a zero result and the position a gradient goes to.
Every shape runs NaN-free (every element compared) and with NaNs at three positions, a corner among
them (NaN outputs compared by mask, everything else exactly).  The buffer is a concat view (ld =
4c + 8, slots at channel offset 8) whose padding channels hold a sentinel that must come back
bit-equal.  Each case asserts the route its shape takes."""
import functools

import pytest
import torch
import torch.nn.functional as F

from yms import _lib as L

pytestmark = pytest.mark.gpu

_DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
_SHAPES = [(1, 1, 1, 8), (1, 3, 4, 8), (2, 5, 7, 16), (1, 13, 17, 40), (3, 20, 20, 64), (1, 20, 20, 24)]
_CASES = [(s, dt) for dt in ("bf16", "f16", "f32") for s in _SHAPES] + \
         [(lbl, dt) for dt in ("bf16", "f16") for lbl in ("largest_fit", "first_unfit")]
OFF = 8


def _edge_plane(dt):
    """h = w of the largest square plane the one-launch route takes at c = 8, stepping upward"""
    s = 1
    while L.lib().yms_sppf_fused_fits(L.dtype_code(dt), s + 1, s + 1, 8):
        s += 1
        assert s < 4096
    return s


def _resolve(shape, dt):
    """-> (n, h, w, c), whether the one-launch route must take it"""
    if shape == "largest_fit":
        s = _edge_plane(dt)
        return (1, s, s, 8), True
    if shape == "first_unfit":
        s = _edge_plane(dt) + 1
        return (1, s, s, 8), False
    return shape, dt != torch.float32


@pytest.fixture
def route():
    prev = L.lib().yms_sppf_route_set(-1)
    yield lambda v: L.lib().yms_sppf_route_set(int(v))
    L.lib().yms_sppf_route_set(prev)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _slot(t, k, c):
    return t[..., OFF + k * c:OFF + (k + 1) * c]


@functools.lru_cache(maxsize=None)
def _inputs(shape, dt, nan):
    """-> (buf with slot 0 set, g0, forward reference [3 x NCHW fp32]) on the CPU, built once per case"""
    n, h, w, c = shape
    g = torch.Generator().manual_seed(1000 * n + 100 * h + 10 * w + c + (7 if nan else 0))
    ld = 4 * c + OFF
    x0 = torch.randint(-4, 5, (n, h, w, c), generator=g).float() * 0.25
    neg = torch.rand(n, h, w, c, generator=g) < 0.5
    x0 = torch.where((x0 == 0) & neg, torch.tensor(-0.0), x0)        # both zeros
    if nan:
        x0[0, 0, 0, 0] = float("nan")                                  # a corner
        x0[n - 1, h // 2, w // 2, c - 1] = float("nan")
        x0[0, h - 1, w // 3, c // 2] = float("nan")
    buf = torch.full((n, h, w, ld), 5.0)                               # slots 1..3: to be overwritten
    buf[..., :OFF] = -7.5                                              # padding sentinel
    buf[..., OFF:OFF + c] = x0
    buf = buf.to(dt)
    if dt == torch.float32:
        # multiples of 1/64 up to 4: through three pools at most 26^3 of them meet, so every partial
        # sum is a multiple of 1/64 below 2^17 -- exact in fp32, whatever the order
        g0 = torch.randint(-256, 257, (n, h, w, ld), generator=g).float() / 64
    else:
        g0 = torch.randn(n, h, w, ld, generator=g).to(dt)
    x = _slot(buf, 0, c).float().permute(0, 3, 1, 2).contiguous()      # the dtype-rounded input
    ref = []
    for _ in range(3):
        x = F.max_pool2d(x, 5, 1, 2)
        ref.append(x)
    return buf, g0, ref


def _run(buf, g0, shape, dt):
    n, h, w, c = shape
    ld = buf.shape[-1]
    b = buf.cuda()
    L.call("yms_sppf_pool_fwd", L.dtype_code(dt), n, h, w, c, b.data_ptr(), ld, OFF, L.stream_ptr())
    gb = g0.cuda()
    ws = torch.empty(L.lib().yms_sppf_ws_bytes(n, h, w, c), dtype=torch.uint8, device="cuda")
    L.call("yms_sppf_pool_bwd", L.dtype_code(dt), n, h, w, c, b.data_ptr(), ld, OFF, gb.data_ptr(), ld, OFF,
           ws.data_ptr(), L.stream_ptr())
    torch.cuda.synchronize()
    return b.cpu(), gb.cpu()


@pytest.mark.parametrize("nan", [False, True], ids=["finite", "nan"])
@pytest.mark.parametrize("shape,dtn", _CASES, ids=[f"{s}-{d}" for s, d in _CASES])
def test_sppf_chain_matches_torch_and_per_pool_route(shape, dtn, nan, route):
    dt = _DT[dtn]
    shape, fused = _resolve(shape, dt)
    n, h, w, c = shape
    assert bool(L.lib().yms_sppf_fused_fits(L.dtype_code(dt), h, w, c)) == fused
    buf, g0, ref = _inputs(shape, dt, nan)
    route(1)
    assert L.lib().yms_sppf_route_set(-1) == 1
    y1, gb1 = _run(buf, g0, shape, dt)
    route(0)
    y0, gb0 = _run(buf, g0, shape, dt)

    # forward: padding and slot 0 untouched, slots 1..3 equal to torch's chain, zero signs included
    assert torch.equal(_bits(y1[..., :OFF + c]), _bits(buf[..., :OFF + c]))
    for k in (1, 2, 3):
        got = _slot(y1, k, c).float().permute(0, 3, 1, 2)
        r = ref[k - 1]
        ok = ~torch.isnan(r)
        assert nan or ok.all()
        assert torch.equal(torch.isnan(got), ~ok), k
        assert torch.equal(got[ok], r[ok]), k
        assert torch.equal(torch.signbit(got[ok]), torch.signbit(r[ok])), k
    # regression pin: the two routes agree bit for bit (NaNs by mask)
    ok = ~torch.isnan(y0.float())
    assert torch.equal(torch.isnan(y1.float()), ~ok)
    assert torch.equal(_bits(y1)[ok], _bits(y0)[ok])

    # backward against torch's max_pool2d backward on the forward's own slots, each slot's gradient
    # rounded to the dtype before it feeds the next pool
    xs = y1.float()
    rg = g0.float().clone()
    for k in (3, 2, 1):
        xin = _slot(xs, k - 1, c).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        F.max_pool2d(xin, 5, 1, 2).backward(_slot(rg, k, c).permute(0, 3, 1, 2).contiguous())
        rg[..., OFF + (k - 1) * c:OFF + k * c] = \
            (_slot(rg, k - 1, c) + xin.grad.permute(0, 2, 3, 1)).to(dt).float()
    assert torch.equal(_bits(_slot(gb1, 3, c)), _bits(_slot(g0, 3, c)))           # slot 3 is only read
    assert torch.equal(_bits(gb1[..., :OFF]), _bits(g0[..., :OFF]))               # padding
    got = gb1.float()
    if dt == torch.float32:
        assert torch.equal(got, rg)              # exact addends (see _inputs): any order gives the same sum
    else:
        # fp32 sums of the same addends in another order: one rounding step of the dtype at most
        tol = 2 ** -7 if dt == torch.bfloat16 else 2 ** -10
        d = (got - rg).abs()
        assert (d <= tol * rg.abs() + 1e-6).all(), d.max().item()
    assert torch.equal(_bits(gb1), _bits(gb0))   # regression pin: same addends, order and rounding points
