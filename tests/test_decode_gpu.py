"""yms_head_decode (with and without the fused NMS prep) and yms_dfl through the C-ABI against an
fp64 torch evaluation of the reference head's eval decode (yolov8_head.py:127-158, DFL
components.py:162-191) on the dtype-rounded logits: per side softmax over 16 bins -> expectation,
anchors at (x + 0.5, y + 0.5), lt = a - d[:2], rb = a + d[2:], ((lt + rb) / 2, rb - lt) x stride,
sigmoid of the class logits.

Tolerance of the decode.  The same formula is evaluated in fp32 torch on the CPU on every input of
test_head_decode_matches_fp64; its largest error against fp64 is measured (module fixture), and the
kernel may be 4x as far from fp64 (the device expf and the shuffle-tree summation order differ from
torch's by a few ulp), never further than the fp32 whole-model golden test allows (1e-4 of the
largest box coordinate, 1e-5 absolute on probabilities).  Measured: the fp32 CPU evaluation is up to
1.6e-7 of the largest box coordinate from fp64 on boxes (2.4e-8 .. 1.6e-7 over the cases) and up to
8.8e-8 on probabilities (4.9e-8 .. 8.8e-8), so the kernel's bound is 6.4e-7 on boxes, relative to
the largest box coordinate of the case, and 3.5e-7 absolute on probabilities."""
import ctypes

import pytest
import torch

from hiputil import DT, r8
from yms import _lib as L

pytestmark = pytest.mark.gpu

DTS = ["bf16", "f16", "f32"]
LEVEL_SETS = {
    "one": ([(5, 7)], [8.0]),
    "three": ([(8, 8), (4, 4), (2, 2)], [8.0, 16.0, 32.0]),
    "four": ([(6, 10), (3, 5), (2, 3), (1, 2)], [8.0, 16.0, 32.0, 64.0]),
}
BOX_CAP, PROB_CAP = 1e-4, 1e-5


def make_levels(levels, n, nc, no_ld, dtype, seed):
    """Raw head maps [n, h, w, no_ld] (64 DFL logits, nc class logits, NaN in the padding channels):
    randn x 3; a block of saturated anchors (one DFL bin at +40, the others -40, class logits +-30);
    a block whose class logits are multiples of 0.5 in [-2, 2] (equal maxima on different lanes --
    classes c and c + 16 -- and on the same lane)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for h, w in levels:
        t = torch.randn(n, h * w, no_ld, generator=g) * 3
        k = max(1, (h * w) // 3)
        sat = torch.full((n, k, 4, 16), -40.0)
        sat.scatter_(3, torch.randint(0, 16, (n, k, 4, 1), generator=g), 40.0)
        t[:, :k, :64] = sat.view(n, k, 64)
        t[:, :k, 64:64 + nc] = torch.randint(0, 2, (n, k, nc), generator=g).float() * 60 - 30
        q = torch.randint(-4, 5, (n, h * w - 2 * k, nc), generator=g).float() * 0.5 if h * w > 2 * k else None
        if q is not None:
            t[:, 2 * k:, 64:64 + nc] = q
        t[:, :, 64 + nc:] = float("nan")
        out.append(t.view(n, h, w, no_ld).to(dtype))
    return out


def ref_decode(lv, nc, strides, fd):
    """[n, A, 4 + nc] in precision fd from the (dtype-rounded) level maps."""
    outs = []
    for t, st in zip(lv, strides):
        n, h, w, _ = t.shape
        v = t[..., :64 + nc].to(fd).reshape(n, h * w, 64 + nc)
        d = (v[..., :64].reshape(n, h * w, 4, 16).softmax(-1) * torch.arange(16, dtype=fd)).sum(-1)
        a = torch.stack([torch.arange(w, dtype=fd).repeat(h) + 0.5,
                         torch.arange(h, dtype=fd).repeat_interleave(w) + 0.5], -1)
        lt, rb = a - d[..., :2], a + d[..., 2:]
        box = torch.cat([(lt + rb) / 2, rb - lt], -1) * st
        outs.append(torch.cat([box, torch.sigmoid(v[..., 64:])], -1))
    return torch.cat(outs, 1)


def errors(got, ref):
    """(largest box error relative to the largest |box coordinate|, largest probability error)"""
    got, ref = got.double(), ref.double()
    return (((got[..., :4] - ref[..., :4]).abs().max() / ref[..., :4].abs().max()).item(),
            (got[..., 4:] - ref[..., 4:]).abs().max().item())


NCS = [1, 3, 16, 17, 80]


def case_inputs(lset, nc, dt):
    levels, _ = LEVEL_SETS[lset]
    for n in (1, 3):
        for no_ld in (r8(64 + nc), r8(64 + nc) + 16):
            yield n, no_ld, make_levels(levels, n, nc, no_ld, DT[dt], 1000 * n + nc + no_ld)


@pytest.fixture(scope="module")
def decode_refs():
    """fp64 references of every case (computed once) and the kernel's bound: 4x the largest error of the
    fp32 CPU evaluation over all of them, capped."""
    refs, eb, ep = {}, 0.0, 0.0
    for lset, (_, strides) in LEVEL_SETS.items():
        for nc in NCS:
            for dt in DTS:
                for n, no_ld, lv in case_inputs(lset, nc, dt):
                    ref = ref_decode(lv, nc, strides, torch.float64)
                    b, p = errors(ref_decode(lv, nc, strides, torch.float32), ref)
                    refs[lset, nc, dt, n, no_ld] = (lv, ref)
                    eb, ep = max(eb, b), max(ep, p)
    assert 0 < eb and 0 < ep
    print(f"decode: fp32 CPU evaluation vs fp64: box {eb:.3g} prob {ep:.3g}")
    return refs, min(4 * eb, BOX_CAP), min(4 * ep, PROB_CAP)


def run_decode(lv, nc, levels, strides, no_ld, dt, fused=False, conf=0.0):
    n = lv[0].shape[0]
    A = sum(h * w for h, w in levels)
    dev = [t.cuda() for t in lv]
    ptrs = (ctypes.c_void_p * len(dev))(*[t.data_ptr() for t in dev])
    hs = (ctypes.c_int * len(dev))(*[h for h, _ in levels])
    ws = (ctypes.c_int * len(dev))(*[w for _, w in levels])
    st = (ctypes.c_float * len(dev))(*strides)
    flat = torch.full((n * A * (4 + nc) + 64,), float("nan"), device="cuda")
    bxy = sc = lb = None
    if fused:
        bxy = torch.full((n * A * 4 + 16,), float("nan"), device="cuda")
        sc = torch.full((n * A + 16,), float("nan"), device="cuda")
        lb = torch.full((n * A + 16,), -7, dtype=torch.int32, device="cuda")
    L.call("yms_head_decode", L.dtype_code(DT[dt]), n, nc, len(dev), ptrs, hs, ws, no_ld, st, flat.data_ptr(),
           ctypes.c_float(conf), L.ptr(bxy), L.ptr(sc), L.ptr(lb), L.stream_ptr())
    torch.cuda.synchronize()
    assert torch.isnan(flat[n * A * (4 + nc):]).all()
    out = flat[:n * A * (4 + nc)].view(n, A, 4 + nc)
    if not fused:
        return out
    assert torch.isnan(bxy[n * A * 4:]).all() and torch.isnan(sc[n * A:]).all() and (lb[n * A:] == -7).all()
    return out, bxy[:n * A * 4].view(n, A, 4), sc[:n * A].view(n, A), lb[:n * A].view(n, A)


def run_prep(out, nc, conf):
    n, A = out.shape[:2]
    bxy = torch.full((n, A, 4), float("nan"), device="cuda")
    sc = torch.full((n, A), float("nan"), device="cuda")
    lb = torch.full((n, A), -7, dtype=torch.int32, device="cuda")
    L.call("yms_nms_prep", n, A, nc, out.data_ptr(), ctypes.c_float(conf), bxy.data_ptr(), sc.data_ptr(),
           lb.data_ptr(), L.stream_ptr())
    torch.cuda.synchronize()
    return bxy, sc, lb


def first_max_label(p):
    """smallest index among the maxima (not argmax, whose tie rule is unspecified)"""
    nc = p.shape[-1]
    idx = torch.arange(nc, device=p.device).expand_as(p)
    return torch.where(p == p.max(-1, keepdim=True).values, idx, torch.full_like(idx, 1 << 30)).min(-1).values


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("nc", NCS)
@pytest.mark.parametrize("lset", sorted(LEVEL_SETS))
def test_head_decode_matches_fp64(lset, nc, dt, decode_refs):
    """Boxes and probabilities against fp64 within 4x the fp32 CPU evaluation's error (module
    docstring); batch 1 and 3, a tight no_ld and one 16 wider, the padding channels NaN and the whole
    output finite.  Then the fused NMS prep: `out` bit-identical to the plain call, the three fused
    outputs bit-identical to yms_nms_prep on that `out`, the label the smallest index among the
    maxima, and with conf set to a score that occurs (the median), label == -1 exactly where
    score <= conf."""
    levels, strides = LEVEL_SETS[lset]
    refs, bb, bp = decode_refs
    for n in (1, 3):
        for no_ld in (r8(64 + nc), r8(64 + nc) + 16):
            lv, ref = refs[lset, nc, dt, n, no_ld]
            out = run_decode(lv, nc, levels, strides, no_ld, dt)
            assert torch.isfinite(out).all()
            eb, ep = errors(out.cpu(), ref)
            print(f"decode {lset} nc={nc} {dt} n={n} no_ld={no_ld}: kernel box {eb:.3g} prob {ep:.3g}")
            assert eb <= bb and ep <= bp, (n, no_ld, eb, bb, ep, bp)
            # fused prep
            conf = out[..., 4:].max(-1).values.median().item()
            for cf in (0.25, conf):
                o2, bxy, sc, lb = run_decode(lv, nc, levels, strides, no_ld, dt, fused=True, conf=cf)
                assert torch.equal(bits(o2), bits(out))
                pb, ps, pl = run_prep(out, nc, cf)
                assert torch.equal(bits(bxy), bits(pb)) and torch.equal(bits(sc), bits(ps)) and torch.equal(lb, pl)
                p = out[..., 4:]
                assert torch.equal(sc, p.max(-1).values)
                want = torch.where(sc > cf, first_max_label(p), torch.full_like(lb, -1).long())
                assert torch.equal(lb.long(), want)
            assert (sc == conf).any() and ((lb == -1) == (sc <= conf)).all()
            if nc > 1:
                assert (lb >= 0).any() and (lb == -1).any()


def test_head_decode_grid_stride(decode_refs):
    """33 images x (80^2 + 40^2 + 20^2) = 277,200 anchors, nc = 1, bf16: above the 16,384 blocks x 16
    anchors of one grid pass.  Random logits drawn on the device, and the fp64 reference evaluated
    there (only this case: the host would need seconds); the same bound as the small cases."""
    _, bb, bp = decode_refs
    levels, strides, n, nc, no_ld = [(80, 80), (40, 40), (20, 20)], [8.0, 16.0, 32.0], 33, 1, 72
    g = torch.Generator(device="cuda").manual_seed(5)
    lv = []
    for h, w in levels:
        t = torch.randn(n, h, w, no_ld, generator=g, device="cuda") * 3
        t[..., 64 + nc:] = float("nan")
        lv.append(t.to(torch.bfloat16))
    with torch.device("cuda"):
        ref = ref_decode(lv, nc, strides, torch.float64)
    out, bxy, sc, lb = run_decode(lv, nc, levels, strides, no_ld, "bf16", fused=True, conf=0.5)
    assert torch.isfinite(out).all()
    eb, ep = errors(out, ref)
    print(f"decode grid-stride: kernel box {eb:.3g} prob {ep:.3g}")
    assert eb <= bb and ep <= bp, (eb, bb, ep, bp)
    pb, ps, pl = run_prep(out, nc, 0.5)
    assert torch.equal(bits(bxy), bits(pb)) and torch.equal(bits(sc), bits(ps)) and torch.equal(lb, pl)
    assert torch.equal(lb.long(), torch.where(sc > 0.5, 0, -1))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("ch", [1, 8, 16, 17])
def test_dfl_matches_fp64(ch, dt):
    """Standalone DFL integral x [n][4 ch][A] -> [n][4][A] = sum_j j softmax_j against fp64 on the
    rounded inputs, logits up to +-100 (exp overflows without the max subtraction), A of 1, 255
    (one block minus a thread) and 8400, batch 1 and 3.  fp32 within the project's 1e-5; a 16-bit
    output within one rounding step of its dtype (2^-8 relative bf16, 2^-11 f16) on top of that.
    1e-5 is relative to the largest |reference| value, as the golden DFL test measures it (ch = 1: the
    expectation is 0 and must come out as 0)."""
    dtype = DT[dt]
    step = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11, "f32": 0.0}[dt]
    for n in (1, 3):
        for A in (1, 255, 8400):
            g = torch.Generator().manual_seed(ch * 100 + A + n)
            x = torch.randn(n, 4 * ch, A, generator=g) * 3
            x[:, :, ::3] = torch.randint(-100, 101, x[:, :, ::3].shape, generator=g).float()
            x = x.to(dtype)
            ref = (x.double().view(n, 4, ch, A).softmax(2) * torch.arange(ch, dtype=torch.float64).view(1, 1, ch, 1)).sum(2)
            xd = x.cuda()
            flat = torch.full((n * 4 * A + 64,), float("nan"), dtype=dtype, device="cuda")
            L.call("yms_dfl", L.dtype_code(dtype), n, A, ch, xd.data_ptr(), flat.data_ptr(), L.stream_ptr())
            torch.cuda.synchronize()
            assert torch.isnan(flat[n * 4 * A:]).all()
            got = flat[:n * 4 * A].view(n, 4, A).double().cpu()
            assert torch.isfinite(got).all()
            err = ((got - ref).abs() - step * ref.abs()).max().item()
            assert err <= 1e-5 * ref.abs().max().item(), (n, A, err)
