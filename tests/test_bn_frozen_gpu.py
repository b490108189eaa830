"""yms_bn_frozen_act_bwd (the one-pass backward of BN with running statistics + act) and yms_bn_fold_mi
through the C-ABI, against fp64 of the formulas on the dtype-rounded inputs:

    da = gy * act'(z*scale + shift),  dz = scale * da,  gres = gy | gres + gy,
    dbeta = sum da,  dgamma = sum da * (z - running_mean) * invstd.

Every buffer is a channel slice [off, off + c) of rows ld wide whose other columns hold a sentinel that
must survive; the partial-row scratch is NaN beyond yms_bn_bwd_rows rows."""
import ctypes
import itertools

import pytest
import torch

from yms import _lib as L

pytestmark = pytest.mark.gpu

SHAPES = [(1, 16, 16, 0), (100, 16, 16, 0), (999, 20, 32, 8), (999, 3, 8, 0), (3001, 40, 48, 0),
          (44801, 64, 64, 0), (25600, 768, 776, 8), (3000, 1152, 1152, 0)]
DTYPES = {"bf16": (torch.bfloat16, L.BF16, 1e-2), "f16": (torch.float16, L.F16, 1e-2), "f32": (torch.float32, L.F32, 1e-5)}
PAD = 7.0


def _slice(t, c, off):
    return t[:, off:off + c]


def _buf(vals, ld, off, dtype):
    """[npix, ld] of the sentinel with vals in columns [off, off + c)."""
    b = torch.full((vals.shape[0], ld), PAD, dtype=dtype, device="cuda")
    b[:, off:off + vals.shape[1]] = vals.to(dtype)
    return b


def _pads_intact(b, c, off):
    return bool((b[:, :off] == PAD).all() and (b[:, off + c:] == PAD).all())


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("npix,c,ld,off", SHAPES)
def test_frozen_bwd_matches_fp64(npix, c, ld, off, dt):
    dtype, code, tol = DTYPES[dt]
    g = torch.Generator().manual_seed(npix + c)
    z0 = _buf(torch.randn(npix, c, generator=g), ld, off, dtype)
    gy = _buf(torch.randn(npix, c, generator=g), ld, off, dtype)
    r0 = _buf(torch.randn(npix, c, generator=g), ld, off, dtype)
    sc = (torch.rand(c, generator=g) + 0.5).cuda()
    sh = (torch.randn(c, generator=g) * 0.2).cuda()
    mi = torch.stack([torch.randn(c, generator=g) * 0.3, torch.rand(c, generator=g) + 0.5]).cuda().contiguous()
    zf, gf, rf = (_slice(t, c, off).double() for t in (z0, gy, r0))
    rows = L.lib().yms_bn_bwd_rows(npix, c)
    st = L.stream_ptr()
    for act in (L.ACT_SILU, L.ACT_NONE):
        # the fp64 reference, once per activation
        a = zf * sc.double() + sh.double()
        s = torch.sigmoid(a)
        da = gf * (s * (1 + a * (1 - s))) if act == L.ACT_SILU else gf
        ref_dz = sc.double() * da
        ref_db = da.sum(0)
        ref_dg = (da * (zf - mi[0].double()) * mi[1].double()).sum(0)
        for res, inplace, (want_dg, want_db) in itertools.product(
                (None, "store", "acc"), (False, True), ((1, 1), (1, 0), (0, 1), (0, 0))):
            z = z0.clone()
            out = z if inplace else torch.full_like(z0, PAD)
            gres = None if res is None else r0.clone()
            sums = want_dg or want_db
            ws = torch.full((rows + 16, 2, c), float("nan"), device="cuda")
            cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
            dg = [torch.full((c,), float("nan"), device="cuda") for _ in range(2)]
            db = [torch.full((c,), float("nan"), device="cuda") for _ in range(2)]
            for k in range(2 if sums else 1):        # twice: the counter is reusable, the sums bit-equal
                if k:
                    z.copy_(z0)
                    if gres is not None:
                        gres.copy_(r0)
                L.call("yms_bn_frozen_act_bwd", code, npix, c, z.data_ptr(), ld, off, gy.data_ptr(), ld, off,
                       sc.data_ptr(), sh.data_ptr(), mi.data_ptr() if sums else None, act, out.data_ptr(), ld, off,
                       L.ptr(gres), ld if gres is not None else 0, off if gres is not None else 0, int(res == "acc"),
                       ws.data_ptr() if sums else None, cnt.data_ptr() if sums else None,
                       dg[k].data_ptr() if want_dg else None, db[k].data_ptr() if want_db else None, st)
            torch.cuda.synchronize()
            what = (act, res, inplace, want_dg, want_db)
            err = (_slice(out, c, off).double() - ref_dz).abs().max().item()
            assert err <= tol * (1 + ref_dz.abs().max().item()), (what, err)
            assert _pads_intact(out, c, off), what
            if not inplace:
                assert torch.equal(z, z0), what
            if gres is not None:
                ref_r = (rf + gf) if res == "acc" else gf
                err = (_slice(gres, c, off).double() - ref_r).abs().max().item()
                assert err <= tol * (1 + ref_r.abs().max().item()), (what, err)
                assert _pads_intact(gres, c, off), what
            for want, got, ref in ((want_dg, dg, ref_dg), (want_db, db, ref_db)):
                if want:
                    rel = ((got[0].double() - ref).norm() / ref.norm()).item()
                    assert rel < 1e-5, (what, rel)
                    assert torch.equal(got[0], got[1]), what
                else:
                    assert torch.isnan(got[0]).all(), what
            assert int(cnt[0]) == 0, what
            if sums:
                assert torch.isnan(ws[rows:]).all() and torch.isfinite(ws[:rows]).all(), what
            else:
                assert torch.isnan(ws).all(), what


def test_rejects_bad_jobs():
    """Validated before any launch: sums without mean_invstd / ws / counter, a slice past its row."""
    z = torch.zeros(8, 16, device="cuda")
    v = torch.zeros(32, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    p, vp = z.data_ptr(), v.data_ptr()

    def status(c=16, off=0, mi=vp, ws=vp, counter=cnt.data_ptr()):
        return L.lib().yms_bn_frozen_act_bwd(L.F32, 8, c, p, 16, off, p, 16, 0, vp, vp, mi, L.ACT_SILU, p, 16, 0,
                                             None, 0, 0, 0, ws, counter, vp, vp, L.stream_ptr())

    assert status() == 0
    for bad in (dict(mi=None), dict(ws=None), dict(counter=None), dict(off=8), dict(c=0)):
        assert status(**bad) != 0, bad
    torch.cuda.synchronize()


@pytest.mark.parametrize("c,mi_ld,off", [(3, 8, 0), (64, 64, 0), (80, 144, 64), (1152, 1152, 0)])
def test_fold_mi_matches_fp64_and_bn_fold(c, mi_ld, off):
    """scale / shift are yms_bn_fold's bits; (running_mean, invstd) land in the channel slice [off, off + c)
    of a [2][mi_ld] table whose other entries stay; the batched form gives the solo call's bits."""
    g = torch.Generator().manual_seed(c)
    gam, bet, rm = (torch.randn(c, generator=g).cuda() for _ in range(3))
    rv = (torch.rand(c, generator=g) * 3 + 0.01).cuda()
    eps = 1e-3
    st = L.stream_ptr()
    sc0, sh0 = torch.empty(c, device="cuda"), torch.empty(c, device="cuda")
    L.call("yms_bn_fold", c, gam.data_ptr(), bet.data_ptr(), rm.data_ptr(), rv.data_ptr(), ctypes.c_float(eps),
           sc0.data_ptr(), sh0.data_ptr(), st)
    # one arena for both forms: [scale | shift | table] solo, then the same again batched
    arena = torch.full((2, 2 * c + 2 * mi_ld), PAD, device="cuda")
    o_sc, o_sh, o_mi = 0, 4 * c, 4 * (2 * c + off)
    base = arena[0].data_ptr()
    L.call("yms_bn_fold_mi", c, gam.data_ptr(), bet.data_ptr(), rm.data_ptr(), rv.data_ptr(), ctypes.c_float(eps),
           base + o_sc, base + o_sh, base + o_mi, mi_ld, st)
    job = L.BnFoldJob(gam.data_ptr(), bet.data_ptr(), rm.data_ptr(), rv.data_ptr(), eps, c, mi_ld, o_sc, o_sh, o_mi)
    table = torch.frombuffer(bytearray(bytes(job)), dtype=torch.uint8).cuda()
    L.call("yms_bn_fold_mi_batched", 1, table.data_ptr(), c, arena[1].data_ptr(), st)
    torch.cuda.synchronize()
    assert torch.equal(arena[0], arena[1])
    sc, sh, mi = arena[0][:c], arena[0][c:2 * c], arena[0][2 * c:].view(2, mi_ld)
    assert torch.equal(sc, sc0) and torch.equal(sh, sh0)
    assert torch.equal(mi[0, off:off + c], rm)
    ref = 1.0 / (rv.double() + eps).sqrt()
    assert ((mi[1, off:off + c].double() - ref).abs() / ref).max().item() < 1e-6
    keep = torch.ones(mi_ld, dtype=torch.bool, device="cuda")
    keep[off:off + c] = False
    assert (mi[:, keep] == PAD).all()
