"""Grouped entry points (yms_*_group) against the same jobs as solo calls, through the C-ABI: a grouped
launch decomposes every member exactly as its solo call does, so outputs, statistics rows (counts
included), partial rows, dgamma / dbeta / coef and running statistics must be EQUAL bit for bit.

Members are the head's three levels in small: B = 3 on 16x16 / 8x8 / 4x4 maps = 768 rows (several
128-row tiles), 192 (a ragged last tile) and 48 (less than one tile).  cout 80 has 10 16-byte chunks
per tap (the per-lane loader, not the scalar-tap one); c = 67 takes the c % 8 != 0 serial loops."""
import ctypes

import pytest
import torch

from hiputil import DT, nhwc, pack, r8, shape, stats_buffer
from yms import _lib as L

pytestmark = pytest.mark.gpu

B, MAPS = 3, (16, 8, 4)


def _arr(jobs):
    return (type(jobs[0]) * len(jobs))(*jobs)


def _bits(t):
    """Integer view, so that NaN fill patterns compare equal."""
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def _same(a, b):
    assert len(a) == len(b)
    for i, (u, v) in enumerate(zip(a, b)):
        assert torch.equal(_bits(u), _bits(v)), f"output {i} differs between the grouped and the solo calls"


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- convolution forward -------------------------------------------------------------------
class FwdCase:
    """One conv per (hw, cin, cout, k) spec, all inputs built once; run() writes fresh outputs."""

    def __init__(self, specs, dt, stats, res=False, bias=False):
        self.dtype, self.stats = DT[dt], stats
        g = _gen(len(specs) * 131 + sum(s[1] + s[2] for s in specs))
        self.m = []
        for hw, cin, cout, k in specs:
            sh = shape(B, hw, hw, cin, cout, k, 1, self.dtype)
            x = nhwc(torch.randn(B, cin, hw, hw, generator=g), self.dtype)
            wp = pack(torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5, sh, self.dtype, 0)
            sc = None if (stats or bias) else (torch.rand(cout, generator=g) + 0.5).cuda()
            shf = None if stats else (torch.randn(cout, generator=g) * 0.1).cuda()
            r = nhwc(torch.randn(B, cout, hw, hw, generator=g), self.dtype) if res else None
            self.m.append((sh, x, wp, sc, shf, r))

    def jobs(self):
        outs, jobs = [], []
        for sh, x, wp, sc, shf, r in self.m:
            y = torch.full((B, sh.ho, sh.wo, r8(sh.cout)), 7.0, dtype=self.dtype, device="cuda")
            outs.append(y)
            st = None
            if self.stats:
                sp = ctypes.pointer(sh)
                st = stats_buffer(L.lib().yms_conv_stats_rows(sp), L.lib().yms_conv_stats_ld(sp))
                outs.append(st)
            act = L.ACT_NONE if (self.stats or sc is None) else L.ACT_SILU
            jobs.append(L.ConvFwdJob(sh, x.data_ptr(), x.shape[-1], 0, wp.data_ptr(), y.data_ptr(), y.shape[-1], 0,
                                     L.ptr(sc), L.ptr(shf), act, L.ptr(r), r.shape[-1] if r is not None else 0, 0,
                                     L.ptr(st)))
        return jobs, outs

    def run(self, grouped):
        jobs, outs = self.jobs()
        if grouped:
            L.call("yms_conv_fwd_group", len(jobs), _arr(jobs), L.stream_ptr())
        else:
            for j in jobs:
                L.call_job("yms_conv_fwd", j, L.stream_ptr())
        torch.cuda.synchronize()
        return outs

    def launches(self):
        jobs, _ = self.jobs()
        return L.lib().yms_conv_fwd_group_launches(len(jobs), _arr(jobs))

    def check(self):
        solo = self.run(False)
        _same(self.run(True), solo)
        return solo


CONVS = [(32, 64, 3), (64, 80, 3), (128, 64, 3), (128, 80, 3), (64, 64, 1), (80, 80, 1)]


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("cin,cout,k", CONVS)
def test_conv_fwd_group_equals_solo(cin, cout, k, dt):
    specs = [(hw, cin, cout, k) for hw in MAPS]
    for stats, res, bias in ((True, False, False), (False, True, False), (False, False, False), (False, False, True)):
        case = FwdCase(specs, dt, stats, res, bias)
        outs = case.check()
        assert all(torch.isfinite(o.float()).all() for o in outs[::2 if stats else 1])   # every y fully written
        n = case.launches()
        if dt == "f32":
            assert n == 3                   # fp32 runs conv_nt_kernel: the solo fallback, one call per job
        elif k == 3 and cin <= 64 and cout == 64:
            assert n == 2                   # the 16x16 member takes the direct 3x3 kernel: solo + one group of two
        else:
            assert n == 1


def test_conv_fwd_group_sizes_and_mixed_keys():
    one = FwdCase([(8, 128, 80, 3)], "bf16", True)
    one.check()
    assert one.launches() == 1
    two = FwdCase([(16, 128, 80, 3), (4, 64, 80, 3)], "bf16", True)
    two.check()
    assert two.launches() == 1
    # cout 64 (128 x 64 tiles) and cout 80 (128 x 128 tiles) are two kernel variants: two launches
    mixed = FwdCase([(16, 128, 64, 3), (16, 128, 80, 3), (4, 128, 64, 3), (8, 128, 80, 3)], "bf16", True)
    mixed.check()
    assert mixed.launches() == 2
    # ... and a variant with one member runs that member solo
    odd = FwdCase([(16, 128, 64, 3), (8, 128, 80, 3), (4, 128, 80, 3)], "bf16", False)
    odd.check()
    assert odd.launches() == 2
    # five members of one variant: four in one launch, the fifth solo
    five = FwdCase([(hw, 128, 80, 3) for hw in (16, 8, 4, 8, 4)], "bf16", True)
    five.check()
    assert five.launches() == 2


# ---- input gradient ------------------------------------------------------------------------
class DgradCase:
    def __init__(self, specs, dt):
        self.dtype = DT[dt]
        g = _gen(17 + sum(s[1] + s[2] for s in specs))
        self.m = []
        for hw, cin, cout, k in specs:
            sh = shape(B, hw, hw, cin, cout, k, 1, self.dtype)
            dz = nhwc(torch.randn(B, cout, hw, hw, generator=g), self.dtype)     # padding channels zero
            wpt = pack(torch.randn(cout, cin, k, k, generator=g) / (cout * k * k) ** 0.5, sh, self.dtype, 1)
            dx0 = nhwc(torch.randn(B, cin, hw, hw, generator=g), self.dtype)
            self.m.append((sh, dz, wpt, dx0))

    def jobs(self, acc):
        outs = [dx0.clone() for _, _, _, dx0 in self.m]
        jobs = [L.ConvDgradJob(sh, dz.data_ptr(), dz.shape[-1], 0, wpt.data_ptr(), dx.data_ptr(), dx.shape[-1], 0, acc)
                for (sh, dz, wpt, _), dx in zip(self.m, outs)]
        return jobs, outs

    def run(self, grouped, acc):
        jobs, outs = self.jobs(acc)
        if grouped:
            L.call("yms_conv_dgrad_group", len(jobs), _arr(jobs), L.stream_ptr())
        else:
            for j in jobs:
                L.call_job("yms_conv_dgrad", j, L.stream_ptr())
        torch.cuda.synchronize()
        return outs

    def launches(self):
        jobs, _ = self.jobs(0)
        return L.lib().yms_conv_dgrad_group_launches(len(jobs), _arr(jobs))


# (128, 67, 3): the sibling pair's input gradient, K = 9 * (64 + 3) over a dz with zero padding channels
@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("cin,cout,k", CONVS + [(128, 67, 3), (64, 144, 3)])
def test_conv_dgrad_group_equals_solo(cin, cout, k, dt):
    case = DgradCase([(hw, cin, cout, k) for hw in MAPS], dt)
    for acc in (0, 1):
        solo = case.run(False, acc)
        _same(case.run(True, acc), solo)
        assert all(torch.isfinite(o.float()).all() for o in solo)
    n = case.launches()
    if dt == "f32":
        assert n == 3
    elif cin <= 32:
        assert n == 3                       # dx of <= 32 channels: the 256 x 32 tile variant is not grouped
    elif k == 3 and cout <= 64 and cin <= 64:
        assert n == 2                       # 16x16: the direct 3x3 input-gradient kernel
    else:
        assert n == 1


def test_conv_dgrad_group_sizes_and_mixed_keys():
    for specs, n in (([(8, 128, 80, 3)], 1), ([(16, 128, 80, 3), (4, 128, 67, 3)], 1),
                     ([(16, 64, 80, 3), (16, 128, 80, 3), (8, 64, 80, 3), (4, 128, 80, 3)], 2)):
        case = DgradCase(specs, "bf16")
        _same(case.run(True, 0), case.run(False, 0))
        assert case.launches() == n


# ---- BN family -----------------------------------------------------------------------------
NPIX = tuple(B * hw * hw for hw in MAPS)
CHANS = [(64, 64, 64), (80, 80, 80), (67, 67, 67), (64, 80, 67)]


def _act_buf(npix, c, dtype, g, fill=None):
    t = torch.zeros(npix, r8(c), dtype=dtype, device="cuda")
    t[:, :c] = (torch.randn(npix, c, generator=g) if fill is None else torch.full((npix, c), fill)).to(dtype)
    return t


@pytest.mark.parametrize("cs", CHANS)
def test_bn_finalize_group_equals_solo(cs):
    g = _gen(sum(cs))
    rows_of = (5, 2, 1)
    tabs = []
    for c, rows, npix in zip(cs, rows_of, NPIX):
        ld = 128
        st = torch.randn(rows * (2 * ld + 1), generator=g)
        st[rows * ld * 2:] = npix / rows                       # counts
        st[:rows * 2 * ld].view(rows, 2, ld)[:, 1].abs_()
        tabs.append((c, rows, ld, npix, st.cuda(), torch.rand(c, generator=g).cuda(), torch.randn(c, generator=g).cuda()))

    def run(grouped):
        outs, jobs = [], []
        for c, rows, ld, npix, st, gam, bet in tabs:
            rm, rv = torch.zeros(c, device="cuda"), torch.ones(c, device="cuda")
            mi = torch.full((2, c + 8), float("nan"), device="cuda")
            sc, sh = torch.empty(c, device="cuda"), torch.empty(c, device="cuda")
            stc = st.clone()
            outs += [rm, rv, mi, sc, sh, stc]
            jobs.append(L.BnFinalizeJob(c, stc.data_ptr(), rows, ld, npix, gam.data_ptr(), bet.data_ptr(), rm.data_ptr(),
                                        rv.data_ptr(), 0.03, 1e-3, mi.data_ptr(), c + 8, sc.data_ptr(), sh.data_ptr()))
        if grouped:
            L.call("yms_bn_finalize_group", len(jobs), _arr(jobs), L.stream_ptr())
        else:
            for j in jobs:
                L.call_job("yms_bn_finalize_ld", j, L.stream_ptr())
        torch.cuda.synchronize()
        return outs

    solo = run(False)
    _same(run(True), solo)
    assert all(torch.isfinite(o).all() for o in solo[3::6])       # scale


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("cs", CHANS)
def test_bn_pass_groups_equal_solo(cs, dt):
    """affine (residual on / off), then the backward chain reduce -> finalize -> apply (gres off /
    store / accumulate) and the bias reduce, each pass grouped against solo on the same inputs."""
    dtype, code = DT[dt], L.dtype_code(DT[dt])
    g = _gen(sum(cs) + 5)
    st = L.stream_ptr()
    mem = []
    for c, npix in zip(cs, NPIX):
        mem.append(dict(c=c, npix=npix, ld=r8(c), z=_act_buf(npix, c, dtype, g), gy=_act_buf(npix, c, dtype, g),
                        res=_act_buf(npix, c, dtype, g), sc=(torch.rand(c, generator=g) + 0.5).cuda(),
                        sh=(torch.randn(c, generator=g) * 0.2).cuda(),
                        mi=torch.cat([torch.randn(c, generator=g) * 0.1, torch.rand(c, generator=g) + 0.5]).cuda(),
                        rows=L.lib().yms_bn_bwd_rows(npix, c)))

    def affine(grouped, with_res):
        outs, jobs = [], []
        for m in mem:
            y = torch.full_like(m["z"], 7.0)
            outs.append(y)
            jobs.append(L.BnPassJob(npix=m["npix"], c=m["c"], z=m["z"].data_ptr(), z_ld=m["ld"], scale=m["sc"].data_ptr(),
                                    shift=m["sh"].data_ptr(), act=L.ACT_SILU, out=y.data_ptr(), out_ld=m["ld"],
                                    res=m["res"].data_ptr() if with_res else None, res_ld=m["ld"] if with_res else 0))
        if grouped:
            L.call("yms_affine_act_group", code, len(jobs), _arr(jobs), st)
        else:
            for j in jobs:
                L.call_job("yms_affine_act", j, st, code)
        torch.cuda.synchronize()
        return outs

    for with_res in (False, True):
        _same(affine(True, with_res), affine(False, with_res))

    def backward(grouped, gres_mode):
        outs, red, fin, app = [], [], [], []
        for m in mem:
            c, npix, ld = m["c"], m["npix"], m["ld"]
            ws = torch.full((m["rows"] + 4, 2, c), float("nan"), device="cuda")
            dg, db, coef = (torch.empty(c, device="cuda"), torch.empty(c, device="cuda"), torch.empty(2 * c, device="cuda"))
            dz = torch.full_like(m["z"], 7.0)
            gres = m["res"].clone()
            outs += [ws, dg, db, coef, dz, gres]
            common = dict(npix=npix, c=c, z=m["z"].data_ptr(), z_ld=ld, gy=m["gy"].data_ptr(), gy_ld=ld,
                          scale=m["sc"].data_ptr(), shift=m["sh"].data_ptr(), mean_invstd=m["mi"].data_ptr(),
                          act=L.ACT_SILU)
            red.append(L.BnPassJob(ws=ws.data_ptr(), **common))
            fin.append(L.BnBwdFinalizeJob(c, ws.data_ptr(), m["rows"], npix, dg.data_ptr(), db.data_ptr(), coef.data_ptr()))
            app.append(L.BnPassJob(coef=coef.data_ptr(), out=dz.data_ptr(), out_ld=ld,
                                   res=gres.data_ptr() if gres_mode else None, res_ld=ld if gres_mode else 0,
                                   res_acc=int(gres_mode == 2), **common))
        if grouped:
            L.call("yms_bn_act_bwd_reduce_group", code, len(red), _arr(red), st)
            L.call("yms_bn_act_bwd_finalize_group", len(fin), _arr(fin), st)
            L.call("yms_bn_act_bwd_apply_group", code, len(app), _arr(app), st)
        else:
            for j in red:
                L.call_job("yms_bn_act_bwd_reduce", j, st, code)
            for j in fin:
                L.call_job("yms_bn_act_bwd_finalize", j, st)
            for j in app:
                L.call_job("yms_bn_act_bwd_apply", j, st, code)
        torch.cuda.synchronize()
        return outs

    for gres_mode in (0, 1, 2):
        solo = backward(False, gres_mode)
        _same(backward(True, gres_mode), solo)
        for m, ws in zip(mem, solo[::6]):
            assert torch.isfinite(ws[:m["rows"]]).all() and torch.isnan(ws[m["rows"]:]).all()

    def bias(grouped):
        outs, jobs = [], []
        cnt = torch.zeros(4 * len(mem), dtype=torch.int32, device="cuda")
        for i, m in enumerate(mem):
            ws = torch.full((m["rows"] + 4, 2, m["c"]), float("nan"), device="cuda")
            db = torch.empty(m["c"], device="cuda")
            outs += [ws, db]
            jobs.append(L.BnPassJob(npix=m["npix"], c=m["c"], gy=m["gy"].data_ptr(), gy_ld=m["ld"], ws=ws.data_ptr(),
                                    counter=cnt.data_ptr() + 16 * i, dbias=db.data_ptr()))
        if grouped:
            L.call("yms_bias_bwd_group", code, len(jobs), _arr(jobs), st)
        else:
            for j in jobs:
                L.call_job("yms_bias_bwd", j, st, code)
        torch.cuda.synchronize()
        assert int(cnt.abs().sum()) == 0          # every member's arrival counter is back at zero
        return outs

    solo = bias(False)
    _same(bias(True), solo)
    for m, db in zip(mem, solo[1::2]):
        ref = m["gy"][:, :m["c"]].double().sum(0)
        assert ((db.double() - ref).abs().max() <= 1e-3 * (ref.abs().max() + 1)).item()


def test_bn_group_sizes():
    """One job (the solo call), two, and nine (eight in one launch and one solo)."""
    g = _gen(3)
    for n in (1, 2, 9):
        zs = [_act_buf(48 + 16 * i, 64, torch.bfloat16, g) for i in range(n)]
        sc, sh = torch.rand(64, generator=g).cuda(), torch.randn(64, generator=g).cuda()
        res = []
        for grouped in (True, False):
            ys = [torch.full_like(z, 7.0) for z in zs]
            jobs = [L.BnPassJob(npix=z.shape[0], c=64, z=z.data_ptr(), z_ld=64, scale=sc.data_ptr(), shift=sh.data_ptr(),
                                act=L.ACT_SILU, out=y.data_ptr(), out_ld=64) for z, y in zip(zs, ys)]
            if grouped:
                L.call("yms_affine_act_group", L.BF16, n, _arr(jobs), L.stream_ptr())
            else:
                for j in jobs:
                    L.call_job("yms_affine_act", j, L.stream_ptr(), L.BF16)
            torch.cuda.synchronize()
            res.append(ys)
        _same(*res)
        assert all(torch.isfinite(y.float()).all() and (y != 7.0).any() for y in res[0])
