"""The persistent kernels' tile walks at small shapes: with the CU count overridden (yms_cu_count_set) a
block of the implicit-GEMM forward, the direct 3x3 kernels, the depthwise strip / MFMA kernels and the
split-K weight gradients owns several tiles, which on a full device happens only at bench size.  The cases
and the proof that they walk are in tile_walk_cases.py / test_tile_walk_cpu.py.

Every case runs under the device's own count and under each override, against the reference and tolerance of
the kernel's own test file (fp32 torch on dtype-rounded operands; fp64 for the depthwise kernels and the
weight gradients).  Where the arithmetic of an output element does not depend on which block computes its
tile -- forward outputs, input gradients, eval outputs end to end -- the result under an override must equal
the default-grid result bit for bit.  Where the grid changes the order of a sum -- merged BN moments, split-K
weight gradients, BN-reduce partial rows -- there is no bit identity, and the reference tolerance holds.

Outputs and workspaces are prefilled with NaN, the slack around a channel slice with a guard value that must
survive, padding channels with the zeros that must stay."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import tile_walk_cases as T
from hiputil import DT, check_moments, nchw, nhwc, pack, r8, ref_conv, shape, split_stats, stats_buffer
from tile_walk_cases import cu_count  # noqa: F401  (fixture)
from test_conv_gpu import TOL, _close                     # 1e-2 / 2e-3 of max|ref| (bf16 / f16); dgrad twice that
from yms import _lib as L

pytestmark = pytest.mark.gpu
GUARD = 3.0
DEV = "cuda"


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def _same_bits(a, b, what):
    assert torch.equal(_bits(a), _bits(b)), f"{what}: differs from the default-grid result"


def out_buf(n, h, w, c, dtype, ld, off, body=None):
    """[n, h, w, ld] with the guard value outside [off, off + r8(c)), zeros in the padding channels and NaN (or
    body, NCHW fp32) in the c channels"""
    y = torch.full((n, h, w, ld), GUARD, dtype=dtype, device=DEV)
    y[..., off:off + r8(c)] = 0
    y[..., off:off + c] = float("nan") if body is None else body.permute(0, 2, 3, 1).to(dtype).to(DEV)
    return y


def body_of(y, c, off):
    """the c channels (NCHW fp32, host) after checking slack and padding"""
    assert (y[..., :off] == GUARD).all() and (y[..., off + r8(c):] == GUARD).all(), "slack outside the slice written"
    assert (y[..., off + c:off + r8(c)] == 0).all(), "padding channels not zero"
    got = nchw(y, c, off).cpu()
    assert torch.isfinite(got).all(), "an output element was not written"
    return got


def conv_fwd(sh, xb, xoff, wp, y, yoff, sc=None, sf=None, act=0, res=None, roff=0, stats=None):
    L.call("yms_conv_fwd", ctypes.pointer(sh), xb.data_ptr(), xb.shape[-1], xoff, wp.data_ptr(), y.data_ptr(),
           y.shape[-1], yoff, L.ptr(sc), L.ptr(sf), act, L.ptr(res), res.shape[-1] if res is not None else 0, roff,
           L.ptr(stats), L.stream_ptr())


def fwd_three_epilogues(sh, x, wt, dt, seed):
    """-> run(): statistics | BN + SiLU + residual into a channel slice | plain affine, each checked against
    the fp32 reference; returns the raw output buffers for the bit comparison between grids"""
    dtype = DT[dt]
    n, cout, s = sh.n, sh.cout, sh.stride
    g = torch.Generator().manual_seed(seed)
    sc = torch.rand(cout, generator=g) + 0.5
    sf = torch.randn(cout, generator=g) * 0.1
    res = torch.randn(n, cout, sh.ho, sh.wo, generator=g)
    z = ref_conv(x, wt, s, dtype)
    aff = z * sc.view(1, -1, 1, 1) + sf.view(1, -1, 1, 1)
    full = F.silu(aff) + res.to(dtype).float()
    xb = nhwc(x, dtype, ld=r8(sh.cin) + 16, off=8)             # x in a channel slice as well
    rb = nhwc(res, dtype, ld=r8(cout) + 24, off=16)
    wp = pack(wt, sh, dtype, 0)
    scd, sfd = sc.to(DEV), sf.to(DEV)
    sp = ctypes.pointer(sh)

    def run():
        # statistics: pre-BN z, one moment row per block (and 128-row half), every row written, counts = pixels
        rows, ld = L.lib().yms_conv_stats_rows(sp), L.lib().yms_conv_stats_ld(sp)
        buf = stats_buffer(rows, ld)
        y0 = out_buf(n, sh.ho, sh.wo, cout, dtype, r8(cout), 0)
        conv_fwd(sh, xb, 8, wp, y0, 0, stats=buf)
        _close(body_of(y0, cout, 0), z, TOL[dt])
        check_moments(split_stats(buf, rows, ld), z, 1e-3)     # merged in another order per grid: tolerance only
        y1 = out_buf(n, sh.ho, sh.wo, cout, dtype, r8(cout) + 32, 8)
        conv_fwd(sh, xb, 8, wp, y1, 8, scd, sfd, L.ACT_SILU, rb, 16)
        _close(body_of(y1, cout, 8), full, TOL[dt])
        y2 = out_buf(n, sh.ho, sh.wo, cout, dtype, r8(cout), 0)
        conv_fwd(sh, xb, 8, wp, y2, 0, scd, sfd, L.ACT_NONE)
        _close(body_of(y2, cout, 0), aff, TOL[dt])
        return y0, y1, y2
    return run


def run_under(cu_count, overrides, run, names):
    base = run()
    for ov in overrides:
        cu_count(ov)
        for a, b, nm in zip(run(), base, names):
            _same_bits(a, b, f"{nm}, {ov} CUs")
    cu_count(0)


# ---- persistent implicit-GEMM forward -------------------------------------------------------------------
@pytest.mark.parametrize("dt", T.LOWP)
@pytest.mark.parametrize("case", T.NTP, ids=T.case_id)
def test_ntp_fwd_walk(case, dt, cu_count):
    n, cin, h, w, cout, k, s = case[:7]
    g = torch.Generator().manual_seed(sum(case))
    x = torch.randn(n, cin, h, w, generator=g) + 0.5          # non-zero mean: centred moments matter
    wt = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    sh = T.ntp_shape(case, dt)
    run_under(cu_count, T.OVERRIDES, fwd_three_epilogues(sh, x, wt, dt, 1 + sum(case)),
              ("statistics z", "BN + SiLU + residual", "affine"))


@pytest.mark.parametrize("dt", T.LOWP)
@pytest.mark.parametrize("cin,cout,k", T.GROUP_CONVS)
def test_ntp_group_equals_solo_walking(cin, cout, k, dt, cu_count):
    """members of 38 / 14 / 2 tiles in one grouped launch: bit-equal to the solo calls under every setting (the
    statistics rows included: a member's sub-grid is its solo grid), and the outputs bit-equal across settings"""
    import test_group_gpu as G
    assert G.B == 3
    specs = [(hw, cin, cout, k) for hw in T.GROUP_MAPS]
    for stats, res in ((True, False), (False, True), (False, False)):
        case = G.FwdCase(specs, dt, stats, res)
        assert case.launches() == 1
        base = case.check()
        for ov in T.OVERRIDES:
            cu_count(ov)
            solo = case.check()
            assert case.launches() == 1
            ys = slice(0, None, 2) if stats else slice(None)
            assert all(torch.isfinite(o.float()).all() for o in solo[ys])       # every y fully written
            for a, b in zip(solo[ys], base[ys]):
                _same_bits(a, b, f"member output, {ov} CUs")
        cu_count(0)


# ---- direct 3x3 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", T.LOWP)
@pytest.mark.parametrize("case", T.DIRECT, ids=T.case_id)
def test_direct_fwd_walk(case, dt, cu_count):
    n, cin, h, w, cout = case
    g = torch.Generator().manual_seed(sum(case))
    x = torch.randn(n, cin, h, w, generator=g) + 0.5
    wt = torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
    sh = shape(n, h, w, cin, cout, 3, 1, DT[dt])
    run_under(cu_count, T.OVERRIDES, fwd_three_epilogues(sh, x, wt, dt, 2 + sum(case)),
              ("statistics z", "BN + SiLU + residual", "affine"))


def dgrad_store_accumulate(sh, wt, dz, dt, seed):
    """-> run(): yms_conv_dgrad onto NaN (store) and onto a base (accumulate), dx a channel slice"""
    dtype = DT[dt]
    n, cin, h, w, s = sh.n, sh.cin, sh.h, sh.w, sh.stride
    xr = torch.zeros(n, cin, h, w, requires_grad=True)
    F.conv2d(xr, wt.to(dtype).float(), None, s, 1).backward(dz.to(dtype).float())
    base = torch.randn(n, cin, h, w, generator=torch.Generator().manual_seed(seed))
    wpt = pack(wt, sh, dtype, 1)
    dzb = nhwc(dz, dtype, ld=r8(sh.cout) + 8, off=0)
    sp = ctypes.pointer(sh)

    def run():
        outs = []
        for acc in (0, 1):
            dx = out_buf(n, h, w, cin, dtype, r8(cin) + 24, 8, base if acc else None)
            L.call("yms_conv_dgrad", sp, dzb.data_ptr(), dzb.shape[-1], 0, wpt.data_ptr(), dx.data_ptr(), dx.shape[-1], 8,
                   acc, L.stream_ptr())
            exp = xr.grad + (base.to(dtype).float() if acc else 0)
            _close(body_of(dx, cin, 8), exp, TOL[dt] * 2)
            outs.append(dx)
        return outs
    return run


@pytest.mark.parametrize("dt", T.LOWP)
@pytest.mark.parametrize("case", T.DIRECT, ids=T.case_id)
def test_direct_dgrad_walk(case, dt, cu_count):
    n, cred, h, w, cin = case          # the input gradient reduces over the conv's cout
    g = torch.Generator().manual_seed(11 + sum(case))
    wt = torch.randn(cred, cin, 3, 3, generator=g) / (cred * 9) ** 0.5
    dz = torch.randn(n, cred, h, w, generator=g)
    sh = shape(n, h, w, cin, cred, 3, 1, DT[dt])
    run_under(cu_count, T.OVERRIDES, dgrad_store_accumulate(sh, wt, dz, dt, 5 + sum(case)), ("dx store", "dx accumulate"))


@pytest.mark.parametrize("dt", T.LOWP)
@pytest.mark.parametrize("case", T.DIRECT_S2, ids=T.case_id)
def test_direct_dgrad_stride2_walk(case, dt, cu_count):
    n, cin, h, w, cout = case
    g = torch.Generator().manual_seed(13 + sum(case))
    wt = torch.randn(cout, cin, 3, 3, generator=g) / (cout * 9) ** 0.5
    sh = shape(n, h, w, cin, cout, 3, 2, DT[dt])
    dz = torch.randn(n, cout, sh.ho, sh.wo, generator=g)
    run_under(cu_count, T.OVERRIDES, dgrad_store_accumulate(sh, wt, dz, dt, 7 + sum(case)), ("dx store", "dx accumulate"))


@pytest.mark.parametrize("dt", T.LOWP)
@pytest.mark.parametrize("case", T.BNRED, ids=T.case_id)
def test_dgrad_bnred_walk(case, dt, cu_count):
    """the fused BN-reduce epilogue against the separate path of test_dgrad_bnred_gpu.py (dx bit-identical to
    yms_conv_dgrad's under the same setting, every partial row written, dgamma / dbeta / coefficients within 2e-5
    of the separate path and of fp64: the partial rows are summed in another order per grid)"""
    import test_dgrad_bnred_gpu as B
    sp = ctypes.pointer(shape(case[0], case[2], case[3], case[1], case[4], 3, case[5], DT[dt]))
    for ov in (0,) + T.OVERRIDES:
        cu_count(ov)
        rows = L.lib().yms_conv_dgrad_bnred_rows(sp)
        assert rows == ov if ov else rows >= 1                 # one block per CU (B._run would skip at 0 rows)
        for act in ((1, 0) if dt == "bf16" else (1,)):       # SiLU / none, as that file runs them
            B._run(case, dt, act)
    cu_count(0)


# ---- depthwise ---------------------------------------------------------------------------------------------------
def dw_outputs(cs):
    """train forward z, eval forward (fixed scale / shift + SiLU) and the stored input gradient, for the bit
    comparison between grids"""
    import test_dwconv_edges_gpu as E
    n, h, w, c, k = cs.shp
    sc = torch.linspace(0.5, 1.5, c).to(DEV)
    sf = torch.linspace(-0.1, 0.1, c).to(DEV)
    y, _ = cs.fwd(cs.v["y"], sc, sf, L.ACT_SILU)
    z, _ = cs.fwd(cs.v["z"])
    dx, pre = E.out_view((n, h, w), c, cs.dtype, cs.v["dx"])
    L.call("yms_dwconv_dgrad", cs.sp, cs.dzb.data_ptr(), cs.dzb.shape[-1], cs.v["dz"][0], cs.wd.data_ptr(),
           dx.data_ptr(), dx.shape[-1], cs.v["dx"][0], 0, L.stream_ptr())
    E.body_of(dx, pre, c, cs.v["dx"])
    return y, z, dx


@pytest.mark.parametrize("dt,shp", T.DW_CASES, ids=lambda v: v if isinstance(v, str) else T.case_id(v))
def test_dwconv_walk_through_views(shp, dt, cu_count):
    """eval and train forward, dgrad and weight gradient of test_dwconv_edges_gpu.run_all_passes (hostile slack,
    NaN prefills, guarded workspace) under 1 / 2 / 3 CUs: strips of several tiles with a shorter last strip,
    several units per MFMA block with a partial last group, several tiles per weight-gradient block.  Override 2
    is the multi-strip case in a device-independent form."""
    import test_dwconv_edges_gpu as E
    cs = E.Case(shp, dt)              # operands and fp64 references, built once for all settings
    base = dw_outputs(cs)
    for ov in T.DW_OVERRIDES:
        cu_count(ov)
        if dt != "f32":
            assert T.dw_ws_rows(shp, dt) == T.DW_WS_ROWS[shp][ov - 1]
        E.check_eval(cs)
        E.check_train(cs)                 # moments per tile / unit: rows and counts as under the default
        E.check_dgrad(cs)
        E.check_wgrad(cs)                 # partial rows per strip / unit group / block: tolerance only
        for a, b, nm in zip(dw_outputs(cs), base, ("eval y", "train z", "dx")):
            _same_bits(a, b, f"{nm}, {ov} CUs")
    cu_count(0)


# ---- split-K weight gradients ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", T.LOWP)
@pytest.mark.parametrize("route,shp", T.WG_CASES, ids=lambda v: v if isinstance(v, str) else T.case_id(v))
def test_wgrad_one_split_and_many(route, shp, dt, cu_count, monkeypatch):
    """one split (override 1: each block walks every pixel of its tile) and as many as the work allows (2048),
    store and accumulate, operands in channel slices, workspace sized under the same setting and NaN-filled.
    The split count changes the order of the sum: the bound of the route's own test, no bit identity."""
    for key, v in T.WG_ENV[route].items():
        monkeypatch.setenv(key, v)
    n, cin, h, w, cout, k, s = shp
    dtype = DT[dt]
    g = torch.Generator().manual_seed(n * 7919 + cin * 31 + h + w + cout + s + k)
    x = torch.randn(n, cin, h, w, generator=g)
    sh = shape(n, h, w, cin, cout, k, s, dtype)
    dz = torch.randn(n, cout, sh.ho, sh.wo, generator=g)
    ref = torch.nn.grad.conv2d_weight(x.to(dtype).double(), (cout, cin, k, k), dz.to(dtype).double(), stride=s,
                                      padding=k // 2)
    sp = ctypes.pointer(sh)
    xb = nhwc(x, dtype, ld=r8(cin) + 16, off=8)
    dzb = nhwc(dz, dtype, ld=r8(cout) + 16, off=16)
    sizes = []
    for ov in (0,) + T.WG_OVERRIDES:
        cu_count(ov)
        wsb = L.lib().yms_conv_wgrad_ws_bytes(sp)
        sizes.append(wsb)
        ws = torch.full((wsb // 4 + 1,), float("nan"), dtype=torch.float32, device=DEV)
        ws[-1] = GUARD
        for acc in (0, 1):
            dw = torch.full((cout, cin, k, k), 0.25 if acc else float("nan"), device=DEV)
            L.call("yms_conv_wgrad", sp, xb.data_ptr(), xb.shape[-1], 8, dzb.data_ptr(), dzb.shape[-1], 16,
                   ws.data_ptr(), wsb, dw.data_ptr(), acc, L.stream_ptr())
            got = dw.double().cpu() - (0.25 if acc else 0.0)
            assert torch.isfinite(got).all(), (ov, acc)
            if route == "tt":             # the register-staged kernel's bound in test_conv_dgrad_wgrad
                _close(got, ref, 2e-3)
            else:                         # test_wgrad_ring / test_wgrad_3x3_halo
                rel = ((got - ref).norm() / ref.norm()).item()
                assert rel < 1e-5 and (got - ref).abs().max().item() <= 1e-5 * ref.abs().max().item() + 1e-6, (ov, acc, rel)
        assert ws[-1].item() == GUARD, "wrote past the workspace"
    cu_count(0)
    assert sizes[1] == T.wg_slab_bytes(route, shp) and sizes[2] >= 3 * sizes[1]


# ---- through the plans -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v", T.PLAN_MODELS)
def test_eval_forward_and_decode_bit_identical_under_one_cu(v, cu_count):
    """a fresh module per setting on the same state dict, the override constant from plan build to the last
    kernel: the decoded eval output does not depend on which block computed which tile"""
    from oracle import model_ref, ms_ref
    from yolov8.yolov8 import YOLOv8
    nc = 80
    sd = (ms_ref if v.startswith("ms") else model_ref).init_params(v, nc)
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(9)).to(DEV)
    outs = []
    for ov in (0, 1):
        cu_count(ov)
        m = YOLOv8(v, nc).to(DEV)
        m.load_state_dict(sd)
        m.eval()
        m.head.stride = torch.tensor([8.0, 16.0, 32.0])
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = m(x)
        torch.cuda.synchronize()
        outs.append(y.clone())
        del m
    cu_count(0)
    assert outs[0].shape[0] == 2 and outs[0].shape[-1] == 4 + nc and torch.isfinite(outs[0]).all()
    _same_bits(outs[1], outs[0], "decoded eval output, 1 CU")


def test_c2f_lowp_train_grads_under_one_cu(cu_count):
    """test_model_gpu.test_c2f_lowp_train_grads with every grid sized for one CU: the module is built, planned
    and run under the override; tolerances as there"""
    import test_model_gpu as MG
    cu_count(1)
    MG.c2f_lowp_train_grads(torch.bfloat16)
    torch.cuda.synchronize()
    cu_count(0)
