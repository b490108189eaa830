"""Argument checks of the depthwise entry points (yms_dwconv_fwd / dgrad / wgrad) and of the branch-sum
kernels (yms_add_views / yms_add_grad2): each row is a valid call with ONE argument broken and returns
YMS_ERR_INVALID before any launch.  No GPU needed: the pointers are host dummies that are never
dereferenced.  The host sizing functions answer 0 for the shapes the entry points reject.

The valid calls themselves (`baselines`) cannot be made here, so this file alone does not show that a row
fails for its labelled reason and not because its baseline is already invalid:
test_dwconv_edges_gpu.py::test_argument_table_baselines_are_valid makes every baseline on device memory
and expects YMS_OK."""
import ctypes

from yms import _lib as L

INVALID = 1        # YMS_ERR_INVALID (include/yms.h)
BAD_DT = 7
_buf = (ctypes.c_float * 16)()
HOST = ctypes.addressof(_buf)


def _sh(n=1, h=4, w=4, c=16, k=3, dt=L.BF16):
    return ctypes.pointer(L.DwShape(n, h, w, c, k, dt))


def baselines(P):
    """{label: (entry point, {arg name: value} in call order)}: the valid calls the rows break, every
    pointer = P (at most 16 MiB are touched behind it)"""
    fwd = dict(s=_sh(), x=P, x_ld=32, x_off=8, w=P, y=P, y_ld=40, y_off=16, scale=P, shift=P, act=L.ACT_SILU,
               stats=None, stats_ld=0, stream=None)
    out = {
        "fwd_eval": ("yms_dwconv_fwd", fwd),
        # statistics on: the row stride must hold the channels
        "fwd_train": ("yms_dwconv_fwd", dict(fwd, scale=None, shift=None, act=L.ACT_NONE, stats=P, stats_ld=16)),
        "dgrad": ("yms_dwconv_dgrad", dict(s=_sh(k=7), dz=P, dz_ld=32, dz_off=8, w=P, dx=P, dx_ld=40, dx_off=16, acc=0,
                                           stream=None)),
    }
    # weight gradient: strip / MFMA / register-prefetch / tile route
    for label, s in (("strip", _sh()), ("mfma", _sh(k=9)), ("prefetch", _sh(n=2, h=40, w=80, c=64, k=7)),
                     ("tile", _sh(k=5, dt=L.F32))):
        c = s.contents.c
        need = L.lib().yms_dwconv_wgrad_ws_bytes(s)
        assert s.contents.k ** 2 * c * 4 <= need <= 16 << 20
        out["wgrad_" + label] = ("yms_dwconv_wgrad", dict(s=s, x=P, x_ld=c + 16, x_off=8, dz=P, dz_ld=c + 24, dz_off=16,
                                                          ws=P, ws_bytes=need, dw=P, acc=0, stream=None))
    add = dict(dtype=L.BF16, npix=4, c=16, a=P, a_ld=32, a_off=8, b=P, b_ld=40, b_off=16, y=P, y_ld=48, y_off=24,
               acc=0, stream=None)
    out["add_views"] = ("yms_add_views", add)
    # b = NULL (the branch-sum backward form)
    out["add_views_no_b"] = ("yms_add_views", dict(add, b=None, b_ld=0, b_off=0, acc=1))
    out["add_grad2"] = ("yms_add_grad2", dict(dtype=L.F16, npix=4, c=16, g=P, g_ld=32, g_off=8, ga=P, ga_ld=40, ga_off=16,
                                              acc1=0, gb=P, gb_ld=48, gb_off=24, acc2=1, stream=None))
    return out


def _rows(label, **broken):
    """broken: {row label: {arg name: bad value}} applied to baselines(HOST)[label]"""
    name, good = baselines(HOST)[label]
    fn = getattr(L.lib(), name)
    for row, change in broken.items():
        assert set(change) <= set(good), (label, row)
        args = [change.get(k, v) for k, v in good.items()]
        assert fn(*args) == INVALID, (label, row)
    return good


# the shapes dw_shape_ok refuses (every depthwise entry point and both sizing functions)
BAD_SHAPES = dict(k4=_sh(k=4), k1=_sh(k=1), k11=_sh(k=11), c_mod8=_sh(c=12), c0=_sh(c=0), n0=_sh(n=0), h0=_sh(h=0),
                  w0=_sh(w=0), dtype_high=_sh(dt=BAD_DT), dtype_neg=_sh(dt=-1), null=None)


def _shape_rows():
    return {"shape_" + k: dict(s=v) for k, v in BAD_SHAPES.items()}


def _view_rows(name, c=16, ld=32):
    """ld % 8, off % 8, off + c > ld and a negative offset for the view (name, name_ld, name_off)"""
    return {name + "_ld_mod8": {name + "_ld": ld + 4}, name + "_off_mod8": {name + "_off": 4},
            name + "_over": {name + "_off": ld - c + 8}, name + "_off_neg": {name + "_off": -8},
            name + "_ld_small": {name + "_ld": c - 8, name + "_off": 0}}


def test_sizing_functions_return_zero_for_rejected_shapes():
    lib = L.lib()
    assert lib.yms_dwconv_stats_rows(_sh()) > 0 and lib.yms_dwconv_wgrad_ws_bytes(_sh()) > 0
    for label, s in BAD_SHAPES.items():
        assert lib.yms_dwconv_stats_rows(s) == 0, label
        assert lib.yms_dwconv_wgrad_ws_bytes(s) == 0, label


def test_dwconv_fwd_argument_validation():
    _rows("fwd_eval", x_null=dict(x=None), w_null=dict(w=None), y_null=dict(y=None),
          **_shape_rows(), **_view_rows("x", ld=32), **_view_rows("y", ld=40))
    _rows("fwd_train", stats_ld_small=dict(stats_ld=8), stats_ld_zero=dict(stats_ld=0),
          stats_ld_neg=dict(stats_ld=-16), x_null=dict(x=None), **_shape_rows(), **_view_rows("y", ld=40))


def test_dwconv_dgrad_argument_validation():
    _rows("dgrad", dz_null=dict(dz=None), w_null=dict(w=None), dx_null=dict(dx=None),
          **_shape_rows(), **_view_rows("dz", ld=32), **_view_rows("dx", ld=40))


def test_dwconv_wgrad_argument_validation():
    for label in ("strip", "mfma", "prefetch", "tile"):
        good = baselines(HOST)["wgrad_" + label][1]
        c, need = good["s"].contents.c, good["ws_bytes"]
        _rows("wgrad_" + label, ws_one_byte_short=dict(ws_bytes=need - 1), ws_bytes_zero=dict(ws_bytes=0),
              x_null=dict(x=None), dz_null=dict(dz=None), ws_null=dict(ws=None), dw_null=dict(dw=None),
              **_shape_rows(), **_view_rows("x", c=c, ld=c + 16), **_view_rows("dz", c=c, ld=c + 24))


def test_add_views_argument_validation():
    common = dict(dtype_high=dict(dtype=BAD_DT), dtype_neg=dict(dtype=-1), npix0=dict(npix=0), npix_neg=dict(npix=-3),
                  c_mod8=dict(c=12), c0=dict(c=0), a_null=dict(a=None), y_null=dict(y=None))
    _rows("add_views", **common, **_view_rows("a", ld=32), **_view_rows("b", ld=40), **_view_rows("y", ld=48))
    # b = NULL: the other views are still checked
    _rows("add_views_no_b", **common, **_view_rows("a", ld=32), **_view_rows("y", ld=48))


def test_add_grad2_argument_validation():
    _rows("add_grad2", dtype_high=dict(dtype=BAD_DT), dtype_neg=dict(dtype=-1), npix0=dict(npix=0),
          c_mod8=dict(c=12), c0=dict(c=0), g_null=dict(g=None), ga_null=dict(ga=None), gb_null=dict(gb=None),
          **_view_rows("g", ld=32), **_view_rows("ga", ld=40), **_view_rows("gb", ld=48))
