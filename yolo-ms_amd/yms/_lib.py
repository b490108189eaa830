"""ctypes binding of libyms.so (C-ABI declared in include/yms.h).

The HIP library is mandatory: there is no CPU or eager-PyTorch fallback.  If the
shared object is missing or a call returns a non-zero status, a RuntimeError is
raised immediately.  torch must be imported before the library is loaded so that
libyms.so binds to the HIP runtime already loaded by torch (same soname).
"""
from __future__ import annotations

import ctypes
import operator
import os
import types

import torch  # noqa: F401  (loads the process' HIP runtime first)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("YMS_LIB") or os.path.join(_HERE, "libyms.so")   # YMS_LIB: dev A/B builds (tools/ab_lib.sh)

F32, BF16, F16 = 0, 1, 2
ACT_NONE, ACT_SILU = 0, 1

_DT = {torch.float32: F32, torch.bfloat16: BF16, torch.float16: F16}


def dtype_code(dt):
    try:
        return _DT[dt]
    except KeyError:
        raise RuntimeError(f"yms: unsupported dtype {dt}; use float32, bfloat16 or float16") from None


class ConvShape(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int) for k in
                ("n", "h", "w", "cin", "cout", "k", "stride", "pad", "ho", "wo", "dtype")]


class DwShape(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int) for k in ("n", "h", "w", "c", "k", "dtype")]


class PackJob(ctypes.Structure):
    _fields_ = [("w", ctypes.c_void_p), ("packed", ctypes.c_void_p)] + [
        (k, ctypes.c_int) for k in ("cout", "cin", "ks", "rows", "kp_elems", "c8_in", "for_dgrad", "dtype")] + [
        ("w2", ctypes.c_void_p), ("split", ctypes.c_int)]


_P = ctypes.c_void_p
_I = ctypes.c_int


def _fields(spec):
    """'name:type ...' -> ctypes _fields_ (p pointer, i int, l long, f float, s ConvShape by value)."""
    t = {"p": ctypes.c_void_p, "i": ctypes.c_int, "l": ctypes.c_long, "f": ctypes.c_float, "s": ConvShape}
    return [(n, t[k]) for n, k in (f.split(":") for f in spec.split())]


# job records of the grouped entry points (include/yms.h)
class ConvFwdJob(ctypes.Structure):
    _fields_ = _fields("shape:s x:p x_ld:i x_off:i wpacked:p y:p y_ld:i y_off:i scale:p shift:p act:i "
                       "res:p res_ld:i res_off:i stats:p")


class ConvDgradJob(ctypes.Structure):
    _fields_ = _fields("shape:s dz:p dz_ld:i dz_off:i wpacked_t:p dx:p dx_ld:i dx_off:i accumulate:i")


class BnFinalizeJob(ctypes.Structure):
    _fields_ = _fields("c:i stats:p rows:i stats_ld:i count:l gamma:p beta:p rmean:p rvar:p momentum:f eps:f "
                       "mean_invstd:p mi_ld:i scale:p shift:p")


class BnPassJob(ctypes.Structure):
    _fields_ = _fields("npix:l c:i z:p z_ld:i z_off:i gy:p gy_ld:i gy_off:i scale:p shift:p mean_invstd:p coef:p "
                       "act:i out:p out_ld:i out_off:i res:p res_ld:i res_off:i res_acc:i ws:p counter:p dbias:p")


class BnFoldJob(ctypes.Structure):
    _fields_ = _fields("gamma:p beta:p rmean:p rvar:p eps:f c:i mi_ld:i scale:l shift:l mean_invstd:l")


class BnBwdFinalizeJob(ctypes.Structure):
    _fields_ = _fields("c:i ws:p rows:i count:l dgamma:p dbeta:p coef:p")


# optimizer records (include/yms.h, "optimizer step")
OPTIM_SGD, OPTIM_ADAM, OPTIM_ADAMW = 0, 1, 2
OPTIM_GRAD_NONE, OPTIM_GRAD_ABS, OPTIM_EMA = 1, 2, 4
OPTIM_MAX_GROUPS = 8
OPTIM_EMA_TAU, OPTIM_EMA_EXPMOM = 0, 1
OPTIM_SCHED_LR, OPTIM_SCHED_MOMENTUM = 0, 1
OPTIM_SCHED_LINEAR, OPTIM_SCHED_COSINE = 0, 1
OPTIM_MAX_SEGMENTS = 8


class OptimJob(ctypes.Structure):
    _fields_ = [("param", ctypes.c_void_p)] + [(k, ctypes.c_int64) for k in
                                                ("grad", "state0", "state1", "ema", "count")] + [
        ("group", ctypes.c_int), ("flags", ctypes.c_int)]


class OptimChunk(ctypes.Structure):
    _fields_ = [("p", ctypes.c_void_p), ("g", ctypes.c_int64), ("s0", ctypes.c_void_p), ("s1", ctypes.c_void_p),
                ("e", ctypes.c_void_p), ("n", ctypes.c_int), ("group", ctypes.c_short), ("flags", ctypes.c_short)]


class OptimHyper(ctypes.Structure):
    _fields_ = [(k, ctypes.c_double) for k in ("max_norm", "skip_nonfinite", "ema_decay", "ema_tau")] + [
        ("group", ctypes.c_double * 8 * OPTIM_MAX_GROUPS)]


class OptimSegment(ctypes.Structure):
    _fields_ = [(k, ctypes.c_double) for k in ("begin", "end", "start", "stop")] + [
        (k, ctypes.c_int) for k in ("target", "shape", "groups", "pad")]


class OptimExt(ctypes.Structure):
    _fields_ = [("ema_rule", ctypes.c_double), ("nsegments", ctypes.c_double),
                ("seg", OptimSegment * OPTIM_MAX_SEGMENTS)]


_L = ctypes.c_long
_F = ctypes.c_float
_D = ctypes.c_double
_SZ = ctypes.c_size_t
_SP = ctypes.POINTER(ConvShape)
_DP = ctypes.POINTER(DwShape)

_SIGS = {
    "yms_version": (ctypes.c_char_p, []),
    "yms_status_string": (ctypes.c_char_p, [_I]),
    "yms_conv_packed_elems": (_SZ, [_SP, _I]),
    "yms_conv_pack_weight": (_I, [_SP, _P, _P, _I, _P]),
    "yms_pack_job_init": (_I, [_SP, _P, _P, _I, ctypes.POINTER(PackJob)]),
    "yms_conv_pack_weights_batched": (_I, [_I, _P, _P, _P]),
    "yms_conv_stats_rows": (_I, [_SP]),
    "yms_conv_stats_ld": (_I, [_SP]),
    "yms_conv_direct_set": (_I, [_I]),
    "yms_cu_count_set": (_I, [_I]),
    "yms_conv_fwd": (_I, [_SP, _P, _I, _I, _P, _P, _I, _I, _P, _P, _I, _P, _I, _I, _P, _P]),
    "yms_conv_stem_supported": (_I, [_SP]),
    "yms_conv_stem_stats_rows": (_I, [_SP]),
    "yms_conv_stem_fwd": (_I, [_SP, _P, _P, _P, _I, _I, _P, _P, _I, _P, _I, _P]),
    "yms_conv_stem_wgrad_ws_bytes": (_SZ, [_SP]),
    "yms_conv_stem_wgrad": (_I, [_SP, _P, _P, _I, _I, _P, _I, _I, _P, _P, _P, _P, _I, _P, _SZ, _P, _I, _P]),
    "yms_conv_dgrad": (_I, [_SP, _P, _I, _I, _P, _P, _I, _I, _I, _P]),
    "yms_conv_dgrad_bnred_rows": (_I, [_SP]),
    "yms_conv_dgrad_bnred": (_I, [_SP, _P, _I, _I, _P, _P, _I, _I, _I, _P, _I, _I, _P, _P, _P, _I, _P, _P]),
    "yms_conv_fwd_group": (_I, [_I, _P, _P]),
    "yms_conv_dgrad_group": (_I, [_I, _P, _P]),
    "yms_conv_fwd_group_launches": (_I, [_I, _P]),
    "yms_conv_dgrad_group_launches": (_I, [_I, _P]),
    "yms_conv_wgrad_ws_bytes": (_SZ, [_SP]),
    "yms_conv_wgrad": (_I, [_SP, _P, _I, _I, _P, _I, _I, _P, _SZ, _P, _I, _P]),
    "yms_bn_fold": (_I, [_I, _P, _P, _P, _P, _F, _P, _P, _P]),
    "yms_bn_finalize": (_I, [_I, _P, _I, _I, _L, _P, _P, _P, _P, _F, _F, _P, _P, _P, _P]),
    "yms_bn_finalize_ld": (_I, [_I, _P, _I, _I, _L, _P, _P, _P, _P, _F, _F, _P, _I, _P, _P, _P]),
    "yms_affine_act": (_I, [_I, _L, _I, _P, _I, _I, _P, _P, _I, _P, _I, _I, _P, _I, _I, _P]),
    "yms_bn_bwd_rows": (_I, [_L, _I]),
    "yms_bn_act_bwd_reduce": (_I, [_I, _L, _I, _P, _I, _I, _P, _I, _I, _P, _P, _P, _I, _P, _P]),
    "yms_bn_act_bwd_finalize": (_I, [_I, _P, _I, _L, _P, _P, _P, _P]),
    "yms_bn_act_bwd_apply": (_I, [_I, _L, _I, _P, _I, _I, _P, _I, _I, _P, _P, _P, _P, _I, _P, _I, _I,
                                  _P, _I, _I, _I, _P]),
    "yms_bn_act_bwd_reduce_finalize": (_I, [_I, _L, _I, _P, _I, _I, _P, _I, _I, _P, _P, _P, _I, _P, _P, _P, _P,
                                            _P, _P]),
    "yms_bias_bwd": (_I, [_I, _L, _I, _P, _I, _I, _P, _P, _P, _P]),
    "yms_bn_frozen_act_bwd": (_I, [_I, _L, _I, _P, _I, _I, _P, _I, _I, _P, _P, _P, _I, _P, _I, _I, _P, _I, _I, _I,
                                   _P, _P, _P, _P, _P]),
    "yms_bn_fold_mi": (_I, [_I, _P, _P, _P, _P, _F, _P, _P, _P, _I, _P]),
    "yms_bn_fold_mi_batched": (_I, [_I, _P, _I, _P, _P]),
    "yms_bn_finalize_group": (_I, [_I, _P, _P]),
    "yms_affine_act_group": (_I, [_I, _I, _P, _P]),
    "yms_bn_act_bwd_reduce_group": (_I, [_I, _I, _P, _P]),
    "yms_bn_act_bwd_finalize_group": (_I, [_I, _P, _P]),
    "yms_bn_act_bwd_apply_group": (_I, [_I, _I, _P, _P]),
    "yms_bias_bwd_group": (_I, [_I, _I, _P, _P]),
    "yms_sppf_ws_bytes": (_SZ, [_I, _I, _I, _I]),
    "yms_sppf_pool_fwd": (_I, [_I, _I, _I, _I, _I, _P, _I, _I, _P]),
    "yms_sppf_pool_bwd": (_I, [_I, _I, _I, _I, _I, _P, _I, _I, _P, _I, _I, _P, _P]),
    "yms_sppf_fused_fits": (_I, [_I, _I, _I, _I]),
    "yms_sppf_route_set": (_I, [_I]),
    "yms_upsample2x_fwd": (_I, [_I, _I, _I, _I, _I, _P, _I, _I, _P, _I, _I, _P]),
    "yms_upsample2x_bwd": (_I, [_I, _I, _I, _I, _I, _P, _I, _I, _P, _I, _I, _I, _P]),
    "yms_pack_input": (_I, [_I, _I, _I, _I, _I, _P, _P, _I, _P]),
    "yms_nhwc_to_nchw": (_I, [_I, _I, _I, _I, _I, _I, _P, _I, _I, _P, _P]),
    "yms_nchw_to_nhwc": (_I, [_I, _I, _I, _I, _I, _I, _P, _P, _I, _I, _I, _P]),
    "yms_cast": (_I, [_I, _I, _L, _P, _P, _P]),
    "yms_zero": (_I, [_P, _SZ, _P]),
    "yms_copy": (_I, [_P, _P, _SZ, _P]),
    "yms_dwconv_stats_rows": (_I, [_DP]),
    "yms_dwconv_fwd": (_I, [_DP, _P, _I, _I, _P, _P, _I, _I, _P, _P, _I, _P, _I, _P]),
    "yms_dwconv_dgrad": (_I, [_DP, _P, _I, _I, _P, _P, _I, _I, _I, _P]),
    "yms_dwconv_wgrad_ws_bytes": (_SZ, [_DP]),
    "yms_dwconv_wgrad": (_I, [_DP, _P, _I, _I, _P, _I, _I, _P, _SZ, _P, _I, _P]),
    "yms_add_views": (_I, [_I, _L, _I, _P, _I, _I, _P, _I, _I, _P, _I, _I, _I, _P]),
    "yms_add_grad2": (_I, [_I, _L, _I, _P, _I, _I, _P, _I, _I, _I, _P, _I, _I, _I, _P]),
    "yms_map_match": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P]),
    "yms_map_accumulate": (_I, [_I, _P, _P, _P, _P, _P, _I, _P, _P, _P]),
    "yms_map_match_coco": (_I, [_I, _I, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _I, _P]),
    "yms_map_accumulate_coco": (_I, [_I, _P, _P, _P, _P, _P, _P, _I, _I, _P, _P, _P]),
    "yms_map_match_coco_fixed": (_I, [_I, _I, _P, _P, _P, _P, _I, _P, _P, _P, _I, _P, _I, _L, _L, _P, _P, _P, _P, _P,
                                      _P, _P, _P]),
    "yms_map_match_coco_gt": (_I, [_I, _I, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _I, _P, _P, _P]),
    "yms_map_match_coco_fixed_gt": (_I, [_I, _I, _P, _P, _P, _P, _I, _P, _P, _P, _I, _P, _I, _L, _L, _P, _P, _P, _P,
                                         _P, _P, _P, _P, _P, _P]),
    "yms_map_accumulate_coco_dev_ws_bytes": (_SZ, [_L, _I, _I]),
    "yms_map_accumulate_coco_dev": (_I, [_L, _L, _P, _P, _P, _P, _P, _I, _I, _P, _P, _P, _P, _SZ, _P]),
    "yms_det_loss_ws_bytes": (_SZ, [_I, _I, _I, _I]),
    "yms_stream_create_cu_subset": (_I, [_I, _I, ctypes.POINTER(ctypes.c_void_p)]),
    "yms_resize_normalize": (_I, [_I, _I, _P, _I, _I, _P, _P, _P, _P]),
    "yms_augment_image_bytes": (_SZ, []),
    "yms_augment_normalize": (_I, [_I, _I, _P, _I, _I, _P, _P, _P, _P]),
    "yms_mosaic_image_bytes": (_SZ, []),
    "yms_mosaic_normalize": (_I, [_I, _I, _P, _I, _I, _P, _P, _P, _P]),
    "yms_tgt_tile_bytes": (_SZ, []),
    "yms_tgt_layer_bytes": (_SZ, []),
    "yms_box_targets": (_I, [_I, _P, _I, _P, _P, _P, _L, _I, _P, _P]),
    "yms_det_loss": (_I, [_I, _I, _I, _I, _P, _P, _P, _P, _P, _I, _P, _I, _F, _F, _I, _P, _P, _P, _SZ, _P, _P]),
    "yms_scale_by_device_scalar": (_I, [_I, _I, _P, _P, _P, _P]),
    "yms_tal_loss_ws_bytes": (_SZ, [_I, _I, _I, _I]),
    "yms_tal_loss": (_I, [_I, _I, _I, _I, _P, _P, _P, _P, _P, _I, _P, _I, _F, _F, _I, _F, _F, _P, _P, _SZ, _P, _P, _P,
                          _P]),
    "yms_dsl_loss_ws_bytes": (_SZ, [_I, _I, _I, _I]),
    "yms_dsl_loss": (_I, [_I, _I, _I, _I, _P, _P, _P, _P, _P, _I, _P, _I, _F, _F, _I, _F, _F, _F, _P, _P, _SZ, _P, _P,
                          _P, _P, _P]),
    "yms_head_decode": (_I, [_I, _I, _I, _I, _P, _P, _P, _I, _P, _P, _F, _P, _P, _P, _P]),
    "yms_dfl": (_I, [_I, _I, _I, _I, _P, _P, _P]),
    "yms_nms_prep": (_I, [_I, _I, _I, _P, _F, _P, _P, _P, _P]),
    "yms_nms_ws_bytes": (_SZ, [_I, _I, _I]),
    "yms_nms_ws_bytes_min": (_SZ, [_I, _I, _I]),
    "yms_nms_classwise": (_I, [_I, _I, _I, _P, _P, _P, _D, _P, _P, _P, _P, _SZ, _P]),
    "yms_nms_single": (_I, [_I, _P, _P, _D, _P, _P, _P, _SZ, _P]),
    "yms_det_ws_bytes": (_SZ, [_I, _I, _I, _I]),
    "yms_det_candidates": (_I, [_I, _I, _I, _P, _F, _I, _P, _I, _P, _P, _P, _P, _P, _P, _P, _SZ, _P]),
    "yms_det_finalize": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "yms_det_finalize_vote": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _D, _P, _P, _P, _P]),
    "yms_tta_merge": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "yms_tile_merge_max_blocks": (_I, []),
    "yms_tile_merge": (_I, [_I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "yms_optim_chunk_elems": (_I, []),
    "yms_optim_table_chunks": (_L, [_I, _P]),
    "yms_optim_table_bytes": (_SZ, [_I, _P]),
    "yms_optim_table_build": (_I, [_I, _P, _P, _P, _P, _P, _SZ]),
    "yms_optim_norm_partials": (_I, [_L]),
    "yms_optim_grad_norm": (_I, [_P, _L, _P, _P, _P]),
    "yms_optim_step": (_I, [_I, _P, _L, _P, _P, _P, _P, _I, _P]),
    "yms_optim_step_ext": (_I, [_I, _P, _L, _P, _P, _P, _P, _P, _P, _I, _P]),
    "yms_optim_swap": (_I, [_P, _L, _P]),
}

EXPORTED = tuple(_SIGS)
_lib = None


def lib():
    """Load libyms.so (raises RuntimeError when the HIP extension has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"yms: HIP library {LIB_PATH} not found -- build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` (make -C yolo-ms_amd/csrc)")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(status, what):
    if status != 0:
        msg = lib().yms_status_string(status).decode()
        raise RuntimeError(f"yms: {what} failed: {msg} (status {status})")


_prof = None
_CONV = ("yms_conv_fwd", "yms_conv_dgrad", "yms_conv_dgrad_bnred", "yms_conv_wgrad", "yms_conv_stem_fwd")
_DW = ("yms_dwconv_fwd", "yms_dwconv_dgrad", "yms_dwconv_wgrad")
# grouped entry points (njobs, job array right before the stream): priced as the sum of their members;
# the BN-family ones are recorded under their solo names, the ones the benchmark's rooflines count
# (the grouped convs keep their own yms_conv_* names)
_GROUP_AS = {"yms_conv_fwd_group": "yms_conv_fwd", "yms_conv_dgrad_group": "yms_conv_dgrad",
             "yms_affine_act_group": "yms_affine_act", "yms_bn_act_bwd_reduce_group": "yms_bn_act_bwd_reduce",
             "yms_bn_act_bwd_apply_group": "yms_bn_act_bwd_apply", "yms_bn_finalize_group": "yms_bn_finalize",
             "yms_bn_act_bwd_finalize_group": "yms_bn_act_bwd_finalize", "yms_bias_bwd_group": "yms_bias_bwd"}
# launches whose hipStream_t is the last argument (status-returning entry points ending in a void*)
# (host-only entry points whose last pointer is a host buffer are listed out explicitly)
_HOST_ONLY = {"yms_map_accumulate", "yms_map_accumulate_coco", "yms_pack_job_init", "yms_conv_fwd_group_launches",
              "yms_conv_dgrad_group_launches"}
_STREAM_LAST = {n for n, (res, args) in _SIGS.items()
                if res is _I and args and args[-1] is _P and n not in _HOST_ONLY}


_FN = {}


def _elt(dt):
    return 4 if dt == F32 else 2


# Solo entry points with a job record: their argument order before the stream, as fields of the record
# ("dtype": the call's own): call_job unpacks a record by it, _work names a positional call's arguments.
_ARGS = {k: v.split() for k, v in {
    "yms_conv_fwd": "shape x x_ld x_off wpacked y y_ld y_off scale shift act res res_ld res_off stats",
    "yms_conv_dgrad": "shape dz dz_ld dz_off wpacked_t dx dx_ld dx_off accumulate",
    "yms_bn_finalize": "c stats rows stats_ld count gamma beta rmean rvar momentum eps mean_invstd scale shift",
    "yms_bn_finalize_ld": "c stats rows stats_ld count gamma beta rmean rvar momentum eps mean_invstd mi_ld scale shift",
    "yms_affine_act": "dtype npix c z z_ld z_off scale shift act res res_ld res_off out out_ld out_off",
    "yms_bn_act_bwd_reduce": "dtype npix c z z_ld z_off gy gy_ld gy_off scale shift mean_invstd act ws",
    "yms_bn_act_bwd_finalize": "c ws rows count dgamma dbeta coef",
    "yms_bn_act_bwd_apply": "dtype npix c z z_ld z_off gy gy_ld gy_off scale shift mean_invstd coef act "
                            "out out_ld out_off res res_ld res_off res_acc",
    "yms_bias_bwd": "dtype npix c gy gy_ld gy_off ws counter dbias",
    "yms_bn_frozen_act_bwd": "dtype npix c z z_ld z_off gy gy_ld gy_off scale shift mean_invstd act "
                             "out out_ld out_off res res_ld res_off res_acc ws counter",     # + dgamma, dbeta
}.items()}
_JOB_ARGS = {k: operator.attrgetter(*[f for f in v if f != "dtype"]) for k, v in _ARGS.items()}


def job_args(name, job, dtype=None):
    """Solo entry point `name`'s arguments before the stream (ctypes passes a ConvShape field by address)."""
    a = _JOB_ARGS[name](job)
    return a if _ARGS[name][0] != "dtype" else (dtype,) + a


def call_job(name, job, stream, dtype=None):
    call(name, *job_args(name, job, dtype), stream)


def _work(name, args):
    """(algorithmic FLOPs, algorithmic HBM bytes) of one launch: every operand read or written once.
    Convs: input + output + weights (fp32 weight gradient); depthwise: the same with fp32 [C][k][k]
    weights (FLOPs = 2 n h w c k^2, VALU); BN / branch-sum elementwise passes: their streams."""
    solo = _GROUP_AS.get(name)
    if solo is not None:             # the sum of the members, each priced as its solo call
        works = [_work_job(solo, j, args[0]) for j in args[-2][:args[-3]]]
        return sum(w[0] for w in works), sum(w[1] for w in works)
    if name in _ARGS:
        return _work_job(name, types.SimpleNamespace(**dict(zip(_ARGS[name], args))), args[0])
    if name in _CONV:
        return _work_job(name, types.SimpleNamespace(shape=args[0]), None)
    if name in _DW:
        d = args[0].contents
        vol = d.n * d.h * d.w * d.c
        return 2 * vol * d.k * d.k, 2 * vol * _elt(d.dtype) + 4 * d.c * d.k * d.k
    if name in ("yms_add_views", "yms_add_grad2"):
        vol = args[1] * args[2] * _elt(args[0])
        if name == "yms_add_views":
            return 0, (2 + (args[6] is not None) + bool(args[12])) * vol
        return 0, (3 + bool(args[9]) + bool(args[13])) * vol       # add_grad2: gy -> ga, gb
    return 0, 0


def _work_job(name, j, dtype):
    """_work of solo entry point `name` from its arguments by name (dtype: its own first argument, if any)."""
    if name in _CONV:
        sh = getattr(j.shape, "contents", j.shape)     # a pointer (positional call) or the job's own shape
        fl = 2 * sh.n * sh.ho * sh.wo * sh.cout * sh.cin * sh.k * sh.k
        es = _elt(sh.dtype)
        act = (sh.n * sh.h * sh.w * sh.cin + sh.n * sh.ho * sh.wo * sh.cout) * es
        if name == "yms_conv_dgrad_bnred":             # + the producer's z at the dx pixels
            act += sh.n * sh.h * sh.w * sh.cin * es
        return fl, act + sh.cout * sh.cin * sh.k * sh.k * (4 if name == "yms_conv_wgrad" else es)
    vol = j.npix * j.c * _elt(dtype) if hasattr(j, "npix") else 0
    if name == "yms_bn_act_bwd_reduce":
        return 0, 2 * vol                                          # z, gy
    if name == "yms_affine_act":
        return 0, (2 + (j.res is not None)) * vol                  # z (+res) -> y
    if name in ("yms_bn_act_bwd_apply", "yms_bn_frozen_act_bwd"):
        return 0, (3 + (j.res is not None) * (1 + bool(j.res_acc))) * vol   # z, gy -> dz (+ gres)
    return 0, 0


def call(name, *args):
    if _prof is None:
        fn = _FN.get(name)
        if fn is None:
            fn = _FN[name] = getattr(lib(), name)
        st = fn(*args)
        if st != 0:
            check(st, name)
        return
    s = torch.cuda.Event(enable_timing=True)
    e = torch.cuda.Event(enable_timing=True)
    # entry points take their hipStream_t last: time them on the stream they run on (weight
    # gradients run on the backward's side stream)
    st = torch.cuda.ExternalStream(args[-1]) if name in _STREAM_LAST and args[-1] else None
    s.record(st)
    check(getattr(lib(), name)(*args), name)
    e.record(st)
    fl, nb = _work(name, args)
    _prof.append((name if name.startswith("yms_conv_") else _GROUP_AS.get(name, name), s, e, fl, nb))


def profile_begin():
    """Record a HIP event pair around every C-ABI launch (diagnostic): conv launches on the
    stream they are issued to, everything else on the current stream."""
    global _prof
    _prof = []


def profile_end(peak_tflops=2500.0, peak_gbs=8000.0, valu_tflops=157.3):
    """-> {name: [calls, total_ms, flops, bytes, roofline_ms, hbm_bound_calls]} for the launches
    since profile_begin().  roofline_ms sums, per launch, max(flops / peak, bytes / peak_gbs): the
    time the launch would take at the roofline of its own arithmetic intensity (peak = the dense
    MFMA rate for convs, the fp32 VALU rate for the depthwise kernels)."""
    global _prof
    torch.cuda.synchronize()
    out = {}
    for name, s, e, fl, nb in _prof:
        r = out.setdefault(name, [0, 0.0, 0, 0, 0.0, 0])
        r[0] += 1
        r[1] += s.elapsed_time(e)
        r[2] += fl
        r[3] += nb
        pk = valu_tflops if name in _DW else peak_tflops
        t_f, t_b = fl / (pk * 1e9), nb / (peak_gbs * 1e6)   # ms
        r[4] += max(t_f, t_b)
        r[5] += int(t_b > t_f)
    _prof = None
    return out


def stream_ptr(device=None):
    return torch.cuda.current_stream(device).cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()
