"""Test-time augmentation around ``yms.ops.detect``: the same images are run at several input sizes,
some flipped, and the views' decoded predictions are mapped back to each original image, concatenated
(one launch, csrc/tta.hip) and put through ONE detect -- candidates, NMS, max_det -- optionally with box
voting (``detect(vote=True)``).  The same merge serves a model ensemble: predictions of different
models over the same images are just more views.

These are this package's semantics, not a port.  ultralytics' ``augment=True`` resizes the already
letterboxed tensor by 1 / 0.83 / 0.67 (flipping the middle view) and pads it to the stride; the
RTMDet-lineage ``tta_model`` behind the YOLO-MS numbers resizes to three sizes, each with and without a
flip.  Here EVERY VIEW IS LETTERBOXED FROM THE ORIGINAL IMAGE directly into the view's size (one
yms_mosaic_normalize launch per view, a flip being a stage on the letterbox layer), so a view never
resamples a resampled image and each view has exact frames of its own.  Neither package is installed:
parity with ultralytics / mmyolo is UNPINNED, as for ``detect``.

Rows.  A view's prediction has its rows level by level, finest first; level i of an (H, W) view has
(H / s_i) * (W / s_i) rows.  The merged tensor holds view 0's chosen rows, then view 1's, ...; with
row counts c_v and prefix sums off_v = c_0 + ... + c_{v-1}, merged row m belongs to the view v with
off_v <= m < off_{v+1} and is that view's anchor rows[v][0] + (m - off_v).  ``Detections.anchors`` of
``detect_views`` / ``detect_tta`` are such merged rows; ``Views.locate`` does the arithmetic."""
from __future__ import annotations

import ctypes
import math

import torch

from . import _lib as L
from . import data as D
from . import ops

MAX_VIEWS = 8


def view_sizes(size, scales, stride=32):
    """[(H_v, W_v)] for the base ``size`` (int or (H, W)) and each scale: ceil(H s / stride) * stride,
    ultralytics' scale_img rule (the scaled side, padded up to the grid)."""
    H, W = (size, size) if isinstance(size, int) else size
    return [(math.ceil(H * s / stride) * stride, math.ceil(W * s / stride) * stride) for s in scales]


def _hw(s):
    return (int(s), int(s)) if isinstance(s, (int, float)) else (int(s[0]), int(s[1]))


def level_rows(size, strides):
    """Rows of each pyramid level of an (H, W) view."""
    H, W = _hw(size)
    return [(H // int(s)) * (W // int(s)) for s in strides]


def trim_rows(sizes, strides):
    """ultralytics' _clip_augmented rule as row ranges [(a0, a1)]: with two or more views the first
    view loses its last (coarsest) level -- the largest view's biggest boxes -- and the last view its
    first (finest) level -- the smallest view's smallest boxes; every other view keeps all rows."""
    out = []
    for v, s in enumerate(sizes):
        rows = level_rows(s, strides)
        a0, a1 = 0, sum(rows)
        if len(sizes) >= 2 and v == 0:
            a1 -= rows[-1]
        if len(sizes) >= 2 and v == len(sizes) - 1:
            a0 += rows[0]
        out.append((a0, a1))
    return out


class Views:
    """predict_views' record: ``preds`` [B, A_v, 4+nc] fp32 per view (view pixels), ``frames`` (a
    yms.data.Frames per view), ``sizes`` [(H_v, W_v)], ``flips`` (bit 0 left-right, bit 1 up-down) and
    the head's ``strides``."""
    __slots__ = ("preds", "frames", "sizes", "flips", "strides")

    def __init__(self, preds, frames, sizes, flips, strides=(8, 16, 32)):
        self.preds, self.frames = list(preds), list(frames)
        self.sizes, self.flips = [_hw(s) for s in sizes], [int(f) for f in flips]
        self.strides = tuple(strides)

    def rows(self, trim=False):
        if trim:
            return trim_rows(self.sizes, self.strides)
        return [(0, int(p.shape[1])) for p in self.preds]

    def locate(self, row, trim=False):
        """Merged row -> (view, anchor of that view's prediction)."""
        for v, (a0, a1) in enumerate(self.rows(trim)):
            if row < a1 - a0:
                return v, a0 + row
            row -= a1 - a0
        raise IndexError("yms: row beyond the merged tensor")


def _check_views(scales, flips):
    if len(scales) != len(flips):
        raise ValueError("yms: one flip per scale")
    if not 1 <= len(scales) <= MAX_VIEWS:
        raise ValueError(f"yms: 1..{MAX_VIEWS} views")
    if any(int(f) != f or not 0 <= int(f) <= 3 for f in flips):
        raise ValueError("yms: a flip is 0, 1 (left-right), 2 (up-down) or 3 (both)")


def view_plans(shapes, size, flip=0, fill=D.MOSAIC_FILL):
    """Per original (h0, w0) in ``shapes``: (Letterbox, MosaicPlan) of one view of ``size`` = (H, W) --
    the letterbox tile, plus a fliplr / flipud stage on its layer for the flip bits (the matrices
    yms.data.sample_mosaic adds)."""
    H, W = _hw(size)
    out = []
    for h0, w0 in shapes:
        lb = D.Letterbox(h0, w0, H, W)
        plan = lb.plan(0, fill)
        ly = plan.layers[0]
        if flip & 1:
            ly.add([[-1, 0, W - 1], [0, 1, 0], [0, 0, 1]], W, H, D.AUG_CLAMP, "fliplr")
        if flip & 2:
            ly.add([[1, 0, 0], [0, -1, H - 1], [0, 0, 1]], W, H, D.AUG_CLAMP, "flipud")
        out.append((lb, plan))
    return out


def view_batch(images, size, flip=0, fill=D.MOSAIC_FILL, mean=D.IMAGENET_MEAN, std=D.IMAGENET_STD,
               dtype=torch.float32):
    """One view's input: device HWC uint8 originals -> ([B, 3, H, W], Frames), one mosaic_normalize
    launch.  The frames are the letterbox's; the flip is undone by merge_views from its bits."""
    pairs = view_plans([tuple(im.shape[:2]) for im in images], size, flip, fill)
    x = D.mosaic_normalize([[im] for im in images], [p for _, p in pairs], _hw(size), mean, std, dtype)
    return x, D.Frames([lb.frame for lb, _ in pairs], images[0].device)


def predict_views(model, images, size=640, scales=(1.0, 0.83, 0.67), flips=(0, 1, 0), fill=D.MOSAIC_FILL,
                  mean=D.IMAGENET_MEAN, std=D.IMAGENET_STD, dtype=torch.float32):
    """Run ``model`` (eval mode) on every view of the device HWC uint8 ``images`` -> :class:`Views`.
    View v has size view_sizes(size, scales)[v] and flip bits flips[v]; each original is letterboxed
    directly into it (see the module docstring: not ultralytics' resize of the letterboxed tensor)."""
    scales, flips = tuple(scales), tuple(flips)
    _check_views(scales, flips)
    if not images:
        raise ValueError("yms: empty batch")
    if model.training:
        raise RuntimeError("yms: predict_views needs the model in eval mode")
    info = getattr(getattr(model, "head", None), "yms_decode_info", None)
    strides = tuple(int(s) for s in info()["strides"]) if info is not None else (8, 16, 32)
    sizes = view_sizes(size, scales, max(strides))
    preds, frames = [], []
    with torch.no_grad():
        for sz, fl in zip(sizes, flips):
            x, fr = view_batch(images, sz, int(fl), fill, mean, std, dtype)
            preds.append(model(x).float())
            frames.append(fr)
    return Views(preds, frames, sizes, flips, strides)


def merge_views(preds, frames, sizes, flips, rows=None):
    """Decoded predictions of several views of the same B images (preds[v] [B, A_v, 4+nc] fp32, boxes
    in the pixels of an sizes[v] = (H_v, W_v) input that was flipped by flips[v]; frames[v] a Frames
    or a [B, 6] device tensor) -> [B, sum rows, 4+nc] in original-image pixels, unclipped, scores
    untouched: yms_tta_merge, one launch, no host sync.  rows[v] = (a0, a1) takes a row range of view
    v (default: all).  The views may come from different models (an ensemble) as long as they share
    the images and the classes."""
    nv = len(preds)
    if not 1 <= nv <= MAX_VIEWS or not len(frames) == len(sizes) == len(flips) == nv:
        raise ValueError(f"yms: merge_views takes 1..{MAX_VIEWS} views with one frames, size and flip each")
    if rows is None:
        rows = [(0, int(p.shape[1])) for p in preds]
    if len(rows) != nv:
        raise ValueError("yms: one row range per view")
    ops._cuda(*preds)
    dev = preds[0].device
    if preds[0].dim() != 3 or preds[0].shape[2] < 5:
        raise ValueError("yms: merge_views expects [B, A, 4+nc] predictions")
    B, no = int(preds[0].shape[0]), int(preds[0].shape[2])
    ps, fs = [], []
    for p, f, (a0, a1), fl in zip(preds, frames, rows, flips):
        if p.dim() != 3 or p.shape[0] != B or p.shape[2] != no or p.device != dev:
            raise ValueError("yms: the views' predictions must share batch, classes and device")
        if not 0 <= a0 < a1 <= p.shape[1]:
            raise ValueError("yms: a view's row range must be a non-empty part of its rows")
        if int(fl) != fl or not 0 <= int(fl) <= 3:
            raise ValueError("yms: a flip is 0, 1 (left-right), 2 (up-down) or 3 (both)")
        f = getattr(f, "tensor", f)
        ops._cuda(f)
        if tuple(f.shape) != (B, 6) or f.dtype != torch.float32 or f.device != dev:
            raise ValueError("yms: frames must be [B, 6] fp32 tensors on the predictions' device")
        ps.append(p.detach().float().contiguous())
        fs.append(f.contiguous())
    R = sum(a1 - a0 for a0, a1 in rows)
    if R * (no - 4) >= 2 ** 31:
        raise ValueError("yms: merged rows * nc must stay below 2^31")
    hw = [_hw(s) for s in sizes]
    out = torch.empty((B, R, no), dtype=torch.float32, device=dev)
    P, I = ctypes.c_void_p * nv, ctypes.c_int * nv
    L.call("yms_tta_merge", B, no - 4, nv, P(*[p.data_ptr() for p in ps]), I(*[int(p.shape[1]) for p in ps]),
           I(*[int(r[0]) for r in rows]), I(*[int(r[1]) for r in rows]), I(*[h for h, _ in hw]),
           I(*[w for _, w in hw]), I(*[int(f) for f in flips]), P(*[f.data_ptr() for f in fs]), out.data_ptr(),
           L.stream_ptr(dev))
    return out


def identity_frames(frames):
    """[B, 6] device frames (1, 1, 0, 0, w0, h0) from a view's frames: detect's un-map then only clips
    to each original image.  Device ops only."""
    f = getattr(frames, "tensor", frames)
    out = torch.zeros_like(f)
    out[:, :2] = 1.0
    out[:, 4:] = f[:, 4:]
    return out


def detect_views(views, trim=False, **detect_kwargs):
    """merge_views, then ``yms.ops.detect`` on the merged tensor with identity frames -> Detections in
    original-image coordinates, clipped to each image.  ``trim`` drops trim_rows' levels.  Every
    keyword of detect passes through (``vote=True`` for box voting); ``Detections.anchors`` are merged
    rows (``views.locate``)."""
    if "frames" in detect_kwargs:
        raise ValueError("yms: detect_views supplies the frames itself")
    merged = merge_views(views.preds, views.frames, views.sizes, views.flips, views.rows(trim))
    return ops.detect(merged, frames=identity_frames(views.frames[0]), **detect_kwargs)


def detect_tta(model, images, size=640, scales=(1.0, 0.83, 0.67), flips=(0, 1, 0), trim=False,
               fill=D.MOSAIC_FILL, mean=D.IMAGENET_MEAN, std=D.IMAGENET_STD, dtype=torch.float32,
               **detect_kwargs):
    """detect_views(predict_views(...)): the whole multi-view inference of a batch of device HWC uint8
    originals -> Detections in original-image coordinates.  No host synchronisation beyond the frames
    upload that letterbox_normalize also does, once per view.  Parity with ultralytics' augment=True /
    mmyolo's tta_model UNPINNED (module docstring)."""
    views = predict_views(model, images, size, scales, flips, fill, mean, std, dtype)
    return detect_views(views, trim, **detect_kwargs)
