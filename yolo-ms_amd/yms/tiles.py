"""Tiled (sliced) inference around ``yms.ops.detect`` for images much larger than the model's input:
every image is cut into overlapping windows at native resolution, each window is drawn into one
``tile`` x ``tile`` input, all inputs run through the model, the tiles' decoded predictions are mapped
back to their image and gathered into one tensor (one launch, csrc/tile.hip yms_tile_merge) and ONE
detect -- candidates, NMS, max_det, optionally box voting -- finishes.  SAHI popularised the scheme; it
is not installed, and these are this package's semantics, not a port: parity with SAHI is UNPINNED, as
parity with ultralytics is for ``detect`` and ``yms.tta``.  No accuracy effect is claimed.

The grid (``slice_grid``).  span = tile / zoom source pixels per window side (it must be an integer),
step = span - int(span * overlap) with 0 <= overlap < 1.  Per axis the window starts are 0, step,
2 step, ... while the previous window has not reached the image end; a window that would cross the end
is shifted back so that it ends on the border (start = max(0, size - span)) and is dropped if it then
equals the previous one (under the loop rule just stated the previous window always ends before the
border, so the guard never fires; it is kept as part of the rule).  An axis shorter than span gets the
single window [0, size) and the rest of the tile is fill.  Windows are (x0, y0, x1, y1), row-major.

The slots (``tile_plans``).  With ``full_view`` slot 0 of an image is the whole image letterboxed into
tile x tile (yms.data.Letterbox, its frame, no bounds); then one slot per window, drawn 1:1 (``zoom`` =
1) by the mosaic kernel as a one-tile MosaicPlan on a tile x tile canvas: nw = round(w0 zoom), nh =
round(h0 zoom), ox = -x0 zoom, oy = -y0 zoom, rect = the window's extent on the canvas, fill
MOSAIC_FILL.  The slot's frame is (zoom, zoom, -x0 zoom, -y0 zoom): orig = (v - pad) / gain.

Suppression (``edge``).  A box that a tile's cut has truncated is a bad box of an object that a
neighbouring tile (the overlap) or the full view sees whole.  With ``edge`` = e (pixels of the tile
input, >= 0) a row is suppressed when its box crosses a bound: lo_x = e where x0 > 0 (else -inf), hi_x
= (x1 - x0) zoom - e where x1 < w0 (else +inf), the same in y -- only sides that are cuts, never the
image's own border.  Comparisons are strict (a side on the bound stays).  A suppressed row keeps its
place with every score -1, which no ``conf`` >= 0 admits.  ``edge=None`` (default) suppresses nothing.
Use it with ``full_view=True`` and an overlap wider than the objects that matter, or objects larger
than the overlap are lost at every cut.

Rows.  All inputs share one size, hence one row count A (level by level, finest first).  Slot s of an
image owns merged rows [s A, (s + 1) A); S is the largest slot count in the batch and an image with
fewer slots has empty ones at the end (boxes 0, scores -1).  ``Detections.anchors`` of ``detect_tiles``
are merged rows; ``Tiles.locate`` maps one back to (slot, window, anchor).

Limits: at most 65535 images per call, S A nc < 2^31 (detect's limit on the merged rows)."""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib as L
from . import data as D
from . import ops

INF = float("inf")
# yms_tile_slot (include/yms.h): 48-byte records
SLOT_DTYPE = np.dtype([("tile", np.int32), ("gain_x", np.float32), ("gain_y", np.float32), ("pad_x", np.float32),
                       ("pad_y", np.float32), ("lo_x", np.float32), ("lo_y", np.float32), ("hi_x", np.float32),
                       ("hi_y", np.float32), ("reserved", np.int32, 3)])
MAX_IMAGES = 65535


def _span_step(tile, overlap, zoom):
    tile = int(tile)
    if tile < 1:
        raise ValueError("yms: tile must be a positive size")
    if not zoom > 0:
        raise ValueError("yms: zoom must be positive")
    if not 0 <= overlap < 1:
        raise ValueError("yms: overlap must be in [0, 1)")
    span = tile / zoom
    if span != int(span) or span < 1:
        raise ValueError("yms: tile / zoom must be a whole number of source pixels")
    span = int(span)
    return span, span - int(span * overlap)


def _axis(size, span, step):
    if size <= span:
        return [(0, size)]
    out, s = [], 0
    while True:
        if s + span >= size:                                   # reaches or would cross the end
            s = max(0, size - span)
            if not out or out[-1][0] != s:
                out.append((s, s + span))
            return out
        out.append((s, s + span))
        s += step


def slice_grid(h0, w0, tile, overlap=0.2, zoom=1.0):
    """Source windows [(x0, y0, x1, y1)] of an h0 x w0 image, row-major (module docstring: the grid)."""
    h0, w0 = int(h0), int(w0)
    if h0 < 1 or w0 < 1:
        raise ValueError("yms: slice_grid needs a positive image size")
    span, step = _span_step(tile, overlap, zoom)
    return [(x0, y0, x1, y1) for y0, y1 in _axis(h0, span, step) for x0, x1 in _axis(w0, span, step)]


class Slot:
    """One slot of an image: ``plan`` (the MosaicPlan that draws its input from the image), ``frame``
    (gain_x, gain_y, pad_x, pad_y), ``bounds`` (lo_x, lo_y, hi_x, hi_y) and ``window`` (None: the full
    view)."""
    __slots__ = ("plan", "frame", "bounds", "window")

    def __init__(self, plan, frame, bounds, window):
        self.plan, self.frame, self.bounds, self.window = plan, tuple(frame), tuple(bounds), window


def tile_plans(shapes, tile, overlap=0.2, zoom=1.0, full_view=True, edge=None, fill=D.MOSAIC_FILL):
    """Per original (h0, w0) in ``shapes`` the list of its :class:`Slot` (module docstring: the slots,
    suppression)."""
    tile = int(tile)
    _span_step(tile, overlap, zoom)
    if edge is not None and not edge >= 0:
        raise ValueError("yms: edge must be None or >= 0")
    out = []
    for h0, w0 in shapes:
        h0, w0 = int(h0), int(w0)
        slots = []
        if full_view:
            lb = D.Letterbox(h0, w0, tile, tile)
            slots.append(Slot(lb.plan(0, fill), lb.frame[:4], (-INF, -INF, INF, INF), None))
        for x0, y0, x1, y1 in slice_grid(h0, w0, tile, overlap, zoom):
            ly = D.MosaicLayer(tile, tile, fill=fill)
            rect = (0, 0, min(tile, round((x1 - x0) * zoom)), min(tile, round((y1 - y0) * zoom)))
            ly.tiles = [D.MosaicTile(0, h0, w0, max(1, round(w0 * zoom)), max(1, round(h0 * zoom)), -x0 * zoom,
                                     -y0 * zoom, rect)]
            ly.applied.append("tile")
            bounds = (-INF, -INF, INF, INF)
            if edge is not None:
                bounds = (edge if x0 > 0 else -INF, edge if y0 > 0 else -INF,
                          (x1 - x0) * zoom - edge if x1 < w0 else INF, (y1 - y0) * zoom - edge if y1 < h0 else INF)
            slots.append(Slot(D.MosaicPlan([ly]), (zoom, zoom, -x0 * zoom, -y0 * zoom), bounds, (x0, y0, x1, y1)))
        out.append(slots)
    return out


def slot_table(plans, S=None):
    """Host table of yms_tile_slot records [n, S] for ``plans`` (tile_plans' result): tile inputs are
    numbered image by image, slot by slot; slots beyond an image's own are empty (tile -1)."""
    S = max(len(p) for p in plans) if S is None else S
    tab = np.zeros((len(plans), S), SLOT_DTYPE)
    tab["tile"] = -1
    tab["gain_x"] = tab["gain_y"] = 1.0
    tab["lo_x"] = tab["lo_y"] = -INF
    tab["hi_x"] = tab["hi_y"] = INF
    t = 0
    for b, slots in enumerate(plans):
        for s, sl in enumerate(slots):
            tab[b, s] = (t, *sl.frame, *sl.bounds, (0, 0, 0))
            t += 1
    return tab


class Tiles:
    """predict_tiles' record: ``pred`` [T_pad, A, 4+nc] fp32 (tile-input pixels; inputs beyond the
    last real one are blank padding that no table entry names), ``table`` (device uint8 view of the
    [n, S] yms_tile_slot records) and ``table_host`` (the same, numpy), ``windows`` per image,
    ``shapes`` [(h0, w0)], ``slots`` (= S), ``full_view``, ``tile`` and the head's ``strides``."""
    __slots__ = ("pred", "table", "table_host", "windows", "shapes", "slots", "full_view", "tile", "strides")

    def __init__(self, pred, table, table_host, windows, shapes, slots, full_view, tile, strides=(8, 16, 32)):
        self.pred, self.table, self.table_host = pred, table, table_host
        self.windows, self.shapes, self.slots = windows, shapes, int(slots)
        self.full_view, self.tile, self.strides = bool(full_view), int(tile), tuple(strides)

    def locate(self, image, row):
        """Merged row of ``image`` -> (slot, window (x0, y0, x1, y1) or None for the full view, anchor
        of that tile's prediction)."""
        A = int(self.pred.shape[1])
        slot, anchor = divmod(int(row), A)
        k = slot - int(self.full_view)
        if row < 0 or k >= len(self.windows[image]):
            raise IndexError("yms: row beyond the image's slots")
        return slot, (None if k < 0 else self.windows[image][k]), anchor


def _blank_plan(tile, fill, shape):
    """An all-fill input: one tile (over an image of ``shape``, never sampled) with an empty rect."""
    ly = D.MosaicLayer(tile, tile, fill=fill)
    ly.tiles = [D.MosaicTile(0, shape[0], shape[1], shape[1], shape[0], 0, 0, (0, 0, 0, 0))]
    return D.MosaicPlan([ly])


def predict_tiles(model, images, tile=640, overlap=0.2, zoom=1.0, full_view=True, edge=None, tile_batch=32,
                  fill=D.MOSAIC_FILL, mean=D.IMAGENET_MEAN, std=D.IMAGENET_STD, dtype=torch.float32):
    """Run ``model`` (eval mode) on every tile of the device HWC uint8 ``images`` (any sizes) ->
    :class:`Tiles`.  All tiles of all images are drawn by mosaic_normalize in chunks of exactly
    ``tile_batch`` inputs -- the last chunk padded with blank all-fill inputs, so the model only ever
    sees one batch shape -- and each chunk's output is stored into one preallocated buffer.  The slot
    table is uploaded once, from pinned memory."""
    if model.training:
        raise RuntimeError("yms: predict_tiles needs the model in eval mode")
    info = getattr(getattr(model, "head", None), "yms_decode_info", None)
    strides = tuple(int(s) for s in info()["strides"]) if info is not None else (8, 16, 32)
    tile, tile_batch = int(tile), int(tile_batch)
    if tile < 1 or tile % max(strides) != 0:
        raise ValueError(f"yms: tile must be a positive multiple of the head's largest stride {max(strides)}")
    if tile_batch < 1:
        raise ValueError("yms: tile_batch must be at least 1")
    if not images:
        raise ValueError("yms: empty batch")
    if len(images) > MAX_IMAGES:
        raise ValueError(f"yms: at most {MAX_IMAGES} images per call")
    shapes = [(int(im.shape[0]), int(im.shape[1])) for im in images]
    plans = tile_plans(shapes, tile, overlap, zoom, full_view, edge, fill)
    ops._cuda(*images)
    dev = images[0].device
    host = slot_table(plans)
    inputs = [(im, sl.plan) for im, slots in zip(images, plans) for sl in slots]
    T = len(inputs)
    T_pad = math.ceil(T / tile_batch) * tile_batch
    inputs += [(images[0], _blank_plan(tile, fill, shapes[0]))] * (T_pad - T)
    pinned = torch.from_numpy(host.reshape(-1).view(np.uint8)).pin_memory()
    table = pinned.to(dev, non_blocking=True)
    pred = None
    with torch.no_grad():
        for k in range(0, T_pad, tile_batch):
            chunk = inputs[k:k + tile_batch]
            x = D.mosaic_normalize([[im] for im, _ in chunk], [p for _, p in chunk], (tile, tile), mean, std, dtype)
            y = model(x)
            if pred is None:
                if y.dim() != 3 or y.shape[0] != tile_batch or y.shape[2] < 5:
                    raise ValueError("yms: the model must return [tile_batch, A, 4+nc] decoded predictions")
                pred = torch.empty((T_pad, int(y.shape[1]), int(y.shape[2])), dtype=torch.float32, device=dev)
            pred[k:k + tile_batch] = y
    return Tiles(pred, table, host, [[sl.window for sl in slots if sl.window is not None] for slots in plans],
                 shapes, host.shape[1], full_view, tile, strides)


def merge_slots(pred, table, n, S):
    """yms_tile_merge on raw tensors: ``pred`` [T, A, 4+nc] fp32 and a device ``table`` of n * S
    yms_tile_slot records (uint8 bytes) -> [n, S * A, 4+nc].  One launch, no host sync."""
    ops._cuda(pred, table)
    if pred.dim() != 3 or pred.shape[2] < 5 or pred.dtype != torch.float32 or not pred.is_contiguous():
        raise ValueError("yms: merge expects contiguous [T, A, 4+nc] fp32 predictions")
    n, S = int(n), int(S)
    if table.dtype != torch.uint8 or not table.is_contiguous() or table.numel() != n * S * SLOT_DTYPE.itemsize \
            or table.device != pred.device:
        raise ValueError("yms: the slot table must hold n * S 48-byte records on the predictions' device")
    T, A, no = (int(v) for v in pred.shape)
    if not 1 <= n <= MAX_IMAGES or S < 1:
        raise ValueError(f"yms: 1..{MAX_IMAGES} images with at least one slot each")
    if S * A * (no - 4) >= 2 ** 31:
        raise ValueError("yms: merged rows * nc must stay below 2^31")
    out = torch.empty((n, S * A, no), dtype=torch.float32, device=pred.device)
    L.call("yms_tile_merge", n, S, A, no - 4, T, pred.data_ptr(), table.data_ptr(), out.data_ptr(),
           L.stream_ptr(pred.device))
    return out


def merge_tiles(tiles):
    """The tiles' predictions -> [B, S * A, 4+nc] in original-image pixels, unclipped; suppressed rows
    and empty slots carry scores of -1 (module docstring).  One launch, no host sync."""
    return merge_slots(tiles.pred, tiles.table, len(tiles.shapes), tiles.slots)


def detect_tiles(model, images, tile=640, overlap=0.2, zoom=1.0, full_view=True, edge=None, tile_batch=32,
                 fill=D.MOSAIC_FILL, mean=D.IMAGENET_MEAN, std=D.IMAGENET_STD, dtype=torch.float32, **detect_kwargs):
    """ops.detect(merge_tiles(predict_tiles(...)), frames=(1, 1, 0, 0, w0, h0) per image, **detect_kwargs)
    -> Detections in original-image pixels, clipped to each image.  Every keyword of detect passes
    through (``vote=True`` for box voting) except ``frames``; ``Detections.anchors`` are merged rows
    (``Tiles.locate``).  Parity with SAHI UNPINNED (module docstring)."""
    if "frames" in detect_kwargs:
        raise ValueError("yms: detect_tiles supplies the frames itself")
    tiles = predict_tiles(model, images, tile, overlap, zoom, full_view, edge, tile_batch, fill, mean, std, dtype)
    frames = D.Frames([(1.0, 1.0, 0.0, 0.0, w0, h0) for h0, w0 in tiles.shapes], tiles.pred.device)
    return ops.detect(merge_tiles(tiles), frames=frames, **detect_kwargs)
