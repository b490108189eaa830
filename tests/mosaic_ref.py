"""numpy fp32 replay of csrc/preprocess.hip mosaic_normalize_kernel for one record -- TEST
INFRASTRUCTURE ONLY.  The kernel is compiled without FMA contraction and evaluates plain fp32
operations in source order; this evaluates the same operations in the same order, on the values
the record holds (fp32), with oracle.preprocess_ref's HSV and border helpers.  Parity with
ultralytics / cv2 is unpinned (neither is installed); this pins the kernel to its stated semantics.
"""
from __future__ import annotations

import numpy as np

from oracle.preprocess_ref import CONSTANT, REFLECT101, F32, _reflect101, hsv_shift8
from yms import data as D


class FakeImage:
    """What yms.data.mosaic_struct asks of a device image, for a host array."""

    def __init__(self, h, w):
        self.shape = (h, w, 3)

    def data_ptr(self):
        return 0

    def stride(self, d):
        return (self.shape[1] * 3, 3, 1)[d]


def record_of(plan, images):
    """-> (layers, r) as the kernel reads them: the numbers of yms.data.mosaic_struct's record (fp32,
    taken from the ctypes record itself) with each tile's host image in place of its pointer.
    plan: MosaicPlan over the image list ``images``, or a plain AugPlan over its one image."""
    images = list(images) if isinstance(images, (list, tuple)) else [images]
    rec = D.mosaic_struct(plan, [FakeImage(*im.shape[:2]) for im in images])
    srcs = [[t.src for t in ly.tiles] for ly in plan.layers] if isinstance(plan, D.MosaicPlan) else [[0]]
    layers = []
    for lr, src in zip(rec.layer[:rec.nlayer], srcs):
        stages = [(np.array(lr.st[k].m[:], F32), lr.st[k].in_w, lr.st[k].in_h, lr.st[k].border)
                  for k in range(lr.nst)]
        tiles = [(images[s], (q.x0, q.y0, q.x1, q.y1), F32(q.sx), F32(q.sy), F32(q.tx), F32(q.ty))
                 for q, s in zip(lr.tile[:lr.ntile], src)]
        layers.append({"fill": F32(lr.fill), "do_hsv": lr.do_hsv, "hsv": tuple(F32(v) for v in lr.hsv[:]),
                       "stages": stages, "tiles": tiles})
    return layers, F32(rec.r)


def _layer(ly, out_h, out_w):
    """[out_h * out_w, 3] fp32 pixel values (0..255) of one layer."""
    oy, ox = np.meshgrid(np.arange(out_h, dtype=F32), np.arange(out_w, dtype=F32), indexing="ij")
    x, y = ox.reshape(-1), oy.reshape(-1)
    blank = np.zeros(x.shape, bool)
    for m, in_w, in_h, border in reversed(ly["stages"]):
        X = m[0] * x + m[1] * y + m[2]
        Y = m[3] * x + m[4] * y + m[5]
        Z = m[6] * x + m[7] * y + m[8]
        with np.errstate(divide="ignore", invalid="ignore"):
            x, y = (X / Z).astype(F32), (Y / Z).astype(F32)
        bad = ~((np.abs(x) < F32(1e7)) & (np.abs(y) < F32(1e7)))
        blank |= bad
        x = np.where(bad, F32(0), x)
        y = np.where(bad, F32(0), y)
        if border == REFLECT101:
            x, y = _reflect101(x, in_w), _reflect101(y, in_h)
        else:
            if border == CONSTANT:
                blank |= (x < F32(-0.5)) | (y < F32(-0.5)) | (x > F32(in_w) - F32(0.5)) | (y > F32(in_h) - F32(0.5))
            x = np.minimum(np.maximum(x, F32(0)), F32(in_w - 1)).astype(F32)
            y = np.minimum(np.maximum(y, F32(0)), F32(in_h - 1)).astype(F32)
    # a pixel that went blank in a later stage kept walking here on a stand-in coordinate; it is fill
    ix = np.floor(x + F32(0.5)).astype(np.int64)
    iy = np.floor(y + F32(0.5)).astype(np.int64)
    sel = np.full(x.shape, -1)
    for t, (_, (x0, y0, x1, y1), *_m) in enumerate(ly["tiles"]):
        sel = np.where((ix >= x0) & (ix < x1) & (iy >= y0) & (iy < y1), t, sel)
    sel = np.where(blank, -1, sel)
    fill = np.full((1, 3), ly["fill"], F32)
    if ly["do_hsv"] & 2:
        fill = hsv_shift8(fill, ly["hsv"])
    v = np.broadcast_to(fill, (x.size, 3)).astype(F32).copy()
    for t, (img, _, sx, sy, tx, ty) in enumerate(ly["tiles"]):
        on = sel == t
        if not on.any():
            continue
        h, w = img.shape[:2]
        xs = (sx * x[on] + tx).astype(F32)
        ys = (sy * y[on] + ty).astype(F32)
        xs = np.minimum(np.maximum(xs, F32(0)), F32(w - 1)).astype(F32)
        ys = np.minimum(np.maximum(ys, F32(0)), F32(h - 1)).astype(F32)
        x0 = np.minimum(np.floor(xs).astype(np.int64), w - 1)
        y0 = np.minimum(np.floor(ys).astype(np.int64), h - 1)
        fx = (xs - x0.astype(F32)).astype(F32)[:, None]
        fy = (ys - y0.astype(F32)).astype(F32)[:, None]
        x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
        src = img.astype(F32)
        taps = [src[y0, x0], src[y0, x1], src[y1, x0], src[y1, x1]]
        if ly["do_hsv"] & 1:
            taps = [hsv_shift8(q, ly["hsv"]) for q in taps]
        top = taps[0] + fx * (taps[1] - taps[0])
        bot = taps[2] + fx * (taps[3] - taps[2])
        v[on] = (top + fy * (bot - top)).astype(F32)
    return v, sel


def mosaic_normalize(layers, r, out_h, out_w, mean, std, return_sel=False):
    """(layers, r) of record_of -> CHW float32 normalised image (and, on request, each layer's
    per-pixel tile index, -1 = fill, as [out_h, out_w] arrays)."""
    vals = [_layer(ly, out_h, out_w) for ly in layers]
    v = vals[0][0]
    for b, _ in vals[1:]:
        v = (b + F32(r) * (v - b)).astype(F32)
    mean, std = np.asarray(mean, F32), np.asarray(std, F32)
    sc = F32(1) / (F32(255) * std)
    bb = -mean / std
    out = (v * sc + bb).reshape(out_h, out_w, 3).transpose(2, 0, 1).astype(F32)
    if return_sel:
        return out, [s.reshape(out_h, out_w) for _, s in vals]
    return out
