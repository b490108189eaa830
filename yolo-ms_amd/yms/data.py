"""Input pipeline: the reference's COCO dataset + collate (yolov8/tools/dataset.py)
with the per-sample Resize / Normalize / ToTensorV2 moved to the GPU.

The reference decodes each image with PIL, transforms it on the host with albumentations (cv2
bilinear resize, normalize, HWC -> CHW fp32) and stacks fp32 tensors in ``collate_fn``
(dataset.py:143-267).  Here the host only decodes (PIL) and parses the annotations; the uint8 RGB
images travel to the GPU as decoded (a quarter of the fp32 bytes over PCIe, pinned + async), and
one ``yms_resize_normalize`` launch produces the whole ``[B, 3, H, W]`` batch (csrc/preprocess.hip).
Targets keep the reference's format: per image ``[n, 5]`` = (class, cx, cy, w, h) normalised,
collated to ``[M, 6]`` with the batch index first (dataset.py:235-267).

Annotations are read with the ``json`` module in pycocotools' orders (image ids sorted, category
ids in file order, annotations per image in file order); pycocotools, albumentations and cv2 are
not installed here.

Training augmentation (dataset.py:84-131, the albumentations chain HueSaturationValue -> Rotate ->
ShiftScaleRotate -> RandomScale -> Affine(shear) -> Perspective -> HorizontalFlip / VerticalFlip ->
Resize -> Normalize with BboxParams(coco, min_visibility 0.1, min_area 1)) is restated:
``sample_augmentation`` draws each image's transforms on the host in that order with
albumentations' probabilities and parameter distributions, composes them into a chain of
pixel-coordinate stages, and ``augment_normalize`` applies the whole chain plus Normalize in ONE
GPU launch (csrc/preprocess.hip: one bilinear sample per output pixel instead of one resampling
per transform); ``transform_boxes`` moves the COCO boxes through the same stages (corner
envelopes, clipped once at the end, then the visibility / area filters).  albumentations and cv2
are not installed, so parity with them is UNPINNED; the GPU kernel is pinned
to the restatement in oracle/preprocess_ref.py.

Mosaic and MixUp (the config's ``mosaic`` / ``mixup`` keys, which the reference's transform list
never reads) are opt-in through ``COCODataset(..., mosaic=True)``: YOLOv5's semantics restated,
sampled on the host (``sample_mosaic``, ``mosaic_boxes``) and composed on the GPU in one launch
(``mosaic_normalize``); see the section below.

Evaluation with the published AP protocol is opt-in too: ``letterbox_normalize`` (ultralytics'
LetterBox restated, drawn by the Mosaic kernel) returns the batch and its frames, which
``yms.ops.detect(frames=...)`` uses to map boxes back to the original images;
``COCODataset(..., is_train=False, letterbox=True)`` + ``collate_to_gpu`` is the loader for it.
"""
from __future__ import annotations

import ctypes
import json
import os
from collections import defaultdict

import numpy as np
import torch

from . import _lib as L

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


class PrepImage(ctypes.Structure):
    """csrc/preprocess.hip PrepImage: one decoded HWC uint8 image on the device."""
    _fields_ = [("src", ctypes.c_void_p), ("h", ctypes.c_int), ("w", ctypes.c_int), ("pitch", ctypes.c_int),
                ("flags", ctypes.c_int)]


def to_device(images, device, pin=True):
    """uint8 HWC numpy / torch images -> device uint8 tensors (pinned host staging, async copies)."""
    out = []
    for im in images:
        t = torch.as_tensor(np.ascontiguousarray(im)) if not isinstance(im, torch.Tensor) else im.contiguous()
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
            raise ValueError(f"yms: expected HWC uint8 RGB images, got {tuple(t.shape)} {t.dtype}")
        if t.device.type != "cuda":
            if pin:
                t = t.pin_memory()
            t = t.to(device, non_blocking=True)
        out.append(t)
    return out


def resize_normalize(images, size, mean=IMAGENET_MEAN, std=IMAGENET_STD, flips=None, dtype=torch.float32):
    """Device HWC uint8 images (any sizes) -> [B, 3, H, W] normalised batch on the GPU
    (A.Resize(INTER_LINEAR) + A.Normalize + ToTensorV2 + torch.stack).  flips: per-image bit 0 =
    horizontal, bit 1 = vertical (applied before the resize, as in the training transform)."""
    if not images:
        raise ValueError("yms: empty batch")
    dev = images[0].device
    if dev.type != "cuda":
        raise RuntimeError("yms: resize_normalize runs on ROCm GPU tensors only (no CPU fallback)")
    H, W = size
    n = len(images)
    tab = (PrepImage * n)()
    for i, im in enumerate(images):
        if im.device != dev or im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3 or im.stride(2) != 1 \
                or im.stride(1) != 3:
            raise ValueError("yms: images must be contiguous HWC uint8 RGB tensors on one device")
        tab[i] = PrepImage(im.data_ptr(), im.shape[0], im.shape[1], im.stride(0), int(flips[i]) if flips else 0)
    tab_dev = torch.frombuffer(bytearray(tab), dtype=torch.uint8).to(dev, non_blocking=False)
    out = torch.empty((n, 3, H, W), dtype=dtype, device=dev)
    L.call("yms_resize_normalize", L.dtype_code(dtype), n, tab_dev.data_ptr(), H, W,
           (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std), out.data_ptr(), L.stream_ptr(dev))
    # keep the images and the table alive until the kernel has read them (stream-ordered frees)
    for im in images:
        im.record_stream(torch.cuda.current_stream(dev))
    tab_dev.record_stream(torch.cuda.current_stream(dev))
    return out


# ------------------------------------------------------------------------------------------
# training augmentation (dataset.py:84-131)
# ------------------------------------------------------------------------------------------
AUG_REFLECT101, AUG_CLAMP, AUG_CONSTANT = 0, 1, 2
AUG_MAX_STAGES = 8


class AugStage(ctypes.Structure):
    """One geometric stage: m maps OUTPUT pixel-index coordinates to the input frame (in_w x in_h)."""
    _fields_ = [("m", ctypes.c_float * 9), ("in_w", ctypes.c_int), ("in_h", ctypes.c_int),
                ("border", ctypes.c_int), ("pad_", ctypes.c_int)]


class AugImage(ctypes.Structure):
    """csrc/preprocess.hip AugImage (checked against yms_augment_image_bytes())."""
    _fields_ = [("src", ctypes.c_void_p), ("h", ctypes.c_int), ("w", ctypes.c_int), ("pitch", ctypes.c_int),
                ("nst", ctypes.c_int), ("hsv", ctypes.c_float * 3), ("do_hsv", ctypes.c_int),
                ("st", AugStage * AUG_MAX_STAGES)]


class AugPlan:
    """One image's sampled transform: optional HSV shift (LUT units) and geometric stages, each
    (F, in_w, in_h, out_w, out_h, border) with F the 3x3 FORWARD map of pixel-index coordinates
    (input -> output; homogeneous)."""

    def __init__(self, h, w):
        self.src_h, self.src_w = h, w
        self.hsv = None
        self.stages = []
        self.applied = []          # names of the transforms drawn (diagnostics / tests)

    @property
    def frame(self):
        if self.stages:
            return self.stages[-1][3], self.stages[-1][4]
        return self.src_w, self.src_h

    def add(self, F, out_w, out_h, border, name):
        in_w, in_h = self.frame
        self.stages.append((np.asarray(F, np.float64), in_w, in_h, int(out_w), int(out_h), border))
        self.applied.append(name)


def _rot_matrix(cx, cy, deg, scale=1.0):
    """cv2.getRotationMatrix2D(center, angle, scale) as a 3x3 (positive angle = counter-clockwise)."""
    a = np.deg2rad(deg)
    al, be = scale * np.cos(a), scale * np.sin(a)
    return np.array([[al, be, (1 - al) * cx - be * cy], [-be, al, be * cx + (1 - al) * cy], [0, 0, 1]])


def _resize_matrix(in_w, in_h, out_w, out_h):
    """cv2.resize INTER_LINEAR pixel-centre map, input index -> output index."""
    sx, sy = in_w / out_w, in_h / out_h
    return np.array([[1 / sx, 0, 0.5 / sx - 0.5], [0, 1 / sy, 0.5 / sy - 0.5], [0, 0, 1]])


def _homography(src, dst):
    """cv2.getPerspectiveTransform: the 3x3 H with dst ~ H src for four point pairs."""
    A, b = [], []
    for (x, y), (u, v) in zip(src, dst):
        A.append([x, y, 1, 0, 0, 0, -u * x, -u * y])
        A.append([0, 0, 0, x, y, 1, -v * x, -v * y])
        b += [u, v]
    h = np.linalg.solve(np.asarray(A, np.float64), np.asarray(b, np.float64))
    return np.append(h, 1.0).reshape(3, 3)


def sample_augmentation(rng, tp, h, w, out_h, out_w, is_train=True):
    """dataset.py:89-131 for one image of h x w pixels: each transform of the training list is
    drawn with albumentations' probability (p = 0.5; the flips p = fliplr / flipud) and parameter
    distribution, in list order, from the numpy Generator ``rng``; then the final Resize.
    tp: the config's augmentation dict (hsv_h/s/v, degrees, translate, scale, shear, perspective,
    fliplr, flipud)."""
    tp = tp or {}
    plan = AugPlan(h, w)
    if is_train:
        hl, sl, vl = (int(tp.get(k, 0) * 100) for k in ("hsv_h", "hsv_s", "hsv_v"))
        if tp.get("hsv_h", 0) > 0 or tp.get("hsv_s", 0) > 0 or tp.get("hsv_v", 0) > 0:
            if rng.random() < 0.5:     # A.HueSaturationValue(hue_shift_limit, sat_shift_limit, val_shift_limit)
                plan.hsv = (rng.uniform(-hl, hl), rng.uniform(-sl, sl), rng.uniform(-vl, vl))
                plan.applied.append("hsv")
        if tp.get("degrees", 0) > 0 and rng.random() < 0.5:       # A.Rotate(limit=degrees), reflect-101
            fw, fh = plan.frame
            ang = rng.uniform(-tp["degrees"], tp["degrees"])
            plan.add(_rot_matrix((fw - 1) / 2, (fh - 1) / 2, ang), fw, fh, AUG_REFLECT101, "rotate")
        if tp.get("translate", 0) > 0 and rng.random() < 0.5:     # A.ShiftScaleRotate(shift only), reflect-101
            fw, fh = plan.frame
            t = tp["translate"]
            dx, dy = rng.uniform(-t, t), rng.uniform(-t, t)
            plan.add(np.array([[1, 0, dx * fw], [0, 1, dy * fh], [0, 0, 1]]), fw, fh, AUG_REFLECT101, "shift")
        if tp.get("scale", 0) > 0 and rng.random() < 0.5:         # A.RandomScale(scale_limit): resized frame
            fw, fh = plan.frame
            sc = rng.uniform(1 - tp["scale"], 1 + tp["scale"])
            nw, nh = max(1, int(fw * sc)), max(1, int(fh * sc))
            plan.add(_resize_matrix(fw, fh, nw, nh), nw, nh, AUG_CLAMP, "scale")
        if tp.get("shear", 0) > 0 and rng.random() < 0.5:         # A.Affine(shear x / y in degrees), constant 0
            fw, fh = plan.frame
            shx, shy = (np.tan(np.deg2rad(rng.uniform(-tp["shear"], tp["shear"]))) for _ in range(2))
            cx, cy = (fw - 1) / 2, (fh - 1) / 2
            Sm = np.array([[1, shx, 0], [shy, 1, 0], [0, 0, 1]])
            T0 = np.array([[1, 0, -cx], [0, 1, -cy], [0, 0, 1]])
            T1 = np.array([[1, 0, cx], [0, 1, cy], [0, 0, 1]])
            plan.add(T1 @ Sm @ T0, fw, fh, AUG_CONSTANT, "shear")
        if tp.get("perspective", 0) > 0 and rng.random() < 0.5:   # A.Perspective(scale=(0, p)), keep_size
            fw, fh = plan.frame
            sc = rng.uniform(0, tp["perspective"])
            j = np.mod(np.abs(rng.normal(0, sc, (4, 2))), 0.32)
            quad = [(j[0, 0] * fw, j[0, 1] * fh), ((1 - j[1, 0]) * fw, j[1, 1] * fh),
                    ((1 - j[2, 0]) * fw, (1 - j[2, 1]) * fh), (j[3, 0] * fw, (1 - j[3, 1]) * fh)]
            quad = [(x - 0.5, y - 0.5) for x, y in quad]
            rect = [(0, 0), (fw - 1, 0), (fw - 1, fh - 1), (0, fh - 1)]
            plan.add(_homography(quad, rect), fw, fh, AUG_CONSTANT, "perspective")
        if tp.get("fliplr", 0) > 0 and rng.random() < tp["fliplr"]:
            fw, fh = plan.frame
            plan.add(np.array([[-1, 0, fw - 1], [0, 1, 0], [0, 0, 1]]), fw, fh, AUG_CLAMP, "fliplr")
        if tp.get("flipud", 0) > 0 and rng.random() < tp["flipud"]:
            fw, fh = plan.frame
            plan.add(np.array([[1, 0, 0], [0, -1, fh - 1], [0, 0, 1]]), fw, fh, AUG_CLAMP, "flipud")
    fw, fh = plan.frame
    plan.add(_resize_matrix(fw, fh, out_w, out_h), out_w, out_h, AUG_CLAMP, "resize")
    if len(plan.stages) > AUG_MAX_STAGES:
        raise RuntimeError("yms: augmentation chain longer than AUG_MAX_STAGES")
    return plan


def _fill_stages(st, stages):
    """AugStage records (output -> input frame, the inverse of each forward map) of a plan's stages."""
    for k, (F, in_w, in_h, _, _, border) in enumerate(stages):
        M = np.linalg.inv(F)
        M = M / M[2, 2] if abs(M[2, 2]) > 1e-12 else M
        st[k].m[:] = [float(v) for v in M.reshape(-1)]
        st[k].in_w, st[k].in_h, st[k].border = in_w, in_h, border


def plan_struct(plan, image):
    """AugImage record of one plan over a device HWC uint8 image tensor."""
    rec = AugImage()
    rec.src = image.data_ptr()
    rec.h, rec.w, rec.pitch = image.shape[0], image.shape[1], image.stride(0)
    if (rec.h, rec.w) != (plan.src_h, plan.src_w):
        raise ValueError("yms: augmentation plan sampled for another image size")
    rec.nst = len(plan.stages)
    if plan.hsv is not None:
        rec.do_hsv = 1
        rec.hsv[:] = [float(v) for v in plan.hsv]
    _fill_stages(rec.st, plan.stages)
    return rec


def augment_normalize(images, plans, size, mean=IMAGENET_MEAN, std=IMAGENET_STD, dtype=torch.float32):
    """Device HWC uint8 images + their sampled plans -> [B, 3, H, W] augmented, resized, normalised
    batch in one launch (yms_augment_normalize)."""
    if not images or len(images) != len(plans):
        raise ValueError("yms: one augmentation plan per image")
    dev = images[0].device
    if dev.type != "cuda":
        raise RuntimeError("yms: augment_normalize runs on ROCm GPU tensors only (no CPU fallback)")
    if L.lib().yms_augment_image_bytes() != ctypes.sizeof(AugImage):
        raise RuntimeError("yms: AugImage layout differs from the library's")
    H, W = size
    n = len(images)
    tab = (AugImage * n)()
    for i, (im, pl) in enumerate(zip(images, plans)):
        if im.device != dev or im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3 or im.stride(2) != 1 \
                or im.stride(1) != 3:
            raise ValueError("yms: images must be contiguous HWC uint8 RGB tensors on one device")
        if pl.frame != (W, H):
            raise ValueError("yms: plan's final Resize does not produce the batch size")
        tab[i] = plan_struct(pl, im)
    tab_dev = torch.frombuffer(bytearray(tab), dtype=torch.uint8).to(dev, non_blocking=False)
    out = torch.empty((n, 3, H, W), dtype=dtype, device=dev)
    L.call("yms_augment_normalize", L.dtype_code(dtype), n, tab_dev.data_ptr(), H, W,
           (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std), out.data_ptr(), L.stream_ptr(dev))
    for im in images:
        im.record_stream(torch.cuda.current_stream(dev))
    tab_dev.record_stream(torch.cuda.current_stream(dev))
    return out


def transform_boxes(boxes, labels, plan, min_visibility=0.1, min_area=1.0):
    """COCO [x, y, w, h] pixel boxes of the plan's source image -> [n, 5] targets (class, cx, cy, w, h
    normalised to the final frame).  Each box's corners go through every stage (continuous pixel
    coordinates, X = index + 0.5); the box is the envelope of its transformed corners, clipped to
    the final frame once; BboxParams(min_visibility=0.1, min_area=1) then drop boxes whose clipped
    area is below 10% of the unclipped one or below 1 px, and the reference's final checks apply
    (dataset.py:84-88, :218-228)."""
    out_w, out_h = plan.frame
    rows = []
    for (x, y, w, h), c in zip(boxes, labels):
        P = np.array([[x, y], [x + w, y], [x + w, y + h], [x, y + h]], np.float64) - 0.5
        for F, *_ in plan.stages:
            q = np.c_[P, np.ones(4)] @ F.T
            P = q[:, :2] / q[:, 2:3]
        P = P + 0.5
        x0, y0 = P.min(0)
        x1, y1 = P.max(0)
        area = (x1 - x0) * (y1 - y0)
        cx0, cy0 = min(max(x0, 0.0), out_w), min(max(y0, 0.0), out_h)
        cx1, cy1 = min(max(x1, 0.0), out_w), min(max(y1, 0.0), out_h)
        carea = max(cx1 - cx0, 0.0) * max(cy1 - cy0, 0.0)
        if area <= 0 or carea / area < min_visibility or carea < min_area:
            continue
        bw, bh = cx1 - cx0, cy1 - cy0
        cxn, cyn, wn, hn = (cx0 + bw / 2) / out_w, (cy0 + bh / 2) / out_h, bw / out_w, bh / out_h
        if wn > 1e-3 and hn > 1e-3 and 0 <= cxn <= 1 and 0 <= cyn <= 1 and 0 <= wn <= 1 and 0 <= hn <= 1:
            rows.append([c, cxn, cyn, wn, hn])
    return torch.tensor(rows, dtype=torch.float32) if rows else torch.empty(0, 5)


def flip_targets(t, flags):
    """[n, 5] (class, cx, cy, w, h) normalised targets of a flipped image."""
    t = t.clone()
    if flags & 1:
        t[:, 1] = 1.0 - t[:, 1]
    if flags & 2:
        t[:, 2] = 1.0 - t[:, 2]
    return t


def coco_boxes_to_targets(boxes, labels, img_w, img_h, out_w, out_h):
    """COCO [x, y, w, h] pixel boxes of an (img_w x img_h) image -> [n, 5] targets after the resize to
    (out_w x out_h), with the reference's filters (A.BboxParams min_area = 1 px in the output
    image, dataset.py:85-88; final checks :218-228)."""
    rows = []
    for (x, y, w, h), c in zip(boxes, labels):
        sx, sy = out_w / img_w, out_h / img_h
        xr, yr, wr, hr = x * sx, y * sy, w * sx, h * sy
        if wr * hr < 1.0:
            continue
        cx, cy, wn, hn = (xr + wr / 2) / out_w, (yr + hr / 2) / out_h, wr / out_w, hr / out_h
        if wn > 1e-3 and hn > 1e-3 and 0 <= cx <= 1 and 0 <= cy <= 1 and 0 <= wn <= 1 and 0 <= hn <= 1:
            rows.append([c, cx, cy, wn, hn])
    return torch.tensor(rows, dtype=torch.float32) if rows else torch.empty(0, 5)


# ------------------------------------------------------------------------------------------
# Mosaic and MixUp (opt-in; the published YOLOv5 load_mosaic / random_perspective / mixup, restated)
# ------------------------------------------------------------------------------------------
# The reference's config carries ``mosaic`` and ``mixup`` but its transform list never reads them,
# so the semantics are YOLOv5's.  One LAYER is a canvas of 2W x 2H pixels filled with 114, a centre
# (xc, yc), and four letterbox-resized TILES anchored at the centre (TL's bottom-right corner, TR's
# bottom-left, BL's top-right, BR's top-left) and cropped by the canvas edge only; then ONE
# constant-border stage canvas -> output (M = T S R P C, the border drawn in the fill), the flips
# and the HSV shift (applied to the fill too).  MixUp blends two independent layers,
# b + r (a - b) with r ~ Beta(32, 32), and concatenates their targets.  The GPU evaluates a record
# in one launch (csrc/preprocess.hip mosaic_normalize_kernel): the stage walk of augment_normalize
# plus the tile choice, one bilinear sample of one source per layer.  ultralytics and cv2 are not
# installed: parity with them is UNPINNED; the kernel is pinned to tests/mosaic_ref.py.
MOS_MAX_TILES, MOS_MAX_LAYERS = 4, 2
MOSAIC_FILL = 114.0


class MosTile(ctypes.Structure):
    """One tile: the source image, its canvas rect [x0, x1) x [y0, y1) and the map from a canvas pixel
    index to a source pixel index, xs = sx * x + tx."""
    _fields_ = [("src", ctypes.c_void_p), ("h", ctypes.c_int), ("w", ctypes.c_int), ("pitch", ctypes.c_int),
                ("pad_", ctypes.c_int), ("x0", ctypes.c_int), ("y0", ctypes.c_int), ("x1", ctypes.c_int),
                ("y1", ctypes.c_int), ("sx", ctypes.c_float), ("sy", ctypes.c_float), ("tx", ctypes.c_float),
                ("ty", ctypes.c_float)]


class MosLayer(ctypes.Structure):
    """do_hsv: bit 0 shifts the taps, bit 1 the fill."""
    _fields_ = [("fill", ctypes.c_float), ("nst", ctypes.c_int), ("ntile", ctypes.c_int), ("do_hsv", ctypes.c_int),
                ("hsv", ctypes.c_float * 3), ("pad_", ctypes.c_int), ("st", AugStage * AUG_MAX_STAGES),
                ("tile", MosTile * MOS_MAX_TILES)]


class MosImage(ctypes.Structure):
    """csrc/preprocess.hip MosImage (checked against yms_mosaic_image_bytes()): one output image."""
    _fields_ = [("nlayer", ctypes.c_int), ("r", ctypes.c_float), ("layer", MosLayer * MOS_MAX_LAYERS)]


class MosaicTile:
    """Source ``src`` (index into the sample's image list, h x w pixels) resized to nw x nh with its
    column 0 / row 0 at canvas (ox, oy) -- possibly negative -- and visible in ``rect`` = (x0, y0, x1, y1)."""

    def __init__(self, src, h, w, nw, nh, ox, oy, rect):
        self.src, self.h, self.w, self.nw, self.nh, self.ox, self.oy = src, h, w, nw, nh, ox, oy
        self.rect = tuple(int(v) for v in rect)

    @property
    def map(self):
        """(sx, sy, tx, ty) in float64: the resize's half-pixel rule, canvas index -> source index."""
        sx, sy = self.w / self.nw, self.h / self.nh
        return sx, sy, (0.5 - self.ox) * sx - 0.5, (0.5 - self.oy) * sy - 0.5


class MosaicLayer(AugPlan):
    """One mosaic layer: an AugPlan whose source frame is the canvas (stages, hsv and ``applied`` as
    there), plus the canvas fill, the centre and the tiles in TL, TR, BL, BR order."""

    def __init__(self, canvas_h, canvas_w, fill=MOSAIC_FILL):
        super().__init__(canvas_h, canvas_w)
        self.fill = float(fill)
        self.center = None
        self.tiles = []


class MosaicPlan:
    """One output image: one layer (Mosaic) or two (MixUp, ``r`` the weight of layer 0) over the
    sample's image list; ``applied`` names what was drawn (diagnostics / tests)."""

    def __init__(self, layers, r=1.0):
        self.layers = list(layers)
        self.r = float(r)
        if not 1 <= len(self.layers) <= MOS_MAX_LAYERS:
            raise ValueError("yms: a MosaicPlan has one or two layers")

    @property
    def applied(self):
        return ["mosaic"] + (["mixup"] if len(self.layers) > 1 else []) + [a for ly in self.layers for a in ly.applied]

    @property
    def frame(self):
        return self.layers[0].frame


def mosaic_tiles(sizes, xc, yc, out_h, out_w):
    """The four tiles of sources ``sizes`` = [(h0, w0)] x 4 (TL, TR, BL, BR) about the centre (xc, yc)."""
    tiles = []
    for k, (h0, w0) in enumerate(sizes):
        r = min(out_w / w0, out_h / h0)
        nw, nh = max(1, round(w0 * r)), max(1, round(h0 * r))
        ox = xc - nw if k in (0, 2) else xc
        oy = yc - nh if k in (0, 1) else yc
        rect = (max(ox, 0), max(oy, 0), min(ox + nw, 2 * out_w), min(oy + nh, 2 * out_h))
        tiles.append(MosaicTile(k, h0, w0, nw, nh, ox, oy, rect))
    return tiles


def sample_mosaic(rng, tp, sizes, out_h, out_w, center=None):
    """One mosaic layer over four sources of ``sizes`` = [(h, w)] x 4 for an out_h x out_w output.
    Draws from the numpy Generator ``rng``, in this order (every uniform is drawn even where its
    limit is 0, so the stream does not depend on the config):
      1. xc = int(U(W/2, 3W/2)), yc = int(U(H/2, 3H/2))   (``center`` overrides them after the draw);
      2. one permutation of 0..3: position TL, TR, BL, BR gets source perm[position];
      3. perspective P[2,0], P[2,1] ~ U(-perspective, perspective);
      4. rotation angle ~ U(-degrees, degrees), gain ~ U(1 - scale, 1 + scale);
      5. shear S[0,1], S[1,0] = tan(U(-shear, shear) degrees);
      6. translation U(0.5 - translate, 0.5 + translate) * W, then * H;
      7. the flips, then the HSV shift, each exactly as sample_augmentation draws them.
    The canvas stage's forward matrix is T S R P C with C the translation by (-W, -H)."""
    tp = tp or {}
    W, H = int(out_w), int(out_h)
    ly = MosaicLayer(2 * H, 2 * W)
    xc, yc = int(rng.uniform(W / 2, 3 * W / 2)), int(rng.uniform(H / 2, 3 * H / 2))
    if center is not None:
        xc, yc = (int(v) for v in center)
    ly.center = (xc, yc)
    perm = [int(v) for v in rng.permutation(4)]
    ly.tiles = mosaic_tiles([sizes[k] for k in perm], xc, yc, H, W)
    for t, k in zip(ly.tiles, perm):
        t.src = k
    C = np.array([[1, 0, -W], [0, 1, -H], [0, 0, 1]], np.float64)
    p = tp.get("perspective", 0)
    P = np.eye(3)
    P[2, 0], P[2, 1] = rng.uniform(-p, p), rng.uniform(-p, p)
    deg, sc = tp.get("degrees", 0), tp.get("scale", 0)
    ang = rng.uniform(-deg, deg)
    R = _rot_matrix(0, 0, ang, rng.uniform(1 - sc, 1 + sc))
    sh = tp.get("shear", 0)
    S = np.eye(3)
    S[0, 1] = np.tan(np.deg2rad(rng.uniform(-sh, sh)))
    S[1, 0] = np.tan(np.deg2rad(rng.uniform(-sh, sh)))
    tr = tp.get("translate", 0)
    T = np.eye(3)
    T[0, 2] = rng.uniform(0.5 - tr, 0.5 + tr) * W
    T[1, 2] = rng.uniform(0.5 - tr, 0.5 + tr) * H
    ly.add(T @ S @ R @ P @ C, W, H, AUG_CONSTANT, "affine")
    if p > 0:
        ly.applied.append("perspective")
    if tp.get("fliplr", 0) > 0 and rng.random() < tp["fliplr"]:
        ly.add(np.array([[-1, 0, W - 1], [0, 1, 0], [0, 0, 1]]), W, H, AUG_CLAMP, "fliplr")
    if tp.get("flipud", 0) > 0 and rng.random() < tp["flipud"]:
        ly.add(np.array([[1, 0, 0], [0, -1, H - 1], [0, 0, 1]]), W, H, AUG_CLAMP, "flipud")
    hl, sl, vl = (int(tp.get(k, 0) * 100) for k in ("hsv_h", "hsv_s", "hsv_v"))
    if tp.get("hsv_h", 0) > 0 or tp.get("hsv_s", 0) > 0 or tp.get("hsv_v", 0) > 0:
        if rng.random() < 0.5:
            ly.hsv = (rng.uniform(-hl, hl), rng.uniform(-sl, sl), rng.uniform(-vl, vl))
            ly.applied.append("hsv")
    return ly


def _envelope(P, stages):
    """Corner envelope (x0, y0, x1, y1) of continuous-coordinate corners P [4, 2] after the stages."""
    P = np.asarray(P, np.float64) - 0.5
    for F, *_ in stages:
        q = np.c_[P, np.ones(4)] @ F.T
        P = q[:, :2] / q[:, 2:3]
    P = P + 0.5
    return (*P.min(0), *P.max(0))


def _corners(x0, y0, x1, y1):
    return [[x0, y0], [x1, y0], [x1, y1], [x0, y1]]


def mosaic_boxes(layer, annotations, min_visibility=0.1, min_area=1.0):
    """[n, 5] targets (class, cx, cy, w, h normalised to the output) of one layer.  annotations:
    per image of the sample's list, (COCO [x, y, w, h] pixel boxes, labels).  Each box of a tile's
    source is mapped to the canvas through the tile's resize, intersected with the tile's rect (and
    dropped if nothing is left); the clipped AND the unclipped canvas box go through the canvas stages
    as corner envelopes, the clipped one is then clipped to the output frame, and transform_boxes'
    filters apply with the unclipped envelope as the visibility's denominator."""
    out_w, out_h = layer.frame
    rows = []
    for t in layer.tiles:
        boxes, labels = annotations[t.src]
        gx, gy = t.nw / t.w, t.nh / t.h
        rx0, ry0, rx1, ry1 = t.rect
        for (x, y, w, h), c in zip(boxes, labels):
            u = (t.ox + x * gx, t.oy + y * gy, t.ox + (x + w) * gx, t.oy + (y + h) * gy)
            k = (max(u[0], rx0), max(u[1], ry0), min(u[2], rx1), min(u[3], ry1))
            if k[2] <= k[0] or k[3] <= k[1]:
                continue
            ux0, uy0, ux1, uy1 = _envelope(_corners(*u), layer.stages)
            x0, y0, x1, y1 = _envelope(_corners(*k), layer.stages)
            area = (ux1 - ux0) * (uy1 - uy0)
            cx0, cy0 = min(max(x0, 0.0), out_w), min(max(y0, 0.0), out_h)
            cx1, cy1 = min(max(x1, 0.0), out_w), min(max(y1, 0.0), out_h)
            carea = max(cx1 - cx0, 0.0) * max(cy1 - cy0, 0.0)
            if area <= 0 or carea / area < min_visibility or carea < min_area:
                continue
            bw, bh = cx1 - cx0, cy1 - cy0
            cxn, cyn, wn, hn = (cx0 + bw / 2) / out_w, (cy0 + bh / 2) / out_h, bw / out_w, bh / out_h
            if wn > 1e-3 and hn > 1e-3 and 0 <= cxn <= 1 and 0 <= cyn <= 1 and 0 <= wn <= 1 and 0 <= hn <= 1:
                rows.append([c, cxn, cyn, wn, hn])
    return torch.tensor(rows, dtype=torch.float32) if rows else torch.empty(0, 5)


def mosaic_targets(plan, annotations):
    """The plan's targets: its layers' mosaic_boxes, concatenated."""
    return torch.cat([mosaic_boxes(ly, annotations) for ly in plan.layers], 0)


def _check_image(im, dev=None):
    if (dev is not None and im.device != dev) or im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3 \
            or im.stride(2) != 1 or im.stride(1) != 3:
        raise ValueError("yms: images must be contiguous HWC uint8 RGB tensors on one device")


def mosaic_struct(plan, images):
    """MosImage record of a MosaicPlan over its sample's device image list -- or of a plain AugPlan
    over its one image, as the degenerate layer: fill 0, no HSV on the fill, one tile that is the
    source itself (rect = stage 0's input frame, identity map)."""
    rec = MosImage()
    if isinstance(plan, MosaicPlan):
        layers = plan.layers
        rec.r = plan.r
    else:
        image = images[0] if isinstance(images, (list, tuple)) else images
        if tuple(image.shape[:2]) != (plan.src_h, plan.src_w):
            raise ValueError("yms: augmentation plan sampled for another image size")
        ly = MosaicLayer(plan.src_h, plan.src_w, fill=0.0)
        ly.hsv, ly.stages = plan.hsv, plan.stages
        ly.tiles = [MosaicTile(0, plan.src_h, plan.src_w, plan.src_w, plan.src_h, 0, 0,
                               (0, 0, plan.src_w, plan.src_h))]
        layers, images = [ly], [image]
        rec.r = 1.0
    rec.nlayer = len(layers)
    for lr, ly in zip(rec.layer, layers):
        if len(ly.stages) > AUG_MAX_STAGES or not 1 <= len(ly.tiles) <= MOS_MAX_TILES:
            raise ValueError("yms: a layer has at most AUG_MAX_STAGES stages and one to four tiles")
        lr.fill, lr.nst, lr.ntile = ly.fill, len(ly.stages), len(ly.tiles)
        if ly.hsv is not None:
            lr.do_hsv = 3 if isinstance(plan, MosaicPlan) else 1
            lr.hsv[:] = [float(v) for v in ly.hsv]
        _fill_stages(lr.st, ly.stages)
        for tr, t in zip(lr.tile, ly.tiles):
            im = images[t.src]
            if tuple(im.shape[:2]) != (t.h, t.w):
                raise ValueError("yms: mosaic tile sampled for another image size")
            tr.src, tr.h, tr.w, tr.pitch = im.data_ptr(), t.h, t.w, im.stride(0)
            tr.x0, tr.y0, tr.x1, tr.y1 = t.rect
            tr.sx, tr.sy, tr.tx, tr.ty = t.map
    return rec


def mosaic_normalize(images, plans, size, mean=IMAGENET_MEAN, std=IMAGENET_STD, dtype=torch.float32):
    """One launch (yms_mosaic_normalize) for a batch of mosaic and plain samples -> [B, 3, H, W].
    images[i]: the device image list of MosaicPlan plans[i], or the one device image of a plain
    AugPlan (expressed as the degenerate record, for which the output is augment_normalize's)."""
    if not images or len(images) != len(plans):
        raise ValueError("yms: one plan per sample")
    samples = [list(im) if isinstance(im, (list, tuple)) else [im] for im in images]
    dev = samples[0][0].device
    if dev.type != "cuda":
        raise RuntimeError("yms: mosaic_normalize runs on ROCm GPU tensors only (no CPU fallback)")
    if L.lib().yms_mosaic_image_bytes() != ctypes.sizeof(MosImage):
        raise RuntimeError("yms: MosImage layout differs from the library's")
    H, W = size
    n = len(samples)
    tab = (MosImage * n)()
    for i, (ims, pl) in enumerate(zip(samples, plans)):
        for im in ims:
            _check_image(im, dev)
        if pl.frame != (W, H):
            raise ValueError("yms: plan does not produce the batch size")
        tab[i] = mosaic_struct(pl, ims)
    tab_dev = torch.frombuffer(bytearray(tab), dtype=torch.uint8).to(dev, non_blocking=False)
    out = torch.empty((n, 3, H, W), dtype=dtype, device=dev)
    L.call("yms_mosaic_normalize", L.dtype_code(dtype), n, tab_dev.data_ptr(), H, W,
           (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std), out.data_ptr(), L.stream_ptr(dev))
    for ims in samples:
        for im in ims:
            im.record_stream(torch.cuda.current_stream(dev))
    tab_dev.record_stream(torch.cuda.current_stream(dev))
    return out


# ------------------------------------------------------------------------------------------
# Letterbox (opt-in; the evaluation input of the published YOLOv8 / YOLO-MS AP) and its frames
# ------------------------------------------------------------------------------------------
# ultralytics' LetterBox with scaleup on and centred, restated (ultralytics is not installed: parity
# UNPINNED): the image is resized by one gain r so that it fits the input, and centred on a canvas
# of 114.  A FRAME is what maps a box in input pixels back to its original image:
# (gain_x, gain_y, pad_x, pad_y, w0, h0), coordinate -> min(max((v - pad) / gain, 0), w0 | h0)
# (yms.ops.detect(frames=...)).  On the GPU a letterboxed image is a one-layer, one-tile record of
# yms_mosaic_normalize: canvas = output, no stage, the tile at (left, top) with the resize's
# half-pixel map -- no kernel of its own.
class Letterbox:
    """LetterBox geometry of an h0 x w0 image in an H x W input: r = min(H / h0, W / w0), the
    resized size nw, nh = round(w0 r), round(h0 r), and its corner left = round((W - nw) / 2 - 0.1),
    top = round((H - nh) / 2 - 0.1) (Python's round, as ultralytics calls it)."""

    def __init__(self, h0, w0, H, W):
        self.h0, self.w0, self.H, self.W = int(h0), int(w0), int(H), int(W)
        if min(self.h0, self.w0, self.H, self.W) < 1:
            raise ValueError("yms: letterbox needs positive sizes")
        self.r = min(self.H / self.h0, self.W / self.w0)
        self.nw = min(self.W, max(1, round(self.w0 * self.r)))
        self.nh = min(self.H, max(1, round(self.h0 * self.r)))
        self.left = max(0, round((self.W - self.nw) / 2 - 0.1))
        self.top = max(0, round((self.H - self.nh) / 2 - 0.1))

    @property
    def frame(self):
        return (self.r, self.r, float(self.left), float(self.top), float(self.w0), float(self.h0))

    def plan(self, src=0, fill=MOSAIC_FILL):
        """The MosaicPlan that draws it: one layer without stages, one tile."""
        ly = MosaicLayer(self.H, self.W, fill=fill)
        ly.tiles = [MosaicTile(src, self.h0, self.w0, self.nw, self.nh, self.left, self.top,
                               (self.left, self.top, self.left + self.nw, self.top + self.nh))]
        ly.applied.append("letterbox")
        return MosaicPlan([ly])


class Frames:
    """A batch's frames: ``host`` [B, 6] float32 numpy, ``tensor`` the same on the device (None
    without a device)."""

    def __init__(self, rows, device):
        self.host = np.asarray(rows, np.float32).reshape(-1, 6)
        self.tensor = None if device is None else torch.from_numpy(self.host).to(device)


def frames_stretch(sizes, size, device="cuda"):
    """Frames of resize_normalize's plain stretch of originals ``sizes`` = [(h0, w0)] to ``size`` =
    (H, W): gains W / w0 and H / h0, no padding."""
    H, W = size
    return Frames([(W / w0, H / h0, 0.0, 0.0, w0, h0) for h0, w0 in sizes], device)


def letterbox_normalize(images, size, fill=MOSAIC_FILL, mean=IMAGENET_MEAN, std=IMAGENET_STD, dtype=torch.float32):
    """Device HWC uint8 images (any sizes) -> ([B, 3, H, W] letterboxed, normalised batch, Frames), in
    one yms_mosaic_normalize launch."""
    if not images:
        raise ValueError("yms: empty batch")
    H, W = size
    boxes = [Letterbox(im.shape[0], im.shape[1], H, W) for im in images]
    out = mosaic_normalize([[im] for im in images], [lb.plan(0, fill) for lb in boxes], size, mean, std, dtype)
    return out, Frames([lb.frame for lb in boxes], images[0].device)


class COCODetection(torch.utils.data.Dataset):
    """dataset.py COCODataset's data source (image list, category map, annotation filters) without
    pycocotools; ``__getitem__`` returns (decoded HWC uint8 image, [n, 5] targets for ``img_size``),
    and ``collate_fn`` (or :func:`collate_to_gpu`) builds the GPU batch."""

    def __init__(self, images_dir, annotations_file, img_size=(640, 640), num_classes=80, fliplr=0.0, flipud=0.0,
                 seed=0):
        if not os.path.exists(annotations_file):
            raise FileNotFoundError(f"Annotations file not found: {annotations_file}")
        if not os.path.isdir(images_dir):
            raise NotADirectoryError(f"Images directory not found: {images_dir}")
        self.images_dir = images_dir
        self.img_h, self.img_w = img_size
        self.num_classes = num_classes
        self.fliplr, self.flipud = fliplr, flipud
        self.seed = int(seed)
        self._draws = 0
        d = json.load(open(annotations_file))
        self.imgs = {im["id"]: im for im in d.get("images", [])}
        self.img_to_anns = defaultdict(list)
        for a in d.get("annotations", []):
            self.img_to_anns[a["image_id"]].append(a)
        self.image_ids = [i for i in sorted(self.imgs)
                          if os.path.exists(os.path.join(images_dir, self.imgs[i]["file_name"]))]
        self.cat_ids = [c["id"] for c in d.get("categories", [])][:num_classes]
        self.cat2label = {c: i for i, c in enumerate(self.cat_ids)}
        self.label2cat = {i: c for i, c in enumerate(self.cat_ids)}

    def __len__(self):
        return len(self.image_ids)

    def annotations(self, idx):
        """-> (COCO [x, y, w, h] boxes, labels) kept by dataset.py:159-172's filters."""
        boxes, labels = [], []
        for a in self.img_to_anns[self.image_ids[idx]]:
            if a.get("iscrowd", 0) != 0 or not a.get("area", 0) > 0:
                continue
            lab = self.cat2label.get(a["category_id"])
            if lab is None:
                continue
            x, y, w, h = a["bbox"]
            if w <= 0 or h <= 0:
                continue
            boxes.append([x, y, w, h])
            labels.append(lab)
        return boxes, labels

    def eval_annotations(self, idx):
        """The image's ground truths as COCOeval keeps them: every annotation of a known category, crowd
        and zero-area ones included (``annotations`` drops those, as training must) -> {'boxes' [k, 4] fp32
        xyxy in original-image pixels (where ``detect``'s letterbox un-mapping puts its detections), 'labels'
        [k] int64, 'iscrowd' [k] uint8, 'area' [k] fp32: the annotation's own ``area`` -- the mask's on COCO
        -- or w*h where it has none}, numpy arrays as ``CocoEvaluator.pad_targets(..., flags=True)`` and
        ``MeanAveragePrecision.update`` take them."""
        boxes, labels, crowd, area = [], [], [], []
        for a in self.img_to_anns[self.image_ids[idx]]:
            lab = self.cat2label.get(a["category_id"])
            if lab is None:
                continue
            x, y, w, h = a["bbox"]
            boxes.append([x, y, x + w, y + h])
            labels.append(lab)
            crowd.append(1 if a.get("iscrowd", 0) else 0)
            area.append(a["area"] if "area" in a else w * h)
        return {"boxes": np.asarray(boxes, np.float32).reshape(-1, 4), "labels": np.asarray(labels, np.int64),
                "iscrowd": np.asarray(crowd, np.uint8), "area": np.asarray(area, np.float32)}

    def __getitem__(self, idx):
        from PIL import Image
        info = self.imgs[self.image_ids[idx]]
        image = np.array(Image.open(os.path.join(self.images_dir, info["file_name"])).convert("RGB"))
        boxes, labels = self.annotations(idx)
        h0, w0 = image.shape[:2]
        t = coco_boxes_to_targets(boxes, labels, w0, h0, self.img_w, self.img_h)
        rng = self.sample_rng(idx)
        flags = (int(rng.random() < self.fliplr) if self.fliplr > 0 else 0) | \
                ((int(rng.random() < self.flipud) << 1) if self.flipud > 0 else 0)
        if flags:
            t = flip_targets(t, flags)
        return image, t, flags

    def sample_rng(self, idx):
        """Generator for one sample's random draws, seeded from (dataset seed, process stream, idx,
        draw count).  In a DataLoader worker the stream is torch's per-worker seed (base seed drawn
        anew for every epoch's iterator + worker id), so workers and epochs draw different streams;
        in the main process it is torch.initial_seed() and the draw counter moves epochs apart.  A
        Generator created once in __init__ would be forked unchanged into every worker instead."""
        info = torch.utils.data.get_worker_info()
        stream = info.seed if info is not None else torch.initial_seed()
        self._draws += 1
        return np.random.default_rng([self.seed, stream & 0xFFFFFFFFFFFFFFFF, int(idx), self._draws])

    def collate_fn(self, batch):
        """Host half of the collate: images stay decoded uint8; targets -> [M, 6] (dataset.py:235-267)."""
        return collate_targets(batch)


class COCODataset(COCODetection):
    """dataset.py:12-233 ``COCODataset(images_dir, annotations_file, transform_params=None,
    is_train=True, img_size=(640, 640), num_classes=80)``: the training transform of
    ``transform_params`` (the config's ``augmentation`` dict) is sampled per sample on the host
    (``sample_augmentation``) and applied on the GPU by the collate (``collate_to_gpu``);
    ``is_train=False`` keeps only the Resize.  ``__getitem__`` -> (decoded HWC uint8 image,
    [n, 5] targets in the augmented frame, AugPlan).

    ``mosaic=True`` opts into Mosaic / MixUp (training only): ``transform_params["mosaic"]`` and
    ``["mixup"]`` are then probabilities.  A sample's first draw decides Mosaic (no draw when the
    probability is 0); a mosaic sample draws three more dataset indices (uniform, repeats allowed),
    its layer (``sample_mosaic``), then decides MixUp (no draw when its probability is 0), which
    draws four indices, a second independent layer and r ~ Beta(32, 32).  ``__getitem__`` returns
    (list of decoded images, [n, 5] targets, MosaicPlan) for such a sample and the plain tuple
    otherwise, drawn from the same generator after the decision.  With ``mosaic=False`` (the
    default) both keys are ignored and no extra number is drawn.  ``ds.mosaic`` may be set at any
    time, e.g. to close Mosaic for the last epochs -- but DataLoader workers hold copies of the
    dataset made when their iterator started (with ``persistent_workers=True`` for the whole run),
    so a change reaches them only through a new iterator / DataLoader."""

    def __init__(self, images_dir, annotations_file, transform_params=None, is_train=True, img_size=(640, 640),
                 num_classes=80, seed=0, mosaic=False, letterbox=False):
        super().__init__(images_dir, annotations_file, img_size=img_size, num_classes=num_classes, seed=seed)
        self.transform_params = dict(transform_params or {})
        self.is_train = is_train
        self.mosaic = mosaic
        # evaluation only (is_train=False): __getitem__ -> (image, [n, 5] targets = (class, x1, y1, x2, y2)
        # in ORIGINAL-image pixels, Letterbox), and collate_to_gpu returns the batch's Frames as a third
        # value -- detections un-letterboxed by yms.ops.detect(frames=...) are compared with these targets
        self.letterbox = letterbox

    def _load(self, idx):
        from PIL import Image
        info = self.imgs[self.image_ids[idx]]
        image = np.array(Image.open(os.path.join(self.images_dir, info["file_name"])).convert("RGB"))
        return image, self.annotations(idx)

    def _mosaic_layer(self, rng, idxs, images, anns):
        """One layer over dataset indices ``idxs``, its sources appended to the sample's lists."""
        base = len(images)
        for i in idxs:
            im, an = self._load(int(i))
            images.append(im)
            anns.append(an)
        ly = sample_mosaic(rng, self.transform_params, [im.shape[:2] for im in images[base:]], self.img_h, self.img_w)
        for t in ly.tiles:
            t.src += base
        return ly

    def __getitem__(self, idx):
        if torch.is_tensor(idx):
            idx = idx.item()
        if not isinstance(idx, int):
            raise TypeError(f"Index should be an integer, got {type(idx).__name__} instead.")
        rng = self.sample_rng(idx)
        tp = self.transform_params
        if self.mosaic and self.is_train and tp.get("mosaic", 0) > 0 and rng.random() < tp["mosaic"]:
            images, anns = [], []
            layers = [self._mosaic_layer(rng, [idx, *rng.integers(0, len(self), 3)], images, anns)]
            r = 1.0
            if tp.get("mixup", 0) > 0 and rng.random() < tp["mixup"]:
                layers.append(self._mosaic_layer(rng, rng.integers(0, len(self), 4), images, anns))
                r = rng.beta(32.0, 32.0)
            plan = MosaicPlan(layers, r)
            return images, mosaic_targets(plan, anns), plan
        image, (boxes, labels) = self._load(idx)
        h0, w0 = image.shape[:2]
        if self.letterbox and not self.is_train:
            rows = [[c, x, y, x + w, y + h] for (x, y, w, h), c in zip(boxes, labels)]
            t = torch.tensor(rows, dtype=torch.float32) if rows else torch.empty(0, 5)
            return image, t, Letterbox(h0, w0, self.img_h, self.img_w)
        plan = sample_augmentation(rng, tp, h0, w0, self.img_h, self.img_w, self.is_train)
        return image, transform_boxes(boxes, labels, plan), plan


def collate_targets(batch):
    """[(image, [n, 5] targets, flags or AugPlan)] -> (images, flags / plans, [M, 6] targets with the
    batch index first).  A mosaic sample's entry is (image list, targets, MosaicPlan); its image list
    stays one entry of ``images``."""
    images, flags, rows = [], [], []
    for i, (img, t, f) in enumerate(batch):
        images.append(img)
        flags.append(f)
        if t.shape[0] > 0:
            rows.append(torch.cat([torch.full((t.shape[0], 1), float(i)), t], 1))
    targets = torch.cat(rows, 0) if rows else torch.empty(0, 6)
    return images, flags, targets


def collate_to_gpu(batch, img_size, device, dtype=torch.float32, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """dataset.py collate_fn output on the GPU: ([B, 3, H, W] normalised images, [M, 6] targets).
    A batch with at least one mosaic sample goes through mosaic_normalize whole (its plain samples
    as degenerate records: still one launch); any other batch takes the paths it took before.
    A batch of COCODataset(is_train=False, letterbox=True) samples is letterboxed instead and comes
    back as (images, [M, 6] targets = (image, class, x1, y1, x2, y2) in original pixels, Frames)."""
    images, extra, targets = collate_targets(batch)
    if extra and all(isinstance(e, Letterbox) for e in extra):     # COCODataset(is_train=False, letterbox=True)
        x, frames = letterbox_normalize(to_device(images, device), img_size, MOSAIC_FILL, mean, std, dtype)
        return x, targets.to(device, non_blocking=True), frames
    if any(isinstance(e, MosaicPlan) for e in extra):
        dev_images = [to_device(im, device) if isinstance(im, (list, tuple)) else to_device([im], device)[0]
                      for im in images]
        x = mosaic_normalize(dev_images, extra, img_size, mean, std, dtype)
        return x, targets.to(device, non_blocking=True)
    dev_images = to_device(images, device)
    if extra and isinstance(extra[0], AugPlan):
        x = augment_normalize(dev_images, extra, img_size, mean, std, dtype)
    else:
        x = resize_normalize(dev_images, img_size, mean, std, extra, dtype)
    return x, targets.to(device, non_blocking=True)
