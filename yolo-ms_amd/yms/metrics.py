"""Detection mAP on the MI355X path, standing in for
``torchmetrics.detection.MeanAveragePrecision(box_format='xyxy', iou_type='bbox', ...)``.

``iou_thresholds=[0.5]`` is the reference's validation metric, read as ``map_50``
(yolov8/tools/train.py:41-47, 146, 152-153): ``update()`` runs the detection <-> ground-truth
matching on the GPU (``yms_map_match``, one wave per image) and ``compute()`` the per-class
precision / recall accumulation and 101-point interpolation in the native host code
(``yms_map_accumulate``).

Any other setting -- ``iou_thresholds=None`` is COCO's 0.50:0.05:0.95 -- is the full COCOeval
summary (bbox, no crowd): ``update()`` matches every (threshold, area range) pair in one launch
(``yms_map_match_coco``: up to 16 thresholds x all / small / medium / large with COCOeval's ignore
rules), ``compute()`` fills COCOeval's precision[T][101][K][4][3] and recall[T][K][4][3] tables on
the host (``yms_map_accumulate_coco``, maxDets 1 / 10 / 100) and averages them into AP, AP50, AP75,
APs/m/l and AR@1/10/100, ARs/m/l.

COCOeval semantics throughout; parity is against the restatements oracle/map_ref.py and
tests/cocoeval_ref.py (torchmetrics / pycocotools are not installed: unpinned)."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib as L

MAX_THRESHOLDS = 16
N_AREAS = 4                  # all, small, medium, large
MAX_DETS = (1, 10, 100)


def _hp(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a.size else None


class MeanAveragePrecision:
    def __init__(self, box_format="xyxy", iou_type="bbox", iou_thresholds=None, **_ignored):
        if box_format != "xyxy" or iou_type != "bbox":
            raise ValueError("yms.metrics.MeanAveragePrecision implements box_format='xyxy', iou_type='bbox'")
        if iou_thresholds is None:
            thr = np.linspace(.5, .95, int(np.round((.95 - .5) / .05)) + 1, endpoint=True)
        else:
            thr = np.asarray(list(iou_thresholds), dtype=np.float64).reshape(-1)
        if not 1 <= thr.size <= MAX_THRESHOLDS:
            raise ValueError(f"yms.metrics.MeanAveragePrecision takes 1 to {MAX_THRESHOLDS} iou_thresholds")
        if not (np.all(thr > 0) and np.all(thr <= 1) and np.all(np.diff(thr) > 0)):
            raise ValueError("iou_thresholds must be increasing values in (0, 1]")
        self.iou_thresholds = thr
        # the reference's setting keeps its own kernel, accumulation and result keys
        self._coco = not (iou_thresholds is not None and list(iou_thresholds) == [0.5])
        self.reset()

    def reset(self):
        self._scores, self._labels, self._image, self._tp, self._kept = [], [], [], [], []
        self._rank, self._matched, self._ignored, self._glabels, self._gignore = [], [], [], [], []
        self._ngt = {}
        self._n_images = 0

    def to(self, device):      # torchmetrics-style no-op (state lives on the host)
        return self

    def update(self, preds, targets):
        if len(preds) != len(targets):
            raise ValueError("preds and targets must have the same length")
        if not preds:
            return
        dev = next((p["boxes"].device for p in preds if isinstance(p["boxes"], torch.Tensor)), None)
        if dev is None or dev.type != "cuda":
            raise RuntimeError("yms: mAP matching runs on ROCm GPU tensors only (no CPU fallback)")
        db = torch.cat([p["boxes"].reshape(-1, 4).float() for p in preds]).contiguous()
        ds = torch.cat([p["scores"].reshape(-1).float() for p in preds]).contiguous()
        dl = torch.cat([p["labels"].reshape(-1).to(torch.int32) for p in preds]).contiguous()
        gb = torch.cat([t["boxes"].reshape(-1, 4).float().to(dev) for t in targets]).contiguous()
        gl = torch.cat([t["labels"].reshape(-1).to(torch.int32).to(dev) for t in targets]).contiguous()
        nd = [int(p["scores"].numel()) for p in preds]
        ng = [int(t["labels"].numel()) for t in targets]
        doff = torch.tensor(np.concatenate([[0], np.cumsum(nd)]), dtype=torch.int32, device=dev)
        goff = torch.tensor(np.concatenate([[0], np.cumsum(ng)]), dtype=torch.int32, device=dev)
        n = int(sum(nd))
        D = max(n, 1)
        image = np.repeat(np.arange(self._n_images, self._n_images + len(preds), dtype=np.int32), nd)
        if self._coco:
            G = max(int(sum(ng)), 1)
            matched = torch.zeros(N_AREAS, D, dtype=torch.int16, device=dev)
            ignored = torch.zeros(N_AREAS, D, dtype=torch.int16, device=dev)
            gign = torch.zeros(G, dtype=torch.uint8, device=dev)
            rank = torch.empty(2 * D, dtype=torch.int32, device=dev)
            thr = self.iou_thresholds
            L.call("yms_map_match_coco", len(preds), n, L.ptr(db) if n else None, L.ptr(ds) if n else None,
                   L.ptr(dl) if n else None, doff.data_ptr(), L.ptr(gb) if gb.numel() else None,
                   L.ptr(gl) if gl.numel() else None, goff.data_ptr(), int(thr.size), _hp(thr), matched.data_ptr(),
                   ignored.data_ptr(), gign.data_ptr(), rank.data_ptr(), max(ng) if ng else 0, L.stream_ptr(dev))
            self._scores.append(ds.cpu().numpy())
            self._labels.append(dl.cpu().numpy())
            self._rank.append(rank[:n].cpu().numpy())
            self._matched.append(matched[:, :n].cpu().numpy().view(np.uint16))
            self._ignored.append(ignored[:, :n].cpu().numpy().view(np.uint16))
            self._glabels.append(gl.cpu().numpy())
            self._gignore.append(gign[:int(sum(ng))].cpu().numpy())
            self._image.append(image)
            self._n_images += len(preds)
            return
        tp = torch.zeros(D, dtype=torch.uint8, device=dev)
        kept = torch.zeros(D, dtype=torch.uint8, device=dev)
        rank = torch.empty(D, dtype=torch.int32, device=dev)
        L.call("yms_map_match", len(preds), L.ptr(db) if db.numel() else None, L.ptr(ds) if ds.numel() else None,
               L.ptr(dl) if dl.numel() else None, doff.data_ptr(), L.ptr(gb) if gb.numel() else None,
               L.ptr(gl) if gl.numel() else None, goff.data_ptr(), tp.data_ptr(), kept.data_ptr(), rank.data_ptr(),
               max(ng) if ng else 0, L.stream_ptr(dev))
        self._scores.append(ds.cpu().numpy())
        self._labels.append(dl.cpu().numpy())
        self._tp.append(tp[:n].cpu().numpy())
        self._kept.append(kept[:n].cpu().numpy())
        self._image.append(image)
        for c in gl.cpu().numpy().tolist():
            self._ngt[c] = self._ngt.get(c, 0) + 1
        self._n_images += len(preds)

    def compute(self):
        if self._coco:
            return self._compute_coco()
        cat = (lambda xs, dt: np.ascontiguousarray(np.concatenate(xs).astype(dt)) if xs else np.zeros(0, dt))
        sc, lb = cat(self._scores, np.float32), cat(self._labels, np.int32)
        im, tp, kp = cat(self._image, np.int32), cat(self._tp, np.uint8), cat(self._kept, np.uint8)
        ncls = max([int(lb.max()) + 1 if lb.size else 0] + [c + 1 for c in self._ngt] + [1])
        ngt = np.zeros(ncls, dtype=np.int32)
        for c, k in self._ngt.items():
            if c >= 0:
                ngt[c] = k
        ap = np.zeros(ncls, dtype=np.float64)
        m = np.zeros(1, dtype=np.float64)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a.size else None
        L.check(L.lib().yms_map_accumulate(int(sc.size), p(sc), p(lb), p(im), p(tp), p(kp), ncls, p(ngt), p(ap), p(m)),
                "yms_map_accumulate")
        per = {c: float(ap[c]) for c in range(ncls) if ngt[c] > 0}
        mv = torch.tensor(float(m[0]), dtype=torch.float64)
        return {"map": mv, "map_50": mv.clone(), "map_per_class": per}

    def tables(self):
        """COCOeval's ``eval['precision']`` [T, 101, K, 4, 3] and ``eval['recall']`` [T, K, 4, 3] (float64,
        -1 for cells without a non-ignored ground truth) and the per-(class, area) count of those."""
        if not self._coco:
            raise RuntimeError("yms: the precision / recall tables belong to the COCO mode (iou_thresholds != [0.5])")
        cat = (lambda xs, dt: np.ascontiguousarray(np.concatenate(xs).astype(dt)) if xs else np.zeros(0, dt))
        sc, lb = cat(self._scores, np.float32), cat(self._labels, np.int32)
        im, rk = cat(self._image, np.int32), cat(self._rank, np.int32)
        cat2 = (lambda xs: np.ascontiguousarray(np.concatenate(xs, axis=1)) if xs
                else np.zeros((N_AREAS, 0), np.uint16))
        mt, ig = cat2(self._matched), cat2(self._ignored)
        gl, gi = cat(self._glabels, np.int32), cat(self._gignore, np.uint8)
        K = max([int(lb.max()) + 1 if lb.size else 0, int(gl.max()) + 1 if gl.size else 0, 1])
        npig = np.zeros((K, N_AREAS), dtype=np.int32)
        ok = gl >= 0
        for a in range(N_AREAS):
            np.add.at(npig[:, a], gl[ok & (((gi >> a) & 1) == 0)], 1)
        T = int(self.iou_thresholds.size)
        precision = np.empty((T, 101, K, N_AREAS, len(MAX_DETS)), dtype=np.float64)
        recall = np.empty((T, K, N_AREAS, len(MAX_DETS)), dtype=np.float64)
        L.check(L.lib().yms_map_accumulate_coco(int(sc.size), _hp(sc), _hp(lb), _hp(im), _hp(rk), _hp(mt), _hp(ig), T,
                                                K, _hp(npig), _hp(precision), _hp(recall)),
                "yms_map_accumulate_coco")
        return precision, recall, npig

    def _compute_coco(self):
        precision, recall, npig = self.tables()
        thr = self.iou_thresholds

        def mean(s):
            s = s[s > -1]
            return float(np.mean(s)) if s.size else -1.0

        def ap(area=0, iou=None):
            s = precision
            if iou is not None:
                s = s[np.isclose(thr, iou)]
            return mean(s[:, :, :, area, 2])

        def ar(area=0, md=2):
            return mean(recall[:, :, area, md])

        f = lambda v: torch.tensor(v, dtype=torch.float64)
        classes = [c for c in range(npig.shape[0]) if npig[c, 0] > 0]
        return {
            "map": f(ap()), "map_50": f(ap(iou=0.5)), "map_75": f(ap(iou=0.75)),
            "map_small": f(ap(1)), "map_medium": f(ap(2)), "map_large": f(ap(3)),
            "mar_1": f(ar(md=0)), "mar_10": f(ar(md=1)), "mar_100": f(ar(md=2)),
            "mar_small": f(ar(1)), "mar_medium": f(ar(2)), "mar_large": f(ar(3)),
            "map_per_class": {c: mean(precision[:, :, c, 0, 2]) for c in classes},
            "mar_100_per_class": {c: mean(recall[:, c, 0, 2]) for c in classes},
            "classes": torch.tensor(np.unique(np.concatenate(
                [np.zeros(0, np.int32)] + self._labels + self._glabels)).astype(np.int32)),
        }
