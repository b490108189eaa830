"""YOLO-MS's own loss on the MI355X (opt-in): the published YOLO-MS recipe comes from the RTMDet
lineage and trains with the dynamic soft-label assigner, Quality Focal Loss (QFL) on the class logits
and GIoU on the boxes, both weighted by the matched IoU.  The HIP kernels of csrc/dsl_loss.hip compute
it together with its analytic gradient.  ``ComputeLoss`` / ``SimplifiedYOLOLoss`` keep the reference's
semantics and ``TaskAlignedLoss`` YOLOv8's; this module is the loss of the MS family's recipe for
users who want it.

Semantics (tests/dsl_ref.py is the plain-torch restatement and the definition; DESIGN.md "Dynamic
soft-label loss"):

* anchors, decode and target rows as in ``yolov8.tools.tal_loss``: centre ``(gx + .5, gy + .5) *
  stride``, predicted xyxy box from the softmax-expected DFL bins times the stride; rows whose image is
  outside ``[0, B)`` or whose class is outside ``[0, nc)`` are ignored.  Everything below is per image,
  over its valid rows ``j`` in target order;
* candidates: the anchors whose centre lies more than 1e-9 px inside at least one GT of the image, one
  set shared by all its GTs; an image without candidates assigns nothing;
* ``iou(a, j)``: the project's plain IoU (``bbox_iou(xywh=False)``), NaN -> 0;
* ``cost(a, j) = sum_c BCEwithlogits(x[a, c], y_c) |y_c - sigmoid(x[a, c])| ** beta`` (``y = iou`` at
  class_j, 0 elsewhere) ``- log(iou + 1e-7) * iou_weight + 10 ** min(dist / stride_a - radius, 30)``,
  ``dist`` the pixel distance between the anchor centre and the GT centre;
* dynamic k: ``k_j = max(1, floor(sum of the min(topk, n_cand) largest iou(., j) over the candidates))``;
  GT j selects its ``k_j`` candidates of lowest cost (ties: lower anchor index), also when it contains
  no anchor centre itself;
* an anchor selected once belongs to its selector; one selected several times goes to the GT of lowest
  cost among ALL the image's valid GTs (lowest row on a tie), even one that did not select it;
* soft label ``t(a) = iou(a, j_assigned)`` (may be 0); ``norm = max(sum t, 1)``; assignment, t and norm
  carry no gradient;
* ``cls = sum QFL / norm`` (``BCEwithlogits(x, t) |t - sigmoid(x)| ** beta`` at the assigned anchor's
  class, ``softplus(x) sigmoid(x) ** beta`` everywhere else), ``box = sum_fg (1 - GIoU) t / norm``,
  ``dfl = sum_fg (two-bin DFL cross entropy, mean of the 4 sides, distances clamped to [0, 14.99]) t /
  norm``; ``total = box_gain box + cls_gain cls + dfl_gain dfl`` (2, 1, 0: the recipe has no DFL term,
  its value is still reported).  There is no factor B.

Deliberate deviations: IoU / GIoU are this project's formulas (eps 1e-7 in the union and the enclosing
area; mmdet clamps at 1e-6); the prior's exponent is capped at 30 so that it stays finite in fp32 (1e30
absorbs the other cost terms in fp32 and fp64 alike); the tie rules above, which ``torch.topk`` /
``argmin`` leave open; ``norm`` is per process, with no mean over ranks.  mmdet / mmyolo are not
dependencies and were not available to compare against: parity with them is UNPINNED; the kernels are
pinned to tests/dsl_ref.py.
"""
from __future__ import annotations

import ctypes
import math

import torch
from torch import nn

from yms import _lib as L
from yolov8.tools.loss import _FusedLossFn, _loss_items, _prepare

MAX_TOPK = 13


def _check(topk, radius, iou_weight, beta):
    if not 1 <= int(topk) <= MAX_TOPK:
        raise ValueError(f"yms: topk must be in 1..{MAX_TOPK}")
    if not (math.isfinite(radius) and radius >= 0 and math.isfinite(iou_weight) and iou_weight >= 0):
        raise ValueError("yms: radius and iou_weight must be finite and >= 0")
    if not (math.isfinite(beta) and beta >= 1):
        raise ValueError("yms: beta must be finite and >= 1")


def dsl_loss(preds, targets, nc, img_size, strides=(8.0, 16.0, 32.0), topk=13, radius=3.0, iou_weight=3.0, beta=2.0,
             gains=(2.0, 1.0, 0.0), need_grad=True, return_assignment=False):
    """-> (out [5] fp32 device tensor = total, box, cls, dfl, norm; list of gradient maps shaped like
    ``preds`` (channels-last, same dtype) or None) and, ``return_assignment``, a third element
    (assign_gt [B, A] int32: target row or -1, assign_score [B, A] fp32: t(a), dynamic_k [M] int32: 0
    for ignored rows and rows of an image without candidates); anchors level-major, then row-major.
    No host sync."""
    _check(topk, float(radius), float(iou_weight), float(beta))
    p = _prepare("dynamic soft-label", preds, targets, nc, img_size, strides, need_grad)
    agt = asc = dk = None
    if return_assignment:
        agt = torch.empty((p.B, p.A), dtype=torch.int32, device=p.dev)
        asc = torch.empty((p.B, p.A), dtype=torch.float32, device=p.dev)
        dk = torch.empty((p.M,), dtype=torch.int32, device=p.dev)
    wsb = L.lib().yms_dsl_loss_ws_bytes(p.B, p.A, nc, p.M)
    ws_t = torch.empty(wsb, dtype=torch.uint8, device=p.dev)
    out = torch.empty(5, dtype=torch.float32, device=p.dev)
    L.call("yms_dsl_loss", *p.args, int(topk), ctypes.c_float(float(radius)), ctypes.c_float(float(iou_weight)),
           ctypes.c_float(float(beta)), (ctypes.c_float * 3)(*[float(x) for x in gains]), ws_t.data_ptr(), wsb,
           out.data_ptr(), L.ptr(agt), L.ptr(asc), L.ptr(dk) if p.M else None, L.stream_ptr(p.dev))
    if return_assignment:
        return out, p.ungrad(), (agt, asc, dk)
    return out, p.ungrad()


class _DslLossFn(_FusedLossFn):
    @staticmethod
    def forward(ctx, cfg, targets, *preds):
        return _FusedLossFn.run(ctx, dsl_loss, cfg, targets, preds)


class DynamicSoftLabelLoss(nn.Module):
    """``ComputeLoss``'s constructor shape and call for YOLO-MS's own loss (module docstring):
    ``forward(preds_from_head, targets_collated) -> (total_loss, {"loss_box", "loss_cls", "loss_dfl",
    "total_loss"})``."""

    def __init__(self, model_head, num_classes, device, img_size, strides=(8.0, 16.0, 32.0), topk=13,
                 soft_center_radius=3.0, iou_weight=3.0, beta=2.0, box=2.0, cls=1.0, dfl=0.0):
        super().__init__()
        _check(topk, float(soft_center_radius), float(iou_weight), float(beta))
        self.model_head = model_head
        self.num_classes = num_classes
        self.device = device
        self.img_size_h, self.img_size_w = img_size[0], img_size[1]
        self.strides = torch.tensor([float(s) for s in strides], device=device)
        self._strides = tuple(float(s) for s in strides)
        self.topk = int(topk)
        self.soft_center_radius, self.iou_weight, self.beta = float(soft_center_radius), float(iou_weight), float(beta)
        self.lambda_box, self.lambda_cls, self.lambda_dfl = float(box), float(cls), float(dfl)

    def forward(self, preds_from_head, targets_collated):
        total, terms = self.loss_tensor(preds_from_head, targets_collated)
        return total, _loss_items(total, terms)

    def loss_tensor(self, preds_from_head, targets_collated):
        """-> (total [] device tensor, differentiable; terms [3] device tensor (box, cls, dfl), not
        differentiable); no host sync."""
        cfg = (self.num_classes, (self.img_size_h, self.img_size_w), self._strides, self.topk,
               self.soft_center_radius, self.iou_weight, self.beta,
               (self.lambda_box, self.lambda_cls, self.lambda_dfl))
        return _DslLossFn.apply(cfg, targets_collated, *preds_from_head)
