"""Task-aligned assigner loss on the MI355X (opt-in): YOLOv8's published ``v8DetectionLoss`` with
its ``TaskAlignedAssigner``, computed by the HIP kernels of csrc/tal_loss.hip together with its
analytic gradient.  ``ComputeLoss`` / ``SimplifiedYOLOLoss`` keep the reference's own semantics;
this module is the loss of the published training recipe for users who want it.

Semantics (tests/tal_ref.py is the plain-torch restatement and the definition; DESIGN.md
"Task-aligned loss"):

* anchor centre ``(gx + .5, gy + .5) * stride``; predicted box ``((gx + .5 - e0) s, (gy + .5 - e1) s,
  (gx + .5 + e2) s, (gy + .5 + e3) s)`` with ``e`` the softmax-expected DFL bin of each side;
* per (GT j, anchor a of its image): ``inside`` = the centre lies more than 1e-9 px inside the GT,
  ``ov = max(CIoU, 0)``, ``m = sigmoid(logit[a, class_j]) ** alpha * ov ** beta``;
* positives of j: the first ``min(topk, #inside)`` inside anchors by (m descending, anchor index
  ascending); an anchor claimed once belongs to its claimant, one claimed several times to the GT
  with the largest ``ov`` among all the image's GTs it lies inside (lowest target row on a tie);
* target score ``t(a) = m(a, j) * max_ov_j / (max_m_j + 1e-9)`` (maxima over the anchors finally
  assigned to j) at class_j; ``tss = max(sum t, 1)``; assignment, t and tss carry no gradient;
* ``cls = sum BCE(x, target) / tss``, ``box = sum_fg (1 - CIoU) t / tss``, ``dfl = sum_fg
  (two-bin DFL cross entropy, mean of the 4 sides, distances clamped to [0, 14.99]) t / tss``;
  ``total = B * (box_gain box + cls_gain cls + dfl_gain dfl)``.

Target rows whose image is outside ``[0, B)`` or whose class is outside ``[0, nc)`` are ignored.

One deliberate deviation: CIoU is this project's formula (``yolov8.tools.loss.bbox_iou(xywh=False,
CIoU=True)``, eps added to the union and to the heights inside the arctangents); ultralytics adds
its eps to the box heights and the enclosing diagonal instead, a difference of order 1e-7.  Ties
of the top-k and its all-zero case, which ``torch.topk`` leaves unspecified, are defined above.
The ultralytics package is not a dependency and was not available to compare against: parity with
it is UNPINNED; the kernels are pinned to tests/tal_ref.py.
"""
from __future__ import annotations

import ctypes

import torch
from torch import nn

from yms import _lib as L
from yolov8.tools.loss import _FusedLossFn, _loss_items, _prepare


def tal_loss(preds, targets, nc, img_size, strides=(8.0, 16.0, 32.0), topk=10, alpha=0.5, beta=6.0,
             lambdas=(7.5, 0.5, 1.5), need_grad=True, return_assignment=False):
    """-> (out [4] fp32 device tensor = total, box, cls, dfl; list of gradient maps shaped like
    ``preds`` (channels-last, same dtype) or None) and, ``return_assignment``, a third element
    (assign_gt [B, A] int32: target row or -1, assign_score [B, A] fp32: t(a)); anchors level-major,
    then row-major.  No host sync."""
    if not 1 <= int(topk) <= 10:
        raise ValueError("yms: topk must be in 1..10")
    p = _prepare("task-aligned", preds, targets, nc, img_size, strides, need_grad)
    agt = asc = None
    if return_assignment:
        agt = torch.empty((p.B, p.A), dtype=torch.int32, device=p.dev)
        asc = torch.empty((p.B, p.A), dtype=torch.float32, device=p.dev)
    wsb = L.lib().yms_tal_loss_ws_bytes(p.B, p.A, nc, p.M)
    ws_t = torch.empty(wsb, dtype=torch.uint8, device=p.dev)
    out = torch.empty(4, dtype=torch.float32, device=p.dev)
    L.call("yms_tal_loss", *p.args, int(topk), ctypes.c_float(float(alpha)), ctypes.c_float(float(beta)),
           (ctypes.c_float * 3)(*[float(x) for x in lambdas]), ws_t.data_ptr(), wsb, out.data_ptr(), L.ptr(agt),
           L.ptr(asc), L.stream_ptr(p.dev))
    if return_assignment:
        return out, p.ungrad(), (agt, asc)
    return out, p.ungrad()


class _TalLossFn(_FusedLossFn):
    @staticmethod
    def forward(ctx, cfg, targets, *preds):
        return _FusedLossFn.run(ctx, tal_loss, cfg, targets, preds)


class TaskAlignedLoss(nn.Module):
    """``ComputeLoss``'s constructor shape and call for the task-aligned loss (module docstring):
    ``forward(preds_from_head, targets_collated) -> (total_loss, {"loss_box", "loss_cls", "loss_dfl",
    "total_loss"})``."""

    def __init__(self, model_head, num_classes, device, img_size, strides=(8.0, 16.0, 32.0), topk=10, alpha=0.5,
                 beta=6.0, box=7.5, cls=0.5, dfl=1.5):
        super().__init__()
        if not 1 <= int(topk) <= 10:
            raise ValueError("yms: topk must be in 1..10")
        self.model_head = model_head
        self.num_classes = num_classes
        self.device = device
        self.img_size_h, self.img_size_w = img_size[0], img_size[1]
        self.strides = torch.tensor([float(s) for s in strides], device=device)
        self._strides = tuple(float(s) for s in strides)
        self.topk, self.alpha, self.beta = int(topk), float(alpha), float(beta)
        self.lambda_box, self.lambda_cls, self.lambda_dfl = float(box), float(cls), float(dfl)

    def forward(self, preds_from_head, targets_collated):
        total, terms = self.loss_tensor(preds_from_head, targets_collated)
        return total, _loss_items(total, terms)

    def loss_tensor(self, preds_from_head, targets_collated):
        """-> (total [] device tensor, differentiable; terms [3] device tensor (box, cls, dfl), not
        differentiable); no host sync."""
        cfg = (self.num_classes, (self.img_size_h, self.img_size_w), self._strides, self.topk, self.alpha,
               self.beta, (self.lambda_box, self.lambda_cls, self.lambda_dfl))
        return _TalLossFn.apply(cfg, targets_collated, *preds_from_head)
