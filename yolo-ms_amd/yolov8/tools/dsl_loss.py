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
from yolov8.tools.loss import DFL_CH, _nhwc, _storage_elems

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
    if not preds or any(p.device.type != "cuda" for p in preds):
        raise RuntimeError("yms: the dynamic soft-label loss runs on ROCm GPU tensors only (no CPU fallback)")
    if len(preds) > 4 or len(strides) < len(preds):
        raise ValueError("yms: 1-4 head levels with one stride each")
    _check(topk, float(radius), float(iou_weight), float(beta))
    dt = preds[0].dtype
    B = preds[0].shape[0]
    C = 4 * DFL_CH + nc
    for p in preds:
        if p.dim() != 4 or p.shape[0] != B or p.shape[1] != C or p.dtype != dt:
            raise ValueError(f"yms: head maps must be [B, {C}, H, W] of one dtype, got {tuple(p.shape)} {p.dtype}")
    bases = [_nhwc(p) for p in preds]
    ld = bases[0][1]
    if any(b[1] != ld for b in bases):          # one channel stride for every level: repack
        ld = (C + 7) // 8 * 8
        bases = []
        for p in preds:
            t = torch.zeros((B, p.shape[2], p.shape[3], ld), dtype=dt, device=p.device)
            t[..., :C] = p.permute(0, 2, 3, 1)
            bases.append((t, ld))
    dev = preds[0].device
    tg = targets.to(device=dev, dtype=torch.float32).reshape(-1, 6).contiguous()
    M = tg.shape[0]
    hs = [p.shape[2] for p in preds]
    ws = [p.shape[3] for p in preds]
    A = sum(h * w for h, w in zip(hs, ws))
    grads = None
    if need_grad:
        mk = torch.zeros if ld != C else torch.empty
        grads = [mk((B, h, w, ld), dtype=dt, device=dev) for h, w in zip(hs, ws)]
    agt = asc = dk = None
    if return_assignment:
        agt = torch.empty((B, A), dtype=torch.int32, device=dev)
        asc = torch.empty((B, A), dtype=torch.float32, device=dev)
        dk = torch.empty((M,), dtype=torch.int32, device=dev)
    wsb = L.lib().yms_dsl_loss_ws_bytes(B, A, nc, M)
    ws_t = torch.empty(wsb, dtype=torch.uint8, device=dev)
    out = torch.empty(5, dtype=torch.float32, device=dev)
    n = len(preds)
    maps = (ctypes.c_void_p * n)(*[b[0].data_ptr() for b in bases])
    gptr = (ctypes.c_void_p * n)(*[g.data_ptr() for g in grads]) if grads is not None else None
    img_h, img_w = img_size
    L.call("yms_dsl_loss", L.dtype_code(dt), B, nc, n, maps, gptr, (ctypes.c_int * n)(*hs), (ctypes.c_int * n)(*ws),
           (ctypes.c_float * n)(*[float(s) for s in strides[:n]]), ld, tg.data_ptr() if M else None, M,
           ctypes.c_float(float(img_w)), ctypes.c_float(float(img_h)), int(topk), ctypes.c_float(float(radius)),
           ctypes.c_float(float(iou_weight)), ctypes.c_float(float(beta)),
           (ctypes.c_float * 3)(*[float(x) for x in gains]), ws_t.data_ptr(), wsb, out.data_ptr(), L.ptr(agt),
           L.ptr(asc), L.ptr(dk) if M else None, L.stream_ptr(dev))
    if grads is not None:
        grads = [g[..., :C].permute(0, 3, 1, 2) for g in grads]
    if return_assignment:
        return out, grads, (agt, asc, dk)
    return out, grads


class _DslLossFn(torch.autograd.Function):
    """-> (total [], terms [3] = box, cls, dfl).  The kernels produce d(total)/d(maps) only, so the
    terms are marked non-differentiable, as in ``yolov8.tools.tal_loss._TalLossFn``."""

    @staticmethod
    def forward(ctx, cfg, targets, *preds):
        out, grads = dsl_loss(list(preds), targets, *cfg, need_grad=any(p.requires_grad for p in preds))
        ctx.grads = grads
        ctx.n_preds = len(preds)
        terms = out[1:4].clone()
        ctx.mark_non_differentiable(terms)
        return out[0].clone(), terms

    @staticmethod
    def backward(ctx, g, _gterms):
        grads = ctx.grads
        ctx.grads = None
        if grads is None:
            return (None, None) + (None,) * ctx.n_preds
        # grads *= g in place on the device (a no-op launch for the 1.0 seed of loss.backward())
        gf = g.detach().to(torch.float32).contiguous()
        n = len(grads)
        L.call("yms_scale_by_device_scalar", L.dtype_code(grads[0].dtype), n,
               (ctypes.c_void_p * n)(*[gr.data_ptr() for gr in grads]),
               (ctypes.c_long * n)(*[_storage_elems(gr) for gr in grads]), gf.data_ptr(), L.stream_ptr(gf.device))
        return (None, None, *grads)


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
        vals = torch.cat([total.detach().view(1), terms]).cpu().tolist()
        items = {"loss_box": vals[1], "loss_cls": vals[2], "loss_dfl": vals[3], "total_loss": vals[0]}
        return total, items

    def loss_tensor(self, preds_from_head, targets_collated):
        """-> (total [] device tensor, differentiable; terms [3] device tensor (box, cls, dfl), not
        differentiable); no host sync."""
        cfg = (self.num_classes, (self.img_size_h, self.img_size_w), self._strides, self.topk,
               self.soft_center_radius, self.iou_weight, self.beta,
               (self.lambda_box, self.lambda_cls, self.lambda_dfl))
        return _DslLossFn.apply(cfg, targets_collated, *preds_from_head)
