// What the NMS prep decides per anchor, shared by nms_prep_kernel (head_nms.hip) and the candidate
// stage of the COCO-protocol detect (detect.hip), so both write the same bits for the same anchor;
// and the NMS's overlap predicate, shared by its kernels and detect.hip's box voting.
#pragma once
#include "yms_common.hpp"

#pragma clang fp contract(off)   // both users compile their whole file this way

namespace yms {

// One anchor's best class over its row q = (cx, cy, w, h, score[nc]), computed by the 16 lanes
// `sub` = 0..15 of the anchor's group: lane `sub` walks classes sub, sub + 16, ... (loads batched 8
// deep; nc = 80: one batch), then the lanes combine by xor shuffles -- max score, ties to the lower
// class.  Lane 0 of the group holds the result.
__device__ __forceinline__ void nms_pick16(const float* q, int nc, int sub, float& best, int& bl) {
  best = -INFINITY;
  bl = 0x7fffffff;
  bool any = false;
  for (int c0 = sub; c0 < nc; c0 += 128) {
    float v8[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int c = c0 + 16 * u;
      v8[u] = c < nc ? q[4 + c] : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int c = c0 + 16 * u;
      if (c < nc && (!any || v8[u] > best)) { best = v8[u]; bl = c; any = true; }
    }
  }
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) {
    const float ob = __shfl_xor(best, off, 16);
    const int ol = __shfl_xor(bl, off, 16);
    if (ob > best || (ob == best && ol < bl)) { best = ob; bl = ol; }
  }
}

// (cx, cy, w, h) -> (x1, y1, x2, y2); compiled without FP contraction in both users.
__device__ __forceinline__ float4 nms_xyxy(const float* q) {
  const float cx = q[0], cy = q[1], w = q[2], h = q[3];
  return make_float4(cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2);
}

// The NMS's overlap predicate, torchvision's CPU kernel op for op (fp32, no +1, the ratio compared as
// a double); the class-wise NMS kernels and the box voting of yms_det_finalize_vote decide with this
// one function, so that no rounding can make the two disagree on a pair.
__device__ __forceinline__ bool iou_gt(const float4& i, const float4& j, double thr) {
  const float iarea = (i.z - i.x) * (i.w - i.y);
  const float jarea = (j.z - j.x) * (j.w - j.y);
  const float xx1 = fmaxf(i.x, j.x);
  const float yy1 = fmaxf(i.y, j.y);
  const float xx2 = fminf(i.z, j.z);
  const float yy2 = fminf(i.w, j.w);
  const float w = fmaxf(0.0f, xx2 - xx1);
  const float h = fmaxf(0.0f, yy2 - yy1);
  const float inter = w * h;
  const float ovr = inter / (iarea + jarea - inter);
  return (double)ovr > thr;
}

}  // namespace yms
