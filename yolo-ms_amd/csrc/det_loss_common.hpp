// Device helpers shared by the two detection losses (det_loss.hip: the reference's ComputeLoss;
// tal_loss.hip: the task-aligned assigner loss): head-map addressing, the DFL softmax, the IoU
// family with its analytic gradient, BCE-with-logits and the fixed-order block sum.
#pragma once
#include <cmath>

#include "yms_common.hpp"

namespace yms {

constexpr int DL_DFL = 16;              // bins per side (the head's reg_max)
constexpr int DL_TOPK = 10;
constexpr float DL_EPS = 1e-7f;
constexpr int DL_MAXL = 4;

struct LossLevels {
  const void* x[DL_MAXL];   // head maps, NHWC with channel stride ld
  void* g[DL_MAXL];         // gradients (same layout), may be null
  int h[DL_MAXL], w[DL_MAXL], off[DL_MAXL + 1];
  float stride[DL_MAXL];
  int nl, ld;
};

__device__ __forceinline__ int level_of(const LossLevels& L, int a) {
  int l = 0;
  while (l + 1 < L.nl && a >= L.off[l + 1]) ++l;
  return l;
}
// anchor a of image b -> element offset of its row, level, and pixel centre (loss.py:424-431)
__device__ __forceinline__ long anchor_row(const LossLevels& L, int b, int a, int& l, float& ax, float& ay) {
  l = level_of(L, a);
  const int r = a - L.off[l], hy = r / L.w[l], wx = r - hy * L.w[l];
  ax = ((float)wx + 0.5f) * L.stride[l];
  ay = ((float)hy + 0.5f) * L.stride[l];
  return (((long)b * L.h[l] + hy) * L.w[l] + wx) * L.ld;
}

template <typename T>
__device__ __forceinline__ void load_dist(const T* row, float (&v)[4 * DL_DFL]) {
#pragma unroll
  for (int k = 0; k < 4 * DL_DFL / 8; ++k) {
    float t[8];
    Vec8<T>::load(row + 8 * k, t);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[8 * k + i] = t[i];
  }
}

template <typename T>
__device__ __forceinline__ void store_dist(T* row, const float (&v)[4 * DL_DFL]) {
#pragma unroll
  for (int k = 0; k < 4 * DL_DFL / 8; ++k) {
    float t[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) t[i] = v[8 * k + i];
    Vec8<T>::store(row + 8 * k, t);
  }
}

// softmax of each side's bins in place (v -> probabilities), expected bin index e[s], and the
// log-sum-exp of each side's logits (log-probabilities as logit - lse, as log_softmax)
__device__ __forceinline__ void dfl_softmax(float (&v)[4 * DL_DFL], float (&e)[4], float (&lse)[4]) {
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    float m = v[s * DL_DFL];
#pragma unroll
    for (int i = 1; i < DL_DFL; ++i) m = fmaxf(m, v[s * DL_DFL + i]);
    float z = 0.f;
#pragma unroll
    for (int i = 0; i < DL_DFL; ++i) {
      const float q = expf(v[s * DL_DFL + i] - m);
      v[s * DL_DFL + i] = q;
      z += q;
    }
    lse[s] = m + logf(z);
    const float iz = 1.0f / z;
    float ex = 0.f;
#pragma unroll
    for (int i = 0; i < DL_DFL; ++i) {
      v[s * DL_DFL + i] *= iz;
      ex += v[s * DL_DFL + i] * (float)i;
    }
    e[s] = ex;
  }
}

// (cx, cy, w, h) -> x1 y1 x2 y2 as bbox_iou converts (loss.py:26-29)
__device__ __forceinline__ void cxcywh_to_xyxy(const float* c, float (&b)[4]) {
  b[0] = c[0] - c[2] / 2;
  b[1] = c[1] - c[3] / 2;
  b[2] = c[0] + c[2] / 2;
  b[3] = c[1] + c[3] / 2;
}

// IoU (iou_type 0) / GIoU (1) / DIoU (2) / CIoU (3) of xyxy boxes p, g as bbox_iou computes them
// (loss.py:9-91) and, GRAD, d(value)/d(p0..p3) in dp (CIoU's alpha detached)
template <bool GRAD>
__device__ __forceinline__ float box_iou_grad(const float (&p)[4], const float (&g)[4], int iou_type,
                                              float (&dp)[4]) {
  // IoU terms
  const float iwr = fminf(p[2], g[2]) - fmaxf(p[0], g[0]);
  const float ihr = fminf(p[3], g[3]) - fmaxf(p[1], g[1]);
  const float iw = fmaxf(iwr, 0.f), ih = fmaxf(ihr, 0.f);
  const float inter = iw * ih;
  const float w1 = p[2] - p[0], h1 = p[3] - p[1], w2 = g[2] - g[0], h2 = g[3] - g[1];
  const float un = w1 * h1 + w2 * h2 - inter + DL_EPS;
  const float iou = inter / un;
  float val = iou;
  // d(val)/d(p0..p3)
#pragma unroll
  for (int k = 0; k < 4; ++k) dp[k] = 0.f;
  if (GRAD) {
    // d iou = (d inter * un - inter * d un) / un^2,  d un = d(w1 h1) - d inter
    float di[4] = {0.f, 0.f, 0.f, 0.f};
    if (iwr >= 0.f) {         // clamp(min=0) passes the gradient at 0 (torch semantics)
      if (p[2] < g[2]) di[2] += ih;
      if (p[0] > g[0]) di[0] -= ih;
    }
    if (ihr >= 0.f) {
      if (p[3] < g[3]) di[3] += iw;
      if (p[1] > g[1]) di[1] -= iw;
    }
    const float da[4] = {-h1, -w1, h1, w1};
    const float iu2 = 1.f / (un * un);
#pragma unroll
    for (int k = 0; k < 4; ++k) dp[k] = (di[k] * un - inter * (da[k] - di[k])) * iu2;
  }
  if (iou_type != 0) {
    const float cwr = fmaxf(p[2], g[2]) - fminf(p[0], g[0]);
    const float chr = fmaxf(p[3], g[3]) - fminf(p[1], g[1]);
    const float cw = fmaxf(cwr, 0.f), ch = fmaxf(chr, 0.f);
    if (iou_type == 1) {       // GIoU
      const float ca = cw * ch + DL_EPS;
      val = iou - (ca - un) / ca;
      if (GRAD) {
        // d[-(ca - un)/ca] = -(d ca * un ... ) : -(1 - un/ca) -> d = (d un * ca - un * d ca) / ca^2
        float dca[4] = {0.f, 0.f, 0.f, 0.f};
        if (cwr >= 0.f) {
          if (p[2] > g[2]) dca[2] += ch;
          if (p[0] < g[0]) dca[0] -= ch;
        }
        if (chr >= 0.f) {
          if (p[3] > g[3]) dca[3] += cw;
          if (p[1] < g[1]) dca[1] -= cw;
        }
        // un' = d(w1 h1) - d inter: recompute d inter from dp is messy; rebuild it
        float di[4] = {0.f, 0.f, 0.f, 0.f};
        if (iwr >= 0.f) { if (p[2] < g[2]) di[2] += ih; if (p[0] > g[0]) di[0] -= ih; }
        if (ihr >= 0.f) { if (p[3] < g[3]) di[3] += iw; if (p[1] > g[1]) di[1] -= iw; }
        const float da[4] = {-h1, -w1, h1, w1};
#pragma unroll
        for (int k = 0; k < 4; ++k) dp[k] += ((da[k] - di[k]) * ca - un * dca[k]) / (ca * ca);
      }
    } else {                   // DIoU / CIoU
      const float rx = (p[0] + p[2]) / 2 - (g[0] + g[2]) / 2;
      const float ry = (p[1] + p[3]) / 2 - (g[1] + g[3]) / 2;
      const float rho2 = rx * rx + ry * ry;
      const float c2 = cw * cw + ch * ch;
      const float dterm = rho2 / c2;
      val = iou - dterm;
      if (GRAD) {
        // d(rho2/c2) = (d rho2 c2 - rho2 d c2) / c2^2
        const float drho[4] = {rx, ry, rx, ry};            // d rho2 / d p_k = 2 r * 1/2
        float dc2[4] = {0.f, 0.f, 0.f, 0.f};
        if (cwr >= 0.f) {
          if (p[2] > g[2]) dc2[2] += 2.f * cw;
          if (p[0] < g[0]) dc2[0] -= 2.f * cw;
        }
        if (chr >= 0.f) {
          if (p[3] > g[3]) dc2[3] += 2.f * ch;
          if (p[1] < g[1]) dc2[1] -= 2.f * ch;
        }
        const float ic = 1.f / (c2 * c2);
#pragma unroll
        for (int k = 0; k < 4; ++k) dp[k] -= (drho[k] * c2 - rho2 * dc2[k]) * ic;
      }
      if (iou_type == 3) {     // CIoU: - alpha v, alpha detached
        const float at = atanf(w2 / (h2 + DL_EPS)) - atanf(w1 / (h1 + DL_EPS));
        const float k4 = 4.f / (float)(M_PI * M_PI);
        const float vv = k4 * at * at;
        const float alpha = vv / (1.f - iou + vv + DL_EPS);
        val -= alpha * vv;
        if (GRAD) {
          // d v / d(w1, h1): v = k4 at^2, at = atan(w2/(h2+eps)) - atan(w1/(h1+eps))
          const float hh = h1 + DL_EPS;
          const float q = w1 / hh;
          const float den = 1.f / (1.f + q * q);
          const float dat_dw1 = -den / hh, dat_dh1 = den * w1 / (hh * hh);
          const float dv_dw1 = 2.f * k4 * at * dat_dw1, dv_dh1 = 2.f * k4 * at * dat_dh1;
          // w1 = p2 - p0, h1 = p3 - p1
          dp[0] += alpha * dv_dw1;
          dp[2] -= alpha * dv_dw1;
          dp[1] += alpha * dv_dh1;
          dp[3] -= alpha * dv_dh1;
        }
      }
    }
  }
  return val;
}

// BCEWithLogits value (1 - t) x + (1 + (pw - 1) t) softplus(-x) and its derivative
// sigmoid(x) (1 + (pw - 1) t) - pw t, from one exponential and one logarithm
__device__ __forceinline__ float bce_logits(float x, float t, float pw, float& dx) {
  const float e = __expf(-fabsf(x));
  const float r = __builtin_amdgcn_rcpf(1.f + e);
  const float sig = x >= 0.f ? r : e * r;
  const float lw = 1.f + (pw - 1.f) * t;
  dx = sig * lw - pw * t;
  // log(1 + e) by the hardware logarithm: absolute error ~1e-7 (also where e < eps and log1p
  // would keep more relative digits of a ~1e-7 term), well inside the loss tolerance
  return (1.f - t) * x + lw * (fmaxf(-x, 0.f) + __logf(1.f + e));
}

// block partial sums (fixed order) of one float per thread -> part[slot]
__device__ __forceinline__ void block_sum_store(float v, float* part, long slot) {
  __shared__ float s[4];
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) part[slot] = (s[0] + s[1]) + (s[2] + s[3]);
  __syncthreads();
}

}  // namespace yms
