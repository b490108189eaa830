// Device helpers shared by the detection losses (det_loss.hip: the reference's ComputeLoss;
// tal_loss.hip: the task-aligned assigner loss; dsl_loss.hip: the dynamic soft-label assigner loss): head-map addressing, the DFL softmax, the IoU
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

// ---- shared by the anchor-based assigner losses (tal_loss.hip, dsl_loss.hip) ------------------
constexpr float TAL_INSIDE_EPS = 1e-9f;
constexpr float TAL_DFL_MAX = (float)(DL_DFL - 1) - 0.01f;

// target row -> false when ignored (image outside [0, B) or class outside [0, nc)); image, class
// and the GT's xyxy box in pixels
__device__ __forceinline__ bool tal_row(const float* t, int B, int nc, float img_w, float img_h, int& b, int& cls,
                                        float (&g)[4]) {
  if (!(t[0] >= 0.f && t[0] < (float)B && t[1] >= 0.f && t[1] < (float)nc)) return false;
  b = (int)t[0];
  cls = (int)t[1];
  const float gc[4] = {t[2] * img_w, t[3] * img_h, t[4] * img_w, t[5] * img_h};
  cxcywh_to_xyxy(gc, g);
  return true;
}

__device__ __forceinline__ bool tal_inside(float ax, float ay, const float (&g)[4]) {
  return fminf(fminf(ax - g[0], ay - g[1]), fminf(g[2] - ax, g[3] - ay)) > TAL_INSIDE_EPS;
}

// block b of 256 threads: image b's valid target rows in target order -> rows[b * M ..], nrows[b]
// (global memory, so no limit on the rows of one image)
__device__ __forceinline__ void tal_list_rows(const float* tg, int M, int B, int nc, int* rows, int* nrows) {
  const int b = blockIdx.x, tid = threadIdx.x;
  int* mine = rows + (long)b * M;
  __shared__ int wcnt[4];
  int base = 0;
  for (int j0 = 0; j0 < M; j0 += 256) {
    const int j = j0 + tid;
    bool hit = false;
    if (j < M) {
      const float* t = tg + (long)j * 6;
      hit = t[0] >= 0.f && t[0] < (float)B && t[1] >= 0.f && t[1] < (float)nc && (int)t[0] == b;
    }
    const unsigned long long bal = __ballot(hit);
    if ((tid & 63) == 0) wcnt[tid >> 6] = __popcll(bal);
    __syncthreads();
    int pos = base;
    for (int q = 0; q < (tid >> 6); ++q) pos += wcnt[q];
    if (hit) mine[pos + __popcll(bal & ((1ull << (tid & 63)) - 1ull))] = j;
    base += (wcnt[0] + wcnt[1]) + (wcnt[2] + wcnt[3]);
    __syncthreads();
  }
  if (tid == 0) nrows[b] = base;
}

// fixed-order fp64 sum of one value per thread over a 256-thread block -> every thread
__device__ __forceinline__ double tal_block_sum(double v, double* sh) {
  __syncthreads();
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  return sh[0];
}

// 1 - IoU-family value (IOU: box_iou_grad's iou_type) and the DFL value (1/4 of the sides' two-bin cross entropies) of one foreground anchor
// and, GRAD, d/d logits scaled by sb, sd, left in v
template <bool GRAD, int IOU>
__device__ __forceinline__ void tal_box_dfl(float (&v)[4 * DL_DFL], float ax, float ay, float stride,
                                            const float (&g)[4], float sb, float sd, float& lbox, float& ldfl) {
  // DFL targets in stride units, clamped into the bins, read before the softmax
  const float dist[4] = {ax - g[0], ay - g[1], g[2] - ax, g[3] - ay};
  int li[4];
  float wl[4], wr[4], xl[4], xr[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const float d = fminf(fmaxf(dist[s] / stride, 0.f), TAL_DFL_MAX);
    const float fl = floorf(d);
    wr[s] = d - fl;
    wl[s] = 1.0f - wr[s];
    li[s] = (int)fl;                    // 0..14: the right bin li + 1 <= 15
    xl[s] = xr[s] = 0.f;
#pragma unroll
    for (int i = 0; i < DL_DFL; ++i) {  // selects, not a runtime index: v stays in registers
      xl[s] = i == li[s] ? v[s * DL_DFL + i] : xl[s];
      xr[s] = i == li[s] + 1 ? v[s * DL_DFL + i] : xr[s];
    }
  }
  float e[4], lse[4];
  dfl_softmax(v, e, lse);     // v: probabilities
  const float p[4] = {ax - e[0] * stride, ay - e[1] * stride, ax + e[2] * stride, ay + e[3] * stride};
  float dp[4];
  lbox = 1.f - box_iou_grad<GRAD>(p, g, IOU, dp);
  float dfl = 0.f;
#pragma unroll
  for (int s = 0; s < 4; ++s) dfl += (lse[s] - xl[s]) * wl[s] + (lse[s] - xr[s]) * wr[s];
  ldfl = 0.25f * dfl;
  if (GRAD) {
    // loss 1 - val -> d/dp = -dp; p0 = ax - e0 s (d/de0 = -s), p2 = ax + e2 s (d/de2 = s)
    const float k = sb * stride;
    const float ge[4] = {dp[0] * k, dp[1] * k, -dp[2] * k, -dp[3] * k};
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int i = 0; i < DL_DFL; ++i) {
        const float pr = v[s * DL_DFL + i];
        float gi = ge[s] * pr * ((float)i - e[s]);      // d e_s / d logit_i = p_i (i - e_s)
        gi += sd * (pr - (i == li[s] ? wl[s] : 0.f) - (i == li[s] + 1 ? wr[s] : 0.f));
        v[s * DL_DFL + i] = gi;
      }
  }
}

}  // namespace yms
