// Shared by the three detection losses (det_loss.hip: the reference's ComputeLoss; tal_loss.hip:
// the task-aligned assigner loss; dsl_loss.hip: the dynamic soft-label assigner loss).  Device:
// head-map addressing, the DFL softmax, the IoU family with its analytic gradient, BCE-with-logits,
// the fixed-order block sum and the block selection primitives (sorted insert, arg-extreme round,
// pop, count sum).  Host: the entries' argument checks and LossLevels fill, the dispatch on the map
// dtype.  What only the two assigner losses share is in assign_loss_common.hpp.
#pragma once
#include <cmath>
#include <cstddef>

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

// ---- block selection: every thread of a 256-thread block keeps a short sorted list of (value,
// index) and the block draws the lists' best entries one round at a time.  DESC: largest value
// first (sentinel -1, every real value is >= 0), else smallest first (sentinel +inf); equal values
// rank by lower index.  The exchange slots are shared by every call within one kernel.
constexpr int SEL_NONE = 0x7fffffff;     // index of a sentinel entry
template <bool DESC>
__device__ __forceinline__ float sel_sentinel() { return DESC ? -1.f : INFINITY; }
template <bool DESC>
__device__ __forceinline__ bool sel_before(float a, float b) { return DESC ? a > b : a < b; }

template <bool DESC, int N>
__device__ __forceinline__ void sel_clear(float (&v)[N]) {
#pragma unroll
  for (int q = 0; q < N; ++q) v[q] = sel_sentinel<DESC>();
}
template <bool DESC, int N>
__device__ __forceinline__ void sel_clear(float (&v)[N], int (&ix)[N]) {
#pragma unroll
  for (int q = 0; q < N; ++q) { v[q] = sel_sentinel<DESC>(); ix[q] = SEL_NONE; }
}

// thread-local sorted insert, in two steps: `if (sel_enters<DESC>(v, x)) sel_insert<DESC>(v, ix, x, i);`
// (the test stays at the call site: folded into sel_insert, the compiler reuses its load of the tail
// for the last step of the insert and the three selection kernels need 4 to 17 more registers).
// A thread meets its indices in ascending order, so the strict comparisons keep the earlier of
// equals first (an equal later index ranks after); NaN never enters.
template <bool DESC, int N>
__device__ __forceinline__ bool sel_enters(const float (&v)[N], float x) { return sel_before<DESC>(x, v[N - 1]); }
template <bool DESC, int N>
__device__ __forceinline__ void sel_insert(float (&v)[N], int (&ix)[N], float cv, int ci) {
#pragma unroll
  for (int q = 0; q < N; ++q) {
    if (sel_before<DESC>(cv, v[q])) {
      const float tv = v[q];
      const int ti = ix[q];
      v[q] = cv; ix[q] = ci;
      cv = tv; ci = ti;
    }
  }
}
// the same for values alone
template <bool DESC, int N>
__device__ __forceinline__ void sel_insert(float (&v)[N], float cv) {
#pragma unroll
  for (int q = 0; q < N; ++q) {
    if (sel_before<DESC>(cv, v[q])) { const float tv = v[q]; v[q] = cv; cv = tv; }
  }
}

// one round: block arg-extreme over every thread's list head (v, ix) -> the winner's value, index
// and owner thread, to every thread: value first, then lower index.  INDEXED = false is the round
// of a list of values alone (below): value first, then lower owner thread, and no index travels;
// the waves' winners are scanned in ascending owner order, so there the strict comparison suffices.
// The caller pops the owner's head with sel_pop, whose barrier frees the slots for the next round.
struct SelSlots {
  float rv[4];
  int ri[4], rt[4];
};
__device__ __forceinline__ SelSlots& sel_slots() {     // one set per kernel, whatever rounds it runs
  __shared__ SelSlots s;
  return s;
}
template <bool DESC, bool INDEXED = true>
__device__ __forceinline__ void sel_round(float v, int ix, float& wv, int& wi, int& wo) {
  SelSlots& s = sel_slots();
  const int tid = threadIdx.x;
  int owner = tid;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const float ov = __shfl_xor(v, m);
    const int oo = __shfl_xor(owner, m), oi = INDEXED ? __shfl_xor(ix, m) : oo;
    if (sel_before<DESC>(ov, v) || (ov == v && oi < (INDEXED ? ix : owner))) { v = ov; ix = oi; owner = oo; }
  }
  if ((tid & 63) == 0) {
    s.rv[tid >> 6] = v;
    s.rt[tid >> 6] = owner;
    if (INDEXED) s.ri[tid >> 6] = ix;
  }
  __syncthreads();
  wv = s.rv[0];
  wo = s.rt[0];
  wi = INDEXED ? s.ri[0] : wo;
  for (int q = 1; q < 4; ++q)
    if (sel_before<DESC>(s.rv[q], wv) || (INDEXED && s.rv[q] == wv && s.ri[q] < wi)) {
      wv = s.rv[q];
      wo = s.rt[q];
      wi = INDEXED ? s.ri[q] : wo;
    }
}
template <bool DESC>
__device__ __forceinline__ void sel_round(float v, float& wv, int& wo) {
  int wi;
  sel_round<DESC, false>(v, 0, wv, wi, wo);
}

// pop the head of the thread for which `mine` holds (the round's owner); the list refills with
// sentinels, so an emptied list offers the sentinel.  Every thread of the block calls it.
template <bool DESC, int N>
__device__ __forceinline__ void sel_pop(float (&v)[N], int (&ix)[N], bool mine) {
  if (mine) {
#pragma unroll
    for (int q = 0; q < N - 1; ++q) { v[q] = v[q + 1]; ix[q] = ix[q + 1]; }
    v[N - 1] = sel_sentinel<DESC>();
    ix[N - 1] = SEL_NONE;
  }
  __syncthreads();
}
template <bool DESC, int N>
__device__ __forceinline__ void sel_pop(float (&v)[N], bool mine) {
  if (mine) {
#pragma unroll
    for (int q = 0; q < N - 1; ++q) v[q] = v[q + 1];
    v[N - 1] = sel_sentinel<DESC>();
  }
  __syncthreads();
}

// sum of one int per thread over the block's four waves -> every thread
__device__ __forceinline__ int block_count_sum(int c) {
  __shared__ int scnt[4];
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) c += __shfl_xor(c, m);
  if ((threadIdx.x & 63) == 0) scnt[threadIdx.x >> 6] = c;
  __syncthreads();
  return (scnt[0] + scnt[1]) + (scnt[2] + scnt[3]);
}

// ---- host side, shared by the three entries --------------------------------------------------
// Argument checks common to yms_det_loss / yms_tal_loss / yms_dsl_loss (YMS_ERR_INVALID before
// YMS_ERR_UNSUPPORTED), then the levels and the anchor count.  Returns before any launch.
inline yms_status loss_levels(int batch, int nc, int nlevels, const void* const* maps, void* const* grads,
                              const int* hs, const int* ws_, const float* strides, int ld, const float* targets,
                              int n_targets, float img_w, float img_h, LossLevels& L, int& A) {
  if (batch <= 0 || nc <= 0 || nlevels <= 0 || nlevels > DL_MAXL || !maps || !hs || !ws_ || !strides ||
      n_targets < 0 || (n_targets > 0 && !targets))
    return YMS_ERR_INVALID;
  if (!(img_w > 0.f) || !(img_h > 0.f) || !std::isfinite(img_w) || !std::isfinite(img_h)) return YMS_ERR_INVALID;
  if (ld < 4 * DL_DFL + nc || ld % 8) return YMS_ERR_INVALID;
  long a_total = 0;
  for (int l = 0; l < nlevels; ++l) {
    if (!maps[l] || hs[l] <= 0 || ws_[l] <= 0 || !(strides[l] > 0.f) || !std::isfinite(strides[l]))
      return YMS_ERR_INVALID;
    if (grads && !grads[l]) return YMS_ERR_INVALID;
    a_total += (long)hs[l] * ws_[l];
    if (a_total >= (1l << 31)) return YMS_ERR_UNSUPPORTED;
  }
  if (a_total * ((nc + 7) / 8) >= (1l << 31) - 256) return YMS_ERR_UNSUPPORTED;
  if (batch > 65535) return YMS_ERR_UNSUPPORTED;          // images are the grid's y dimension
  L = LossLevels{};
  L.nl = nlevels;
  L.ld = ld;
  A = 0;
  for (int l = 0; l < nlevels; ++l) {
    L.x[l] = maps[l];
    L.g[l] = grads ? grads[l] : nullptr;
    L.h[l] = hs[l];
    L.w[l] = ws_[l];
    L.stride[l] = strides[l];
    L.off[l] = A;
    A += hs[l] * ws_[l];
  }
  L.off[nlevels] = A;
  return YMS_OK;
}

inline bool map_dtype_ok(int dtype) { return dtype == YMS_F32 || dtype == YMS_BF16 || dtype == YMS_F16; }

// launches(MapType<T>{}) with T the element type of `dtype` (map_dtype_ok), then the launch status
template <typename T>
struct MapType { using type = T; };
template <typename F>
inline yms_status launch_for_dtype(int dtype, F&& launches) {
  switch (dtype) {
    case YMS_F32: launches(MapType<float>{}); break;
    case YMS_BF16: launches(MapType<bf16>{}); break;
    case YMS_F16: launches(MapType<f16>{}); break;
    default: return YMS_ERR_INVALID;
  }
  return launch_status();
}

// 256-aligned pieces of a workspace
inline size_t ws_align(size_t x) { return (x + 255) / 256 * 256; }

}  // namespace yms
