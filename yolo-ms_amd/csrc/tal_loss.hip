// Task-aligned assigner loss on gfx950: YOLOv8's published v8DetectionLoss + TaskAlignedAssigner
// (restated in tests/tal_ref.py, which is the definition; DESIGN.md "Task-aligned loss"), fused with
// its analytic gradient like det_loss.hip.  Opt-in: yms_det_loss keeps the reference's semantics.
//
//   tal_decode_kernel  per anchor: DFL softmax, expected offsets, predicted xyxy box in pixels
//                      ((gx + .5 -+ e) * stride); clears the anchor's claim count / claimant
//   tal_topk_kernel    per target row: over the anchors whose centre lies inside the GT,
//                      m = sigmoid(class logit)^alpha * max(CIoU, 0)^beta; the first
//                      min(topk, #inside) by (m desc, anchor asc) claim their anchor
//                      (integer atomics: count += 1, claimant = min row)
//   assign_rows_kernel per image: its valid target rows, in target order, listed in global memory
//   tal_resolve_kernel per anchor: one claim -> that GT; several -> the GT with the largest overlap
//                      among ALL the image's GTs the anchor lies inside (lowest row on a tie), also
//                      one that did not claim it; the metric and overlap of the final pair, and
//                      per-GT maxima by atomicMax on the bit pattern of the non-negative floats
//   tal_score_kernel   per anchor: target score t = m * max_ov / (max_m + 1e-9), its class; block
//                      partial sums of t
// and then the tail it shares with dsl_loss.hip (assign_loss_common.hpp, where the rows kernel is too):
//   assign_norm_kernel one block: tss = max(sum t, 1) in fp64, fixed order
//   assign_cls_kernel  <TalBce> BCE-with-logits of every anchor x class against t at the assigned
//                      class, gradient scaled by B * lambda_cls / tss (read from device memory)
//   assign_box_kernel  <CIoU> per foreground anchor: (1 - CIoU) t and the two-bin DFL cross entropy t,
//                      and their gradient into the 64 DFL logits (zeros for background anchors)
//   assign_finalize_kernel  fp64 fixed-order sums / tss -> box, cls, dfl, B (7.5 box + 0.5 cls + 1.5 dfl)
//
// The top-k draws its anchors with the block selection primitives of det_loss_common.hpp.
// Deterministic: integer atomics and float maxima only, fixed-order partials, fp64 finals.  No host
// sync.  Target rows are never staged in LDS, so there is no row limit: a GT scans only the grid
// cells around its box, a contested anchor only its image's row list.  The class logits are read
// once (plus one gathered logit per inside pair), the DFL logits twice, the gradient written once.
#include <algorithm>
#include <climits>
#include <cmath>

#include "assign_loss_common.hpp"

namespace yms {

// max(CIoU, 0) of the predicted box and the GT (NaN -> 0)
__device__ __forceinline__ float tal_overlap(const float4 p4, const float (&g)[4]) {
  const float p[4] = {p4.x, p4.y, p4.z, p4.w};
  float dp[4];
  return fmaxf(box_iou_grad<false>(p, g, 3, dp), 0.f);
}

// alignment metric sigmoid(logit)^alpha * ov^beta (NaN -> 0, so every inside anchor ranks)
__device__ __forceinline__ float tal_metric(float logit, float ov, float alpha, float beta) {
  const float sc = 1.f / (1.f + expf(-logit));
  const float m = powf(sc, alpha) * powf(ov, beta);
  return m >= 0.f ? m : 0.f;
}

// bit pattern of a non-negative float (orders like the float; -0 -> +0)
__device__ __forceinline__ unsigned tal_bits(float v) { return __float_as_uint(v) & 0x7fffffffu; }

// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void tal_decode_kernel(LossLevels L, int A, float* pbox, int* cnt, int* agt) {
  const int a = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (a >= A) return;
  int l;
  float ax, ay;
  const long row = anchor_row(L, b, a, l, ax, ay);
  float v[4 * DL_DFL], e[4], lse[4];
  load_dist(reinterpret_cast<const T*>(L.x[l]) + row, v);
  dfl_softmax(v, e, lse);
  const float s = L.stride[l];
  const long i = (long)b * A + a;
  reinterpret_cast<float4*>(pbox)[i] = make_float4(ax - e[0] * s, ay - e[1] * s, ax + e[2] * s, ay + e[3] * s);
  cnt[i] = 0;
  agt[i] = INT_MAX;
}

// per target row j: its positives claim their anchors
template <typename T>
__global__ __launch_bounds__(256) void tal_topk_kernel(LossLevels L, const float* tg, int B, int A, int nc,
                                                       float img_w, float img_h, int topk, float alpha, float beta,
                                                       const float* pbox, int* cnt, int* agt, unsigned* mohat) {
  const int j = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) { mohat[2 * (long)j] = 0u; mohat[2 * (long)j + 1] = 0u; }
  int b, cls;
  float g[4];
  if (!tal_row(tg + (long)j * 6, B, nc, img_w, img_h, b, cls, g)) return;     // block-uniform
  // thread-local top-k, sorted (value desc, index asc); every inside anchor has m >= 0 > -1
  float bv[DL_TOPK];
  int bi[DL_TOPK];
  sel_clear<true>(bv, bi);
  int ninside = 0;
  const float4* pb = reinterpret_cast<const float4*>(pbox) + (long)b * A;
  // only the grid cells around the GT, one cell of slack per side (the exact test follows): per
  // level the rectangle [x0, x0 + rw) x [y0, y0 + rh), cells numbered level-major, then row-major,
  // so every thread still meets its anchors in ascending index.  NaN / huge boxes clamp to empty.
  int x0[DL_MAXL], y0[DL_MAXL], rw[DL_MAXL], pre[DL_MAXL + 1];
  pre[0] = 0;
#pragma unroll
  for (int l = 0; l < DL_MAXL; ++l) {
    x0[l] = y0[l] = rw[l] = 0;
    int n = 0;
    if (l < L.nl) {
      const float s = L.stride[l], W = (float)L.w[l], H = (float)L.h[l];
      x0[l] = (int)fminf(fmaxf(floorf(g[0] / s - 0.5f) - 1.f, 0.f), W);
      y0[l] = (int)fminf(fmaxf(floorf(g[1] / s - 0.5f) - 1.f, 0.f), H);
      const int x1 = (int)fminf(fmaxf(ceilf(g[2] / s - 0.5f) + 1.f, -1.f), W - 1.f);
      const int y1 = (int)fminf(fmaxf(ceilf(g[3] / s - 0.5f) + 1.f, -1.f), H - 1.f);
      rw[l] = max(x1 - x0[l] + 1, 0);
      n = rw[l] * max(y1 - y0[l] + 1, 0);
    }
    pre[l + 1] = pre[l] + n;
  }
  for (int idx = tid; idx < pre[DL_MAXL]; idx += 256) {
    int l = 0;
#pragma unroll
    for (int q = 1; q < DL_MAXL; ++q) l += idx >= pre[q] ? 1 : 0;
    const int r = idx - pre[l], yy = r / rw[l], hy = y0[l] + yy, wx = x0[l] + r - yy * rw[l];
    const int a = L.off[l] + hy * L.w[l] + wx;
    const float ax = ((float)wx + 0.5f) * L.stride[l], ay = ((float)hy + 0.5f) * L.stride[l];    // as anchor_row
    const long row = (((long)b * L.h[l] + hy) * L.w[l] + wx) * L.ld;
    if (!tal_inside(ax, ay, g)) continue;
    ++ninside;
    const float ov = tal_overlap(pb[a], g);
    const float m = tal_metric(to_f(reinterpret_cast<const T*>(L.x[l])[row + 4 * DL_DFL + cls]), ov, alpha, beta);
    if (sel_enters<true>(bv, m)) sel_insert<true>(bv, bi, m, a);
  }
  const int total = block_count_sum(ninside);
  const int k = total < topk ? total : topk;
  // k rounds of block argmax over each thread's current head (value desc, index asc)
  for (int r = 0; r < k; ++r) {
    float wv;
    int wi, wo;
    sel_round<true>(bv[0], bi[0], wv, wi, wo);
    if (tid == 0 && (unsigned)wi < (unsigned)A) {
      atomicAdd(&cnt[(long)b * A + wi], 1);
      atomicMin(&agt[(long)b * A + wi], j);
    }
    sel_pop<true>(bv, bi, tid == wo);
  }
}

// per anchor: its final GT (agt: target row or -1), the pair's metric, the per-GT maxima
template <typename T>
__global__ __launch_bounds__(256) void tal_resolve_kernel(LossLevels L, const float* tg, int M, int B, int A, int nc,
                                                          float img_w, float img_h, float alpha, float beta,
                                                          const float* pbox, const int* cnt, const int* rows,
                                                          const int* nrows, int* agt, float* am, unsigned* mohat) {
  const int a = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (a >= A) return;
  const long i = (long)b * A + a;
  const int c = cnt[i];
  int j = c > 0 ? agt[i] : -1;
  int l;
  float ax, ay;
  const long row = anchor_row(L, b, a, l, ax, ay);
  const float4 p4 = reinterpret_cast<const float4*>(pbox)[i];
  int tb, cls;
  float g[4];
  if (c > 1) {       // contested: the largest overlap among every GT of the image it lies inside
    float best = -1.f;
    j = -1;
    const int* mine = rows + (long)b * M;
    const int n = min(nrows[b], M);
    for (int k = 0; k < n; ++k) {                 // ascending rows: the first maximum is the lowest row
      const int q = mine[k];
      if ((unsigned)q >= (unsigned)M || !tal_row(tg + (long)q * 6, B, nc, img_w, img_h, tb, cls, g) ||
          !tal_inside(ax, ay, g))
        continue;
      const float ov = tal_overlap(p4, g);
      if (ov > best) { best = ov; j = q; }
    }
  }
  if (j < 0 || j >= M || !tal_row(tg + (long)j * 6, B, nc, img_w, img_h, tb, cls, g)) {
    agt[i] = -1;
    am[i] = 0.f;
    return;
  }
  const float ov = tal_overlap(p4, g);
  const float m = tal_metric(to_f(reinterpret_cast<const T*>(L.x[l])[row + 4 * DL_DFL + cls]), ov, alpha, beta);
  agt[i] = j;
  am[i] = m;
  atomicMax(&mohat[2 * (long)j], tal_bits(m));
  atomicMax(&mohat[2 * (long)j + 1], tal_bits(ov));
}

// per anchor: target score and class; block partial sums of the scores
__global__ __launch_bounds__(256) void tal_score_kernel(const float* tg, int A, const int* agt, const float* am,
                                                        const unsigned* mohat, float* tsc, int* acls, float* part,
                                                        int* out_gt, float* out_sc) {
  const int a = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  float t = 0.f;
  if (a < A) {
    const long i = (long)b * A + a;
    const int j = agt[i];
    int cls = -1;
    if (j >= 0) {
      const double mh = (double)__uint_as_float(mohat[2 * (long)j]), oh = (double)__uint_as_float(mohat[2 * (long)j + 1]);
      t = (float)((double)am[i] * oh / (mh + 1e-9));
      cls = (int)tg[(long)j * 6 + 1];
    }
    tsc[i] = t;
    acls[i] = cls;
    if (out_gt) out_gt[i] = j;
    if (out_sc) out_sc[i] = t;
  }
  block_sum_store(t, part, (long)b * gridDim.x + blockIdx.x);
}

// per-logit term of assign_cls_kernel: plain BCE-with-logits
struct TalBce {
  __device__ __forceinline__ float operator()(float x, float t, float& dx) const { return bce_logits(x, t, 1.f, dx); }
};

// workspace: the common pieces, then the pair metrics and the per-GT maxima
struct TalWs {
  AssignWs c;
  size_t am, mohat;
};
static TalWs tal_ws(int B, int A, int nc, int M) {
  TalWs w{assign_ws(B, A, nc, M), 0, 0};
  w.am = w.c.add((size_t)B * A * 4);
  w.mohat = w.c.add((size_t)(M > 0 ? M : 1) * 8);
  return w;
}

}  // namespace yms

using namespace yms;

extern "C" {

size_t yms_tal_loss_ws_bytes(int batch, int anchors, int nc, int n_targets) {
  if (batch <= 0 || anchors <= 0 || nc <= 0 || n_targets < 0) return 0;
  return tal_ws(batch, anchors, nc, n_targets).c.total;
}

yms_status yms_tal_loss(int dtype, int batch, int nc, int nlevels, const void* const* maps, void* const* grads,
                        const int* hs, const int* ws_, const float* strides, int ld, const float* targets,
                        int n_targets, float img_w, float img_h, int topk, float alpha, float beta,
                        const float* lambdas, void* ws, size_t ws_bytes, float* out, int* assign_gt,
                        float* assign_score, void* stream) {
  if (!out || !lambdas || !map_dtype_ok(dtype)) return YMS_ERR_INVALID;
  if (topk < 1 || topk > DL_TOPK || !(alpha >= 0.f) || !(beta >= 0.f) || !std::isfinite(alpha) ||
      !std::isfinite(beta))
    return YMS_ERR_INVALID;
  LossLevels L;
  int A;
  const yms_status bad = loss_levels(batch, nc, nlevels, maps, grads, hs, ws_, strides, ld, targets, n_targets,
                                     img_w, img_h, L, A);
  if (bad != YMS_OK) return bad;
  const TalWs w = tal_ws(batch, A, nc, n_targets);
  if (!ws || ws_bytes < w.c.total) return YMS_ERR_INVALID;
  float* pbox = ws_at<float>(ws, w.c.pbox);
  int* cnt = ws_at<int>(ws, w.c.cnt);
  int* agt = ws_at<int>(ws, w.c.agt);
  int* rows = ws_at<int>(ws, w.c.rows);
  int* nrows = ws_at<int>(ws, w.c.nrows);
  float* am = ws_at<float>(ws, w.am);
  unsigned* mohat = ws_at<unsigned>(ws, w.mohat);
  const int gxb = w.c.gxb, M = n_targets, B = batch;
  hipStream_t st = (hipStream_t)stream;
  return launch_for_dtype(dtype, [&](auto map_type) {
    using T = typename decltype(map_type)::type;
    hipLaunchKernelGGL(tal_decode_kernel<T>, dim3(gxb, B), dim3(256), 0, st, L, A, pbox, cnt, agt);
    if (M > 0) {
      hipLaunchKernelGGL(tal_topk_kernel<T>, dim3(M), dim3(256), 0, st, L, targets, B, A, nc, img_w, img_h, topk,
                         alpha, beta, pbox, cnt, agt, mohat);
      hipLaunchKernelGGL(assign_rows_kernel, dim3(B), dim3(256), 0, st, targets, M, B, nc, rows, nrows);
    }
    hipLaunchKernelGGL(tal_resolve_kernel<T>, dim3(gxb, B), dim3(256), 0, st, L, targets, M, B, A, nc, img_w, img_h,
                       alpha, beta, pbox, cnt, rows, nrows, agt, am, mohat);
    hipLaunchKernelGGL(tal_score_kernel, dim3(gxb, B), dim3(256), 0, st, targets, A, agt, am, mohat,
                       ws_at<float>(ws, w.c.tsc), ws_at<int>(ws, w.c.acls), ws_at<float>(ws, w.c.partt), assign_gt,
                       assign_score);
    // total = B (lam_box box + lam_cls cls + lam_dfl dfl), every term a sum over tss; CIoU
    assign_loss_tail<T, 3>(L, w.c, ws, targets, M, B, A, nc, img_w, img_h, TalBce{}, (float)B, lambdas, out,
                           nullptr, st);
  });
}

}  // extern "C"
