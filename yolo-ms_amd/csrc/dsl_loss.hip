// YOLO-MS's own loss on gfx950 (opt-in): the RTMDet recipe's dynamic soft-label assigner, Quality
// Focal Loss on the class logits and GIoU on the boxes, both weighted by the matched IoU (restated in
// tests/dsl_ref.py, which is the definition; DESIGN.md "Dynamic soft-label loss"), fused with its
// analytic gradient like tal_loss.hip.
//
//   assign_rows_kernel   per image: its valid target rows, in target order, listed in global memory
//   dsl_decode_kernel    per anchor: DFL softmax -> predicted xyxy box in pixels; S(a) = sum over the
//                        classes of the background QFL softplus(x) sigmoid(x)^beta (the class logits
//                        are read once here, not once per GT); candidate flag = the centre lies inside
//                        at least one GT of the image; clears the anchor's claim count / claimant
//   dsl_select_kernel    per target row: ONE scan of the image's candidates keeps, per thread, the 13
//                        largest IoUs and the 13 lowest (cost, anchor), skipping the cost of anchors
//                        whose prior alone exceeds a bound 13 seen costs lie under; block-argmax rounds sum the
//                        min(topk, n_cand) largest IoUs -> k = max(1, floor(sum)); k block-argmin rounds
//                        (cost asc, anchor asc) claim their anchors (integer atomics: count += 1,
//                        claimant = min row)
//   dsl_resolve_kernel   per anchor: one claim -> that GT; several -> the GT of lowest cost among ALL
//                        the image's valid GTs (lowest row on a tie), also one that did not claim it;
//                        t = IoU of the final pair, its class; block partial sums of t
// and then the tail it shares with tal_loss.hip (assign_loss_common.hpp, where the rows kernel is too):
//   assign_norm_kernel   one block: norm = max(sum t, 1) in fp64, fixed order
//   assign_cls_kernel    <DslQfl> QFL of every anchor x class (target t at the assigned class, 0
//                        elsewhere), gradient scaled by cls_gain / norm (read from device memory)
//   assign_box_kernel    <GIoU> per foreground anchor: (1 - GIoU) t and the two-bin DFL cross entropy t,
//                        and their gradient into the 64 DFL logits (zeros for background anchors)
//   assign_finalize_kernel  fp64 fixed-order sums / norm -> total, box, cls, dfl, norm
//
// The lists and rounds of dsl_select_kernel are the block selection primitives of det_loss_common.hpp.
// The cost of a pair comes from ONE function, dsl_pair, for selection and resolution alike, so the
// two passes rank identically.  Deterministic: integer atomics only, fixed-order partials, fp64
// finals.  No host sync.  Target rows are never staged in LDS, so there is no row limit.
#include <algorithm>
#include <climits>
#include <cmath>

#include "assign_loss_common.hpp"

namespace yms {

constexpr int DSL_TOPK = 13;
constexpr float DSL_PRIOR_CAP = 30.f;

struct DslParams {
  float radius, iou_weight, beta;
  int topk;
};

// v^p for v >= 0 (p = 2, the recipe's, without the library call)
__device__ __forceinline__ float dsl_pow(float v, float p) {
  if (p == 1.f) return v;
  if (p == 2.f) return v * v;
  return powf(v, p);
}

// Quality focal term BCEwithlogits(x, t) |t - sigmoid(x)|^beta and its derivative in x
// (t = 0: softplus(x) sigmoid(x)^beta)
__device__ __forceinline__ float dsl_qfl(float x, float t, float beta, float& dx) {
  const float e = __expf(-fabsf(x));
  const float r = __builtin_amdgcn_rcpf(1.f + e);
  const float sig = x >= 0.f ? r : e * r;
  const float bce = (1.f - t) * x + (fmaxf(-x, 0.f) + __logf(1.f + e));
  const float d = t - sig, ad = fabsf(d);
  const float w1 = dsl_pow(ad, beta - 1.f);        // |d|^(beta - 1); beta >= 1
  const float w = w1 * ad;
  const float sgn = d > 0.f ? -1.f : (d < 0.f ? 1.f : 0.f);     // d|d|/dx = -sign(d) sigmoid'
  dx = (sig - t) * w + bce * beta * w1 * sgn * (e * r * r);     // sigmoid' = e r^2
  return bce * w;
}

// plain IoU of the predicted box and the GT (NaN -> 0)
__device__ __forceinline__ float dsl_iou(const float4 p4, const float (&g)[4]) {
  const float p[4] = {p4.x, p4.y, p4.z, p4.w};
  float dp[4];
  const float o = box_iou_grad<false>(p, g, 0, dp);
  return o >= 0.f ? o : 0.f;
}

// soft centre prior 10^min(dist / stride - radius, 30), dist from the anchor centre to the GT centre
__device__ __forceinline__ float dsl_prior(float ax, float ay, float stride, const float (&g)[4], float radius) {
  const float rx = ax - (g[0] + g[2]) * 0.5f, ry = ay - (g[1] + g[3]) * 0.5f;
  const float dist = sqrtf(rx * rx + ry * ry);
  return exp10f(fminf(dist / stride - radius, DSL_PRIOR_CAP));
}

// One (anchor, GT) pair: iou (above) and its assignment cost = [S - background term of the GT's class +
// QFL against the soft label iou] - iou_weight log(iou + 1e-7) + prior.  Used by selection and
// resolution alike.
__device__ __forceinline__ float dsl_pair(const float4 p4, float S, float xcls, float ax, float ay, float stride,
                                          const float (&g)[4], const DslParams& P, float& iou) {
  float dx;
  iou = dsl_iou(p4, g);
  const float ccls = S - dsl_qfl(xcls, 0.f, P.beta, dx) + dsl_qfl(xcls, iou, P.beta, dx);
  const float cbox = -logf(iou + DL_EPS) * P.iou_weight;
  const float cpri = dsl_prior(ax, ay, stride, g, P.radius);
  return ccls + cbox + cpri;
}

// Bound ladder of dsl_select_kernel: lad[q] counts the costs <= DSL_LADDER[q] around the GT centre.
constexpr int DSL_NLAD = 8;
__device__ constexpr float DSL_LADDER[DSL_NLAD] = {4.f, 8.f, 16.f, 32.f, 64.f, 256.f, 4096.f, 1e6f};

// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void dsl_decode_kernel(LossLevels L, const float* tg, int M, int B, int A, int nc,
                                                         float img_w, float img_h, float beta, const int* rows,
                                                         const int* nrows, float* pbox, float* S, int* cand, int* cnt,
                                                         int* agt) {
  const int a = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (a >= A) return;
  int l;
  float ax, ay;
  const long row = anchor_row(L, b, a, l, ax, ay);
  const T* x = reinterpret_cast<const T*>(L.x[l]) + row;
  float e[4];
  {
    float v[4 * DL_DFL], lse[4];
    load_dist(x, v);
    dfl_softmax(v, e, lse);
  }
  const float s = L.stride[l];
  const long i = (long)b * A + a;
  reinterpret_cast<float4*>(pbox)[i] = make_float4(ax - e[0] * s, ay - e[1] * s, ax + e[2] * s, ay + e[3] * s);
  float acc = 0.f;
  for (int c0 = 0; c0 < nc; c0 += 8) {
    const int nv = min(8, nc - c0);
    float xv[8];
    load8(x + 4 * DL_DFL + c0, nv, xv);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      float dx;
      if (k < nv) acc += dsl_qfl(xv[k], 0.f, beta, dx);
    }
  }
  S[i] = acc;
  int flag = 0;
  if (M > 0) {
    const int* mine = rows + (long)b * M;
    const int n = min(nrows[b], M);
    for (int k = 0; k < n && !flag; ++k) {
      const int q = mine[k];
      int tb, cls;
      float g[4];
      if ((unsigned)q < (unsigned)M && tal_row(tg + (long)q * 6, B, nc, img_w, img_h, tb, cls, g) &&
          tal_inside(ax, ay, g))
        flag = 1;
    }
  }
  cand[i] = flag;
  cnt[i] = 0;
  agt[i] = INT_MAX;
}

// per target row j: dynamic k, then its k cheapest candidates claim their anchors
template <typename T>
__global__ __launch_bounds__(256) void dsl_select_kernel(LossLevels L, const float* tg, int B, int A, int nc,
                                                         float img_w, float img_h, DslParams P, const float* pbox,
                                                         const float* S, const int* cand, int* cnt, int* agt,
                                                         int* dyn_k) {
  const int j = blockIdx.x, tid = threadIdx.x;
  int b, cls;
  float g[4];
  if (!tal_row(tg + (long)j * 6, B, nc, img_w, img_h, b, cls, g)) {      // block-uniform
    if (tid == 0 && dyn_k) dyn_k[j] = 0;
    return;
  }
  // thread-local lists: the largest IoUs (desc) and the cheapest (cost asc, anchor asc); a thread meets
  // its anchors in ascending index, so a strict comparison keeps the earlier of equals first
  float tv[DSL_TOPK], cv[DSL_TOPK];
  int ci[DSL_TOPK];
  sel_clear<true>(tv);
  sel_clear<false>(cv, ci);
  int ncand = 0;
  const float4* pb = reinterpret_cast<const float4*>(pbox) + (long)b * A;
  const float* Sb = S + (long)b * A;
  const int* cb = cand + (long)b * A;
  // Far anchors are skipped by an exact bound.  cost >= prior (the class and box terms are >= 0 up to
  // rounding), and once DSL_TOPK candidates with cost <= X are known, no anchor whose prior exceeds X can
  // be among a GT's <= DSL_TOPK cheapest.  X comes from a pre-pass over the 7 x 7 cells around the GT
  // centre on every level (one anchor per thread): the waves count those costs under each rung of a
  // fixed ladder (integer LDS atomics) and every thread takes the lowest rung with DSL_TOPK costs under
  // it (none: no skipping).  A skipped anchor still counts as a candidate and still offers its IoU; the
  // picks do not depend on which anchors were skipped.
  __shared__ int lad[DSL_NLAD];
  if (tid < DSL_NLAD) lad[tid] = 0;
  __syncthreads();
  {
    float cost = INFINITY;
    const int l = tid / 49, r = tid - l * 49;
    if (l < L.nl) {
      const float s = L.stride[l];
      const float fx = floorf((g[0] + g[2]) * 0.5f / s), fy = floorf((g[1] + g[3]) * 0.5f / s);
      const float wxf = fx + (float)(r % 7 - 3), hyf = fy + (float)(r / 7 - 3);
      if (wxf >= 0.f && wxf < (float)L.w[l] && hyf >= 0.f && hyf < (float)L.h[l]) {      // false for NaN
        const int wx = (int)wxf, hy = (int)hyf;
        const int a = L.off[l] + hy * L.w[l] + wx;
        if (cb[a]) {
          const long row = (((long)b * L.h[l] + hy) * L.w[l] + wx) * L.ld;
          const float xc = to_f(reinterpret_cast<const T*>(L.x[l])[row + 4 * DL_DFL + cls]);
          float iou_;
          cost = dsl_pair(pb[a], Sb[a], xc, ((float)wx + 0.5f) * s, ((float)hy + 0.5f) * s, s, g, P, iou_);
        }
      }
    }
#pragma unroll
    for (int q = 0; q < DSL_NLAD; ++q) {
      const int under = __popcll(__ballot(cost <= DSL_LADDER[q]));
      if ((tid & 63) == 0 && under) atomicAdd(&lad[q], under);
    }
  }
  __syncthreads();
  float bound = INFINITY;
#pragma unroll
  for (int q = DSL_NLAD - 1; q >= 0; --q)
    if (lad[q] >= DSL_TOPK) bound = DSL_LADDER[q];
  for (int a = tid; a < A; a += 256) {
    if (cb[a]) {
      ++ncand;
      int l;
      float ax, ay;
      const long row = anchor_row(L, b, a, l, ax, ay);
      const float4 p4 = pb[a];
      const float iou = dsl_iou(p4, g);
      if (sel_enters<true>(tv, iou)) sel_insert<true>(tv, iou);
      // margin: S - background term and the box term may round below 0 by ~1e-6 of their size
      if (!(dsl_prior(ax, ay, L.stride[l], g, P.radius) > bound * 1.0001f + 1.f)) {
        const float xc = to_f(reinterpret_cast<const T*>(L.x[l])[row + 4 * DL_DFL + cls]);
        float iou_;
        const float cost = dsl_pair(p4, Sb[a], xc, ax, ay, L.stride[l], g, P, iou_);
        if (sel_enters<false>(cv, cost)) sel_insert<false>(cv, ci, cost, a);
      }
    }
  }
  const int total = block_count_sum(ncand);
  if (total == 0) {                                   // no candidate in the image: nothing assigned
    if (tid == 0 && dyn_k) dyn_k[j] = 0;
    return;
  }
  // the n = min(topk, n_cand) largest IoUs of the block: n argmax rounds over each thread's head,
  // summed in fp64 in descending order by every thread alike
  const int n = total < P.topk ? total : P.topk;
  double ssum = 0.0;
  for (int r = 0; r < n; ++r) {     // value desc, then lower owner thread
    float wv;
    int wo;
    sel_round<true>(tv[0], wv, wo);
    ssum += (double)fmaxf(wv, 0.f);
    sel_pop<true>(tv, tid == wo);
  }
  int k = (int)floor(ssum);
  k = k < 1 ? 1 : (k > n ? n : k);
  if (tid == 0 && dyn_k) dyn_k[j] = k;
  // k rounds of block argmin over each thread's current head (cost asc, anchor asc)
  for (int r = 0; r < k; ++r) {
    float wv;
    int wi, wo;
    sel_round<false>(cv[0], ci[0], wv, wi, wo);
    if (tid == 0 && (unsigned)wi < (unsigned)A) {
      atomicAdd(&cnt[(long)b * A + wi], 1);
      atomicMin(&agt[(long)b * A + wi], j);
    }
    sel_pop<false>(cv, ci, tid == wo && (unsigned)wi < (unsigned)A);
  }
}

// per anchor: its final GT (target row or -1), soft label t and class; block partial sums of t
template <typename T>
__global__ __launch_bounds__(256) void dsl_resolve_kernel(LossLevels L, const float* tg, int M, int B, int A, int nc,
                                                          float img_w, float img_h, DslParams P, const float* pbox,
                                                          const float* S, const int* cnt, const int* rows,
                                                          const int* nrows, int* agt, float* tsc, int* acls,
                                                          float* part, int* out_gt, float* out_sc) {
  const int a = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  float t = 0.f;
  if (a < A) {
    const long i = (long)b * A + a;
    const int c = cnt[i];
    int j = c > 0 ? agt[i] : -1;
    int acl = -1;
    if (c > 0) {
      int l;
      float ax, ay;
      const long row = anchor_row(L, b, a, l, ax, ay);
      const T* xc = reinterpret_cast<const T*>(L.x[l]) + row + 4 * DL_DFL;
      const float4 p4 = reinterpret_cast<const float4*>(pbox)[i];
      const float Sa = S[i], s = L.stride[l];
      int tb, cls;
      float g[4];
      if (c > 1) {       // contested: the lowest cost among every valid GT of the image
        float best = INFINITY;
        j = -1;
        const int* mine = rows + (long)b * M;
        const int n = min(nrows[b], M);
        for (int k = 0; k < n; ++k) {               // ascending rows: the first minimum is the lowest row
          const int q = mine[k];
          if ((unsigned)q >= (unsigned)M || !tal_row(tg + (long)q * 6, B, nc, img_w, img_h, tb, cls, g)) continue;
          float iou;
          const float cost = dsl_pair(p4, Sa, to_f(xc[cls]), ax, ay, s, g, P, iou);
          if (cost < best) { best = cost; j = q; }
        }
      }
      if (j >= 0 && j < M && tal_row(tg + (long)j * 6, B, nc, img_w, img_h, tb, cls, g)) {
        dsl_pair(p4, Sa, to_f(xc[cls]), ax, ay, s, g, P, t);
        acl = cls;
      } else {
        j = -1;
      }
    }
    agt[i] = j;
    tsc[i] = t;
    acls[i] = acl;
    if (out_gt) out_gt[i] = j;
    if (out_sc) out_sc[i] = t;
  }
  block_sum_store(t, part, (long)b * gridDim.x + blockIdx.x);
}

// per-logit term of assign_cls_kernel: the quality focal term
struct DslQfl {
  float beta;
  __device__ __forceinline__ float operator()(float x, float t, float& dx) const { return dsl_qfl(x, t, beta, dx); }
};

// workspace: the common pieces, then the background sums and the candidate flags
struct DslWs {
  AssignWs c;
  size_t S, cand;
};
static DslWs dsl_ws(int B, int A, int nc, int M) {
  DslWs w{assign_ws(B, A, nc, M), 0, 0};
  w.S = w.c.add((size_t)B * A * 4);
  w.cand = w.c.add((size_t)B * A * 4);
  return w;
}

}  // namespace yms

using namespace yms;

extern "C" {

size_t yms_dsl_loss_ws_bytes(int batch, int anchors, int nc, int n_targets) {
  if (batch <= 0 || anchors <= 0 || nc <= 0 || n_targets < 0) return 0;
  return dsl_ws(batch, anchors, nc, n_targets).c.total;
}

yms_status yms_dsl_loss(int dtype, int batch, int nc, int nlevels, const void* const* maps, void* const* grads,
                        const int* hs, const int* ws_, const float* strides, int ld, const float* targets,
                        int n_targets, float img_w, float img_h, int topk, float radius, float iou_weight,
                        float beta, const float* gains, void* ws, size_t ws_bytes, float* out, int* assign_gt,
                        float* assign_score, int* dynamic_k, void* stream) {
  if (!out || !gains || !map_dtype_ok(dtype)) return YMS_ERR_INVALID;
  if (topk < 1 || topk > DSL_TOPK || !(radius >= 0.f) || !(iou_weight >= 0.f) || !(beta >= 1.f) ||
      !std::isfinite(radius) || !std::isfinite(iou_weight) || !std::isfinite(beta))
    return YMS_ERR_INVALID;
  LossLevels L;
  int A;
  const yms_status bad = loss_levels(batch, nc, nlevels, maps, grads, hs, ws_, strides, ld, targets, n_targets,
                                     img_w, img_h, L, A);
  if (bad != YMS_OK) return bad;
  const DslWs w = dsl_ws(batch, A, nc, n_targets);
  if (!ws || ws_bytes < w.c.total) return YMS_ERR_INVALID;
  float* pbox = ws_at<float>(ws, w.c.pbox);
  int* cnt = ws_at<int>(ws, w.c.cnt);
  int* agt = ws_at<int>(ws, w.c.agt);
  int* rows = ws_at<int>(ws, w.c.rows);
  int* nrows = ws_at<int>(ws, w.c.nrows);
  float* S = ws_at<float>(ws, w.S);
  int* cand = ws_at<int>(ws, w.cand);
  const int gxb = w.c.gxb, M = n_targets, B = batch;
  hipStream_t st = (hipStream_t)stream;
  const DslParams P{radius, iou_weight, beta, topk};
  return launch_for_dtype(dtype, [&](auto map_type) {
    using T = typename decltype(map_type)::type;
    if (M > 0) hipLaunchKernelGGL(assign_rows_kernel, dim3(B), dim3(256), 0, st, targets, M, B, nc, rows, nrows);
    hipLaunchKernelGGL(dsl_decode_kernel<T>, dim3(gxb, B), dim3(256), 0, st, L, targets, M, B, A, nc, img_w, img_h,
                       beta, rows, nrows, pbox, S, cand, cnt, agt);
    if (M > 0)
      hipLaunchKernelGGL(dsl_select_kernel<T>, dim3(M), dim3(256), 0, st, L, targets, B, A, nc, img_w, img_h, P, pbox,
                         S, cand, cnt, agt, dynamic_k);
    hipLaunchKernelGGL(dsl_resolve_kernel<T>, dim3(gxb, B), dim3(256), 0, st, L, targets, M, B, A, nc, img_w, img_h,
                       P, pbox, S, cnt, rows, nrows, agt, ws_at<float>(ws, w.c.tsc), ws_at<int>(ws, w.c.acls),
                       ws_at<float>(ws, w.c.partt), assign_gt, assign_score);
    // total = g_box box + g_cls cls + g_dfl dfl, every term a sum over norm (no factor B); GIoU
    assign_loss_tail<T, 1>(L, w.c, ws, targets, M, B, A, nc, img_w, img_h, DslQfl{beta}, 1.f, gains, out, out + 4,
                           st);
  });
}

}  // extern "C"
