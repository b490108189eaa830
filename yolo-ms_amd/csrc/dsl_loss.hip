// YOLO-MS's own loss on gfx950 (opt-in): the RTMDet recipe's dynamic soft-label assigner, Quality
// Focal Loss on the class logits and GIoU on the boxes, both weighted by the matched IoU (restated in
// tests/dsl_ref.py, which is the definition; DESIGN.md "Dynamic soft-label loss"), fused with its
// analytic gradient like tal_loss.hip.
//
//   dsl_rows_kernel      per image: its valid target rows, in target order, listed in global memory
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
//   dsl_norm_kernel      one block: norm = max(sum t, 1) in fp64, fixed order
//   dsl_cls_kernel       QFL of every anchor x class (target t at the assigned class, 0 elsewhere),
//                        gradient scaled by cls_gain / norm (read from device memory)
//   dsl_box_kernel       per foreground anchor: (1 - GIoU) t and the two-bin DFL cross entropy t, and
//                        their gradient into the 64 DFL logits (zeros for background anchors)
//   dsl_finalize_kernel  fp64 fixed-order sums / norm -> total, box, cls, dfl, norm
//
// The cost of a pair comes from ONE function, dsl_pair, for selection and resolution alike, so the
// two passes rank identically.  Deterministic: integer atomics only, fixed-order partials, fp64
// finals.  No host sync.  Target rows are never staged in LDS, so there is no row limit.
#include <algorithm>
#include <climits>
#include <cmath>

#include "det_loss_common.hpp"

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
#pragma unroll
  for (int q = 0; q < DSL_TOPK; ++q) { tv[q] = -1.f; cv[q] = INFINITY; ci[q] = 0x7fffffff; }
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
      if (iou > tv[DSL_TOPK - 1]) {
        float v = iou;
#pragma unroll
        for (int q = 0; q < DSL_TOPK; ++q) {
          if (v > tv[q]) { const float t_ = tv[q]; tv[q] = v; v = t_; }
        }
      }
      // margin: S - background term and the box term may round below 0 by ~1e-6 of their size
      if (!(dsl_prior(ax, ay, L.stride[l], g, P.radius) > bound * 1.0001f + 1.f)) {
        const float xc = to_f(reinterpret_cast<const T*>(L.x[l])[row + 4 * DL_DFL + cls]);
        float iou_;
        const float cost = dsl_pair(p4, Sb[a], xc, ax, ay, L.stride[l], g, P, iou_);
        if (cost < cv[DSL_TOPK - 1]) {     // strictly less: an equal later index ranks after; NaN never enters
          float v = cost;
          int ix = a;
#pragma unroll
          for (int q = 0; q < DSL_TOPK; ++q) {
            if (v < cv[q]) {
              const float t_ = cv[q];
              const int i_ = ci[q];
              cv[q] = v; ci[q] = ix;
              v = t_; ix = i_;
            }
          }
        }
      }
    }
  }
  __shared__ int scnt[4];
  __shared__ float rv[4];
  __shared__ int ri[4], rt[4];
  int c = ncand;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) c += __shfl_xor(c, m);
  if ((tid & 63) == 0) scnt[tid >> 6] = c;
  __syncthreads();
  const int total = (scnt[0] + scnt[1]) + (scnt[2] + scnt[3]);
  if (total == 0) {                                   // no candidate in the image: nothing assigned
    if (tid == 0 && dyn_k) dyn_k[j] = 0;
    return;
  }
  // the n = min(topk, n_cand) largest IoUs of the block: n argmax rounds over each thread's head,
  // summed in fp64 in descending order by every thread alike
  const int n = total < P.topk ? total : P.topk;
  double ssum = 0.0;
  for (int r = 0; r < n; ++r) {
    float v = tv[0];
    int owner = tid;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const float ov = __shfl_xor(v, m);
      const int oo = __shfl_xor(owner, m);
      if (ov > v || (ov == v && oo < owner)) { v = ov; owner = oo; }
    }
    if ((tid & 63) == 0) { rv[tid >> 6] = v; rt[tid >> 6] = owner; }
    __syncthreads();
    float wv = rv[0];
    int wo = rt[0];
    for (int q = 1; q < 4; ++q)
      if (rv[q] > wv) { wv = rv[q]; wo = rt[q]; }
    ssum += (double)fmaxf(wv, 0.f);
    if (tid == wo) {
#pragma unroll
      for (int q = 0; q < DSL_TOPK - 1; ++q) tv[q] = tv[q + 1];
      tv[DSL_TOPK - 1] = -1.f;
    }
    __syncthreads();
  }
  int k = (int)floor(ssum);
  k = k < 1 ? 1 : (k > n ? n : k);
  if (tid == 0 && dyn_k) dyn_k[j] = k;
  // k rounds of block argmin over each thread's current head (cost asc, anchor asc)
  for (int r = 0; r < k; ++r) {
    float v = cv[0];
    int ix = ci[0];
    int owner = tid;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const float ov = __shfl_xor(v, m);
      const int oi = __shfl_xor(ix, m), oo = __shfl_xor(owner, m);
      if (ov < v || (ov == v && oi < ix)) { v = ov; ix = oi; owner = oo; }
    }
    if ((tid & 63) == 0) { rv[tid >> 6] = v; ri[tid >> 6] = ix; rt[tid >> 6] = owner; }
    __syncthreads();
    float wv = rv[0];
    int wi = ri[0], wo = rt[0];
    for (int q = 1; q < 4; ++q)
      if (rv[q] < wv || (rv[q] == wv && ri[q] < wi)) { wv = rv[q]; wi = ri[q]; wo = rt[q]; }
    if (tid == 0 && (unsigned)wi < (unsigned)A) {
      atomicAdd(&cnt[(long)b * A + wi], 1);
      atomicMin(&agt[(long)b * A + wi], j);
    }
    if (tid == wo && (unsigned)wi < (unsigned)A) {      // pop the winner's head
#pragma unroll
      for (int q = 0; q < DSL_TOPK - 1; ++q) { cv[q] = cv[q + 1]; ci[q] = ci[q + 1]; }
      cv[DSL_TOPK - 1] = INFINITY;
      ci[DSL_TOPK - 1] = 0x7fffffff;
    }
    __syncthreads();
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

__global__ __launch_bounds__(256) void dsl_norm_kernel(long n, const float* part, float* norm) {
  __shared__ double sh[256];
  double s = 0.0;
  for (long i = threadIdx.x; i < n; i += 256) s += (double)part[i];
  const double tot = tal_block_sum(s, sh);
  if (threadIdx.x == 0) norm[0] = (float)fmax(tot, 1.0);
}

// QFL over anchors x classes against the soft labels: thread = (anchor, 8-class chunk)
template <typename T>
__global__ __launch_bounds__(256) void dsl_cls_kernel(LossLevels L, int A, int nc, float beta, const float* tsc,
                                                      const int* acls, const float* norm, float gnum, float* part) {
  const int b = blockIdx.y;
  const int G = (nc + 7) / 8;
  const int i = blockIdx.x * 256 + threadIdx.x;       // A * G < 2^31 (host-checked): 32-bit division
  float acc = 0.f;
  if (i < A * G) {
    const int a = i / G, q = i - a * G;
    const int c0 = q * 8, nv = min(8, nc - c0);
    int l;
    float ax, ay;
    const long row = anchor_row(L, b, a, l, ax, ay) + 4 * DL_DFL + c0;
    float x[8];
    load8(reinterpret_cast<const T*>(L.x[l]) + row, nv, x);
    const int ac = acls[(long)b * A + a];
    const float t = tsc[(long)b * A + a];
    const float gscale = gnum / norm[0];
    float gr[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      gr[k] = 0.f;
      if (k < nv) {
        float dx;
        acc += dsl_qfl(x[k], c0 + k == ac ? t : 0.f, beta, dx);
        gr[k] = dx * gscale;
      }
    }
    if (L.g[l]) store8(reinterpret_cast<T*>(L.g[l]) + row, nv, gr);
  }
  block_sum_store(acc, part, (long)b * gridDim.x + blockIdx.x);
}

// per anchor: weighted box and DFL sums and, GRAD, their gradient into the 64 DFL logits
template <typename T, bool GRAD>
__global__ __launch_bounds__(256) void dsl_box_kernel(LossLevels L, const float* tg, int M, int B, int A, int nc,
                                                      float img_w, float img_h, const int* agt, const float* tsc,
                                                      const float* norm, float nbox, float ndfl, float* part) {
  const int a = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  float lb = 0.f, ld = 0.f;
  if (a < A) {
    const long i = (long)b * A + a;
    const int j = agt[i];
    int l;
    float ax, ay;
    const long row = anchor_row(L, b, a, l, ax, ay);
    float v[4 * DL_DFL];
    int tb, cls;
    float g[4];
    bool fg = false;
    if (j >= 0 && j < M && tal_row(tg + (long)j * 6, B, nc, img_w, img_h, tb, cls, g)) {
      fg = true;
      load_dist(reinterpret_cast<const T*>(L.x[l]) + row, v);
      const float t = tsc[i];
      const float it = GRAD ? t / norm[0] : 0.f;
      float vb, vd;
      tal_box_dfl<GRAD, 1>(v, ax, ay, L.stride[l], g, nbox * it, ndfl * it, vb, vd);
      lb = vb * t;
      ld = vd * t;
    }
    if (GRAD && L.g[l]) {
      if (!fg) {
#pragma unroll
        for (int q = 0; q < 4 * DL_DFL; ++q) v[q] = 0.f;
      }
      store_dist(reinterpret_cast<T*>(L.g[l]) + row, v);
    }
  }
  const long slot = ((long)b * gridDim.x + blockIdx.x) * 2;
  block_sum_store(lb, part, slot + 0);
  block_sum_store(ld, part, slot + 1);
}

__global__ __launch_bounds__(256) void dsl_finalize_kernel(long ncls, const float* pcls, long nbox, const float* pbox,
                                                           const float* norm, float g_box, float g_cls, float g_dfl,
                                                           float* out) {
  __shared__ double sh[256];
  double sc = 0.0, sb = 0.0, sd = 0.0;
  for (long i = threadIdx.x; i < ncls; i += 256) sc += (double)pcls[i];
  for (long i = threadIdx.x; i < nbox; i += 256) { sb += (double)pbox[2 * i]; sd += (double)pbox[2 * i + 1]; }
  sc = tal_block_sum(sc, sh);
  sb = tal_block_sum(sb, sh);
  sd = tal_block_sum(sd, sh);
  if (threadIdx.x != 0) return;
  const double n = (double)norm[0];
  const double lcls = sc / n, lbox = sb / n, ldfl = sd / n;
  out[0] = (float)(g_box * lbox + g_cls * lcls + g_dfl * ldfl);
  out[1] = (float)lbox;
  out[2] = (float)lcls;
  out[3] = (float)ldfl;
  out[4] = (float)n;
}

__global__ __launch_bounds__(256) void dsl_rows_kernel(const float* tg, int M, int B, int nc, int* rows, int* nrows) {
  tal_list_rows(tg, M, B, nc, rows, nrows);
}

// workspace layout (bytes, 256-aligned pieces)
struct DslWs {
  size_t pbox, S, cand, cnt, agt, tsc, acls, rows, nrows, partt, norm, pcls, pboxp, total;
};
static DslWs dsl_ws(int B, int A, int nc, int M) {
  auto al = [](size_t x) { return (x + 255) / 256 * 256; };
  const size_t gxc = (size_t)cdiv((long)A * ((nc + 7) / 8), 256), gxb = (size_t)cdiv(A, 256);
  const size_t ba = (size_t)B * A;
  DslWs w{};
  size_t o = 0;
  w.pbox = o; o += al(ba * 16);
  w.S = o; o += al(ba * 4);
  w.cand = o; o += al(ba * 4);
  w.cnt = o; o += al(ba * 4);
  w.agt = o; o += al(ba * 4);
  w.tsc = o; o += al(ba * 4);
  w.acls = o; o += al(ba * 4);
  w.rows = o; o += al((size_t)B * (size_t)(M > 0 ? M : 1) * 4);
  w.nrows = o; o += al((size_t)B * 4);
  w.partt = o; o += al((size_t)B * gxb * 4);
  w.norm = o; o += 256;
  w.pcls = o; o += al((size_t)B * gxc * 4);
  w.pboxp = o; o += al((size_t)B * gxb * 8);
  w.total = o;
  return w;
}

}  // namespace yms

using namespace yms;

extern "C" {

size_t yms_dsl_loss_ws_bytes(int batch, int anchors, int nc, int n_targets) {
  if (batch <= 0 || anchors <= 0 || nc <= 0 || n_targets < 0) return 0;
  return dsl_ws(batch, anchors, nc, n_targets).total;
}

yms_status yms_dsl_loss(int dtype, int batch, int nc, int nlevels, const void* const* maps, void* const* grads,
                        const int* hs, const int* ws_, const float* strides, int ld, const float* targets,
                        int n_targets, float img_w, float img_h, int topk, float radius, float iou_weight,
                        float beta, const float* gains, void* ws, size_t ws_bytes, float* out, int* assign_gt,
                        float* assign_score, int* dynamic_k, void* stream) {
  if (batch <= 0 || nc <= 0 || nlevels <= 0 || nlevels > DL_MAXL || !maps || !hs || !ws_ || !strides || !out ||
      !gains || n_targets < 0 || (n_targets > 0 && !targets))
    return YMS_ERR_INVALID;
  if (dtype != YMS_F32 && dtype != YMS_BF16 && dtype != YMS_F16) return YMS_ERR_INVALID;
  if (topk < 1 || topk > DSL_TOPK || !(radius >= 0.f) || !(iou_weight >= 0.f) || !(beta >= 1.f) ||
      !std::isfinite(radius) || !std::isfinite(iou_weight) || !std::isfinite(beta) || !(img_w > 0.f) ||
      !(img_h > 0.f) || !std::isfinite(img_w) || !std::isfinite(img_h))
    return YMS_ERR_INVALID;
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
  LossLevels L{};
  L.nl = nlevels;
  L.ld = ld;
  int A = 0;
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
  const DslWs w = dsl_ws(batch, A, nc, n_targets);
  if (!ws || ws_bytes < w.total) return YMS_ERR_INVALID;
  char* base = (char*)ws;
  float* pbox = (float*)(base + w.pbox);
  float* S = (float*)(base + w.S);
  int* cand = (int*)(base + w.cand);
  int* cnt = (int*)(base + w.cnt);
  int* agt = (int*)(base + w.agt);
  float* tsc = (float*)(base + w.tsc);
  int* acls = (int*)(base + w.acls);
  int* rows = (int*)(base + w.rows);
  int* nrows = (int*)(base + w.nrows);
  float* partt = (float*)(base + w.partt);
  float* norm = (float*)(base + w.norm);
  float* pcls = (float*)(base + w.pcls);
  float* pboxp = (float*)(base + w.pboxp);
  const int gxc = cdiv((long)A * ((nc + 7) / 8), 256), gxb = cdiv(A, 256);
  hipStream_t st = (hipStream_t)stream;
  const int M = n_targets, B = batch;
  const DslParams P{radius, iou_weight, beta, topk};
  // total = g_box box + g_cls cls + g_dfl dfl, every term a sum over norm (no factor B)
  const float gcls = gains[1], gbox = gains[0], gdfl = gains[2] * 0.25f;
#define YMS_DSL_CASE(T)                                                                                          \
  if (M > 0) hipLaunchKernelGGL(dsl_rows_kernel, dim3(B), dim3(256), 0, st, targets, M, B, nc, rows, nrows);     \
  hipLaunchKernelGGL(dsl_decode_kernel<T>, dim3(gxb, B), dim3(256), 0, st, L, targets, M, B, A, nc, img_w,       \
                     img_h, beta, rows, nrows, pbox, S, cand, cnt, agt);                                         \
  if (M > 0)                                                                                                     \
    hipLaunchKernelGGL(dsl_select_kernel<T>, dim3(M), dim3(256), 0, st, L, targets, B, A, nc, img_w, img_h, P,   \
                       pbox, S, cand, cnt, agt, dynamic_k);                                                      \
  hipLaunchKernelGGL(dsl_resolve_kernel<T>, dim3(gxb, B), dim3(256), 0, st, L, targets, M, B, A, nc, img_w,      \
                     img_h, P, pbox, S, cnt, rows, nrows, agt, tsc, acls, partt, assign_gt, assign_score);       \
  hipLaunchKernelGGL(dsl_norm_kernel, dim3(1), dim3(256), 0, st, (long)B * gxb, partt, norm);                    \
  hipLaunchKernelGGL(dsl_cls_kernel<T>, dim3(gxc, B), dim3(256), 0, st, L, A, nc, beta, tsc, acls, norm, gcls,   \
                     pcls);                                                                                      \
  if (grads) {                                                                                                   \
    hipLaunchKernelGGL((dsl_box_kernel<T, true>), dim3(gxb, B), dim3(256), 0, st, L, targets, M, B, A, nc,       \
                       img_w, img_h, agt, tsc, norm, gbox, gdfl, pboxp);                                         \
  } else {                                                                                                       \
    hipLaunchKernelGGL((dsl_box_kernel<T, false>), dim3(gxb, B), dim3(256), 0, st, L, targets, M, B, A, nc,      \
                       img_w, img_h, agt, tsc, norm, gbox, gdfl, pboxp);                                         \
  }                                                                                                              \
  hipLaunchKernelGGL(dsl_finalize_kernel, dim3(1), dim3(256), 0, st, (long)B * gxc, pcls, (long)B * gxb, pboxp,  \
                     norm, gains[0], gains[1], gains[2], out);
  switch (dtype) {
    case YMS_F32: { YMS_DSL_CASE(float) break; }
    case YMS_BF16: { YMS_DSL_CASE(bf16) break; }
    default: { YMS_DSL_CASE(f16) break; }
  }
#undef YMS_DSL_CASE
  return launch_status();
}

}  // extern "C"
