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
//   tal_rows_kernel    per image: its valid target rows, in target order, listed in global memory
//   tal_resolve_kernel per anchor: one claim -> that GT; several -> the GT with the largest overlap
//                      among ALL the image's GTs the anchor lies inside (lowest row on a tie), also
//                      one that did not claim it; the metric and overlap of the final pair, and
//                      per-GT maxima by atomicMax on the bit pattern of the non-negative floats
//   tal_score_kernel   per anchor: target score t = m * max_ov / (max_m + 1e-9), its class; block
//                      partial sums of t
//   tal_tss_kernel     one block: tss = max(sum t, 1) in fp64, fixed order
//   tal_cls_kernel     BCE-with-logits of every anchor x class against t at the assigned class,
//                      gradient scaled by B * lambda_cls / tss (read from device memory)
//   tal_box_kernel     per foreground anchor: (1 - CIoU) t and the two-bin DFL cross entropy t,
//                      and their gradient into the 64 DFL logits (zeros for background anchors)
//   tal_finalize_kernel  fp64 fixed-order sums / tss -> box, cls, dfl, B (7.5 box + 0.5 cls + 1.5 dfl)
//
// Deterministic: integer atomics and float maxima only, fixed-order partials, fp64 finals.  No host
// sync.  Target rows are never staged in LDS, so there is no row limit: a GT scans only the grid
// cells around its box, a contested anchor only its image's row list.  The class logits are read
// once (plus one gathered logit per inside pair), the DFL logits twice, the gradient written once.
#include <algorithm>
#include <climits>
#include <cmath>

#include "det_loss_common.hpp"

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
#pragma unroll
  for (int q = 0; q < DL_TOPK; ++q) { bv[q] = -1.f; bi[q] = 0x7fffffff; }
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
    if (m > bv[DL_TOPK - 1]) {     // strictly greater: an equal later index ranks after
      float cv = m;
      int ci = a;
#pragma unroll
      for (int q = 0; q < DL_TOPK; ++q) {
        if (cv > bv[q]) {
          const float tv = bv[q];
          const int ti = bi[q];
          bv[q] = cv; bi[q] = ci;
          cv = tv; ci = ti;
        }
      }
    }
  }
  __shared__ int scnt[4];
  __shared__ float rv[4];
  __shared__ int ri[4], rt[4];
  int c = ninside;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) c += __shfl_xor(c, m);
  if ((tid & 63) == 0) scnt[tid >> 6] = c;
  __syncthreads();
  const int total = (scnt[0] + scnt[1]) + (scnt[2] + scnt[3]);
  const int k = total < topk ? total : topk;
  // k rounds of block argmax over each thread's current head (value desc, index asc)
  for (int r = 0; r < k; ++r) {
    float v = bv[0];
    int ix = bi[0];
    int owner = tid;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const float ov = __shfl_xor(v, m);
      const int oi = __shfl_xor(ix, m), oo = __shfl_xor(owner, m);
      if (ov > v || (ov == v && oi < ix)) { v = ov; ix = oi; owner = oo; }
    }
    if ((tid & 63) == 0) { rv[tid >> 6] = v; ri[tid >> 6] = ix; rt[tid >> 6] = owner; }
    __syncthreads();
    float wv = rv[0];
    int wi = ri[0], wo = rt[0];
    for (int q = 1; q < 4; ++q)
      if (rv[q] > wv || (rv[q] == wv && ri[q] < wi)) { wv = rv[q]; wi = ri[q]; wo = rt[q]; }
    if (tid == 0 && (unsigned)wi < (unsigned)A) {
      atomicAdd(&cnt[(long)b * A + wi], 1);
      atomicMin(&agt[(long)b * A + wi], j);
    }
    if (tid == wo) {                  // pop the winner's head
#pragma unroll
      for (int q = 0; q < DL_TOPK - 1; ++q) { bv[q] = bv[q + 1]; bi[q] = bi[q + 1]; }
      bv[DL_TOPK - 1] = -1.f;
      bi[DL_TOPK - 1] = 0x7fffffff;
    }
    __syncthreads();
  }
}

// per image: its valid target rows in target order -> rows[b * M ..], nrows[b] (global memory, so
// no limit on the rows of one image)
__global__ __launch_bounds__(256) void tal_rows_kernel(const float* tg, int M, int B, int nc, int* rows, int* nrows) {
  tal_list_rows(tg, M, B, nc, rows, nrows);
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

__global__ __launch_bounds__(256) void tal_tss_kernel(long n, const float* part, float* tss) {
  __shared__ double sh[256];
  double s = 0.0;
  for (long i = threadIdx.x; i < n; i += 256) s += (double)part[i];
  const double tot = tal_block_sum(s, sh);
  if (threadIdx.x == 0) tss[0] = (float)fmax(tot, 1.0);
}

// BCE over anchors x classes against the soft targets: thread = (anchor, 8-class chunk)
template <typename T>
__global__ __launch_bounds__(256) void tal_cls_kernel(LossLevels L, int A, int nc, const float* tsc, const int* acls,
                                                      const float* tss, float gnum, float* part) {
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
    const float gscale = gnum / tss[0];
    float gr[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      gr[k] = 0.f;
      if (k < nv) {
        float dx;
        acc += bce_logits(x[k], c0 + k == ac ? t : 0.f, 1.f, dx);
        gr[k] = dx * gscale;
      }
    }
    if (L.g[l]) store8(reinterpret_cast<T*>(L.g[l]) + row, nv, gr);
  }
  block_sum_store(acc, part, (long)b * gridDim.x + blockIdx.x);
}

// per anchor: weighted box and DFL sums and, GRAD, their gradient into the 64 DFL logits
template <typename T, bool GRAD>
__global__ __launch_bounds__(256) void tal_box_kernel(LossLevels L, const float* tg, int M, int B, int A, int nc,
                                                      float img_w, float img_h, const int* agt, const float* tsc,
                                                      const float* tss, float nbox, float ndfl, float* part) {
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
      const float it = GRAD ? t / tss[0] : 0.f;
      float vb, vd;
      tal_box_dfl<GRAD, 3>(v, ax, ay, L.stride[l], g, nbox * it, ndfl * it, vb, vd);
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

__global__ __launch_bounds__(256) void tal_finalize_kernel(int B, long ncls, const float* pcls, long nbox,
                                                           const float* pbox, const float* tss, float lam_box,
                                                           float lam_cls, float lam_dfl, float* out) {
  __shared__ double sh[256];
  double sc = 0.0, sb = 0.0, sd = 0.0;
  for (long i = threadIdx.x; i < ncls; i += 256) sc += (double)pcls[i];
  for (long i = threadIdx.x; i < nbox; i += 256) { sb += (double)pbox[2 * i]; sd += (double)pbox[2 * i + 1]; }
  sc = tal_block_sum(sc, sh);
  sb = tal_block_sum(sb, sh);
  sd = tal_block_sum(sd, sh);
  if (threadIdx.x != 0) return;
  const double n = (double)tss[0];
  const double lcls = sc / n, lbox = sb / n, ldfl = sd / n;
  out[0] = (float)((double)B * (lam_box * lbox + lam_cls * lcls + lam_dfl * ldfl));
  out[1] = (float)lbox;
  out[2] = (float)lcls;
  out[3] = (float)ldfl;
}

// workspace layout (bytes, 256-aligned pieces)
struct TalWs {
  size_t pbox, cnt, agt, am, tsc, acls, mohat, rows, nrows, partt, tss, pcls, pboxp, total;
};
static TalWs tal_ws(int B, int A, int nc, int M) {
  auto al = [](size_t x) { return (x + 255) / 256 * 256; };
  const size_t gxc = (size_t)cdiv((long)A * ((nc + 7) / 8), 256), gxb = (size_t)cdiv(A, 256);
  const size_t ba = (size_t)B * A;
  TalWs w{};
  size_t o = 0;
  w.pbox = o; o += al(ba * 16);
  w.cnt = o; o += al(ba * 4);
  w.agt = o; o += al(ba * 4);
  w.am = o; o += al(ba * 4);
  w.tsc = o; o += al(ba * 4);
  w.acls = o; o += al(ba * 4);
  w.mohat = o; o += al((size_t)(M > 0 ? M : 1) * 8);
  w.rows = o; o += al((size_t)B * (size_t)(M > 0 ? M : 1) * 4);
  w.nrows = o; o += al((size_t)B * 4);
  w.partt = o; o += al((size_t)B * gxb * 4);
  w.tss = o; o += 256;
  w.pcls = o; o += al((size_t)B * gxc * 4);
  w.pboxp = o; o += al((size_t)B * gxb * 8);
  w.total = o;
  return w;
}

}  // namespace yms

using namespace yms;

extern "C" {

size_t yms_tal_loss_ws_bytes(int batch, int anchors, int nc, int n_targets) {
  if (batch <= 0 || anchors <= 0 || nc <= 0 || n_targets < 0) return 0;
  return tal_ws(batch, anchors, nc, n_targets).total;
}

yms_status yms_tal_loss(int dtype, int batch, int nc, int nlevels, const void* const* maps, void* const* grads,
                        const int* hs, const int* ws_, const float* strides, int ld, const float* targets,
                        int n_targets, float img_w, float img_h, int topk, float alpha, float beta,
                        const float* lambdas, void* ws, size_t ws_bytes, float* out, int* assign_gt,
                        float* assign_score, void* stream) {
  if (batch <= 0 || nc <= 0 || nlevels <= 0 || nlevels > DL_MAXL || !maps || !hs || !ws_ || !strides || !out ||
      !lambdas || n_targets < 0 || (n_targets > 0 && !targets))
    return YMS_ERR_INVALID;
  if (dtype != YMS_F32 && dtype != YMS_BF16 && dtype != YMS_F16) return YMS_ERR_INVALID;
  if (topk < 1 || topk > DL_TOPK || !(alpha >= 0.f) || !(beta >= 0.f) || !std::isfinite(alpha) ||
      !std::isfinite(beta) || !(img_w > 0.f) || !(img_h > 0.f) || !std::isfinite(img_w) || !std::isfinite(img_h))
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
  const TalWs w = tal_ws(batch, A, nc, n_targets);
  if (!ws || ws_bytes < w.total) return YMS_ERR_INVALID;
  char* base = (char*)ws;
  float* pbox = (float*)(base + w.pbox);
  int* cnt = (int*)(base + w.cnt);
  int* agt = (int*)(base + w.agt);
  float* am = (float*)(base + w.am);
  float* tsc = (float*)(base + w.tsc);
  int* acls = (int*)(base + w.acls);
  unsigned* mohat = (unsigned*)(base + w.mohat);
  int* rows = (int*)(base + w.rows);
  int* nrows = (int*)(base + w.nrows);
  float* partt = (float*)(base + w.partt);
  float* tss = (float*)(base + w.tss);
  float* pcls = (float*)(base + w.pcls);
  float* pboxp = (float*)(base + w.pboxp);
  const int gxc = cdiv((long)A * ((nc + 7) / 8), 256), gxb = cdiv(A, 256);
  hipStream_t st = (hipStream_t)stream;
  const int M = n_targets, B = batch;
  // total = B (lam_box box + lam_cls cls + lam_dfl dfl), every term a sum over tss
  const float gcls = (float)B * lambdas[1], gbox = (float)B * lambdas[0], gdfl = (float)B * lambdas[2] * 0.25f;
#define YMS_TAL_CASE(T)                                                                                          \
  hipLaunchKernelGGL(tal_decode_kernel<T>, dim3(gxb, B), dim3(256), 0, st, L, A, pbox, cnt, agt);                \
  if (M > 0) {                                                                                                   \
    hipLaunchKernelGGL(tal_topk_kernel<T>, dim3(M), dim3(256), 0, st, L, targets, B, A, nc, img_w, img_h, topk,  \
                       alpha, beta, pbox, cnt, agt, mohat);                                                      \
    hipLaunchKernelGGL(tal_rows_kernel, dim3(B), dim3(256), 0, st, targets, M, B, nc, rows, nrows);              \
  }                                                                                                              \
  hipLaunchKernelGGL(tal_resolve_kernel<T>, dim3(gxb, B), dim3(256), 0, st, L, targets, M, B, A, nc, img_w,      \
                     img_h, alpha, beta, pbox, cnt, rows, nrows, agt, am, mohat);                                \
  hipLaunchKernelGGL(tal_score_kernel, dim3(gxb, B), dim3(256), 0, st, targets, A, agt, am, mohat, tsc, acls,    \
                     partt, assign_gt, assign_score);                                                            \
  hipLaunchKernelGGL(tal_tss_kernel, dim3(1), dim3(256), 0, st, (long)B * gxb, partt, tss);                      \
  hipLaunchKernelGGL(tal_cls_kernel<T>, dim3(gxc, B), dim3(256), 0, st, L, A, nc, tsc, acls, tss, gcls, pcls);   \
  if (grads) {                                                                                                   \
    hipLaunchKernelGGL((tal_box_kernel<T, true>), dim3(gxb, B), dim3(256), 0, st, L, targets, M, B, A, nc,       \
                       img_w, img_h, agt, tsc, tss, gbox, gdfl, pboxp);                                          \
  } else {                                                                                                       \
    hipLaunchKernelGGL((tal_box_kernel<T, false>), dim3(gxb, B), dim3(256), 0, st, L, targets, M, B, A, nc,      \
                       img_w, img_h, agt, tsc, tss, gbox, gdfl, pboxp);                                          \
  }                                                                                                              \
  hipLaunchKernelGGL(tal_finalize_kernel, dim3(1), dim3(256), 0, st, B, (long)B * gxc, pcls, (long)B * gxb,      \
                     pboxp, tss, lambdas[0], lambdas[1], lambdas[2], out);
  switch (dtype) {
    case YMS_F32: { YMS_TAL_CASE(float) break; }
    case YMS_BF16: { YMS_TAL_CASE(bf16) break; }
    default: { YMS_TAL_CASE(f16) break; }
  }
#undef YMS_TAL_CASE
  return launch_status();
}

}  // extern "C"
