// Shared by the two anchor-based assigner losses (tal_loss.hip, dsl_loss.hip), which differ in how
// an anchor gets its GT and soft target and are alike after that.  Device helpers: target rows, the
// inside test, the row lister, the fp64 block sum, the box + DFL value and gradient of one anchor.
// Kernels, one definition each:
//
//   assign_rows_kernel      per image: its valid target rows, in target order, listed in global memory
//   assign_norm_kernel      one block: norm = max(sum t, 1) in fp64, fixed order
//   assign_cls_kernel       a per-logit term (functor: BCE / QFL) of every anchor x class against t at
//                           the assigned class, gradient scaled by gnum / norm (read from device memory)
//   assign_box_kernel       per foreground anchor: (1 - IoU-family value) t and the two-bin DFL cross
//                           entropy t, and their gradient into the 64 DFL logits (zeros for background)
//   assign_finalize_kernel  fp64 fixed-order sums / norm -> mult * total, box, cls, dfl[, norm]
//
// Where the losses differ the difference is a template argument (the IoU type, the term functor), so
// each instantiation is the kernel that loss had of its own.  Host: the common part of the workspace
// and the launch tail norm -> cls -> box -> finalize.  The non-template kernels are static: this
// header is part of two translation units of one library.
#pragma once
#include "det_loss_common.hpp"

namespace yms {

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

// ---------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(256) void assign_rows_kernel(const float* tg, int M, int B, int nc, int* rows,
                                                                 int* nrows) {
  tal_list_rows(tg, M, B, nc, rows, nrows);
}

static __global__ __launch_bounds__(256) void assign_norm_kernel(long n, const float* part, float* norm) {
  __shared__ double sh[256];
  double s = 0.0;
  for (long i = threadIdx.x; i < n; i += 256) s += (double)part[i];
  const double tot = tal_block_sum(s, sh);
  if (threadIdx.x == 0) norm[0] = (float)fmax(tot, 1.0);
}

// term(x, t, dx) over anchors x classes against the soft targets: thread = (anchor, 8-class chunk)
template <typename T, typename Term>
__global__ __launch_bounds__(256) void assign_cls_kernel(LossLevels L, int A, int nc, Term term, const float* tsc,
                                                         const int* acls, const float* norm, float gnum,
                                                         float* part) {
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
        acc += term(x[k], c0 + k == ac ? t : 0.f, dx);
        gr[k] = dx * gscale;
      }
    }
    if (L.g[l]) store8(reinterpret_cast<T*>(L.g[l]) + row, nv, gr);
  }
  block_sum_store(acc, part, (long)b * gridDim.x + blockIdx.x);
}

// per anchor: weighted box and DFL sums and, GRAD, their gradient into the 64 DFL logits
template <typename T, bool GRAD, int IOU>
__global__ __launch_bounds__(256) void assign_box_kernel(LossLevels L, const float* tg, int M, int B, int A, int nc,
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
      tal_box_dfl<GRAD, IOU>(v, ax, ay, L.stride[l], g, nbox * it, ndfl * it, vb, vd);
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

// out[0..3] = mult * (g_box box + g_cls cls + g_dfl dfl), box, cls, dfl, every term a sum over
// norm; norm itself to out_norm unless null.  mult = 1 is exact in fp64.
static __global__ __launch_bounds__(256) void assign_finalize_kernel(double mult, long ncls, const float* pcls,
                                                                     long nbox, const float* pbox, const float* norm,
                                                                     float g_box, float g_cls, float g_dfl,
                                                                     float* out, float* out_norm) {
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
  out[0] = (float)(mult * (g_box * lbox + g_cls * lcls + g_dfl * ldfl));
  out[1] = (float)lbox;
  out[2] = (float)lcls;
  out[3] = (float)ldfl;
  if (out_norm) out_norm[0] = (float)n;
}

// ---- host side -------------------------------------------------------------------------------
// The assigner losses' workspace: the pieces both use, laid out once; a loss appends its own with
// add().  Offsets in bytes, 256-aligned pieces.
struct AssignWs {
  size_t pbox, cnt, agt, tsc, acls, rows, nrows, partt, norm, pcls, pboxp, total;
  int gxc, gxb;        // blocks per image of the cls kernel / of the per-anchor kernels
  size_t add(size_t bytes) {
    const size_t o = total;
    total += ws_align(bytes);
    return o;
  }
};
inline AssignWs assign_ws(int B, int A, int nc, int M) {
  AssignWs w{};
  w.gxc = cdiv((long)A * ((nc + 7) / 8), 256);
  w.gxb = cdiv(A, 256);
  const size_t ba = (size_t)B * A, m1 = (size_t)(M > 0 ? M : 1);
  w.pbox = w.add(ba * 16);
  w.cnt = w.add(ba * 4);
  w.agt = w.add(ba * 4);
  w.tsc = w.add(ba * 4);
  w.acls = w.add(ba * 4);
  w.rows = w.add((size_t)B * m1 * 4);
  w.nrows = w.add((size_t)B * 4);
  w.partt = w.add((size_t)B * w.gxb * 4);
  w.norm = w.add(256);
  w.pcls = w.add((size_t)B * w.gxc * 4);
  w.pboxp = w.add((size_t)B * w.gxb * 8);
  return w;
}
template <typename P>
inline P* ws_at(void* ws, size_t off) { return reinterpret_cast<P*>(static_cast<char*>(ws) + off); }

// The launches both losses end with: norm -> cls -> box (with the gradient when the levels carry
// gradient maps) -> finalize.  gains = box, cls, dfl; mult multiplies the total and the gradient.
template <typename T, int IOU, typename Term>
inline void assign_loss_tail(const LossLevels& L, const AssignWs& w, void* ws, const float* targets, int M, int B,
                             int A, int nc, float img_w, float img_h, Term term, float mult, const float* gains,
                             float* out, float* out_norm, hipStream_t st) {
  const int* agt = ws_at<int>(ws, w.agt);
  const int* acls = ws_at<int>(ws, w.acls);
  const float* tsc = ws_at<float>(ws, w.tsc);
  float* norm = ws_at<float>(ws, w.norm);
  float* pcls = ws_at<float>(ws, w.pcls);
  float* pboxp = ws_at<float>(ws, w.pboxp);
  const float gcls = mult * gains[1], gbox = mult * gains[0], gdfl = mult * gains[2] * 0.25f;
  hipLaunchKernelGGL(assign_norm_kernel, dim3(1), dim3(256), 0, st, (long)B * w.gxb, ws_at<float>(ws, w.partt), norm);
  hipLaunchKernelGGL((assign_cls_kernel<T, Term>), dim3(w.gxc, B), dim3(256), 0, st, L, A, nc, term, tsc, acls, norm,
                     gcls, pcls);
  if (L.g[0]) {
    hipLaunchKernelGGL((assign_box_kernel<T, true, IOU>), dim3(w.gxb, B), dim3(256), 0, st, L, targets, M, B, A, nc,
                       img_w, img_h, agt, tsc, norm, gbox, gdfl, pboxp);
  } else {
    hipLaunchKernelGGL((assign_box_kernel<T, false, IOU>), dim3(w.gxb, B), dim3(256), 0, st, L, targets, M, B, A, nc,
                       img_w, img_h, agt, tsc, norm, gbox, gdfl, pboxp);
  }
  hipLaunchKernelGGL(assign_finalize_kernel, dim3(1), dim3(256), 0, st, (double)mult, (long)B * w.gxc, pcls,
                     (long)B * w.gxb, pboxp, norm, gains[0], gains[1], gains[2], out, out_norm);
}

}  // namespace yms
