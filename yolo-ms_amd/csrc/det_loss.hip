// Detection loss and target assignment on gfx950: the semantics of the
// reference's ComputeLoss (yolov8/tools/loss.py:94-677, restated in oracle/loss_ref.py), fused
// with its analytic gradient so one forward launch sequence yields the three loss terms and
// d(total)/d(head maps) in the head maps' own NHWC layout:
//
//   decode_kernel   per anchor: softmax over each side's 16 DFL bins, expected offsets (grid
//                   units, loss.py:127-206), decoded (cx, cy, w, h) in pixels
//   topk_kernel     per target row: plain IoU of every decoded box with the GT (loss.py:252),
//                   k = min(10, #IoU > 0.1) best anchors (ties -> lower index)  (loss.py:312-315),
//                   drawn with the block selection primitives of det_loss_common.hpp
//   assign_kernel   per image, GTs in target order: fg mask, target box / l-t-r-b OVERWRITTEN by
//                   later GTs, class bits accumulated (loss.py:297-365)
//   cls_kernel      BCE-with-logits over every anchor x class: per-image sums + gradient
//                   (the mean is added twice when the image has foreground, loss.py:530/551)
//   box_kernel      per foreground anchor: 1 - CIoU (or IoU / GIoU / DIoU) and the two-bin DFL
//                   cross entropy, per-image sums and NaN flags (loss.py:553-648)
//   boxgrad_kernel  their gradient into the 64 DFL logits (zeros for background anchors,
//                   no box gradient for an image whose box loss was NaN)
//   finalize_kernel per-image means -> batch means -> 7.5 box + 0.5 cls + 1.5 dfl
//
// Reductions are deterministic (fixed-order block partials, fp64 finals).  HBM-bound: the head
// maps are read twice (cls + box) and the gradient written once.  The argument checks and the
// dtype dispatch are the ones of det_loss_common.hpp, shared with tal_loss.hip and dsl_loss.hip.
#include <algorithm>
#include <cmath>

#include "det_loss_common.hpp"

namespace yms {

constexpr float DL_IOU_MIN = 0.1f;
constexpr int DL_ASSIGN_LDS = 4096;     // target rows staged per image in assign_kernel

__device__ __forceinline__ float plain_iou(const float (&p)[4], const float (&g)[4]) {
  const float iw = fmaxf(fminf(p[2], g[2]) - fmaxf(p[0], g[0]), 0.f);
  const float ih = fmaxf(fminf(p[3], g[3]) - fmaxf(p[1], g[1]), 0.f);
  const float inter = iw * ih;
  const float un = (p[2] - p[0]) * (p[3] - p[1]) + (g[2] - g[0]) * (g[3] - g[1]) - inter + DL_EPS;
  return inter / un;
}

// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void decode_kernel(LossLevels L, int A, float* pbox) {
  const int a = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (a >= A) return;
  int l;
  float ax, ay;
  const long row = anchor_row(L, b, a, l, ax, ay);
  float v[4 * DL_DFL], e[4], lse[4];
  load_dist(reinterpret_cast<const T*>(L.x[l]) + row, v);
  dfl_softmax(v, e, lse);
  const float x1 = ax - e[0], y1 = ay - e[1], x2 = ax + e[2], y2 = ay + e[3];
  float4 o = make_float4((x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1);
  reinterpret_cast<float4*>(pbox)[(long)b * A + a] = o;
}

// per target row j: top-k anchors by IoU (value desc, index asc)
__global__ __launch_bounds__(256) void topk_kernel(const float* tg, int B, int A, float img_w, float img_h,
                                                   const float* pbox, int* kcnt, int* kidx) {
  const int j = blockIdx.x, tid = threadIdx.x;
  const float* t = tg + (long)j * 6;
  const int b = (int)t[0];
  if (!(t[0] >= 0.f) || b >= B) {   // not an image of this batch: never assigned
    if (tid == 0) kcnt[j] = 0;
    return;
  }
  const float gc[4] = {t[2] * img_w, t[3] * img_h, t[4] * img_w, t[5] * img_h};
  float g[4];
  cxcywh_to_xyxy(gc, g);
  // thread-local top-k, sorted descending (value desc, index asc)
  float bv[DL_TOPK];
  int bi[DL_TOPK];
  sel_clear<true>(bv, bi);
  int cnt = 0;
  const float4* pb = reinterpret_cast<const float4*>(pbox) + (long)b * A;
  for (int a = tid; a < A; a += 256) {
    const float4 c4 = pb[a];
    const float c[4] = {c4.x, c4.y, c4.z, c4.w};
    float p[4];
    cxcywh_to_xyxy(c, p);
    const float iou = plain_iou(p, g);
    cnt += iou > DL_IOU_MIN ? 1 : 0;
    if (sel_enters<true>(bv, iou)) sel_insert<true>(bv, bi, iou, a);
  }
  const int total = block_count_sum(cnt);
  const int k = total < DL_TOPK ? total : DL_TOPK;
  // k rounds of block argmax over each thread's current head (value desc, index asc)
  for (int r = 0; r < k; ++r) {
    float wv;
    int wi, wo;
    sel_round<true>(bv[0], bi[0], wv, wi, wo);
    if (tid == 0) kidx[(long)j * DL_TOPK + r] = wi;
    sel_pop<true>(bv, bi, tid == wo);
  }
  if (tid == 0) kcnt[j] = k;
}

// per image: apply the GTs in target order
__global__ __launch_bounds__(256) void assign_kernel(const float* tg, int M, int A, int nc, int nw, float img_w,
                                                     float img_h, LossLevels L, const int* kcnt, const int* kidx,
                                                     unsigned char* fg, float* tbox, float* tltrb,
                                                     unsigned* cbits, int* nfg) {
  const int b = blockIdx.x, tid = threadIdx.x;
  unsigned char* f = fg + (long)b * A;
  unsigned* bits = cbits + (long)b * A * nw;
  for (int a = tid; a < A; a += 256) f[a] = 0;
  for (long i = tid; i < (long)A * nw; i += 256) bits[i] = 0u;
  // this image's target rows, in target order (one scan of the image column)
  __shared__ int mine[DL_ASSIGN_LDS];
  __shared__ int nmine;
  if (tid == 0) nmine = 0;
  __syncthreads();
  const bool staged = M <= DL_ASSIGN_LDS;
  if (staged) {
    for (int j0 = 0; j0 < M; j0 += 256) {
      const int j = j0 + tid;
      const bool hit = j < M && tg[(long)j * 6] >= 0.f && (int)tg[(long)j * 6] == b;
      const unsigned long long bal = __ballot(hit);
      __shared__ int wcnt[4];
      if ((tid & 63) == 0) wcnt[tid >> 6] = __popcll(bal);
      __syncthreads();
      int base = nmine;
      for (int q = 0; q < (tid >> 6); ++q) base += wcnt[q];
      if (hit) mine[base + __popcll(bal & ((1ull << (tid & 63)) - 1ull))] = j;
      __syncthreads();
      if (tid == 0) nmine += (wcnt[0] + wcnt[1]) + (wcnt[2] + wcnt[3]);
      __syncthreads();
    }
  }
  const int nj = staged ? nmine : M;
  for (int jj = 0; jj < nj; ++jj) {
    const int j = staged ? mine[jj] : jj;
    const float* t = tg + (long)j * 6;
    if (!staged && (!(t[0] >= 0.f) || (int)t[0] != b)) continue;    // block-uniform
    const int k = kcnt[j];
    const int lab = (int)t[1];
    if (tid < k) {
      const int a = kidx[(long)j * DL_TOPK + tid];
      const float gc[4] = {t[2] * img_w, t[3] * img_h, t[4] * img_w, t[5] * img_h};
      f[a] = 1;
      float4* tb = reinterpret_cast<float4*>(tbox) + (long)b * A + a;
      *tb = make_float4(gc[0], gc[1], gc[2], gc[3]);
      // l-t-r-b distances of the anchor centre to the GT sides (loss.py:327-353)
      const float x1 = gc[0] - gc[2] / 2, y1 = gc[1] - gc[3] / 2;
      const float x2 = gc[0] + gc[2] / 2, y2 = gc[1] + gc[3] / 2;
      int l;
      float ax, ay;
      (void)anchor_row(L, 0, a, l, ax, ay);
      reinterpret_cast<float4*>(tltrb)[(long)b * A + a] = make_float4(ax - x1, ay - y1, x2 - ax, y2 - ay);
      if (lab >= 0 && lab < nc) bits[(long)a * nw + (lab >> 5)] |= 1u << (lab & 31);
    }
    __syncthreads();
  }
  int c = 0;
  for (int a = tid; a < A; a += 256) c += f[a];
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) c += __shfl_xor(c, m);
  __shared__ int sc[4];
  if ((tid & 63) == 0) sc[tid >> 6] = c;
  __syncthreads();
  if (tid == 0) nfg[b] = (sc[0] + sc[1]) + (sc[2] + sc[3]);
}

// BCE over anchors x classes: thread = (anchor, 8-class chunk)
template <typename T>
__global__ __launch_bounds__(256) void cls_kernel(LossLevels L, int A, int nc, int nw, const unsigned* cbits,
                                                  const int* nfg, const float* pos_weight, float gscale,
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
    const unsigned* bits = cbits + ((long)b * A + a) * nw;
    const float f = nfg[b] > 0 ? 2.f : 1.f;      // loss.py:530 + :551
    float gr[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      gr[k] = 0.f;
      if (k < nv) {
        const int c = c0 + k;
        const float t = (bits[c >> 5] >> (c & 31)) & 1u ? 1.f : 0.f;
        const float pw = pos_weight ? pos_weight[c] : 1.f;
        float dx;
        acc += bce_logits(x[k], t, pw, dx);
        gr[k] = dx * f * gscale;
      }
    }
    if (L.g[l]) store8(reinterpret_cast<T*>(L.g[l]) + row, nv, gr);
  }
  block_sum_store(acc, part, (long)b * gridDim.x + blockIdx.x);
}

// box + DFL value of one foreground anchor (and, GRAD, d/d logits scaled by sb, sd)
template <bool GRAD>
__device__ __forceinline__ void box_dfl(float (&v)[4 * DL_DFL], float ax, float ay, float stride,
                                        const float4 tb4, const float4 tl4, int iou_type, float sb, float sd,
                                        float& lbox, float& ldfl) {
  // DFL targets in stride units and their two bins (loss.py:602-630), read before the softmax
  const float tl[4] = {tl4.x / stride, tl4.y / stride, tl4.z / stride, tl4.w / stride};
  int li[4], ri[4];
  float wl[4], wr[4], xl[4], xr[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const float fl = floorf(tl[s]);
    const float fr = floorf(tl[s] + 1.0f);
    wr[s] = tl[s] - fl;
    wl[s] = 1.0f - wr[s];
    li[s] = (int)fminf(fmaxf(fl, 0.f), (float)(DL_DFL - 1));
    ri[s] = (int)fminf(fmaxf(fr, 0.f), (float)(DL_DFL - 1));
    xl[s] = v[s * DL_DFL + li[s]];
    xr[s] = v[s * DL_DFL + ri[s]];
  }
  float e[4], lse[4];
  dfl_softmax(v, e, lse);     // v: probabilities
  // decoded box, converted (cx, cy, w, h) -> xyxy exactly as the reference's chain does
  const float x1 = ax - e[0], y1 = ay - e[1], x2 = ax + e[2], y2 = ay + e[3];
  const float pc[4] = {(x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1};
  const float tc[4] = {tb4.x, tb4.y, tb4.z, tb4.w};
  float p[4], g[4];
  cxcywh_to_xyxy(pc, p);
  cxcywh_to_xyxy(tc, g);
  float dp[4];
  const float val = box_iou_grad<GRAD>(p, g, iou_type, dp);
  lbox = 1.f - val;
  // DFL: two-bin cross entropy, -log_softmax at the two bins (loss.py:644-645)
  float dfl = 0.f;
#pragma unroll
  for (int s = 0; s < 4; ++s) dfl += (lse[s] - xl[s]) * wl[s] + (lse[s] - xr[s]) * wr[s];
  ldfl = dfl;
  if (GRAD) {
    // box: loss 1 - val -> d/dp = -dp; p0 = ax - e0 (d/de0 = -1), p1 = ay - e1, p2 = ax + e2, p3 = ay + e3
    const float ge[4] = {dp[0] * sb, dp[1] * sb, -dp[2] * sb, -dp[3] * sb};
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int i = 0; i < DL_DFL; ++i) {
        const float pr = v[s * DL_DFL + i];
        float gi = ge[s] * pr * ((float)i - e[s]);      // d e_s / d logit_i = p_i (i - e_s)
        gi += sd * (pr - (i == li[s] ? wl[s] : 0.f) - (i == ri[s] ? wr[s] : 0.f));
        v[s * DL_DFL + i] = gi;
      }
  }
}

// per foreground anchor: box and DFL sums, NaN flags
template <typename T>
__global__ __launch_bounds__(256) void box_kernel(LossLevels L, int A, const unsigned char* fg, const float* tbox,
                                                  const float* tltrb, int iou_type, float* part) {
  const int a = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  float lb = 0.f, ld = 0.f, nb = 0.f, nd = 0.f;
  if (a < A && fg[(long)b * A + a]) {
    int l;
    float ax, ay;
    const long row = anchor_row(L, b, a, l, ax, ay);
    float v[4 * DL_DFL];
    load_dist(reinterpret_cast<const T*>(L.x[l]) + row, v);
    const float4 tb = reinterpret_cast<const float4*>(tbox)[(long)b * A + a];
    const float4 tl = reinterpret_cast<const float4*>(tltrb)[(long)b * A + a];
    box_dfl<false>(v, ax, ay, L.stride[l], tb, tl, iou_type, 0.f, 0.f, lb, ld);
    if (isnan(lb)) { nb = 1.f; lb = 0.f; }
    if (isnan(ld)) { nd = 1.f; ld = 0.f; }
  }
  const long slot = ((long)b * gridDim.x + blockIdx.x) * 4;
  block_sum_store(lb, part, slot + 0);
  block_sum_store(ld, part, slot + 1);
  block_sum_store(nb, part, slot + 2);
  block_sum_store(nd, part, slot + 3);
}

// gradient of the box + DFL terms into the 64 DFL logits of every anchor
template <typename T>
__global__ __launch_bounds__(256) void boxgrad_kernel(LossLevels L, int A, const unsigned char* fg,
                                                      const float* tbox, const float* tltrb, int iou_type,
                                                      const float* img_flags, float lam_box, float lam_dfl,
                                                      int B, const int* nfg) {
  const int a = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (a >= A) return;
  int l;
  float ax, ay;
  const long row = anchor_row(L, b, a, l, ax, ay);
  if (!L.g[l]) return;
  T* gp = reinterpret_cast<T*>(L.g[l]) + row;
  float v[4 * DL_DFL];
  if (fg[(long)b * A + a]) {
    load_dist(reinterpret_cast<const T*>(L.x[l]) + row, v);
    const float n = (float)nfg[b];
    // no gradient from a term that was NaN for this image (the reference replaces it by 0)
    const float sb = img_flags[2 * b] != 0.f ? 0.f : lam_box / ((float)B * n);
    const float sd = img_flags[2 * b + 1] != 0.f ? 0.f : lam_dfl / ((float)B * 4.f * n);
    const float4 tb = reinterpret_cast<const float4*>(tbox)[(long)b * A + a];
    const float4 tl = reinterpret_cast<const float4*>(tltrb)[(long)b * A + a];
    float lb, ld;
    box_dfl<true>(v, ax, ay, L.stride[l], tb, tl, iou_type, sb, sd, lb, ld);
  } else {
#pragma unroll
    for (int i = 0; i < 4 * DL_DFL; ++i) v[i] = 0.f;
  }
#pragma unroll
  for (int k = 0; k < 4 * DL_DFL / 8; ++k) {
    float t[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) t[i] = v[8 * k + i];
    Vec8<T>::store(gp + 8 * k, t);
  }
}

// per-image NaN flags from the box partials (needed before the gradient pass)
__global__ void flags_kernel(int B, int gx, const float* part, float* flags) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float nb = 0.f, nd = 0.f;
  for (int k = 0; k < gx; ++k) {
    nb += part[((long)b * gx + k) * 4 + 2];
    nd += part[((long)b * gx + k) * 4 + 3];
  }
  flags[2 * b] = nb;
  flags[2 * b + 1] = nd;
}

// per-image sums in fixed order (one thread per image), then thread 0 combines the images
__global__ __launch_bounds__(256) void finalize_kernel(int B, int A, int nc, int gxc, const float* pcls, int gxb,
                                                       const float* pbox, const int* nfg, float lam_box,
                                                       float lam_cls, float lam_dfl, double* img, float* out) {
  for (int b = threadIdx.x; b < B; b += blockDim.x) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    const float* pc = pcls + (long)b * gxc;
    int k = 0;
    for (; k + 3 < gxc; k += 4) { s0 += pc[k]; s1 += pc[k + 1]; s2 += pc[k + 2]; s3 += pc[k + 3]; }
    for (; k < gxc; ++k) s0 += pc[k];
    const double mean = ((s0 + s1) + (s2 + s3)) / ((double)A * (double)nc);
    double cls = mean, box = 0.0, dfl = 0.0;
    if (nfg[b] > 0) {
      cls = 2.0 * mean;                                  // loss.py:530 + :551
      double sb = 0.0, sd = 0.0, fb = 0.0, fd = 0.0;
      for (int q = 0; q < gxb; ++q) {
        const float* p = pbox + ((long)b * gxb + q) * 4;
        sb += p[0]; sd += p[1]; fb += p[2]; fd += p[3];
      }
      if (fb == 0.0) box = sb / (double)nfg[b];
      if (fd == 0.0) dfl = sd / (4.0 * (double)nfg[b]);
    }
    img[3 * b] = cls;
    img[3 * b + 1] = box;
    img[3 * b + 2] = dfl;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double lcls = 0.0, lbox = 0.0, ldfl = 0.0;
  for (int b = 0; b < B; ++b) { lcls += img[3 * b]; lbox += img[3 * b + 1]; ldfl += img[3 * b + 2]; }
  lbox /= B; lcls /= B; ldfl /= B;
  out[0] = (float)(lam_box * lbox + lam_cls * lcls + lam_dfl * ldfl);
  out[1] = (float)lbox;
  out[2] = (float)lcls;
  out[3] = (float)ldfl;
}

// workspace layout (bytes, 256-aligned pieces)
struct LossWs {
  size_t pbox, kcnt, kidx, fg, tbox, tltrb, cbits, nfg, pcls, pboxp, flags, img, total;
};
static LossWs loss_ws(int B, int A, int nc, int M) {
  const auto al = ws_align;
  const int nw = (nc + 31) / 32;
  const int gxc = cdiv((long)A * ((nc + 7) / 8), 256), gxb = cdiv(A, 256);
  LossWs w{};
  size_t o = 0;
  w.pbox = o; o += al((size_t)B * A * 16);
  w.kcnt = o; o += al((size_t)(M > 0 ? M : 1) * 4);
  w.kidx = o; o += al((size_t)(M > 0 ? M : 1) * DL_TOPK * 4);
  w.fg = o; o += al((size_t)B * A);
  w.tbox = o; o += al((size_t)B * A * 16);
  w.tltrb = o; o += al((size_t)B * A * 16);
  w.cbits = o; o += al((size_t)B * A * nw * 4);
  w.nfg = o; o += al((size_t)B * 4);
  w.pcls = o; o += al((size_t)B * gxc * 4);
  w.pboxp = o; o += al((size_t)B * gxb * 16);
  w.flags = o; o += al((size_t)B * 8);
  w.img = o; o += al((size_t)B * 24);
  w.total = o;
  return w;
}

// d(total)/d(maps) times the incoming loss gradient g (a device scalar), in place.  The fused loss
// writes its map gradients in the forward, before g exists; in the training loop g is the 1.0 seed
// of loss.backward(), so every block reads g and leaves at once -- one short launch instead of an
// elementwise pass over the 155 MB of head gradients (configs[2]).  Otherwise v = T(float(v) *
// float(T(g))): torch's `grad * g.to(grad.dtype)`.
struct ScaleBufs {
  void* p[4];
  long n[4];
};

template <typename T>
__global__ __launch_bounds__(256) void scale_by_dev_kernel(ScaleBufs b, const float* g) {
  const float gv = *g;
  if (gv == 1.0f) return;
  const float s = to_f(from_f<T>(gv));
  T* p = (T*)b.p[blockIdx.y];
  const long n = b.n[blockIdx.y];
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) p[i] = from_f<T>(to_f(p[i]) * s);
}

}  // namespace yms

using namespace yms;

extern "C" {

size_t yms_det_loss_ws_bytes(int batch, int anchors, int nc, int n_targets) {
  if (batch <= 0 || anchors <= 0 || nc <= 0 || n_targets < 0) return 0;
  return loss_ws(batch, anchors, nc, n_targets).total;
}

yms_status yms_det_loss(int dtype, int batch, int nc, int nlevels, const void* const* maps, void* const* grads,
                        const int* hs, const int* ws_, const float* strides, int ld, const float* targets,
                        int n_targets, float img_w, float img_h, int iou_type, const float* pos_weight,
                        const float* lambdas, void* ws, size_t ws_bytes, float* out, void* stream) {
  if (!out || !lambdas || !map_dtype_ok(dtype) || iou_type < 0 || iou_type > 3) return YMS_ERR_INVALID;
  LossLevels L;
  int A;
  const yms_status bad = loss_levels(batch, nc, nlevels, maps, grads, hs, ws_, strides, ld, targets, n_targets,
                                     img_w, img_h, L, A);
  if (bad != YMS_OK) return bad;
  const LossWs w = loss_ws(batch, A, nc, n_targets);
  if (!ws || ws_bytes < w.total) return YMS_ERR_INVALID;
  char* base = (char*)ws;
  float* pbox = (float*)(base + w.pbox);
  int* kcnt = (int*)(base + w.kcnt);
  int* kidx = (int*)(base + w.kidx);
  unsigned char* fg = (unsigned char*)(base + w.fg);
  float* tbox = (float*)(base + w.tbox);
  float* tltrb = (float*)(base + w.tltrb);
  unsigned* cbits = (unsigned*)(base + w.cbits);
  int* nfg = (int*)(base + w.nfg);
  float* pcls = (float*)(base + w.pcls);
  float* pboxp = (float*)(base + w.pboxp);
  float* flags = (float*)(base + w.flags);
  double* img = (double*)(base + w.img);
  const int nw = (nc + 31) / 32;
  const int gxc = cdiv((long)A * ((nc + 7) / 8), 256), gxb = cdiv(A, 256);
  hipStream_t st = (hipStream_t)stream;
  const float gscale = lambdas[1] / ((float)batch * (float)A * (float)nc);
  return launch_for_dtype(dtype, [&](auto map_type) {
    using T = typename decltype(map_type)::type;
    hipLaunchKernelGGL(decode_kernel<T>, dim3(gxb, batch), dim3(256), 0, st, L, A, pbox);
    if (n_targets > 0)
      hipLaunchKernelGGL(topk_kernel, dim3(n_targets), dim3(256), 0, st, targets, batch, A, img_w, img_h, pbox, kcnt,
                         kidx);
    hipLaunchKernelGGL(assign_kernel, dim3(batch), dim3(256), 0, st, targets, n_targets, A, nc, nw, img_w, img_h, L,
                       kcnt, kidx, fg, tbox, tltrb, cbits, nfg);
    hipLaunchKernelGGL(cls_kernel<T>, dim3(gxc, batch), dim3(256), 0, st, L, A, nc, nw, cbits, nfg, pos_weight,
                       gscale, pcls);
    hipLaunchKernelGGL(box_kernel<T>, dim3(gxb, batch), dim3(256), 0, st, L, A, fg, tbox, tltrb, iou_type, pboxp);
    hipLaunchKernelGGL(flags_kernel, dim3(cdiv(batch, 64)), dim3(64), 0, st, batch, gxb, pboxp, flags);
    if (grads)
      hipLaunchKernelGGL(boxgrad_kernel<T>, dim3(gxb, batch), dim3(256), 0, st, L, A, fg, tbox, tltrb, iou_type,
                         flags, lambdas[0], lambdas[2], batch, nfg);
    hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(256), 0, st, batch, A, nc, gxc, pcls, gxb, pboxp, nfg,
                       lambdas[0], lambdas[1], lambdas[2], img, out);
  });
}

yms_status yms_scale_by_device_scalar(int dtype, int nbuf, void* const* bufs, const long* counts, const float* g,
                                      void* stream) {
  if (nbuf < 1 || nbuf > 4 || !bufs || !counts || !g) return YMS_ERR_INVALID;
  ScaleBufs b{};
  long mx = 0;
  for (int i = 0; i < nbuf; ++i) {
    if (!bufs[i] || counts[i] < 0) return YMS_ERR_INVALID;
    b.p[i] = bufs[i];
    b.n[i] = counts[i];
    mx = std::max(mx, counts[i]);
  }
  const dim3 grid((unsigned)std::max<long>(1, std::min<long>(1024, cdiv(mx, 256))), (unsigned)nbuf);
  return launch_for_dtype(dtype, [&](auto map_type) {
    hipLaunchKernelGGL(scale_by_dev_kernel<typename decltype(map_type)::type>, grid, dim3(256), 0,
                       (hipStream_t)stream, b, g);
  });
}

}  // extern "C"
