// Test-time-augmentation view merge for gfx950: the decoded predictions of up to YMS_TTA_MAX_VIEWS
// views of one batch (other input sizes, flipped inputs, or other models over the same images) are
// copied into one [n, R, 4+nc] tensor in original-image pixels, which yms_det_candidates then reads
// like any single view's.
//
// Per view v: pred_v [n, A_v, 4+nc] (cx, cy, w, h in view pixels + scores), the rows [a0_v, a1_v) to
// take, the view's input size, its flip bits and its frames [n, 6] = (gain_x, gain_y, pad_x, pad_y,
// w0, h0).  A box is un-flipped (x -> W_v - x), un-padded and un-scaled with separately rounded fp32
// operations (no contraction), nothing is clipped; the scores are moved as bits.  Each of a row's four
// box numbers depends on that number alone, so the kernel is a flat streaming copy over the output's
// elements in which the elements of columns 0..3 take the un-map: as float4 when 4+nc is a multiple
// of 4 and every base is 16-byte aligned (then every row start is), scalar otherwise.  The per-view
// arguments travel as kernel arguments (yms_head_decode's way): one launch, no table upload.
#include <algorithm>

#include "yms_common.hpp"

#pragma clang fp contract(off)

namespace yms {

constexpr int TTA_MAX_VIEWS = YMS_TTA_MAX_VIEWS;

struct TtaParams {
  const float* pred[TTA_MAX_VIEWS];
  const float* frames[TTA_MAX_VIEWS];
  int A[TTA_MAX_VIEWS], a0[TTA_MAX_VIEWS];
  int roff[TTA_MAX_VIEWS + 1];      // first output row of view v; roff[nviews] = R
  float W[TTA_MAX_VIEWS], H[TTA_MAX_VIEWS];
  int flip[TTA_MAX_VIEWS];
  int nviews, nc, n;
  float* out;
};

// column k (0 cx, 1 cy, 2 w, 3 h) of a box through view v's flip and image b's frame
__device__ __forceinline__ float tta_unmap(const TtaParams& p, int v, const float* f, int k, float x) {
  if (k == 0) {
    if (p.flip[v] & 1) x = p.W[v] - x;
    return (x - f[2]) / f[0];
  }
  if (k == 1) {
    if (p.flip[v] & 2) x = p.H[v] - x;
    return (x - f[3]) / f[1];
  }
  return x / f[k - 2];
}

// VEC = 4: units of float4, unit 0 of a row is its box; VEC = 1: single floats.
template <int VEC>
__global__ __launch_bounds__(256) void tta_merge_kernel(TtaParams p) {
  const int no = 4 + p.nc, upr = no / VEC;                   // units per row
  const int R = p.roff[p.nviews];
  const long total = (long)p.n * R * upr;
  const long stride = (long)gridDim.x * 256;
  for (long t = blockIdx.x * 256L + threadIdx.x; t < total; t += stride) {
    const long row = t / upr;
    const int u = (int)(t - row * upr);
    const int b = (int)(row / R), r = (int)(row - (long)b * R);
    int v = 0;
    while (v + 1 < p.nviews && r >= p.roff[v + 1]) ++v;
    const float* src = p.pred[v] + ((long)b * p.A[v] + p.a0[v] + (r - p.roff[v])) * no;
    float* dst = p.out + row * no;
    if (VEC == 4) {
      float4 x = reinterpret_cast<const float4*>(src)[u];
      if (u == 0) {
        const float* f = p.frames[v] + 6 * (long)b;
        x.x = tta_unmap(p, v, f, 0, x.x);
        x.y = tta_unmap(p, v, f, 1, x.y);
        x.z = tta_unmap(p, v, f, 2, x.z);
        x.w = tta_unmap(p, v, f, 3, x.w);
      }
      reinterpret_cast<float4*>(dst)[u] = x;
    } else {
      float x = src[u];
      if (u < 4) x = tta_unmap(p, v, p.frames[v] + 6 * (long)b, u, x);
      dst[u] = x;
    }
  }
}

}  // namespace yms

using namespace yms;

extern "C" yms_status yms_tta_merge(int n, int nc, int nviews, const float* const* preds, const int* A,
                                    const int* a0, const int* a1, const int* H, const int* W, const int* flips,
                                    const float* const* frames, float* out, void* stream) {
  if (n <= 0 || n > 65535 || nc <= 0 || nviews < 1 || nviews > TTA_MAX_VIEWS) return YMS_ERR_INVALID;
  if (!preds || !A || !a0 || !a1 || !H || !W || !flips || !frames || !out) return YMS_ERR_INVALID;
  TtaParams p;
  long R = 0;
  bool vec = (4 + nc) % 4 == 0 && (uintptr_t)out % 16 == 0;
  for (int v = 0; v < nviews; ++v) {
    if (!preds[v] || !frames[v] || A[v] <= 0 || a0[v] < 0 || a1[v] <= a0[v] || a1[v] > A[v]) return YMS_ERR_INVALID;
    if (H[v] <= 0 || W[v] <= 0 || flips[v] < 0 || flips[v] > 3) return YMS_ERR_INVALID;
    if ((uintptr_t)preds[v] % 4 != 0 || (uintptr_t)frames[v] % 4 != 0) return YMS_ERR_INVALID;
    if ((long)A[v] * (4 + nc) > 0x7fffffffL) return YMS_ERR_INVALID;
    vec = vec && (uintptr_t)preds[v] % 16 == 0;
    p.pred[v] = preds[v];
    p.frames[v] = frames[v];
    p.A[v] = A[v];
    p.a0[v] = a0[v];
    p.roff[v] = (int)R;
    p.W[v] = (float)W[v];
    p.H[v] = (float)H[v];
    p.flip[v] = flips[v];
    R += a1[v] - a0[v];
    if (R * nc >= 0x80000000L) return YMS_ERR_INVALID;
  }
  if ((uintptr_t)out % 4 != 0) return YMS_ERR_INVALID;
  for (int v = nviews; v < TTA_MAX_VIEWS; ++v) {
    p.pred[v] = nullptr; p.frames[v] = nullptr;
    p.A[v] = 0; p.a0[v] = 0; p.W[v] = 0.f; p.H[v] = 0.f; p.flip[v] = 0;
  }
  for (int v = nviews; v <= TTA_MAX_VIEWS; ++v) p.roff[v] = (int)R;
  p.nviews = nviews;
  p.nc = nc;
  p.n = n;
  p.out = out;
  const long units = (long)n * R * ((4 + nc) / (vec ? 4 : 1));
  const unsigned grid = (unsigned)std::min<long>((units + 255) / 256, 256L * 32);   // grid-stride beyond
  hipStream_t st = (hipStream_t)stream;
  if (vec) hipLaunchKernelGGL(tta_merge_kernel<4>, dim3(grid), dim3(256), 0, st, p);
  else hipLaunchKernelGGL(tta_merge_kernel<1>, dim3(grid), dim3(256), 0, st, p);
  return launch_status();
}
