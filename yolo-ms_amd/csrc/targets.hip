// Training targets of a batch of sampled plans, computed on the GPU (yms_box_targets): the host's
// transform_boxes / mosaic_boxes (yms/data.py) restated so that an input pipeline whose images
// stay on the device (yms/cache.py) has no per-box host work left.
//
// One thread per CANDIDATE row.  The host lays the batch out as tiles -- one per (output image,
// layer, source) -- and gives every tile a block of `count` output rows starting at `out0`, one per
// annotation of its source, whether or not the box survives: a survivor's row is
// (image, class, cx, cy, w, h), any other row is (-1, 0, 0, 0, 0, 0), which the three fused losses
// skip.  Nothing is compacted or counted, so the caller reads nothing back.
//
// A row's box goes, in float64 and in exactly this order (tests/targets_ref.py replays it bit for
// bit; contraction is off, so no multiply-add is fused):
//   1. to the canvas: u = (ox + x gx, oy + y gy, ox + (x + w) gx, oy + (y + h) gy);
//   2. clip tiles only: k = u intersected with the tile's rect; nothing left -> dropped.  Else k = u;
//   3. the corner envelopes of u and k through the layer's stages: each corner (X - 0.5, Y - 0.5) ->
//      q_j = (F[j][0] X + F[j][1] Y) + F[j][2], X = q_0 / q_2, Y = q_1 / q_2, per stage; + 0.5 at the end;
//   4. k's envelope clipped to the output frame once;
//   5. dropped when u's envelope has no area, when clipped / unclipped area < 0.1 (min_visibility) or
//      when the clipped area < 1 px (min_area);
//   6. normalised by the frame; kept only if w, h > 1e-3 and cx, cy, w, h lie in [0, 1].
// The only rounding to float32 is the store.  Every table index is checked before it is used: a row
// whose tile names a layer or an annotation outside its table is written as ignored.
#include "yms_common.hpp"

namespace yms {

constexpr int TGT_MAX_STAGES = 8;      // AUG_MAX_STAGES (preprocess.hip)

struct TgtLayer {
  int nst, out_w, out_h, pad_;
  double m[TGT_MAX_STAGES][9];         // FORWARD maps of pixel-index coordinates, as AugPlan.stages holds them
};
struct TgtTile {
  int image, layer;                    // output image index; row of the layer table
  int ann0, count;                     // first row of the annotation table, number of boxes
  int out0;                            // first output row
  int clip;                            // 1: intersect with the rect (a Mosaic tile); 0: a plain sample
  double gx, gy, ox, oy;               // box -> canvas
  double rx0, ry0, rx1, ry1;           // canvas rect
};

__device__ __forceinline__ double dmin(double a, double b) { return b < a ? b : a; }   // Python's min(a, b)
__device__ __forceinline__ double dmax(double a, double b) { return b > a ? b : a; }   // Python's max(a, b)

// envelope (x0, y0, x1, y1) of the box's four corners after the stages
__device__ __forceinline__ void envelope(const TgtLayer& ly, int nst, double bx0, double by0, double bx1, double by1,
                                         double (&e)[4]) {
#pragma clang fp contract(off)
  const double cx[4] = {bx0, bx1, bx1, bx0}, cy[4] = {by0, by0, by1, by1};
  for (int c = 0; c < 4; ++c) {
    double X = cx[c] - 0.5, Y = cy[c] - 0.5;
    for (int s = 0; s < nst; ++s) {
      const double* F = ly.m[s];
      const double q0 = (F[0] * X + F[1] * Y) + F[2];
      const double q1 = (F[3] * X + F[4] * Y) + F[5];
      const double q2 = (F[6] * X + F[7] * Y) + F[8];
      X = q0 / q2;
      Y = q1 / q2;
    }
    X = X + 0.5;
    Y = Y + 0.5;
    if (c == 0) {
      e[0] = e[2] = X;
      e[1] = e[3] = Y;
    } else {
      e[0] = dmin(e[0], X);
      e[1] = dmin(e[1], Y);
      e[2] = dmax(e[2], X);
      e[3] = dmax(e[3], Y);
    }
  }
}

__global__ __launch_bounds__(256) void box_targets_kernel(const TgtTile* __restrict__ tiles, int ntiles,
                                                          const TgtLayer* __restrict__ layers, int nlayers,
                                                          const double* __restrict__ boxes,
                                                          const int* __restrict__ labels, long nann, int m_cap,
                                                          float* __restrict__ out) {
#pragma clang fp contract(off)
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= m_cap) return;
  // the last tile whose first row is not past this one (tiles are sorted by out0)
  int lo = 0, hi = ntiles;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tiles[mid].out0 <= row) lo = mid; else hi = mid;
  }
  const TgtTile t = tiles[lo];
  const int k = row - t.out0;
  const long a = (long)t.ann0 + k;
  float o[6] = {-1.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (k >= 0 && k < t.count && t.layer >= 0 && t.layer < nlayers && a >= 0 && a < nann) {
    const TgtLayer& ly = layers[t.layer];
    const int nst = min(max(ly.nst, 0), TGT_MAX_STAGES);
    const double x = boxes[4 * a], y = boxes[4 * a + 1], w = boxes[4 * a + 2], h = boxes[4 * a + 3];
    const double u0 = t.ox + x * t.gx, u1 = t.oy + y * t.gy;
    const double u2 = t.ox + (x + w) * t.gx, u3 = t.oy + (y + h) * t.gy;
    double k0 = u0, k1 = u1, k2 = u2, k3 = u3;
    bool keep = true;
    if (t.clip) {
      k0 = dmax(u0, t.rx0);
      k1 = dmax(u1, t.ry0);
      k2 = dmin(u2, t.rx1);
      k3 = dmin(u3, t.ry1);
      keep = !(k2 <= k0 || k3 <= k1);
    }
    if (keep) {
      double eu[4], ek[4];
      envelope(ly, nst, u0, u1, u2, u3, eu);
      if (t.clip) {
        envelope(ly, nst, k0, k1, k2, k3, ek);
      } else {
        ek[0] = eu[0]; ek[1] = eu[1]; ek[2] = eu[2]; ek[3] = eu[3];
      }
      const double W = (double)ly.out_w, H = (double)ly.out_h;
      const double area = (eu[2] - eu[0]) * (eu[3] - eu[1]);
      const double cx0 = dmin(dmax(ek[0], 0.0), W), cy0 = dmin(dmax(ek[1], 0.0), H);
      const double cx1 = dmin(dmax(ek[2], 0.0), W), cy1 = dmin(dmax(ek[3], 0.0), H);
      const double carea = dmax(cx1 - cx0, 0.0) * dmax(cy1 - cy0, 0.0);
      if (!(area <= 0.0 || carea / area < 0.1 || carea < 1.0)) {
        const double bw = cx1 - cx0, bh = cy1 - cy0;
        const double cxn = (cx0 + bw / 2.0) / W, cyn = (cy0 + bh / 2.0) / H, wn = bw / W, hn = bh / H;
        if (wn > 1e-3 && hn > 1e-3 && 0.0 <= cxn && cxn <= 1.0 && 0.0 <= cyn && cyn <= 1.0 && 0.0 <= wn &&
            wn <= 1.0 && 0.0 <= hn && hn <= 1.0) {
          o[0] = (float)t.image;
          o[1] = (float)labels[a];
          o[2] = (float)cxn;
          o[3] = (float)cyn;
          o[4] = (float)wn;
          o[5] = (float)hn;
        }
      }
    }
  }
  float2* dst = reinterpret_cast<float2*>(out + (long)row * 6);   // rows of 24 bytes: 8-byte aligned
  dst[0] = make_float2(o[0], o[1]);
  dst[1] = make_float2(o[2], o[3]);
  dst[2] = make_float2(o[4], o[5]);
}

}  // namespace yms

using namespace yms;

extern "C" {

size_t yms_tgt_tile_bytes(void) { return sizeof(TgtTile); }
size_t yms_tgt_layer_bytes(void) { return sizeof(TgtLayer); }

yms_status yms_box_targets(int ntiles, const void* tiles, int nlayers, const void* layers, const double* boxes,
                           const int* labels, long nann, int m_cap, float* out, void* stream) {
  if (m_cap < 0 || ntiles < 0 || nlayers < 0 || nann < 0) return YMS_ERR_INVALID;
  if (m_cap == 0) return YMS_OK;
  if (ntiles == 0 || nlayers == 0 || nann == 0 || !tiles || !layers || !boxes || !labels || !out)
    return YMS_ERR_INVALID;
  if (((uintptr_t)out & 7) != 0 || ((uintptr_t)tiles & 7) != 0 || ((uintptr_t)layers & 7) != 0 ||
      ((uintptr_t)boxes & 7) != 0 || ((uintptr_t)labels & 3) != 0)
    return YMS_ERR_INVALID;
  hipLaunchKernelGGL(box_targets_kernel, dim3((unsigned)cdiv(m_cap, 256)), dim3(256), 0, (hipStream_t)stream,
                     (const TgtTile*)tiles, ntiles, (const TgtLayer*)layers, nlayers, boxes, labels, nann, m_cap, out);
  return launch_status();
}

}  // extern "C"
