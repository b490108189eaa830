// Tiled (sliced) inference merge for gfx950: the decoded predictions of the tile inputs of a batch of
// large images -- every tile one crop at native resolution, all of one input size -- are gathered into
// one [n, S * A, 4+nc] tensor in original-image pixels, which yms_det_candidates then reads like any
// single view's.  Images have different tile counts, so the gather is driven by a DEVICE table of
// n * S slot records (yms_tile_slot): which tile input fills slot s of image b, the slot's un-map
// and its four suppression bounds.
//
// Per row: the box is un-mapped with tta_merge's operations ((v - pad) / gain, v / gain, each rounded
// separately, no contraction); the scores move as bits unless the row's box crosses one of the slot's
// bounds (a box the tile's cut has truncated), in which case every score becomes -1 -- below any conf
// >= 0, so detect never takes it.  An empty slot, or a tile index outside [0, T), writes four zeros and
// -1 scores and reads nothing of pred: the index is device data and is bounds-checked here.
//
// Shape: a streaming copy.  One work item is (slot, chunk of 256 units) and a block walks the items
// with stride gridDim.x, so a block's slot record is uniform (its fields come through the scalar
// cache, as mosaic_normalize_kernel's record does) and only the split unit -> (row, unit of the row)
// is per lane.  A unit is a float4 when 4+nc is a multiple of 4 and pred and out are 16-byte aligned
// (then every row start is), else one float.  A score unit learns its row's verdict by
// re-reading the row's box -- the 16 bytes that the row's unit 0, nearly always a lane of the same
// wave, reads too: an L1 hit, not HBM traffic -- and only in slots that have a finite bound.
#include <algorithm>

#include "yms_common.hpp"

#pragma clang fp contract(off)

namespace yms {

constexpr int TILE_BLOCK = 256;
constexpr int TILE_MAX_BLOCKS = 256 * 32;

static_assert(sizeof(yms_tile_slot) == 48, "yms_tile_slot is 48 bytes");

// true when the box (cx, cy, w, h) crosses a bound of slot s; a NaN compares false everywhere
__device__ __forceinline__ bool tile_cut(const yms_tile_slot& s, float cx, float cy, float w, float h) {
  const float hw = 0.5f * w, hh = 0.5f * h;
  const float x0 = cx - hw, y0 = cy - hh, x1 = cx + hw, y1 = cy + hh;
  return x0 < s.lo_x || y0 < s.lo_y || x1 > s.hi_x || y1 > s.hi_y;
}

// VEC = 4: units of float4, unit 0 of a row is its box; VEC = 1: single floats.
template <int VEC>
__global__ __launch_bounds__(TILE_BLOCK) void tile_merge_kernel(const float* __restrict__ pred,
                                                                const yms_tile_slot* __restrict__ tab,
                                                                float* __restrict__ out, long nslots, int A, int nc,
                                                                int T, int chunks, FastDiv upr_div) {
  const int no = 4 + nc, upr = no / VEC;                     // units per row
  const unsigned ups = (unsigned)A * (unsigned)upr;          // units per slot, <= 2^31 - 1 (host check)
  const long items = nslots * chunks;
  for (long it = blockIdx.x; it < items; it += gridDim.x) {
    const long rec = it / chunks;
    const unsigned unit = (unsigned)(it - rec * chunks) * TILE_BLOCK + threadIdx.x;
    if (unit >= ups) continue;
    const yms_tile_slot& s = tab[rec];                       // uniform per block
    const int a = (int)fdiv(unit, upr_div), u = (int)unit - a * upr;
    const bool live = (unsigned)s.tile < (unsigned)T;        // -1 (empty) and anything else outside pred
    const bool bounded = s.lo_x > -INFINITY || s.lo_y > -INFINITY || s.hi_x < INFINITY || s.hi_y < INFINITY;
    const float* src = pred + ((long)(live ? s.tile : 0) * A + a) * no;
    float* dst = out + (rec * A + a) * no;
    if (VEC == 4) {
      float4 x = u == 0 ? make_float4(0.f, 0.f, 0.f, 0.f) : make_float4(-1.f, -1.f, -1.f, -1.f);
      if (live) {
        x = reinterpret_cast<const float4*>(src)[u];
        if (u == 0) {
          x.x = (x.x - s.pad_x) / s.gain_x;
          x.y = (x.y - s.pad_y) / s.gain_y;
          x.z = x.z / s.gain_x;
          x.w = x.w / s.gain_y;
        } else if (bounded) {
          const float4 bx = reinterpret_cast<const float4*>(src)[0];
          if (tile_cut(s, bx.x, bx.y, bx.z, bx.w)) x = make_float4(-1.f, -1.f, -1.f, -1.f);
        }
      }
      reinterpret_cast<float4*>(dst)[u] = x;
    } else {
      float x = u < 4 ? 0.f : -1.f;
      if (live) {
        x = src[u];
        if (u == 0) x = (x - s.pad_x) / s.gain_x;
        else if (u == 1) x = (x - s.pad_y) / s.gain_y;
        else if (u == 2) x = x / s.gain_x;
        else if (u == 3) x = x / s.gain_y;
        else if (bounded && tile_cut(s, src[0], src[1], src[2], src[3])) x = -1.f;
      }
      dst[u] = x;
    }
  }
}

}  // namespace yms

using namespace yms;

extern "C" int yms_tile_merge_max_blocks(void) { return TILE_MAX_BLOCKS; }

extern "C" yms_status yms_tile_merge(int n, int S, int A, int nc, int T, const float* pred, const yms_tile_slot* table,
                                     float* out, void* stream) {
  if (!pred || !table || !out) return YMS_ERR_INVALID;
  if ((uintptr_t)pred % 4 != 0 || (uintptr_t)table % 4 != 0 || (uintptr_t)out % 4 != 0) return YMS_ERR_INVALID;
  if (n < 1 || n > 65535 || S < 1 || A < 1 || nc < 1 || T < 1) return YMS_ERR_INVALID;
  if ((long)A * (4L + nc) > 0x7fffffffL) return YMS_ERR_INVALID;
  if ((long)S * A * nc >= 0x80000000L) return YMS_ERR_INVALID;
  const bool vec = (4 + nc) % 4 == 0 && (uintptr_t)pred % 16 == 0 && (uintptr_t)out % 16 == 0;
  const int upr = (4 + nc) / (vec ? 4 : 1);
  const long ups = (long)A * upr;
  const int chunks = (int)((ups + TILE_BLOCK - 1) / TILE_BLOCK);
  const long nslots = (long)n * S;
  const unsigned grid = (unsigned)std::min<long>(nslots * chunks, TILE_MAX_BLOCKS);   // item-stride beyond
  const FastDiv d = make_fastdiv((uint32_t)upr);
  hipStream_t st = (hipStream_t)stream;
  if (vec) hipLaunchKernelGGL(tile_merge_kernel<4>, dim3(grid), dim3(TILE_BLOCK), 0, st, pred, table, out, nslots, A, nc, T, chunks, d);
  else hipLaunchKernelGGL(tile_merge_kernel<1>, dim3(grid), dim3(TILE_BLOCK), 0, st, pred, table, out, nslots, A, nc, T, chunks, d);
  return launch_status();
}
