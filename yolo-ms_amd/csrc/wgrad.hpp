// What the three weight-gradient kernels' hosts share (wgrad.hip: the route, the register-staged TT
// kernel and the reduce; wgrad_ring.hip; wgrad_halo.hip): the call's operands, the split-count rule and
// the run-time switches.
#pragma once
#include <cstdlib>

#include "conv_common.hpp"

namespace yms {

// YMS_WG_* switches are read on every call: tests switch them at run time
inline int env_int(const char* name, int dflt) {
  const char* v = getenv(name);
  return v ? atoi(v) : dflt;
}
inline double env_double(const char* name, double dflt) {
  const char* v = getenv(name);
  return v ? atof(v) : dflt;
}

// splits = min(by_work, ceil(blocks_per_cu * CUs / tiles)), then capped so that the slabs' write +
// re-read (slab_rt_bytes per split) stays under `ratio` x the layer's x + dz bytes (data_bytes) while
// >= 256 blocks remain; ratio 0: no cap (wgrad.hip)
int wgrad_splits(int by_work, int tiles, int blocks_per_cu, double data_bytes, double slab_rt_bytes);

// One call's operands and its split of the work: `splits` partial slabs of `per` work units (k-tiles /
// patches) each, as yms_conv_wgrad fitted them to the workspace.
struct WgradArgs {
  const void* x;
  const void* dz;
  int x_ld, x_off, dz_ld, dz_off;   // elements
  float* slab;
  int per, splits;
};

// Fills the operand fields every weight-gradient parameter struct has.  The kernels address x and dz
// as raw buffers with 32-bit offsets: false when a byte extent is not < 2^31 - 2^20.
template <typename P>
inline bool wgrad_operands(P& p, const yms_conv_shape* s, const WgradArgs& a) {
  const long es = elem_size(s->dtype);
  const long dzb = (long)s->n * s->ho * s->wo * a.dz_ld * es, xb = (long)s->n * s->h * s->w * a.x_ld * es;
  if (dzb >= (1l << 31) - (1l << 20) || xb >= (1l << 31) - (1l << 20)) return false;
  p.x = (const char*)a.x;
  p.dz = (const char*)a.dz;
  p.slab = a.slab;
  p.x_ld = a.x_ld; p.x_off = a.x_off; p.dz_ld = a.dz_ld; p.dz_off = a.dz_off;
  p.dz_bytes = (uint32_t)dzb;
  p.x_bytes = (uint32_t)xb;
  return true;
}

}  // namespace yms
