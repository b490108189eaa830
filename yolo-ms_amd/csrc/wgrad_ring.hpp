// Host interface of the LDS-DMA ring weight gradient (wgrad_ring.hip), dispatched from
// wgrad_route / yms_conv_wgrad in wgrad.hip.
#pragma once
#include "wgrad.hpp"

namespace yms {

struct WRPlan {
  int bm, bn, kp;                            // tile rows (co) / columns (tap*cin8+ci), pixels per k-tile
  int cin8, cpt, kc;                         // input channels rounded to 8, 16-B chunks per tap, valid chunks
  int tiles_m, tiles_n, nkt, slab_rows, slab_ld;
  int want_splits;                           // wgrad_splits' count over the nkt k-tiles, before wgrad_route evens it
};

// False when the shape / dtype is not handled here (another weight-gradient kernel runs) or
// YMS_WG_RING=0.
bool wgrad_ring_plan(const yms_conv_shape* s, WRPlan* w);
// Partial slabs [a.splits][slab_rows][slab_ld] (the layout wgrad_reduce_kernel sums).
yms_status wgrad_ring_launch(const yms_conv_shape* s, const WRPlan& w, const WgradArgs& a, hipStream_t st);

}  // namespace yms
