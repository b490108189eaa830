// Host interface of the halo-tiled 3x3 weight gradient (wgrad_halo.hip), dispatched from
// wgrad_route / yms_conv_wgrad in wgrad.hip.
#pragma once
#include "wgrad.hpp"

namespace yms {

struct WHPlan {
  int S, mb, nb, wk, kp, hb;          // kernel variant: stride, co / ci 32-blocks, k-step wave groups,
                                      // pixels and halo capacity
  int TW, R, HR, HC;                  // patch of R x TW output pixels, halo of HR x HC input pixels
  int ptx, pty, npatch;               // patches per row / column, total
  int want_splits;                    // wgrad_splits' count over the patches, before wgrad_route evens it
  int tiles_co, tiles_ci, slab_rows, slab_ld;
};

// False when the shape / dtype is not handled here (the im2col TT kernel runs instead) or
// YMS_WG_HALO=0.
bool wgrad_halo_plan(const yms_conv_shape* s, WHPlan* w);
// Partial slabs [a.splits * wk][slab_rows][9 * cin8] (the layout wgrad_reduce_kernel sums).
yms_status wgrad_halo_launch(const yms_conv_shape* s, const WHPlan& w, const WgradArgs& a, hipStream_t st);

}  // namespace yms
