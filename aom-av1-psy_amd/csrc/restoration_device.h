// What restoration.hip shares with the restoration composites (sgr_search.hip): the unit clip of its kernels and the launch of the self-guided
// filter without the entry point's argument checks.  Not part of the ABI.
#ifndef AOMHIP_CSRC_RESTORATION_DEVICE_H_
#define AOMHIP_CSRC_RESTORATION_DEVICE_H_

#include "common.h"

namespace aomhip {

// A unit as the kernels use it: clipped to the plane and to the stated maximum size.  Identity for every unit the entry points accept -- they can
// only check the optional HOST copy of the list -- and what keeps a bad device-side rectangle from writing past the caller's flt0 / flt1 rows or
// outside the destination plane (it then filters the clipped rectangle).
__device__ __forceinline__ aomhip_rect clip_unit(aomhip_rect u, int plane_w, int plane_h, int max_w, int max_h) {
  u.h_start = min(max(u.h_start, 0), plane_w); u.v_start = min(max(u.v_start, 0), plane_h);
  u.h_end = min(min(u.h_end, plane_w), u.h_start + max_w); u.v_end = min(min(u.v_end, plane_h), u.v_start + max_h);
  return u;
}

// aomhip_selfguided_restoration_batch's launch on the context's stream (its arguments, already checked; n_units > 0).  restoration.hip
void launch_selfguided(aomhip_ctx *ctx, const aomhip_planes *dgd, int dgd_frame, const aomhip_rect *d_units, int n_units, const int32_t *d_sgr_params_idx,
                       int max_unit_width, int max_unit_height, int32_t *d_flt0, int32_t *d_flt1, int flt_stride, int64_t flt_pitch);

}  // namespace aomhip

#endif  // AOMHIP_CSRC_RESTORATION_DEVICE_H_
