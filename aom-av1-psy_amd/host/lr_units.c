/*
 * The restoration-unit limits of one plane (plain C99, host only: no GPU call in this file).
 *
 * aomhip_loop_restoration_filter_units takes the list of units av1_loop_restoration_filter_frame visits.  This is the
 * walk that produces it: foreach_rest_unit_in_tile / av1_foreach_rest_unit_in_row (av1/common/restoration.c:1206-1294)
 * over the single whole-frame tile av1_foreach_rest_unit_in_plane uses (:1296-1310), which hand the visitor, in
 * unit_idx order (row major),
 *   * columns x0 .. x0 + w, w = unit_size, or all that is left when less than 1.5 unit sizes are left (:1213-1221);
 *   * rows cut the same way (:1266-1279) and then moved up by RESTORATION_UNIT_OFFSET >> ss_y = 8 >> ss_y rows so
 *     that they end on a processing-stripe boundary -- except the top of the first row of units and the bottom of
 *     the last one (:1281-1284).
 * The number of units per direction is av1_lr_count_units_in_tile (:62-64).
 */
#include "aomhip.h"

static int count_units(int unit_size, int tile_size) { /* av1_lr_count_units_in_tile */
  const int n = (tile_size + (unit_size >> 1)) / unit_size;
  return n > 1 ? n : 1;
}

int aomhip_lr_units_in_plane(int plane_w, int plane_h, int unit_size, int ss_y, aomhip_rect *units, int cap) {
  if (plane_w < 1 || plane_h < 1 || unit_size < 1 || ss_y < 0 || ss_y > 1 || (cap > 0 && !units)) return -1;
  const int n = count_units(unit_size, plane_w) * count_units(unit_size, plane_h);
  if (cap < n) return -1;
  const int ext_size = unit_size * 3 / 2, voffset = 8 >> ss_y;
  int k = 0;
  for (int y0 = 0; y0 < plane_h;) {
    const int remaining_h = plane_h - y0;
    const int h = remaining_h < ext_size ? remaining_h : unit_size;
    int v_start = y0 - voffset, v_end = y0 + h;
    if (v_start < 0) v_start = 0;
    if (v_end < plane_h) v_end -= voffset;
    for (int x0 = 0; x0 < plane_w;) {
      const int remaining_w = plane_w - x0;
      const int w = remaining_w < ext_size ? remaining_w : unit_size;
      if (k >= cap) return -1;
      units[k].h_start = x0;
      units[k].h_end = x0 + w;
      units[k].v_start = v_start;
      units[k].v_end = v_end;
      ++k;
      x0 += w;
    }
    y0 += h;
  }
  return k;
}
