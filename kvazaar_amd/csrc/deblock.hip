// deblock.hip -- the deblocking filter over one reconstructed frame.
//
// Reference: src/filter.c:83-779 (kvz_filter_deblock_lcu and everything below it).  SURVEY.md section 8(f) row 4.
//
// The reference walks the LCUs in coding order: vertical edges of the LCU, the deferred rightmost 4 pixels of the
// horizontal edges of the LCU to the left, then its own horizontal edges (filter.c:770-779) -- an order built so that
// every horizontal edge sees vertically filtered pixels, i.e. the HEVC process "all vertical edges of the picture, then
// all horizontal edges".  That is what runs here: TWO launches over the frame, one per direction, every 4-pixel edge
// segment its own thread.  Edges are 8 apart and the filter reaches 3 pixels (4 read), so the segments of one pass
// touch disjoint pixels and need no ordering among themselves.
//
// A thread = one luma segment (unit = 8x8 block of the edge grid, 2 segments per unit); the two threads of a unit also
// take the unit's chroma segment, one plane each.  Everything the reference derives from cu_array on the way --
// TU / PU boundary tests, boundary strength incl. the B-slice vector rules, per-CU QP prediction, tc / beta -- is
// derived on the device from a flat copy of the cu_info_t fields (kvz_hip_cu_info, one per 4x4 SCU).
// Lanes walk along x: a wave's loads of one picture row are contiguous (8 B per lane, vertical edges; 4 B, horizontal).
#include "deblock_core.h"

extern "C" int kvz_hip_deblock_frame(kvz_hip_pixel *rec_y, uint32_t stride_y, kvz_hip_pixel *rec_u, kvz_hip_pixel *rec_v, uint32_t stride_c,
                                     int width, int height, const kvz_hip_cu_info *cus, const kvz_hip_deblock_params *params,
                                     kvz_hip_stream s)
{
  KVZ_CHECK_CTX();
  kvz_hip_filter_picture p;
  if (const int rc = deblock_refusal(__func__, deblock_pack(&p, rec_y, stride_y, rec_u, rec_v, stride_c, width, height, cus, nullptr, params) ? &p : nullptr)) return rc;
  return deblock_launch(p, s);
}
