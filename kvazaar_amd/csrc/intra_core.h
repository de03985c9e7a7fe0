// intra_core.h -- the per-pixel arithmetic of intra prediction and the coding-order availability rule, shared by intra.hip
// (batched entries) and intra_recon.hip (whole-picture entry).  Reference: intra-generic.c:37-189, intra.c:35-70, :164-331.
#pragma once

#include "kvz_hip_internal.h"

using namespace kvzhip;

namespace {

constexpr int RS = 68;   // bytes per staged reference array: entries 0 .. 2N (<= 64), zero padded

// intra-generic.c:46-47
__constant__ int c_ang_disp[9] = { 0, 2, 5, 9, 13, 17, 21, 26, 32 };
__constant__ int c_ang_inv[9] = { 0, 4096, 1638, 910, 630, 482, 390, 315, 256 };

struct ang_t { int vertical, disp, inv; };
__device__ __forceinline__ ang_t ang_of(int mode)
{
  ang_t a;
  a.vertical = mode >= 18;
  const int md = a.vertical ? mode - 26 : 10 - mode;
  const int amd = md < 0 ? -md : md;
  a.disp = md < 0 ? -c_ang_disp[amd] : c_ang_disp[amd];
  a.inv = c_ang_inv[amd];
  return a;
}

// intra.c:289-306: which reference kvz_intra_predict hands to the predictor
__device__ __forceinline__ bool use_filtered(int mode, int log2_width, int flags)
{
  if ((flags & KVZ_HIP_INTRA_RAW) || !(flags & KVZ_HIP_INTRA_LUMA) || mode == 1 || log2_width == 2) return false;
  if (mode == 0) return true;
  const int dv = mode > 26 ? mode - 26 : 26 - mode, dh = mode > 10 ? mode - 10 : 10 - mode;
  const int thres = log2_width == 3 ? 7 : (log2_width == 4 ? 1 : 0);
  return (dv < dh ? dv : dh) > thres;
}
// intra.c:314-329: DC edge filter / boundary post-process apply to luma blocks narrower than 32
__device__ __forceinline__ bool luma_edge_filters(int log2_width, int flags)
{
  return !(flags & KVZ_HIP_INTRA_RAW) && (flags & KVZ_HIP_INTRA_LUMA) && log2_width < 5;
}

// Extended main reference of one PU for an angular mode: e[k], k = idx + N, idx = -N .. 2N+1.
// idx >= -1: main[idx + 1]; below: the side reference projected with the inverse angle
// (intra-generic.c:78-93).  Entries the mode never reads are still filled (index clamped).
template <int N>
__device__ __forceinline__ u8 ext_entry(const u8 (*ref)[RS], bool fil, const ang_t &a, int idx)
{
  const u8 *mainr = ref[2 * fil + (a.vertical ? 1 : 0)];
  const u8 *side = ref[2 * fil + (a.vertical ? 0 : 1)];
  if (idx >= -1) return mainr[idx + 1];
  int si = (128 + (-idx - 1) * a.inv) >> 8;
  if (si > 2 * N) si = 2 * N;
  return side[si];
}

__device__ __forceinline__ int dc_value(const u8 (*ref)[RS], int n, int log2_width)
{
  int sum = n;
  for (int i = 1; i <= n; ++i) sum += ref[0][i] + ref[1][i];
  return sum >> (log2_width + 1);
}

// one pixel of the DC prediction (intra.c:217-278)
__device__ __forceinline__ int dc_px(const u8 (*ref)[RS], int dc, bool edge, int x, int y)
{
  if (!edge || (x > 0 && y > 0)) return dc;
  if (x == 0 && y == 0) return (ref[0][1] + 2 * dc + ref[1][1] + 2) >> 2;
  if (y == 0) return (ref[1][x + 1] + 3 * dc + 2) >> 2;
  return (ref[0][y + 1] + 3 * dc + 2) >> 2;
}

// one pixel of the planar prediction (intra-generic.c:155-189, closed form :167-175)
__device__ __forceinline__ int planar_px(const u8 *left, const u8 *top, int n, int log2_width, int x, int y)
{
  const int hor = (n - 1 - x) * left[y + 1] + (x + 1) * top[n + 1];
  const int ver = (n - 1 - y) * top[x + 1] + (y + 1) * left[n + 1];
  return (hor + ver + n) >> (log2_width + 1);
}

// one pixel of an angular prediction in the vertical orientation: row r, column c; e = &ext[N]
__device__ __forceinline__ int ang_px(const u8 *e, int disp, int r, int c)
{
  const int pos = (r + 1) * disp, di = pos >> 5, f = pos & 31;
  return ((32 - f) * e[c + di] + f * e[c + di + 1] + 16) >> 5;
}

// intra_post_process_angular (intra.c:195-208) on column 0 of row r (vertical orientation)
__device__ __forceinline__ int post_px(int v, const u8 *side, int r)
{
  return clampi(v + (((int)side[r + 1] - (int)side[0]) >> 1), 0, 255);
}

// num_ref_pixels_left / num_ref_pixels_top (intra.c:35-70) in closed form.  (ux, uy) = the PU's 4x4 unit inside
// its LCU; s = the largest power of two dividing the coordinate (16 on the LCU border).  Everything left of
// the unit down to the end of its s-aligned group was coded before it, and so was everything above it up to
// the end of the enclosing 2s-aligned group, never more than 64 pixels.
__device__ __forceinline__ int intra_coded_left(int ux, int uy)
{
  const int s = ux ? (ux & -ux) : 16;
  return 4 * (s - (uy & (s - 1)));
}
__device__ __forceinline__ int intra_coded_above(int ux, int uy)
{
  const int s2 = uy ? 2 * (uy & -uy) : 32;
  const int n = 4 * (s2 - (ux & (s2 - 1)));
  return n < 64 ? n : 64;
}

}  // namespace
