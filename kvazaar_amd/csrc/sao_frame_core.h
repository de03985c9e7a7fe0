// sao_frame_core.h -- the kernel and the host side of the two whole-picture SAO reconstruction entries (sao_frame.hip: a picture,
// sao_frame_tiles.hip: a tiled picture).  Everything here has internal linkage: each translation unit gets its own copy and
// instantiates one kernel.  The algorithm is described in sao_frame.hip.
#pragma once

#include "kvz_hip_internal.h"
#include "tile_grid.h"

using namespace kvzhip;

namespace {

// sao_calc_eo_cat (sao-generic.c:34-43)
__device__ __forceinline__ int eo_cat(int a, int b, int c)
{
  const int idx = 2 + ((c > a) - (c < a)) + ((c > b) - (c < b));
  return (int)((0x43021u >> (4 * idx)) & 15u);          // {1, 2, 0, 3, 4} packed in nibbles
}

struct frame_args {
  const u8 *rec[3];
  u8 *dst[3];
  u32 rec_stride[2], dst_stride[2];       // [0] luma, [1] chroma
  int width, height, lcus_x, tiles_y, tiles_c;
  const kvz_hip_sao_info *sao[2];         // [0] luma, [1] chroma records
};
// host: the argument of one picture, for the two single entries and a record of kvz_hip_sao_frames
inline void sao_frame_fill(frame_args &a, const kvz_hip_filter_picture &p)
{
  const bool chroma = p.chroma != 0;
  a.rec[0] = p.rec_y; a.rec[1] = chroma ? p.rec_u : nullptr; a.rec[2] = chroma ? p.rec_v : nullptr;
  a.dst[0] = p.dst_y; a.dst[1] = chroma ? p.dst_u : nullptr; a.dst[2] = chroma ? p.dst_v : nullptr;
  a.rec_stride[0] = p.stride_y; a.rec_stride[1] = p.stride_c;
  a.dst_stride[0] = p.dst_stride_y; a.dst_stride[1] = p.dst_stride_c;
  a.width = p.width; a.height = p.height;
  a.lcus_x = (p.width + 63) >> 6;
  a.tiles_y = a.lcus_x * ((p.height + 15) >> 4);
  a.tiles_c = chroma ? a.lcus_x * ((p.height + 63) >> 6) : 0;
  a.sao[0] = p.sao_luma; a.sao[1] = chroma ? p.sao_chroma : nullptr;
}

// the tile of a tiled picture in pixels of the plane: what stands for the plane where an edge-offset pixel asks for its neighbours
struct px_rect { int x0, y0, x1, y1; };
__device__ __forceinline__ const px_rect &only(const px_rect &q) { return q; }

// one dword of an edge-offset tile.  s: the tile with its ring, `pitch` dwords per row; at: the dword's index in it.
// rect: nothing (the plane, pw x ph) or the pixel's tile
template <int CLS, typename... RECT>
__device__ __forceinline__ u32 edge_dword(const u32 *s, int pitch, int at, int gx, int gy, int pw, int ph, const int *off, RECT... rect)
{
  constexpr int RA = CLS == 0 ? 1 : 0;                         // window row of neighbour a; b lies opposite (sao.h:58-63)
  constexpr int DXA = CLS == 1 ? 0 : (CLS == 3 ? 1 : -1);      // its column step
  int win[3][6];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    if (CLS == 0 && r != 1) continue;
    const u32 l = s[at + (r - 1) * pitch - 1], c = s[at + (r - 1) * pitch], rt = s[at + (r - 1) * pitch + 1];
    win[r][0] = (int)(l >> 24);
#pragma unroll
    for (int k = 0; k < 4; ++k) win[r][1 + k] = (int)((c >> (8 * k)) & 255u);
    win[r][5] = (int)(rt & 255u);
  }
  // a pixel whose neighbour a or b lies outside the plane (the tile) keeps its value: the row / column trimming of sao.c:297-324
  bool oky = CLS == 0 || (gy >= 1 && gy <= ph - 2);
  if constexpr (sizeof...(RECT) != 0) oky = CLS == 0 || (gy >= only(rect...).y0 + 1 && gy <= only(rect...).y1 - 2);
  u32 out = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int px = gx + k, c = win[1][1 + k];
    bool ok = oky && (DXA == 0 || (px >= 1 && px <= pw - 2));
    if constexpr (sizeof...(RECT) != 0) ok = oky && (DXA == 0 || (px >= only(rect...).x0 + 1 && px <= only(rect...).x1 - 2));
    const int cat = eo_cat(win[RA][1 + k + DXA], win[2 - RA][1 + k - DXA], c);
    out |= (u32)(ok ? clampi(c + off[cat], 0, 255) : c) << (8 * k);
  }
  return out;
}

// TILES: nothing (kvz_hip_sao_frame), or the grid of a tiled picture as an optional trailing argument (kvz_hip_sao_frame_tiles).  A
// workgroup's tile lies inside one LCU, so the rectangle is workgroup-uniform.  Without it the instantiation is the kernel as it
// was; each of the two has a translation unit of its own (sao_frame.hip, sao_frame_tiles.hip).
// Or the table of the pictures of a multi-picture call (kvz_hip_sao_frames, sao_frame_multi.hip), the picture being the grid's
// second dimension: `a` is the record's -- the kernel's own is not read -- and the grid is the picture's part of the pool of
// boundaries that the pictures share (tile_grid.h).  A workgroup reads its record from the kernel arguments with scalar loads; one
// beyond its picture's tiles leaves at once.
__device__ __forceinline__ const kvz_hip_tile_grid &only(const kvz_hip_tile_grid &g) { return g; }
struct frame_pic { frame_args a; pic_tiles tiles; int pad; };       // 120 bytes
struct frame_batch { frame_pic p[KVZ_HIP_MAX_CHAIN_PICTURES]; tile_pool pool; };
static_assert(sizeof(frame_pic) == 120 && sizeof(frame_batch) <= 4096, "the records and the pool travel in the kernel arguments");
__device__ __forceinline__ const frame_batch &only(const frame_batch &b) { return b; }
template <typename... T> struct sao_takes_batch { static constexpr bool value = false; };
template <> struct sao_takes_batch<frame_batch> { static constexpr bool value = true; };
template <typename... TILES>
__global__ __launch_bounds__(256) void sao_frame_kernel(frame_args a, TILES... tiles)
{
  __shared__ u32 s_t[10 * 34];              // the larger of 18 x 18 (luma) and 10 x 34 (chroma) dwords
  if constexpr (sao_takes_batch<TILES...>::value) {
    a = only(tiles...).p[blockIdx.y].a;     // every field is read at a constant index: scalar loads, no copy in memory
    if ((int)blockIdx.x >= a.tiles_y + 2 * a.tiles_c) return;
  }
  const int tid = threadIdx.x;
  int b = (int)blockIdx.x, plane = 0;
  if (b >= a.tiles_y) { b -= a.tiles_y; plane = 1; if (b >= a.tiles_c) { b -= a.tiles_c; plane = 2; } }
  const int sh = plane ? 1 : 0, pw = a.width >> sh, ph = a.height >> sh;
  const int tw = plane ? 8 : 16, th = plane ? 32 : 16;         // tile: dwords x rows
  const int tr = b / a.lcus_x, lx = b - tr * a.lcus_x;
  const int tx0 = lx * 4 * tw, ty0 = tr * th;
  const int lcu = (plane ? tr : (ty0 >> 6)) * a.lcus_x + lx;
  // the tile that holds the LCU, where there are tiles: wave-uniform, scalar work
  const auto rect_of = [&](const kvz_hip_tile_grid &g) {
    int cx0, cx1, ry0, ry1;
    tile_span_of(g.col_bd, g.cols, lx, cx0, cx1);
    tile_span_of(g.row_bd, g.rows, plane ? tr : (ty0 >> 6), ry0, ry1);
    const int u = 64 >> sh;
    return px_rect{ u * cx0, u * ry0, min(u * cx1, pw), min(u * ry1, ph) };
  };
  const auto rect_of_picture = [&](const frame_batch &t) {
    const pool_grid g = { t.pool, t.p[blockIdx.y].tiles };
    int cx0, cx1, ry0, ry1;
    tile_col_span_of(g, lx, cx0, cx1);
    tile_row_span_of(g, plane ? tr : (ty0 >> 6), ry0, ry1);
    const int u = 64 >> sh;
    return px_rect{ u * cx0, u * ry0, min(u * cx1, pw), min(u * ry1, ph) };
  };
  const kvz_hip_sao_info &sao = (plane ? a.sao[1] : a.sao[0])[lcu];
  const int is_v = plane == 2, bp = sao.band_position[is_v], cls = sao.eo_class;
  // the plane's five offsets, looked up per pixel: in LDS (a register array indexed by category would live in scratch)
  __shared__ int s_off[5];
  if (tid < 5) s_off[tid] = sao.offsets[5 * is_v + tid];
  // a malformed record is SAO_TYPE_NONE
  const int mode = (sao.type == 1 && bp >= 0 && bp <= 31) ? 1 : ((sao.type == 2 && cls >= 0 && cls <= 3) ? 2 : 0);

  // selected, not indexed: a dynamically indexed kernel argument array is copied to scratch
  const u32 rs = plane ? a.rec_stride[1] : a.rec_stride[0], ds = plane ? a.dst_stride[1] : a.dst_stride[0];
  const u8 *rec = plane == 0 ? a.rec[0] : (plane == 1 ? a.rec[1] : a.rec[2]);
  u8 *dst = plane == 0 ? a.dst[0] : (plane == 1 ? a.dst[1] : a.dst[2]);
  const int c = tid & (tw - 1), r = tid / tw;
  const int gx = tx0 + 4 * c, gy = ty0 + r;
  const bool inside = gx < pw && gy < ph;
  u32 out = 0;
  if (mode == 2) {
    const int pitch = tw + 2, total = pitch * (th + 2);
    for (int i = tid; i < total; i += 256) {
      const int rr = i / pitch, yy = ty0 + rr - 1, xx = tx0 + 4 * (i - rr * pitch - 1);
      s_t[i] = (yy >= 0 && yy < ph && xx >= 0 && xx < pw) ? *(const u32 *)(rec + (size_t)yy * rs + xx) : 0u;
    }
    __syncthreads();
    if (!inside) return;
    const int at = (r + 1) * pitch + c + 1;
    if constexpr (sizeof...(TILES) != 0) {
      px_rect q;                                                // once per workgroup, by the edge workgroups only
      if constexpr (sao_takes_batch<TILES...>::value) q = rect_of_picture(tiles...);
      else q = rect_of(tiles...);
      switch (cls) {
        case 0: out = edge_dword<0>(s_t, pitch, at, gx, gy, pw, ph, s_off, q); break;
        case 1: out = edge_dword<1>(s_t, pitch, at, gx, gy, pw, ph, s_off, q); break;
        case 2: out = edge_dword<2>(s_t, pitch, at, gx, gy, pw, ph, s_off, q); break;
        default: out = edge_dword<3>(s_t, pitch, at, gx, gy, pw, ph, s_off, q); break;
      }
    } else {
      switch (cls) {
        case 0: out = edge_dword<0>(s_t, pitch, at, gx, gy, pw, ph, s_off); break;
        case 1: out = edge_dword<1>(s_t, pitch, at, gx, gy, pw, ph, s_off); break;
        case 2: out = edge_dword<2>(s_t, pitch, at, gx, gy, pw, ph, s_off); break;
        default: out = edge_dword<3>(s_t, pitch, at, gx, gy, pw, ph, s_off); break;
      }
    }
  } else {
    if (mode == 1) __syncthreads();
    if (!inside) return;
    out = *(const u32 *)(rec + (size_t)gy * rs + gx);
    if (mode == 1) {
      // kvz_calc_sao_offset_array (sao.c:164-180) per pixel
      const u32 in = out;
      out = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int val = (int)((in >> (8 * k)) & 255u), band = (val >> 3) - bp;
        const int o = (band >= 0 && band < 4) ? s_off[(band & 3) + 1] : 0;
        out |= (u32)clampi(val + o, 0, 255) << (8 * k);
      }
    }
  }
  *(u32 *)(dst + (size_t)gy * ds + gx) = out;
}

// both single entries, behind their sao_pack; tiles: nothing or the grid
template <typename... TILES>
int sao_frame_launch(const char *entry, const kvz_hip_filter_picture &p, kvz_hip_stream s, TILES... tiles)
{
  if (!sao_luma_info_ok(p)) return kvzhip::invalid_arg(entry);
  if (!sao_luma_planes_ok(p)) return refuse_entry(entry, PLANES_AND_STRIDES);
  if (!sao_chroma_ok(p)) return kvzhip::invalid_arg(entry);
  frame_args a;
  sao_frame_fill(a, p);
  hipLaunchKernelGGL(sao_frame_kernel<TILES...>, dim3((unsigned)(a.tiles_y + 2 * a.tiles_c)), dim3(256), 0, ctx_stream(s), a, tiles...);
  KVZ_CHECK_LAUNCH("sao_frame_kernel");
  return KVZ_HIP_OK;
}

}  // namespace
