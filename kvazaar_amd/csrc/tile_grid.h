// tile_grid.h -- kvz_hip_tile_grid on the device, for the four *_tiles entries of the picture chain (intra_recon_tiles.hip,
// cu_qp_tiles.hip, deblock_tiles.hip, sao_frame_tiles.hip); its host side (tile_grid_make, tile_grid_waves) is in chain_host.h.  At the
// end: the grids of the pictures of a multi-picture call, which share one pool of boundaries (cu_qp_multi.hip, deblock_multi.hip,
// sao_frame_multi.hip; filled on the host by tile_pool_add and tile_pool_pack, chain_host.h, inside the record checks).
//
// The grid travels to every kernel by value (392 bytes of kernel arguments).  The lookups below index it with constants only --
// the loops are fully unrolled and select -- because a dynamically indexed kernel argument array is copied to scratch; with a
// wave-uniform LCU position they are scalar loads, compares and selects.
#pragma once

#include "kvz_hip_internal.h"
#include "chain_host.h"

namespace {

// The lookups walk the boundaries in two parts: the first TILE_NEAR always, the rest only where the grid has more (a wave-uniform
// branch on a kernel argument), so that the grids that occur -- a handful of tiles per direction -- cost a handful of compares.
constexpr int TILE_NEAR = 8;

template <int FROM, int TO>
__device__ __forceinline__ void tile_span_part(const int32_t (&bd)[KVZ_HIP_MAX_TILES_PER_DIM], int n, int l, int &lo, int &hi)
{
#pragma unroll
  for (int i = FROM; i <= TO; ++i) {
    const int b = bd[i];
    if (i <= n) {
      if (b <= l) lo = b;
      else hi = min(hi, b);
    }
  }
}

// the boundaries [lo, hi) of the tile column (row) that holds LCU column (row) l, in LCUs
__device__ __forceinline__ void tile_span_of(const int32_t (&bd)[KVZ_HIP_MAX_TILES_PER_DIM], int n, int l, int &lo, int &hi)
{
  lo = 0;
  hi = 0x7fffffff;
  tile_span_part<1, TILE_NEAR>(bd, n, l, lo, hi);
  if (n > TILE_NEAR) tile_span_part<TILE_NEAR + 1, TILE_MAX>(bd, n, l, lo, hi);
}

template <int FROM, int TO>
__device__ __forceinline__ void tile_at_part(const int32_t (&bd)[KVZ_HIP_MAX_TILES_PER_DIM], int t, int &lo, int &hi)
{
#pragma unroll
  for (int i = FROM; i <= TO; ++i)
    if (i == t) { lo = bd[i]; hi = bd[i + 1]; }
}

// the boundaries of tile column (row) t itself
__device__ __forceinline__ void tile_span_at(const int32_t (&bd)[KVZ_HIP_MAX_TILES_PER_DIM], int t, int &lo, int &hi)
{
  lo = hi = 0;
  if (t < TILE_NEAR) tile_at_part<0, TILE_NEAR - 1>(bd, t, lo, hi);
  else tile_at_part<TILE_NEAR, TILE_MAX - 1>(bd, t, lo, hi);
}

template <int FROM, int TO>
__device__ __forceinline__ bool tile_starts_part(const int32_t (&bd)[KVZ_HIP_MAX_TILES_PER_DIM], int n, int l)
{
  bool hit = false;
#pragma unroll
  for (int i = FROM; i <= TO; ++i) hit = hit || (i <= n && bd[i] == l);
  return hit;
}

// LCU column (row) l is where a tile column (row) other than the first begins, or where the last one ends
__device__ __forceinline__ bool tile_starts_at(const int32_t (&bd)[KVZ_HIP_MAX_TILES_PER_DIM], int n, int l)
{
  bool hit = tile_starts_part<1, TILE_NEAR>(bd, n, l);
  if (n > TILE_NEAR) hit = hit || tile_starts_part<TILE_NEAR + 1, TILE_MAX>(bd, n, l);
  return hit;
}

// ---- the grids of the pictures of a multi-picture call (cu_qp_multi.hip, deblock_multi.hip, sao_frame_multi.hip) ----
// The pool of boundaries and a picture's place in it (pic_tiles) are described in chain_host.h.
struct tile_pool {
  u32 bd[KVZ_HIP_CHAIN_TILE_BOUNDS / 2];
  __device__ __forceinline__ int bound(int i) const { return (int)((bd[i >> 1] >> (16 * (i & 1))) & 0xffffu); }
};
static_assert(sizeof(tile_pool) == 2 * KVZ_HIP_CHAIN_TILE_BOUNDS, "kernel arguments");
// what a kernel hands to the lookups: both live in the kernel arguments, so every read is a scalar load
struct pool_grid { const tile_pool &pool; const pic_tiles &t; };

// The lookups that the shared cores use, for a kvz_hip_tile_grid (the single-picture kernels: the functions above) and for a picture's
// part of the pool (a loop over the boundaries between the first and the last; wave-uniform where the LCU position is).
__device__ __forceinline__ bool tile_col_starts(const kvz_hip_tile_grid &g, int l) { return tile_starts_at(g.col_bd, g.cols, l); }
__device__ __forceinline__ bool tile_row_starts(const kvz_hip_tile_grid &g, int l) { return tile_starts_at(g.row_bd, g.rows, l); }
__device__ __forceinline__ void tile_col_span_of(const kvz_hip_tile_grid &g, int l, int &lo, int &hi) { tile_span_of(g.col_bd, g.cols, l, lo, hi); }
__device__ __forceinline__ void tile_row_span_of(const kvz_hip_tile_grid &g, int l, int &lo, int &hi) { tile_span_of(g.row_bd, g.rows, l, lo, hi); }
__device__ __forceinline__ void tile_col_span_at(const kvz_hip_tile_grid &g, int t, int &lo, int &hi) { tile_span_at(g.col_bd, t, lo, hi); }
__device__ __forceinline__ void tile_row_span_at(const kvz_hip_tile_grid &g, int t, int &lo, int &hi) { tile_span_at(g.row_bd, t, lo, hi); }

__device__ __forceinline__ bool pool_starts(const tile_pool &pool, int at, int n, int last, int l)
{
  bool hit = l == last;
  for (int j = 1; j < n; ++j) hit = hit || pool.bound(at + j) == l;
  return hit;
}
__device__ __forceinline__ void pool_span_of(const tile_pool &pool, int at, int n, int last, int l, int &lo, int &hi)
{
  lo = 0;
  hi = last;
  for (int j = 1; j < n; ++j) {
    const int b = pool.bound(at + j);
    if (b <= l) lo = b;
    else hi = min(hi, b);
  }
}
__device__ __forceinline__ void pool_span_at(const tile_pool &pool, int at, int n, int last, int t, int &lo, int &hi)
{
  lo = t > 0 ? pool.bound(at + t) : 0;
  hi = t + 1 < n ? pool.bound(at + t + 1) : last;
}
__device__ __forceinline__ bool tile_col_starts(const pool_grid &g, int l) { return pool_starts(g.pool, g.t.col_at, g.t.cols, g.t.lcus_x, l); }
__device__ __forceinline__ bool tile_row_starts(const pool_grid &g, int l) { return pool_starts(g.pool, g.t.row_at, g.t.rows, g.t.lcus_y, l); }
__device__ __forceinline__ void tile_col_span_of(const pool_grid &g, int l, int &lo, int &hi) { pool_span_of(g.pool, g.t.col_at, g.t.cols, g.t.lcus_x, l, lo, hi); }
__device__ __forceinline__ void tile_row_span_of(const pool_grid &g, int l, int &lo, int &hi) { pool_span_of(g.pool, g.t.row_at, g.t.rows, g.t.lcus_y, l, lo, hi); }
__device__ __forceinline__ void tile_col_span_at(const pool_grid &g, int t, int &lo, int &hi) { pool_span_at(g.pool, g.t.col_at, g.t.cols, g.t.lcus_x, t, lo, hi); }
__device__ __forceinline__ void tile_row_span_at(const pool_grid &g, int t, int &lo, int &hi) { pool_span_at(g.pool, g.t.row_at, g.t.rows, g.t.lcus_y, t, lo, hi); }

}  // namespace
