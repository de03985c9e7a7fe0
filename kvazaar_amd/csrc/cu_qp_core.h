// cu_qp_core.h -- the kernels of the QP map of a picture (cu_qp.hip: chains are raster runs of the picture, cu_qp_tiles.hip: chains
// are tiles or the LCU rows of tiles).  Everything here has internal linkage: each translation unit gets its own copy.  The algorithm
// is described in cu_qp.hip.
#pragma once

#include "kvz_hip_internal.h"
#include "quant_core.h"
#include "tile_grid.h"

using namespace kvzhip;

namespace {

static_assert(sizeof(kvz_hip_cu_qp_params) == 8 && sizeof(kvz_hip_cu_info) == 20, "layouts documented in kvz_hip.h");

struct cu_qp_args {
  u32 *cus;                      // records as five dwords; depth is byte 1, qp byte 6
  const u8 *cbf;                 // one byte per SCU
  const int8_t *lcu_qp;
  int8_t *lcu_last_qp;
  int cus_stride, lcus_x;
  int width, height;
};
// host: the argument of one picture, for the three entries
inline void cu_qp_fill(cu_qp_args &a, const kvz_hip_filter_picture &p)
{
  a.cus = (u32 *)p.cus; a.cbf = p.cbf; a.lcu_qp = p.lcu_qp; a.lcu_last_qp = p.lcu_last_qp;
  a.cus_stride = p.width >> 2; a.lcus_x = (p.width + 63) >> 6;
  a.width = p.width; a.height = p.height;
}

__device__ __forceinline__ int wave_min(int v)
{
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v = min(v, __shfl_xor(v, m, 64));
  return v;
}

// Thread tid of 256 is SCU (tid & 15, tid >> 4) of the LCU at (X0, Y0).  -> the z-order index (of the top-left SCU) of the CU that
// holds this SCU, walking down from the LCU as set_cu_qps does: a node splits while the record at its top-left has a depth beyond
// the node's (a depth above 3 counts as 3).  The top-left of a node that holds an SCU of the picture lies inside the picture.
// first: the smallest such index among the SCUs of the picture with a non-zero flag, 256 if there is none.  All 256 threads call.
__device__ __forceinline__ int cu_of_scu(const cu_qp_args &a, int X0, int Y0, bool &inside, int &first, int *s_min)
{
  const int tid = threadIdx.x, ux = tid & 15, uy = tid >> 4;
  const int sx0 = X0 >> 2, sy0 = Y0 >> 2;
  inside = X0 + 4 * ux < a.width && Y0 + 4 * uy < a.height;
  int nx = 0, ny = 0, key = 256;
  if (inside) {
    int size = 16;
    for (int d = 0; d < 3; ++d) {
      const u32 head = a.cus[((size_t)(sy0 + ny) * a.cus_stride + sx0 + nx) * 5];
      if (min((int)((head >> 8) & 255u), 3) <= d) break;
      size >>= 1;
      if (ux >= nx + size) nx += size;
      if (uy >= ny + size) ny += size;
    }
    key = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) key |= (((nx >> b) & 1) << (2 * b)) | (((ny >> b) & 1) << (2 * b + 1));
  }
  const bool coded = inside && a.cbf[(size_t)(sy0 + uy) * a.cus_stride + sx0 + ux] != 0;
  const int m = wave_min(coded ? key : 256);
  if ((tid & 63) == 0) s_min[tid >> 6] = m;
  __syncthreads();
  first = min(min(s_min[0], s_min[1]), min(s_min[2], s_min[3]));
  return key;
}

// launch 1 for the LCU (lcu_x, lcu_y) of the picture a; s_min: four ints of LDS
__device__ __forceinline__ void cu_qp_first(const cu_qp_args &a, int lcu_x, int lcu_y, int *s_min)
{
  bool inside;
  int first;
  cu_of_scu(a, 64 * lcu_x, 64 * lcu_y, inside, first, s_min);
  if (threadIdx.x == 0) {
    const size_t lcu = (size_t)lcu_y * a.lcus_x + lcu_x;
    a.lcu_last_qp[lcu] = (int8_t)(first < 256 ? clip_lcu_qp(a.lcu_qp[lcu]) : -1);
  }
}

__global__ __launch_bounds__(256) void cu_qp_first_kernel(cu_qp_args a)
{
  __shared__ int s_min[4];
  cu_qp_first(a, blockIdx.x, blockIdx.y, s_min);
}

// v[i] on entry: the QP that LCU i leaves as last_qp, or -1 if it leaves last_qp as it found it.  On return: last_qp on entry to
// LCU i.  "The last value that is not negative" is associative, so it scans.
// TILES: nothing -- a chain is a raster run of chain_lcus LCUs of the picture (kvz_hip_cu_qp_frame) -- or one tile_chains as an
// optional trailing argument (kvz_hip_cu_qp_frame_tiles, cu_qp_tiles.hip): a chain is a tile, grid (cols, rows), or an LCU row of a
// tile, grid (cols, lcus_y), and its i-th LCU stands at its place in picture raster order; n_lcu and chain_lcus are not read.
// Without it the instantiation is the kernel as it was.
struct tile_chains { kvz_hip_tile_grid grid; int lcus_x, chain_rows; };
__device__ __forceinline__ const tile_chains &only(const tile_chains &c) { return c; }
// Or the table of the pictures of a multi-picture call (kvz_hip_cu_qp_frames, cu_qp_multi.hip), the picture being the grid's third
// dimension: a picture's record is the argument of the kernels above with its chains, 64 bytes, and its grid is its part of the pool
// of boundaries that the pictures share (tile_grid.h); v and start_qp are the record's and the kernel's own are not read.  A
// workgroup reads its record from the kernel arguments with scalar loads; one beyond its picture's chains leaves at once.
struct cu_qp_pic { cu_qp_args a; pic_tiles tiles; u8 chain_rows, start_qp, pad[2]; };
struct cu_qp_batch { cu_qp_pic p[KVZ_HIP_MAX_CHAIN_PICTURES]; tile_pool pool; };
static_assert(sizeof(cu_qp_pic) == 64 && sizeof(cu_qp_batch) <= 4096, "the records and the pool travel in the kernel arguments");
__device__ __forceinline__ const cu_qp_batch &only(const cu_qp_batch &b) { return b; }
template <typename... T> struct cu_qp_takes_batch { static constexpr bool value = false; };
template <> struct cu_qp_takes_batch<cu_qp_batch> { static constexpr bool value = true; };
template <typename... TILES>
__global__ __launch_bounds__(256) void cu_qp_chain_kernel(int8_t *v, int n_lcu, int chain_lcus, int start_qp, TILES... tiles)
{
  constexpr bool TILED = sizeof...(TILES) != 0;
  __shared__ int s_tot[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int begin = blockIdx.x * chain_lcus, end = min(n_lcu, begin + chain_lcus);
  int x0 = 0, x1 = 0, y0 = 0, y1 = 0, lcus_x = 0;
  if constexpr (cu_qp_takes_batch<TILES...>::value) {
    const cu_qp_batch &b = only(tiles...);
    const cu_qp_pic &p = b.p[blockIdx.z];
    if ((int)blockIdx.x >= p.tiles.cols || (int)blockIdx.y >= (p.chain_rows ? p.tiles.lcus_y : p.tiles.rows)) return;
    const pool_grid g = { b.pool, p.tiles };
    tile_col_span_at(g, (int)blockIdx.x, x0, x1);
    if (p.chain_rows) { y0 = (int)blockIdx.y; y1 = y0 + 1; }
    else tile_row_span_at(g, (int)blockIdx.y, y0, y1);
    v = p.a.lcu_last_qp;
    start_qp = p.start_qp;
    lcus_x = p.a.lcus_x;
    begin = 0;
    end = (x1 - x0) * (y1 - y0);
  } else if constexpr (TILED) {
    const tile_chains &c = only(tiles...);
    tile_span_at(c.grid.col_bd, (int)blockIdx.x, x0, x1);
    if (c.chain_rows) { y0 = (int)blockIdx.y; y1 = y0 + 1; }
    else tile_span_at(c.grid.row_bd, (int)blockIdx.y, y0, y1);
    lcus_x = c.lcus_x;
    begin = 0;
    end = (x1 - x0) * (y1 - y0);
  }
  int carry = start_qp;
  for (int base = begin; base < end; base += 256) {
    const int i = base + tid;
    int at = i;
    if constexpr (TILED) {
      const int r = i / (x1 - x0);
      at = (y0 + r) * lcus_x + x0 + (i - r * (x1 - x0));
    }
    int incl = i < end ? (int)v[at] : -1;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int t = __shfl_up(incl, off, 64);
      if (lane >= off && incl < 0) incl = t;
    }
    if (lane == 63) s_tot[wave] = incl;
    __syncthreads();
    int before = -1, total = -1;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int t = s_tot[w];
      if (t >= 0) {
        total = t;
        if (w < wave) before = t;
      }
    }
    int excl = __shfl_up(incl, 1, 64);
    if (lane == 0 || excl < 0) excl = before;
    if (i < end) v[at] = (int8_t)(excl >= 0 ? excl : carry);
    if (total >= 0) carry = total;
    __syncthreads();                                   // s_tot is written again
  }
}

// launch 3 for the LCU (lcu_x, lcu_y) of the picture a
__device__ __forceinline__ void cu_qp_write(const cu_qp_args &a, int lcu_x, int lcu_y, int *s_min)
{
  const int tid = threadIdx.x;
  bool inside;
  int first;
  const int key = cu_of_scu(a, 64 * lcu_x, 64 * lcu_y, inside, first, s_min);
  if (!inside) return;
  const size_t lcu = (size_t)lcu_y * a.lcus_x + lcu_x;
  const int qp = key < first ? (int)a.lcu_last_qp[lcu] : clip_lcu_qp(a.lcu_qp[lcu]);
  const size_t scu = (size_t)(16 * lcu_y + (tid >> 4)) * a.cus_stride + 16 * lcu_x + (tid & 15);
  ((u8 *)a.cus)[scu * 20 + 6] = (u8)qp;
}

__global__ __launch_bounds__(256) void cu_qp_write_kernel(cu_qp_args a)
{
  __shared__ int s_min[4];
  cu_qp_write(a, blockIdx.x, blockIdx.y, s_min);
}

// kvz_hip_cu_qp_frame and kvz_hip_cu_qp_frame_tiles: launches 1 and 3 around the entry's scan.  chains: the grid of the scan; n_lcu,
// chain_lcus and tiles (nothing or the tile_chains): what its kernel takes beside the record's lcu_last_qp and start_qp
template <typename... TILES>
int cu_qp_launch(const kvz_hip_filter_picture &p, kvz_hip_stream s, dim3 chains, int n_lcu, int chain_lcus, TILES... tiles)
{
  cu_qp_args a;
  cu_qp_fill(a, p);
  const dim3 lcus((unsigned)a.lcus_x, (unsigned)((p.height + 63) >> 6));
  hipStream_t st = ctx_stream(s);
  hipLaunchKernelGGL(cu_qp_first_kernel, lcus, dim3(256), 0, st, a);
  KVZ_CHECK_LAUNCH("cu_qp_first_kernel");
  hipLaunchKernelGGL(cu_qp_chain_kernel<TILES...>, chains, dim3(256), 0, st, p.lcu_last_qp, n_lcu, chain_lcus, p.cu_qp.start_qp, tiles...);
  KVZ_CHECK_LAUNCH(sizeof...(TILES) ? "cu_qp_chain_kernel<tiles>" : "cu_qp_chain_kernel");
  hipLaunchKernelGGL(cu_qp_write_kernel, lcus, dim3(256), 0, st, a);
  KVZ_CHECK_LAUNCH("cu_qp_write_kernel");
  return KVZ_HIP_OK;
}

}  // namespace
