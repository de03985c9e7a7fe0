// cu_qp_multi.hip -- kvz_hip_cu_qp_frames: kvz_hip_cu_qp_frame_tiles (cu_qp_tiles.hip) for up to sixteen pictures that do not depend
// on each other, in one call: that entry's three launches, each covering all pictures, the picture being the grid's third dimension.
// The stage is bound by its launches, so what a host with P pictures gains is the launches it no longer repeats.
//
// Launches 1 and 3 call the device functions of cu_qp_core.h that the single-picture kernels call, on the record of the workgroup's
// picture; launch 2 is the instantiation of cu_qp_chain_kernel whose trailing argument is the table of records (cu_qp_batch).  They
// have this translation unit to themselves, so that the single-picture kernels are compiled as they always were.  A record is the
// single entry's kernel argument with the picture's chains; a workgroup reads its own and its tile's boundaries from the kernel
// arguments with scalar loads.  A launch is sized for the largest picture; the surplus workgroups of a smaller one leave at once.
#include "cu_qp_core.h"

static_assert(sizeof(kvz_hip_filter_picture) == 264 && sizeof(kvz_hip_cu_qp_tiles_params) == 8, "layouts documented in kvz_hip.h");

namespace {

// launches 1 (LAST = false) and 3: grid (LCU columns, LCU rows of the largest picture, pictures)
template <bool LAST>
__global__ __launch_bounds__(256) void cu_qp_lcu_multi_kernel(cu_qp_batch b)
{
  __shared__ int s_min[4];
  const cu_qp_pic &p = b.p[blockIdx.z];
  if ((int)blockIdx.x >= p.tiles.lcus_x || (int)blockIdx.y >= p.tiles.lcus_y) return;
  if constexpr (LAST) cu_qp_write(p.a, blockIdx.x, blockIdx.y, s_min);
  else cu_qp_first(p.a, blockIdx.x, blockIdx.y, s_min);
}


}  // namespace

extern "C" {

int kvz_hip_cu_qp_frames(const kvz_hip_filter_picture *pictures, int n_pictures, kvz_hip_stream s)
{
  KVZ_CHAIN_PROLOGUE(pictures, n_pictures);
  cu_qp_batch b;
  __builtin_memset(&b, 0, sizeof b);
  uint16_t bounds[KVZ_HIP_CHAIN_TILE_BOUNDS];
  int used = 0, lcus_x = 0, lcus_y = 0, chains_x = 0, chains_y = 0;
  // every record is checked before anything is launched: a refused call writes nothing
  for (int i = 0; i < n_pictures; ++i) {
    const kvz_hip_filter_picture &p = pictures[i];
    if (!p.cus || !p.cbf || !p.lcu_qp || !p.lcu_last_qp || ((uintptr_t)p.cus & 3)) return refuse_picture(__func__, i, "a null pointer or a misaligned cus");
    if (p.width < 8 || p.height < 8 || ((p.width | p.height) & 7) || p.width > 16384 || p.height > 16384)
      return refuse_picture(__func__, i, "width / height must be multiples of 8 in 8..16384");
    if (p.cu_qp.start_qp < 0 || p.cu_qp.start_qp > 51 || (p.cu_qp.chain_rows != 0 && p.cu_qp.chain_rows != 1))
      return refuse_picture(__func__, i, "start_qp outside 0..51 or chain_rows other than 0 and 1");
    if (p.deblock.chroma != p.chroma) return refuse_picture(__func__, i, "deblock.chroma differs from chroma");
    kvz_hip_tile_grid g;
    if (!tile_grid_make(p.grid, p.width, p.height, &g)) return refuse_picture(__func__, i, "invalid tile grid");
    cu_qp_pic &r = b.p[i];
    if (!tile_pool_add(p.grid, g, bounds, used, &r.tiles))
      return refuse_picture(__func__, i, "the tile grids of the call exceed KVZ_HIP_CHAIN_TILE_BOUNDS boundaries at this record");
    for (int j = 0; j < i; ++j)
      if (p.cus == pictures[j].cus || p.lcu_last_qp == pictures[j].lcu_last_qp) return refuse_picture(__func__, i, "an output shared with another picture");
    r.a.cus = (u32 *)p.cus; r.a.cbf = p.cbf; r.a.lcu_qp = p.lcu_qp; r.a.lcu_last_qp = p.lcu_last_qp;
    r.a.cus_stride = p.width >> 2; r.a.lcus_x = r.tiles.lcus_x;
    r.a.width = p.width; r.a.height = p.height;
    r.chain_rows = (u8)p.cu_qp.chain_rows; r.start_qp = (u8)p.cu_qp.start_qp;
    lcus_x = max(lcus_x, (int)r.tiles.lcus_x);
    lcus_y = max(lcus_y, (int)r.tiles.lcus_y);
    chains_x = max(chains_x, g.cols);
    chains_y = max(chains_y, p.cu_qp.chain_rows ? (int)r.tiles.lcus_y : g.rows);
  }
  tile_pool_pack(bounds, used, b.pool.bd);
  hipStream_t st = ctx_stream(s);
  // the launch sequence depends on the sizes, the grids and chain_rows alone
  const dim3 lcus((unsigned)lcus_x, (unsigned)lcus_y, (unsigned)n_pictures);
  hipLaunchKernelGGL(cu_qp_lcu_multi_kernel<false>, lcus, dim3(256), 0, st, b);
  KVZ_CHECK_LAUNCH("cu_qp_lcu_multi_kernel<first>");
  // launch 2: grid (tile columns, tile rows or LCU rows of the picture with the most, pictures)
  hipLaunchKernelGGL(cu_qp_chain_kernel<cu_qp_batch>, dim3((unsigned)chains_x, (unsigned)chains_y, (unsigned)n_pictures), dim3(256), 0, st,
                     (int8_t *)nullptr, 0, 0, 0, b);
  KVZ_CHECK_LAUNCH("cu_qp_chain_kernel<pictures>");
  hipLaunchKernelGGL(cu_qp_lcu_multi_kernel<true>, lcus, dim3(256), 0, st, b);
  KVZ_CHECK_LAUNCH("cu_qp_lcu_multi_kernel<write>");
  return KVZ_HIP_OK;
}

}  // extern "C"
