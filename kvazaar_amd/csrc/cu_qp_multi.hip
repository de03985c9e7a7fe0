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
  pic_tiles tiles[KVZ_HIP_MAX_CHAIN_PICTURES];
  int used = 0, at = 0, lcus_x = 0, lcus_y = 0, chains_x = 0, chains_y = 0;
  // every record is checked before anything is launched: a refused call writes nothing
  if (const char *why = filter_records_why(pictures, n_pictures, cu_qp_record_why, cu_qp_output_shared, bounds, used, tiles, &at))
    return refuse_picture(__func__, at, why);
  for (int i = 0; i < n_pictures; ++i) {
    const kvz_hip_filter_picture &p = pictures[i];
    cu_qp_pic &r = b.p[i];
    r.tiles = tiles[i];
    cu_qp_fill(r.a, p);
    r.chain_rows = (u8)p.cu_qp.chain_rows; r.start_qp = (u8)p.cu_qp.start_qp;
    lcus_x = max(lcus_x, (int)r.tiles.lcus_x);
    lcus_y = max(lcus_y, (int)r.tiles.lcus_y);
    chains_x = max(chains_x, (int)r.tiles.cols);
    chains_y = max(chains_y, p.cu_qp.chain_rows ? (int)r.tiles.lcus_y : (int)r.tiles.rows);
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
