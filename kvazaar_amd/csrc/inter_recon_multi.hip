// inter_recon_multi.hip -- kvz_hip_inter_recon_frames: kvz_hip_inter_recon_frame (inter_recon.hip) for up to sixteen pictures that
// do not depend on each other, in one call and one launch.  Sixteen tables of sixteen reference pictures would not fit a kernel's
// arguments, and the pictures in flight share most of their references anyway: the call takes ONE pool of up to 48 reference
// pictures, and every record names its pictures by their index in the pool.
//
// The host resolves each record's two reference lists against its table once: pool_of[list][i] = refs[ref_LX[list][i]], or 255
// where ref_LX points outside the table, so that a lane does one byte lookup where the single kernel reads prm.ref_LX, and what it
// gets indexes the pool.  255 is not below n_pool, which is how pu_ok skips such a PU, as the single kernel does.  The grid is the
// sum over the pictures of ceil(tiles / 4) workgroups: a workgroup never spans two pictures, it finds its picture from the records'
// first workgroups with a scalar loop, reads the record and its references with scalar loads, and each of its waves then runs
// predict_tile of inter_recon_core.h, the single kernel's body.  No barrier, no atomics.  The kernels of inter_recon.hip are not
// touched: this kernel has the translation unit to itself.
#include "inter_recon_core.h"
#include "chain_host.h"

static_assert(sizeof(kvz_hip_recon_picture) == 104 && KVZ_HIP_RECON_POOL_PICTURES == 48, "layout documented in kvz_hip.h");

namespace {

struct multi_pic {
  u8 *y, *u, *v;                 // destination planes (u, v null for 4:0:0)
  const u32 *cus;
  u32 stride_y, stride_c;
  int width, height;
  int chroma;
  int first_wg;                  // the picture's first workgroup in the grid
  uint8_t pool_of[2][16];        // per list: pool index of reference i of the list, 255 = none
};
struct multi_args {
  multi_pic p[KVZ_HIP_MAX_CHAIN_PICTURES];
  kvz_hip_ref_picture pool[KVZ_HIP_RECON_POOL_PICTURES];   // pictures that no record names are zero
  int n_pictures, n_pool;
};
static_assert(sizeof(multi_pic) == 88 && sizeof(multi_args) == 3336, "the byte counts kvz_hip.h states");
static_assert(sizeof(multi_args) < 4096, "records and pool travel in the kernel arguments");

// the view of one picture that inter_recon_core.h works on: the table is the pool
struct recon_view {
  const kvz_hip_ref_picture *refs;
  int n_refs;
  u8 *y, *u, *v;
  u32 stride_y, stride_c;
  int width, height;
  int chroma;
};

__global__ __launch_bounds__(256) void inter_recon_frames_kernel(multi_args k)
{
  __shared__ __attribute__((aligned(16))) u8 lds[4][LDS_WAVE];
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  int pic = 0;
  for (int i = 1; i < k.n_pictures; ++i)
    if ((int)blockIdx.x >= k.p[i].first_wg) pic = i;
  const multi_pic &p = k.p[__builtin_amdgcn_readfirstlane(pic)];
  const int tiles_x = (p.width + 15) >> 4, n_tiles = tiles_x * ((p.height + 15) >> 4);
  const int tile = ((int)blockIdx.x - p.first_wg) * 4 + wv;
  if (tile >= n_tiles) return;                             // the picture's tiles are rounded up to whole workgroups
  const int tyi = tile / tiles_x, tx0 = 16 * (tile - tyi * tiles_x), ty0 = 16 * tyi;
  const recon_view a = { k.pool, k.n_pool, p.y, p.u, p.v, p.stride_y, p.stride_c, p.width, p.height, p.chroma };
  predict_tile(lane, lds[wv], a, p.cus, p.width >> 2, p.pool_of, tx0, ty0);
}


}  // namespace

extern "C" {

int kvz_hip_inter_recon_frames(const kvz_hip_recon_picture *pictures, int n_pictures, const kvz_hip_ref_picture *pool, int n_pool,
                               kvz_hip_stream s)
{
  KVZ_CHAIN_PROLOGUE(pictures, n_pictures);
  if (!pool || n_pool < 1 || n_pool > KVZ_HIP_RECON_POOL_PICTURES) return kvzhip::invalid_arg(__func__);
  multi_args k;
  __builtin_memset(&k, 0, sizeof k);
  k.n_pictures = n_pictures;
  k.n_pool = n_pool;
  bool named[KVZ_HIP_RECON_POOL_PICTURES] = { false };
  int first_wg[KVZ_HIP_MAX_CHAIN_PICTURES], at = 0;
  unsigned long long groups = 0;
  // every record is checked before anything is launched: a refused call writes nothing
  if (const char *why = recon_records_why(pictures, n_pictures, pool, n_pool, named, first_wg, groups, &at)) return refuse_picture(__func__, at, why);
  for (int i = 0; i < n_pictures; ++i) {
    const kvz_hip_recon_picture &p = pictures[i];
    const int chroma = p.params.chroma, n_refs = p.params.n_refs;
    multi_pic &a = k.p[i];
    a.y = p.pred_y; a.u = chroma ? p.pred_u : nullptr; a.v = chroma ? p.pred_v : nullptr;
    a.cus = (const u32 *)p.cus;
    a.stride_y = p.stride_y; a.stride_c = p.stride_c;
    a.width = p.width; a.height = p.height;
    a.chroma = chroma ? 1 : 0;
    a.first_wg = first_wg[i];
    for (int l = 0; l < 2; ++l)
      for (int r = 0; r < 16; ++r) a.pool_of[l][r] = p.params.ref_LX[l][r] < n_refs ? p.refs[p.params.ref_LX[l][r]] : 255;
  }
  for (int r = 0; r < n_pool; ++r)
    if (named[r]) k.pool[r] = pool[r];
  // the launch depends on the sizes alone
  hipLaunchKernelGGL(inter_recon_frames_kernel, dim3((unsigned)groups), dim3(256), 0, ctx_stream(s), k);
  KVZ_CHECK_LAUNCH("inter_recon_frames_kernel");
  return KVZ_HIP_OK;
}

}  // extern "C"
