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
  unsigned long long groups = 0;
  // every record is checked before anything is launched: a refused call writes nothing
  for (int i = 0; i < n_pictures; ++i) {
    const kvz_hip_recon_picture &p = pictures[i];
    const int width = p.width, height = p.height, chroma = p.params.chroma, n_refs = p.params.n_refs;
    if (!p.pred_y || !p.cus || ((uintptr_t)p.cus & 3)) return refuse_picture(__func__, i, "pred_y or cus is null, or cus misaligned");
    if (width < 8 || height < 8 || ((width | height) & 7) || p.stride_y < (uint32_t)width)
      return refuse_picture(__func__, i, "width / height must be multiples of 8, stride_y >= the width");
    if (n_refs < 1 || n_refs > KVZ_HIP_MAX_REF_PICTURES) return refuse_picture(__func__, i, "n_refs outside 1..16");
    if (chroma && (!p.pred_u || !p.pred_v || p.stride_c < (uint32_t)(width >> 1)))
      return refuse_picture(__func__, i, "a chroma plane is null, or stride_c below half the width");
    for (int r = 0; r < n_refs; ++r) {
      if (p.refs[r] >= n_pool) return refuse_picture(__func__, i, "a reference index outside the pool");
      if (!ref_ok(pool[p.refs[r]], chroma, width, height))
        return refuse_picture(__func__, i, "a named pool picture of another size, with a missing plane or a short stride");
      named[p.refs[r]] = true;
    }
    for (int j = 0; j < i; ++j)
      if (p.pred_y == pictures[j].pred_y) return refuse_picture(__func__, i, "pred_y shared with another picture");
    multi_pic &a = k.p[i];
    a.y = p.pred_y; a.u = chroma ? p.pred_u : nullptr; a.v = chroma ? p.pred_v : nullptr;
    a.cus = (const u32 *)p.cus;
    a.stride_y = p.stride_y; a.stride_c = p.stride_c;
    a.width = width; a.height = height;
    a.chroma = chroma ? 1 : 0;
    a.first_wg = (int)groups;
    for (int l = 0; l < 2; ++l)
      for (int r = 0; r < 16; ++r) a.pool_of[l][r] = p.params.ref_LX[l][r] < n_refs ? p.refs[p.params.ref_LX[l][r]] : 255;
    groups += ((unsigned long long)((width + 15) >> 4) * (unsigned long long)((height + 15) >> 4) + 3) / 4;
    if (groups > 0x7fffffffull) return refuse_picture(__func__, i, "the pictures of the call exceed the grid");
  }
  // no destination may be a plane of a pool picture that some record names
  for (int i = 0; i < n_pictures; ++i)
    for (int r = 0; r < n_pool; ++r) {
      if (!named[r]) continue;
      const kvz_hip_ref_picture &q = pool[r];
      if (k.p[i].y == q.y || (k.p[i].u && (k.p[i].u == q.u || k.p[i].v == q.v))) return refuse_picture(__func__, i, "a destination plane is a named pool plane");
    }
  for (int r = 0; r < n_pool; ++r)
    if (named[r]) k.pool[r] = pool[r];
  // the launch depends on the sizes alone
  hipLaunchKernelGGL(inter_recon_frames_kernel, dim3((unsigned)groups), dim3(256), 0, ctx_stream(s), k);
  KVZ_CHECK_LAUNCH("inter_recon_frames_kernel");
  return KVZ_HIP_OK;
}

}  // extern "C"
