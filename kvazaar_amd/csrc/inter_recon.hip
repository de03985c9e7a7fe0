// inter_recon.hip -- motion compensation of whole PUs and of a whole picture for gfx950: the Y, U and V prediction
// that kvz_inter_recon_cu (inter.c:492-540) writes into lcu->rec, from PU descriptors (kvz_hip_inter_recon_batch) or
// straight from the CU array (kvz_hip_inter_recon_frame).
//
// Reference: inter_recon_unipred / kvz_inter_recon_bipred (inter.c:314-477), the sample filters of
// ipol-generic.c:122-190, :660-728 on the window of kvz_get_extended_block (:731-784), the blend of
// inter_recon_bipred_generic (picture-generic.c:538-588), the clamped copy inter_cp_with_ext_border (inter.c:277-298).
//
// A predicted sample depends only on its position and on its PU's motion (the clamp of the window is per
// coordinate), so a PU may be cut anywhere.  The unit of work is a RECTANGLE of at most 16x16 luma samples with its
// 8x8 U and V samples, owned by one wave with a private LDS slice and no barrier (the size class of
// sample_small_kernel, ipol.hip): larger PUs are cut into such rectangles, and the frame entry cuts the picture into
// 16x16 tiles and each tile into the pieces of the PUs that cross it.  The arithmetic is that of sample_core_fast
// (ipol.hip): byte windows cut with v_alignbyte, v_dot4_i32_i8 on pixels - 128 for the horizontal pass, a
// transposed int16 plane and v_dot2_i32_i16 for the vertical pass.  Every plane of every reference is reduced to its
// 14-bit sample s (the filtered sample, or pixel << 6 for an integer vector: no window, no filter pass), and the
// rectangle is stored once as clip((s + 32) >> 6) or clip((s0 + s1 + 64) >> 7); (pixel * 64 + 32) >> 6 is the pixel,
// so the copy of an integer uni-predicted plane is the same expression.  The 14-bit samples live in registers only.
// predict_rect and its sample stages are in inter_recon_core.h, which the multi-picture kernel (inter_recon_multi.hip)
// shares.  The walk over a tile's PUs stays written out in inter_recon_frame_kernel below: routed through predict_tile
// of that header the kernel came out with another instruction schedule, and these kernels are to stay as they were.
#include "inter_recon_core.h"

namespace {

struct recon_args {
  kvz_hip_ref_picture refs[KVZ_HIP_MAX_REF_PICTURES];
  int n_refs;
  u8 *y, *u, *v;                 // destination planes
  u32 stride_y, stride_c;
  int width, height;             // luma size of the picture (= of every reference picture)
  int chroma;
};

// A workgroup takes four consecutive descriptors.  A PU of at most 16x16 is one rectangle and belongs to the wave of
// its slot; a larger one is cut into 16x16 tiles (the last of a 24- or 48-wide side is 8 wide) that the four waves
// share.  No barrier: the waves never exchange data.
__global__ __launch_bounds__(256) void inter_recon_batch_kernel(recon_args a, const kvz_hip_inter_pu *__restrict__ pus, size_t count)
{
  __shared__ __attribute__((aligned(16))) u8 lds[4][LDS_WAVE];
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;   // uniform: descriptors go scalar
  const size_t first = (size_t)blockIdx.x * 4;
  for (int j = 0; j < 4; ++j) {
    const size_t i = first + j;
    if (i >= count) break;
    const kvz_hip_inter_pu d = pus[i];
    const motion_t m = { d.mv_dir, { d.ref[0], d.ref[1] }, { { d.mv[0][0], d.mv[0][1] }, { d.mv[1][0], d.mv[1][1] } } };
    if (!pu_ok(a, d.x, d.y, d.width, d.height, m)) continue;
    const int tx = (d.width + 15) >> 4, nt = tx * ((d.height + 15) >> 4);
    if (nt == 1) {
      if (j == wv) predict_rect(lane, lds[wv], a, m, d.x, d.y, d.width, d.height);
      continue;
    }
    for (int t = wv; t < nt; t += 4) {
      const int ty = div_small(t, tx), ox = 16 * (t - ty * tx), oy = 16 * ty;
      predict_rect(lane, lds[wv], a, m, d.x + ox, d.y + oy, min(16, d.width - ox), min(16, d.height - oy));
    }
  }
}

// A wave takes one 16x16 tile of the picture.  Lane l < 16 looks at the SCU (l & 3, l >> 2) of the tile: its record
// gives the CU (depth), the CU's first record the part mode, and the PU that holds the SCU its motion from the record
// at the PU's own top-left SCU (inter.c:498-507).  The wave then works through the distinct PUs of the tile: the
// first pending lane's PU, cut to the tile, is predicted and every SCU inside that rectangle is retired.
__global__ __launch_bounds__(256) void inter_recon_frame_kernel(recon_args a, const u32 *__restrict__ cus, int cus_stride,
                                                                kvz_hip_inter_recon_params prm, int tiles_x, int n_tiles)
{
  __shared__ __attribute__((aligned(16))) u8 lds[4][LDS_WAVE];
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int tile = blockIdx.x * 4 + wv;
  if (tile >= n_tiles) return;
  const int tyi = tile / tiles_x, tx0 = 16 * (tile - tyi * tiles_x), ty0 = 16 * tyi;
  const int px = tx0 + 4 * (lane & 3), py = ty0 + 4 * ((lane >> 2) & 3);       // the lane's SCU, in pixels
  bool valid = lane < 16 && px < a.width && py < a.height;
  int pu_x = 0, pu_y = 0, pu_w = 0, pu_h = 0, dir = 0, r0 = 255, r1 = 255;
  u32 mv0 = 0, mv1 = 0;
  if (valid) {
    const u32 head = cus[((size_t)(py >> 2) * cus_stride + (px >> 2)) * 5];
    const int depth = (head >> 8) & 255;
    valid = (head & 255u) == 2u && depth <= 3;                             // CU_INTER (cu.h:38-43)
    if (valid) {
      const int size = 64 >> depth, cu_x = px & ~(size - 1), cu_y = py & ~(size - 1);
      valid = cu_x + size <= a.width && cu_y + size <= a.height;
      if (valid) {
        const int part = (cus[((size_t)(cu_y >> 2) * cus_stride + (cu_x >> 2)) * 5] >> 16) & 255;
        valid = part < 8;
        if (valid) {
          const int bx = c_split_x[part] * (size >> 2), by = c_split_y[part] * (size >> 2);
          const int ox = px - cu_x, oy = py - cu_y;
          pu_x = cu_x + (bx && ox >= bx ? bx : 0);
          pu_y = cu_y + (by && oy >= by ? by : 0);
          pu_w = bx ? (ox >= bx ? size - bx : bx) : size;
          pu_h = by ? (oy >= by ? size - by : by) : size;
          valid = ((pu_x | pu_y) & 3) == 0;                                // an 8x8 CU in an AMP mode: no such PU
          if (valid) {
            const u32 *rec = cus + ((size_t)(pu_y >> 2) * cus_stride + (pu_x >> 2)) * 5;
            dir = (rec[1] >> 8) & 255;
            mv0 = rec[2];
            mv1 = rec[3];
            const u32 idx = rec[4];
            const int i0 = idx & 255, i1 = (idx >> 8) & 255;
            r0 = i0 < 16 ? prm.ref_LX[0][i0] : 255;
            r1 = i1 < 16 ? prm.ref_LX[1][i1] : 255;
            const motion_t m = { dir, { r0, r1 }, { { 0, 0 }, { 0, 0 } } };
            valid = pu_ok(a, pu_x, pu_y, pu_w, pu_h, m);
          }
        }
      }
    }
  }
  unsigned long long todo = __ballot(valid);
  while (todo) {
    const int l0 = __builtin_ctzll(todo);
    const int ux = __builtin_amdgcn_readlane(pu_x, l0), uy = __builtin_amdgcn_readlane(pu_y, l0);
    const int uw = __builtin_amdgcn_readlane(pu_w, l0), uh = __builtin_amdgcn_readlane(pu_h, l0);
    const u32 v0 = (u32)__builtin_amdgcn_readlane((int)mv0, l0), v1 = (u32)__builtin_amdgcn_readlane((int)mv1, l0);
    const motion_t m = { __builtin_amdgcn_readlane(dir, l0), { __builtin_amdgcn_readlane(r0, l0), __builtin_amdgcn_readlane(r1, l0) },
                         { { (int)(i16)(v0 & 0xffffu), (int)(i16)(v0 >> 16) }, { (int)(i16)(v1 & 0xffffu), (int)(i16)(v1 >> 16) } } };
    // the PU cut to the tile (the PU lies inside the picture, so the rectangle does too)
    const int rx = max(ux, tx0), ry = max(uy, ty0), rxe = min(ux + uw, tx0 + 16), rye = min(uy + uh, ty0 + 16);
    predict_rect(lane, lds[wv], a, m, rx, ry, rxe - rx, rye - ry);
    todo &= ~__ballot(lane < 16 && px >= rx && px < rxe && py >= ry && py < rye);
  }
}

void fill_args(recon_args &a, const kvz_hip_ref_picture *refs, int n_refs, kvz_hip_pixel *pred_y, uint32_t stride_y,
               kvz_hip_pixel *pred_u, kvz_hip_pixel *pred_v, uint32_t stride_c, int width, int height, int chroma)
{
  for (int i = 0; i < KVZ_HIP_MAX_REF_PICTURES; ++i) a.refs[i] = refs[i < n_refs ? i : 0];
  a.n_refs = n_refs;
  a.y = pred_y; a.u = chroma ? pred_u : nullptr; a.v = chroma ? pred_v : nullptr;
  a.stride_y = stride_y; a.stride_c = stride_c;
  a.width = width; a.height = height;
  a.chroma = chroma ? 1 : 0;
}

}  // namespace

extern "C" {

int kvz_hip_inter_recon_batch(const kvz_hip_ref_picture *refs, int n_refs, const kvz_hip_inter_pu *pus, size_t count,
                              kvz_hip_pixel *pred_y, uint32_t stride_y, kvz_hip_pixel *pred_u, kvz_hip_pixel *pred_v, uint32_t stride_c,
                              int chroma, kvz_hip_stream s)
{
  KVZ_CHECK_CTX();
  if (!refs || n_refs < 1 || n_refs > KVZ_HIP_MAX_REF_PICTURES || !pred_y || (chroma && (!pred_u || !pred_v)) || (count && !pus))
    return kvzhip::invalid_arg(__func__);
  const int width = refs[0].width, height = refs[0].height;
  if (!picture_ok_any_size(width, height) || stride_y < (uint32_t)width || (chroma && stride_c < (uint32_t)(width >> 1)) ||
      !refs_ok(refs, n_refs, chroma, width, height) || count > 0x7fffffffu)
    return kvzhip::invalid_arg(__func__);
  if (count == 0) return KVZ_HIP_OK;
  recon_args a;
  fill_args(a, refs, n_refs, pred_y, stride_y, pred_u, pred_v, stride_c, width, height, chroma);
  hipLaunchKernelGGL(inter_recon_batch_kernel, dim3((unsigned)((count + 3) / 4)), dim3(256), 0, ctx_stream(s), a, pus, count);
  KVZ_CHECK_LAUNCH("inter_recon_batch_kernel");
  return KVZ_HIP_OK;
}

int kvz_hip_inter_recon_frame(kvz_hip_pixel *pred_y, uint32_t stride_y, kvz_hip_pixel *pred_u, kvz_hip_pixel *pred_v, uint32_t stride_c,
                              int width, int height, const kvz_hip_cu_info *cus, const kvz_hip_ref_picture *refs,
                              const kvz_hip_inter_recon_params *params, kvz_hip_stream s)
{
  KVZ_CHECK_CTX();
  kvz_hip_recon_picture p;
  if (!recon_pack(&p, pred_y, stride_y, pred_u, pred_v, stride_c, width, height, cus, refs, params) || !recon_arrays_ok(p) || !recon_luma_ok(p) ||
      !recon_n_refs_ok(p) || !recon_chroma_ok(p) || !refs_ok(refs, params->n_refs, params->chroma, width, height))
    return kvzhip::invalid_arg(__func__);
  const int chroma = params->chroma, n_refs = params->n_refs;
  recon_args a;
  fill_args(a, refs, n_refs, pred_y, stride_y, pred_u, pred_v, stride_c, width, height, chroma);
  const int tiles_x = (width + 15) >> 4, n_tiles = tiles_x * ((height + 15) >> 4);
  hipLaunchKernelGGL(inter_recon_frame_kernel, dim3((unsigned)((n_tiles + 3) / 4)), dim3(256), 0, ctx_stream(s), a, (const u32 *)cus,
                     width >> 2, *params, tiles_x, n_tiles);
  KVZ_CHECK_LAUNCH("inter_recon_frame_kernel");
  return KVZ_HIP_OK;
}

}  // extern "C"
