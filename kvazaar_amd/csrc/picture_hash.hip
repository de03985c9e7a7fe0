// picture_hash.hip -- kvz_hip_picture_hash_frame, kvz_hip_picture_hash_frames and kvz_hip_array_checksum_batch: the last stage of the
// picture chain (the checksum of the decoded-picture-hash SEI and the per-plane squared error of a reconstructed picture, for one
// picture or up to sixteen) and the nal group's array_checksum for arbitrary planes.  The kernels are picture_hash_core.h's; the
// record checks are chain_host.h's.  Each entry is two launches: per-block records, then their sums.
#include "picture_hash_core.h"

namespace {

void hash_args_make(const kvz_hip_hash_picture &p, hash_args &a)
{
  const bool chroma = p.chroma != 0, src = p.src.y != nullptr;
  a.rec[0] = p.rec_y; a.rec[1] = chroma ? p.rec_u : nullptr; a.rec[2] = chroma ? p.rec_v : nullptr;
  a.src[0] = src ? p.src.y : nullptr; a.src[1] = src && chroma ? p.src.u : nullptr; a.src[2] = src && chroma ? p.src.v : nullptr;
  a.rec_stride[0] = p.stride_y; a.rec_stride[1] = chroma ? p.stride_c : 0;
  a.src_stride[0] = src ? p.src.stride_y : 0; a.src_stride[1] = src && chroma ? p.src.stride_c : 0;
  a.width = p.width; a.height = p.height;
  a.lcus_x = (p.width + 63) >> 6;
  a.n_lcu = a.lcus_x * ((p.height + 63) >> 6);
  a.lcu_out = p.lcu_out; a.out = p.out;
}

template <int N>
int picture_hash_launch(const hash_batch<N> &b, int n_pictures, int groups, hipStream_t st)
{
  hipLaunchKernelGGL(picture_hash_lcu_kernel<N>, dim3((unsigned)groups, (unsigned)n_pictures), dim3(256), 0, st, b);
  KVZ_CHECK_LAUNCH("picture_hash_lcu_kernel");
  hipLaunchKernelGGL(picture_hash_sum_kernel<N>, dim3((unsigned)n_pictures), dim3(256), 0, st, b);
  KVZ_CHECK_LAUNCH("picture_hash_sum_kernel");
  return KVZ_HIP_OK;
}

}  // namespace

namespace kvzhip {

// kvz_hip_array_checksum_batch with a first row per plane for the mask (y0 == nullptr: 0 everywhere): strategy.hip hands a plane that
// does not fit its staging buffer over in bands of rows.  Errors are reported as `entry`'s.
int array_checksum_launch(const kvz_hip_hash_plane *planes, const int *y0, int n_planes, uint32_t *block_sums, uint32_t *checksums, hipStream_t st,
                          const char *entry)
{
  if (n_planes == 0) return KVZ_HIP_OK;
  if (!planes || n_planes < 0 || n_planes > KVZ_HIP_MAX_HASH_PLANES || !block_sums || !checksums || (((uintptr_t)block_sums | (uintptr_t)checksums) & 3))
    return invalid_arg(entry);
  plane_batch b;
  __builtin_memset(&b, 0, sizeof b);
  size_t blocks = 0;
  for (int i = 0; i < n_planes; ++i) {
    const kvz_hip_hash_plane &p = planes[i];
    if (const char *why = hash_plane_why(p)) {
      char msg[200];
      snprintf(msg, sizeof msg, "%s: invalid argument in plane %d (%s)", entry, i, why);
      set_error_msg(msg);
      return KVZ_HIP_ERR_INVALID;
    }
    plane_args &a = b.p[i];
    a.data = p.data; a.width = p.width; a.height = p.height; a.stride = p.stride;
    a.y0 = y0 ? y0[i] : 0;
    a.first_block = (u32)blocks;
    a.n_blocks = (u32)hash_plane_blocks(p.width, p.height);
    a.blocks_x = (p.width + 63) >> 6;
    blocks += a.n_blocks;
  }
  b.block_sums = block_sums; b.checksums = checksums; b.n_planes = n_planes;
  hipLaunchKernelGGL(array_checksum_block_kernel, dim3((unsigned)blocks), dim3(256), 0, st, b);
  KVZ_CHECK_LAUNCH("array_checksum_block_kernel");
  hipLaunchKernelGGL(array_checksum_sum_kernel, dim3((unsigned)n_planes), dim3(256), 0, st, b);
  KVZ_CHECK_LAUNCH("array_checksum_sum_kernel");
  return KVZ_HIP_OK;
}

}  // namespace kvzhip

extern "C" {

int kvz_hip_picture_hash_frame(const kvz_hip_ref_picture *src, const kvz_hip_pixel *rec_y, uint32_t stride_y, const kvz_hip_pixel *rec_u,
                               const kvz_hip_pixel *rec_v, uint32_t stride_c, int width, int height, int chroma, kvz_hip_lcu_hash *lcu_out,
                               kvz_hip_picture_hash *out, kvz_hip_stream s)
{
  KVZ_CHECK_CTX();
  kvz_hip_hash_picture p;
  __builtin_memset(&p, 0, sizeof p);
  p.width = width; p.height = height; p.chroma = chroma ? 1 : 0;
  if (src && src->y) p.src = *src;
  p.rec_y = rec_y; p.rec_u = rec_u; p.rec_v = rec_v;
  p.stride_y = stride_y; p.stride_c = stride_c;
  p.lcu_out = lcu_out; p.out = out;
  if (const char *why = hash_record_why(&p, 0)) {
    char msg[200];
    snprintf(msg, sizeof msg, "%s: invalid argument (%s)", __func__, why);
    set_error_msg(msg);
    return KVZ_HIP_ERR_INVALID;
  }
  hash_batch<1> b;
  hash_args_make(p, b.p[0]);
  return picture_hash_launch(b, 1, b.p[0].n_lcu, ctx_stream(s));
}

int kvz_hip_picture_hash_frames(const kvz_hip_hash_picture *pictures, int n_pictures, kvz_hip_stream s)
{
  KVZ_CHAIN_PROLOGUE(pictures, n_pictures);
  hash_batch<KVZ_HIP_MAX_CHAIN_PICTURES> b;
  __builtin_memset(&b, 0, sizeof b);
  int groups = 0;
  // every record is checked before anything is launched: a refused call writes nothing
  for (int i = 0; i < n_pictures; ++i) {
    if (const char *why = hash_record_why(pictures, i)) return refuse_picture(__func__, i, why);
    hash_args_make(pictures[i], b.p[i]);
    groups = max(groups, b.p[i].n_lcu);
  }
  // a launch is sized for the largest picture; the surplus workgroups of a smaller one leave at once
  return picture_hash_launch(b, n_pictures, groups, ctx_stream(s));
}

size_t kvz_hip_array_checksum_blocks(int width, int height) { return hash_plane_blocks(width, height); }

int kvz_hip_array_checksum_batch(const kvz_hip_hash_plane *planes, int n_planes, uint32_t *block_sums, uint32_t *checksums, kvz_hip_stream s)
{
  KVZ_CHECK_CTX();
  return array_checksum_launch(planes, nullptr, n_planes, block_sums, checksums, ctx_stream(s), __func__);
}

}  // extern "C"
