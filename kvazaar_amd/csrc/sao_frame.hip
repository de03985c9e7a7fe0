// sao_frame.hip -- sample adaptive offset of a whole picture: per-LCU statistics with the bit-independent candidates, and the
// reconstruction of every LCU and plane.  The stage after kvz_hip_deblock_frame in the picture chain.
//
// Reference: sao_search_luma / sao_search_chroma (sao.c:580-644) for the block geometry, calc_sao_edge_dir (sao-generic.c:82-109),
// calc_sao_bands (sao.c:247-261), sao_search_edge_sao (sao.c:355-400) and calc_sao_band_offsets (sao.c:188-240) without their
// mode bits; kvz_sao_reconstruct (sao.c:278-337) as encoder_sao_reconstruct (encoderstate.c:245-441) applies it.
//
// Statistics: one workgroup per (plane, LCU).  The LCU's rec block is staged in LDS once (dword loads: planes and strides are
// 4-byte aligned, block origins multiples of 32); a work item is one dword of rec with the 3 x 3 dwords around it, so the four
// edge classes and the band histogram all come from that one staging and the source is read once, straight from memory.  The
// edge classes use the packed accumulators of sao.hip's one-wave kernel (fields of a register per category, found with v_perm),
// reduced inside the wave before a handful of LDS atomics across the four waves; the band histogram is one packed LDS counter per
// (wave, band), with runs of equal bands inside a dword merged first.  Everything is integer: no result depends on scheduling.
//
// Reconstruction: one launch for Y, U and V; a workgroup's tile (64 x 16 luma, 32 x 32 chroma pixels, one dword per thread) lies
// inside one LCU, so the SAO record is workgroup-uniform.  Band and copy tiles go from a dword load to a dword store; an edge
// tile is staged in LDS with its one-pixel ring (read across LCU boundaries from the deblocked plane) once.
#include "sao_stats_core.h"

extern "C" {

int kvz_hip_sao_stats_frame(const kvz_hip_ref_picture *src, const kvz_hip_pixel *rec_y, uint32_t stride_y, const kvz_hip_pixel *rec_u,
                            const kvz_hip_pixel *rec_v, uint32_t stride_c, int chroma, kvz_hip_sao_lcu_stats *stats,
                            kvz_hip_sao_lcu_cand *cands, kvz_hip_stream s)
{
  KVZ_CHECK_CTX();
  kvz_hip_filter_picture p;
  if (!sao_stats_pack(&p, src, rec_y, stride_y, rec_u, rec_v, stride_c, chroma, stats, cands) || !sao_stats_out_ok(p)) return kvzhip::invalid_arg(__func__);
  if (!sao_stats_luma_ok(p)) return refuse_entry(__func__, PLANES_AND_STRIDES);
  if (!sao_stats_chroma_ok(p)) return kvzhip::invalid_arg(__func__);
  stats_args a;
  sao_stats_fill(a, p);
  hipLaunchKernelGGL(sao_stats_frame_kernel<>, dim3((unsigned)(a.n_lcu * (chroma ? 3 : 1))), dim3(256), 0, ctx_stream(s), a);
  KVZ_CHECK_LAUNCH("sao_stats_frame_kernel");
  return KVZ_HIP_OK;
}

int kvz_hip_sao_frame(const kvz_hip_pixel *rec_y, uint32_t stride_y, const kvz_hip_pixel *rec_u, const kvz_hip_pixel *rec_v, uint32_t stride_c,
                      kvz_hip_pixel *dst_y, uint32_t dst_stride_y, kvz_hip_pixel *dst_u, kvz_hip_pixel *dst_v, uint32_t dst_stride_c,
                      int width, int height, const kvz_hip_sao_info *sao_luma, const kvz_hip_sao_info *sao_chroma, int chroma,
                      kvz_hip_stream s)
{
  KVZ_CHECK_CTX();
  kvz_hip_filter_picture p;
  sao_pack(&p, rec_y, stride_y, rec_u, rec_v, stride_c, dst_y, dst_stride_y, dst_u, dst_v, dst_stride_c, width, height, sao_luma, sao_chroma, chroma, nullptr);
  return sao_frame_launch(__func__, p, s);
}

}  // extern "C"
