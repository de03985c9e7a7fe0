// scaling_tables.hip -- kvz_hip_scaling_tables_pack: the processed scaling lists of a Kvazaar host (scaling_list_t after
// kvz_scalinglist_process, scalinglist.c:395-411) in the dense layout that kvz_hip_inter_residual_frame_sl and
// kvz_hip_intra_recon_frame_sl index on the device (sl_table_offset, quant_core.h).  Host code only: no device, no context.
#include "kvz_hip_internal.h"
#include "quant_core.h"

static_assert(sizeof(kvz_hip_scaling_tables) == 16, "layout documented in kvz_hip.h");
static_assert(sl_table_offset(3, 5, 5) + 1024 == KVZ_HIP_SL_TABLE_LEN, "the last table ends the array");

extern "C" {

int kvz_hip_scaling_tables_pack(const int32_t *const quant_coeff[4][6][6], const int32_t *const de_quant_coeff[4][6][6],
                                int32_t *quant_out, int32_t *dequant_out)
{
  if (!quant_coeff || !de_quant_coeff || !quant_out || !dequant_out) return kvzhip::invalid_arg(__func__);
  // the reference holds two 32x32 lists, [3][0] and [3][1], and [3][3] is a second name of [3][1] (scalinglist.c:30, :78-95);
  // the three other pointers of that size were never set
  auto held = [](int size_id, int list) { return size_id < 3 || list == 0 || list == 1 || list == 3; };
  for (int size_id = 0; size_id < 4; ++size_id)
    for (int list = 0; list < 6; ++list)
      for (int rem = 0; rem < 6; ++rem)
        if (held(size_id, list) && (!quant_coeff[size_id][list][rem] || !de_quant_coeff[size_id][list][rem])) return kvzhip::invalid_arg(__func__);
  for (int size_id = 0; size_id < 4; ++size_id) {
    const size_t bytes = sizeof(int32_t) << (2 * size_id + 4);
    for (int list = 0; list < 6; ++list) {
      for (int rem = 0; rem < 6; ++rem) {
        const int at = sl_table_offset(size_id, list, rem);
        if (held(size_id, list)) {
          __builtin_memcpy(quant_out + at, quant_coeff[size_id][list][rem], bytes);
          __builtin_memcpy(dequant_out + at, de_quant_coeff[size_id][list][rem], bytes);
        } else {
          __builtin_memset(quant_out + at, 0, bytes);
          __builtin_memset(dequant_out + at, 0, bytes);
        }
      }
    }
  }
  return KVZ_HIP_OK;
}

}  // extern "C"
