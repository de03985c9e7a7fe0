"""ctypes loader for kvazaar_amd/libkvzhip.so (the C ABI of include/kvz_hip.h).

There is no fallback: if the library is missing or no MI355X is usable, the
calls raise.  Nothing in this package imports anything from oracle/."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libkvzhip.so")
_LIB = None

OK = 0


class BlockPair(C.Structure):
    """kvz_hip_block_pair"""
    _fields_ = [("x1", C.c_int32), ("y1", C.c_int32), ("x2", C.c_int32), ("y2", C.c_int32),
                ("width", C.c_int32), ("height", C.c_int32)]


class IpolBlock(C.Structure):
    """kvz_hip_ipol_block"""
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("mv_frac_x", C.c_int32), ("mv_frac_y", C.c_int32),
                ("width", C.c_int32), ("height", C.c_int32)]


class QuantParams(C.Structure):
    """kvz_hip_quant_params"""
    _fields_ = [("qp", C.c_int32), ("slice_is_intra", C.c_int32), ("signhide", C.c_int32),
                ("scaling_list", C.c_int32), ("quant_coeff", C.c_void_p), ("dequant_coeff", C.c_void_p)]


class RectCopy(C.Structure):
    """kvz_hip_rect_copy"""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("src_stride", C.c_uint32), ("dst_stride", C.c_uint32),
                ("w", C.c_int32), ("h", C.c_int32)]


class TilePlane(C.Structure):
    """kvz_hip_tile_plane"""
    _fields_ = [("ext", C.c_void_p), ("device", C.c_int32), ("stride", C.c_uint32),
                ("ext_x", C.c_int32), ("ext_y", C.c_int32), ("ext_w", C.c_int32), ("ext_h", C.c_int32),
                ("own_x", C.c_int32), ("own_y", C.c_int32), ("own_w", C.c_int32), ("own_h", C.c_int32)]


MAX_RECTS = 16      # KVZ_HIP_MAX_RECTS
MAX_TILES_PER_DIM = 48      # KVZ_HIP_MAX_TILES_PER_DIM


class TileGrid(C.Structure):
    """kvz_hip_tile_grid"""
    _fields_ = [("cols", C.c_int32), ("rows", C.c_int32), ("col_bd", C.c_int32 * MAX_TILES_PER_DIM), ("row_bd", C.c_int32 * MAX_TILES_PER_DIM)]


class CuQpTilesParams(C.Structure):
    """kvz_hip_cu_qp_tiles_params"""
    _fields_ = [("start_qp", C.c_int32), ("chain_rows", C.c_int32)]


SL_TABLE_LEN = 48960      # KVZ_HIP_SL_TABLE_LEN


class ScalingTables(C.Structure):
    """kvz_hip_scaling_tables"""
    _fields_ = [("quant", C.c_void_p), ("dequant", C.c_void_p)]


class TrSkip(C.Structure):
    """kvz_hip_trskip"""
    _fields_ = [("bit_cost", C.c_int32), ("reserved", C.c_int32), ("lcu_bit_cost", C.c_void_p)]


class Lossless(C.Structure):
    """kvz_hip_lossless"""
    _fields_ = [("chroma", C.c_int32), ("implicit_rdpcm", C.c_int32), ("reserved", C.c_int32 * 2)]


class RefPicture(C.Structure):
    """kvz_hip_ref_picture"""
    _fields_ = [("y", C.c_void_p), ("u", C.c_void_p), ("v", C.c_void_p), ("stride_y", C.c_uint32), ("stride_c", C.c_uint32),
                ("width", C.c_int32), ("height", C.c_int32)]


class InterResidualParams(C.Structure):
    """kvz_hip_inter_residual_params"""
    _fields_ = [("qp", C.c_int32), ("slice_is_intra", C.c_int32), ("signhide", C.c_int32), ("scaling_list", C.c_int32),
                ("chroma", C.c_int32), ("reserved", C.c_int32)]


MAX_CHAIN_PICTURES = 16      # KVZ_HIP_MAX_CHAIN_PICTURES


class ChainPicture(C.Structure):
    """kvz_hip_chain_picture"""
    _fields_ = [("src", RefPicture), ("rec_y", C.c_void_p), ("rec_u", C.c_void_p), ("rec_v", C.c_void_p),
                ("stride_y", C.c_uint32), ("stride_c", C.c_uint32), ("cus", C.c_void_p), ("intra_modes", C.c_void_p),
                ("coeff_y", C.c_void_p), ("coeff_u", C.c_void_p), ("coeff_v", C.c_void_p), ("cbf_out", C.c_void_p),
                ("costs", C.c_void_p), ("lcu_qp", C.c_void_p), ("params", InterResidualParams)]


CHAIN_TILE_BOUNDS = 256      # KVZ_HIP_CHAIN_TILE_BOUNDS


class ChainPictureTs(C.Structure):
    """kvz_hip_chain_picture_ts"""
    _fields_ = [("pic", ChainPicture), ("grid", C.POINTER(TileGrid)), ("tables", ScalingTables), ("ts", C.POINTER(TrSkip)),
                ("tr_skip_out", C.c_void_p)]


class DeblockParams(C.Structure):
    """kvz_hip_deblock_params"""
    _fields_ = [("beta_offset_div2", C.c_int32), ("tc_offset_div2", C.c_int32), ("qp", C.c_int32), ("frame_qp", C.c_int32),
                ("per_cu_qp", C.c_int32), ("slice_is_b", C.c_int32), ("chroma", C.c_int32), ("reserved", C.c_int32),
                ("ref_LX", (C.c_uint8 * 16) * 2)]


class FilterPicture(C.Structure):
    """kvz_hip_filter_picture"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("chroma", C.c_int32), ("reserved", C.c_int32), ("src", RefPicture),
                ("rec_y", C.c_void_p), ("rec_u", C.c_void_p), ("rec_v", C.c_void_p), ("stride_y", C.c_uint32), ("stride_c", C.c_uint32),
                ("dst_y", C.c_void_p), ("dst_u", C.c_void_p), ("dst_v", C.c_void_p), ("dst_stride_y", C.c_uint32), ("dst_stride_c", C.c_uint32),
                ("cus", C.c_void_p), ("cbf", C.c_void_p), ("lcu_qp", C.c_void_p), ("lcu_last_qp", C.c_void_p), ("stats", C.c_void_p),
                ("cands", C.c_void_p), ("sao_luma", C.c_void_p), ("sao_chroma", C.c_void_p), ("grid", C.POINTER(TileGrid)),
                ("deblock", DeblockParams), ("cu_qp", CuQpTilesParams)]


RECON_POOL_PICTURES = 48     # KVZ_HIP_RECON_POOL_PICTURES


class InterReconParams(C.Structure):
    """kvz_hip_inter_recon_params"""
    _fields_ = [("chroma", C.c_int32), ("n_refs", C.c_int32), ("ref_LX", (C.c_uint8 * 16) * 2)]


class ReconPicture(C.Structure):
    """kvz_hip_recon_picture"""
    _fields_ = [("pred_y", C.c_void_p), ("pred_u", C.c_void_p), ("pred_v", C.c_void_p), ("stride_y", C.c_uint32), ("stride_c", C.c_uint32),
                ("width", C.c_int32), ("height", C.c_int32), ("cus", C.c_void_p), ("refs", C.c_uint8 * 16), ("params", InterReconParams)]


MAX_HASH_PLANES = 48         # KVZ_HIP_MAX_HASH_PLANES


class LcuHash(C.Structure):
    """kvz_hip_lcu_hash"""
    _fields_ = [("checksum", C.c_uint32 * 3), ("sse", C.c_uint32 * 3)]


class PictureHash(C.Structure):
    """kvz_hip_picture_hash"""
    _fields_ = [("checksum", C.c_uint32 * 3), ("n_lcu", C.c_uint32), ("sse", C.c_uint64 * 3)]


class HashPicture(C.Structure):
    """kvz_hip_hash_picture"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("chroma", C.c_int32), ("reserved", C.c_int32), ("src", RefPicture),
                ("rec_y", C.c_void_p), ("rec_u", C.c_void_p), ("rec_v", C.c_void_p), ("stride_y", C.c_uint32), ("stride_c", C.c_uint32),
                ("lcu_out", C.c_void_p), ("out", C.c_void_p)]


class HashPlane(C.Structure):
    """kvz_hip_hash_plane"""
    _fields_ = [("data", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32), ("stride", C.c_uint32), ("reserved", C.c_uint32)]


class CoeffCostParams(C.Structure):
    """kvz_hip_coeff_cost_params"""
    _fields_ = [("signhide", C.c_int32), ("trskip_enable", C.c_int32), ("lossless", C.c_int32), ("reserved", C.c_int32)]


class CoeffPricing(C.Structure):
    """kvz_hip_coeff_pricing"""
    _fields_ = [("ctx_sets", C.c_void_p), ("n_sets", C.c_uint32), ("fast_limit", C.c_int32), ("lcu_ctx", C.c_void_p)]


class RdoqTables(C.Structure):
    """kvz_hip_rdoq_tables"""
    _fields_ = [("quant", C.c_void_p), ("err_scale", C.c_void_p)]


class RdoqSource(C.Structure):
    """kvz_hip_rdoq_source"""
    _fields_ = [("ctx_sets", C.c_void_p), ("states", C.c_void_p), ("lcu_ctx", C.c_void_p), ("tables", RdoqTables), ("n_sets", C.c_uint32),
                ("rdoq_skip", C.c_int32)]


class ChainPictureRdoq(C.Structure):
    """kvz_hip_chain_picture_rdoq"""
    _fields_ = [("pic", ChainPicture), ("grid", C.POINTER(TileGrid)), ("tables", ScalingTables), ("rdoq", C.POINTER(RdoqSource))]


class RdoqParams(C.Structure):
    """kvz_hip_rdoq_params"""
    _fields_ = [("signhide", C.c_int32), ("reserved", C.c_int32 * 3)]


class KvzHipError(RuntimeError):
    pass


_P = C.c_void_p
_SZ = C.c_size_t
_I = C.c_int
_U = C.c_uint32

# name -> (restype, argtypes); every symbol include/kvz_hip.h declares
SIGNATURES = {
    "kvz_hip_init": (_I, [_I]),
    "kvz_hip_set_device": (_I, [_I]),
    "kvz_hip_get_device": (_I, []),
    "kvz_hip_shutdown": (None, []),
    "kvz_hip_device_count": (_I, []),
    "kvz_hip_last_error": (C.c_char_p, []),
    "kvz_hip_device_name": (C.c_char_p, []),
    "kvz_hip_abi_version": (_I, []),
    "kvz_hip_set_tuning": (_I, [C.c_char_p, _I]),
    "kvz_hip_malloc": (_P, [_SZ]),
    "kvz_hip_free": (None, [_P]),
    "kvz_hip_malloc_host": (_P, [_SZ]),
    "kvz_hip_free_host": (None, [_P]),
    "kvz_hip_memcpy_h2d": (_I, [_P, _P, _SZ, _P]),
    "kvz_hip_memcpy_d2h": (_I, [_P, _P, _SZ, _P]),
    "kvz_hip_memset": (_I, [_P, _I, _SZ, _P]),
    "kvz_hip_memcpy_d2d": (_I, [_P, _P, _SZ, _P]),
    "kvz_hip_memcpy_peer": (_I, [_P, _I, _P, _I, _SZ, _P]),
    "kvz_hip_halo_exchange": (_I, [_P, _P, _P, _U, _I, _P]),
    "kvz_hip_copy_rects_batch": (_I, [_P, _I, _P]),
    "kvz_hip_tile_halo_exchange": (_I, [_P, _P, _I, _P]),
    "kvz_hip_stream_create": (_P, []),
    "kvz_hip_stream_destroy": (None, [_P]),
    "kvz_hip_stream_sync": (_I, [_P]),
    "kvz_hip_event_create": (_P, []),
    "kvz_hip_event_destroy": (None, [_P]),
    "kvz_hip_event_record": (_I, [_P, _P]),
    "kvz_hip_event_elapsed_ms": (_I, [_P, _P, C.POINTER(C.c_float)]),
    "kvz_hip_stream_wait_event": (_I, [_P, _P]),
    "kvz_hip_graph_begin": (_I, [_P]),
    "kvz_hip_graph_end": (_I, [_P, C.POINTER(_P)]),
    "kvz_hip_graph_launch": (_I, [_P, _P]),
    "kvz_hip_graph_destroy": (None, [_P]),
    "kvz_hip_sad_nxn_batch": (_I, [_I, _P, _P, _SZ, _P, _P]),
    "kvz_hip_satd_nxn_batch": (_I, [_I, _P, _P, _SZ, _P, _P]),
    "kvz_hip_sad_nxn_dual_batch": (_I, [_I, _P, _SZ, _SZ, _P, _SZ, _P, _P]),
    "kvz_hip_satd_nxn_dual_batch": (_I, [_I, _P, _SZ, _SZ, _P, _SZ, _P, _P]),
    "kvz_hip_reg_sad_batch": (_I, [_P, _U, _P, _U, _P, _SZ, _P, _P]),
    "kvz_hip_image_calc_sad_batch": (_I, [_P, _U, _P, _U, _I, _I, _P, _SZ, _P, _P]),
    "kvz_hip_image_calc_satd_batch": (_I, [_P, _U, _P, _U, _I, _I, _P, _SZ, _P, _P]),
    "kvz_hip_pixels_calc_ssd_batch": (_I, [_P, _U, _P, _U, _P, _SZ, _P, _P]),
    "kvz_hip_satd_any_size_quad_batch": (_I, [_P, _U, _SZ, _P, _U, _P, _SZ, _P, _P]),
    "kvz_hip_ctu_sad_grid_batch": (_I, [_P, _U, _I, _I, _P, _U, _I, _I, _P, _SZ, _P, _I, _P, _P]),
    "kvz_hip_bipred_blend_batch": (_I, [_I, _I, _I, _P, _I, _P, _P, _SZ, _P]),
    "kvz_hip_transform_batch": (_I, [_I, _I, _P, _P, _SZ, _P]),
    "kvz_hip_quant_batch": (_I, [C.POINTER(QuantParams), _P, _P, _I, _I, _I, _SZ, _P]),
    "kvz_hip_dequant_batch": (_I, [C.POINTER(QuantParams), _P, _P, _I, _I, _SZ, _P]),
    "kvz_hip_coeff_abs_sum_batch": (_I, [_P, _SZ, _SZ, _P, _P]),
    "kvz_hip_quantize_residual_batch": (_I, [C.POINTER(QuantParams), _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _SZ, _P]),
    "kvz_hip_residual_batch": (_I, [_P, _P, _P, _SZ, _P]),
    "kvz_hip_reconstruct_batch": (_I, [_P, _P, _P, _SZ, _P]),
    "kvz_hip_quantize_residual_cost_batch": (_I, [C.POINTER(QuantParams), _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _SZ, _P]),
    "kvz_hip_sample_luma_batch": (_I, [_P, _U, _I, _I, _P, _P, _SZ, _I, _P, _P]),
    "kvz_hip_sample_chroma_batch": (_I, [_P, _U, _I, _I, _P, _P, _SZ, _I, _P, _P]),
    "kvz_hip_search_frac_batch": (_I, [_P, _U, _P, _U, _I, _I, _P, _SZ, _P, _P, _P]),
    "kvz_hip_search_pu_batch": (_I, [_P, _U, _I, _I, _P, _U, _I, _I, _P, _SZ, _P, _P, _P]),
    "kvz_hip_search_pu_multi_batch": (_I, [_P, _U, _I, _I, _P, _U, _I, _I, _I, _P, _SZ, _P, _P, _P]),
    "kvz_hip_me_service_create": (_P, [_P]),
    "kvz_hip_me_service_destroy": (None, [_P]),
    "kvz_hip_me_service_put_rect": (_I, [_P, _I, _P, _U, _I, _I, _I, _I]),
    "kvz_hip_me_service_search": (_I, [_P, _P, _P]),
    "kvz_hip_me_service_get_stats": (_I, [_P, _P]),
    "kvz_hip_me_service_plane": (_P, [_P, _I]),
    "kvz_hip_me_service_sad_tables": (_P, [_P, _I, _I, _P, _I, _I, _I]),
    "kvz_hip_bipred_cost_batch": (_I, [_P, _U, _I, _I, _P, _U, _P, _U, _I, _I, _P, _SZ, _P, _P]),
    "kvz_hip_inter_candidates_batch": (_I, [_P, _P, _P, _P, _P, _SZ, _P, _P]),
    "kvz_hip_inter_candidates_multi_batch": (_I, [_P, _I, _P, _SZ, _P, _P]),
    "kvz_hip_intra_build_reference_batch": (_I, [_I, _I, _P, _I, _I, _I, _P, _SZ, _P, _P]),
    "kvz_hip_intra_predict_batch": (_I, [_I, _I, _P, _SZ, _P, _I, _P, _P]),
    "kvz_hip_intra_rough_batch": (_I, [_I, _I, _P, _P, _SZ, _P, _P, _P]),
    "kvz_hip_sao_edge_stats_batch": (_I, [_P, _P, _I, _I, _SZ, _P, _P]),
    "kvz_hip_sao_edge_ddistortion_batch": (_I, [_P, _P, _I, _I, _SZ, _P, _P, _P]),
    "kvz_hip_sao_band_stats_batch": (_I, [_P, _P, _I, _I, _SZ, _P, _P]),
    "kvz_hip_sao_band_ddistortion_batch": (_I, [_P, _P, _I, _I, _SZ, _P, _P, _P, _P]),
    "kvz_hip_sao_reconstruct_color_batch": (_I, [_P, _U, _I, _I, _P, _U, _P, _SZ, _P, _I, _I, _P]),
    "kvz_hip_deblock_frame": (_I, [_P, _U, _P, _P, _U, _I, _I, _P, _P, _P]),
    "kvz_hip_inter_recon_batch": (_I, [_P, _I, _P, _SZ, _P, _U, _P, _P, _U, _I, _P]),
    "kvz_hip_inter_recon_frame": (_I, [_P, _U, _P, _P, _U, _I, _I, _P, _P, _P, _P]),
    "kvz_hip_inter_residual_frame": (_I, [_P, _P, _U, _P, _P, _U, _P, _P, _P, _P, _P, _P, _P, _P]),
    "kvz_hip_intra_recon_frame": (_I, [_P, _P, _U, _P, _P, _U, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "kvz_hip_inter_residual_frame_qp": (_I, [_P, _P, _U, _P, _P, _U, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "kvz_hip_intra_recon_frame_qp": (_I, [_P, _P, _U, _P, _P, _U, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "kvz_hip_cu_qp_frame": (_I, [_P, _P, _I, _I, _P, _P, _P, _P]),
    "kvz_hip_sao_stats_frame": (_I, [_P, _P, _U, _P, _P, _U, _I, _P, _P, _P]),
    "kvz_hip_sao_frame": (_I, [_P, _U, _P, _P, _U, _P, _U, _P, _P, _U, _I, _I, _P, _P, _I, _P]),
    "kvz_hip_intra_recon_frame_tiles": (_I, [_P, _P, _U, _P, _P, _U, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "kvz_hip_cu_qp_frame_tiles": (_I, [_P, _P, _I, _I, _P, _P, _P, _P, _P]),
    "kvz_hip_deblock_frame_tiles": (_I, [_P, _U, _P, _P, _U, _I, _I, _P, _P, _P, _P]),
    "kvz_hip_sao_frame_tiles": (_I, [_P, _U, _P, _P, _U, _P, _U, _P, _P, _U, _I, _I, _P, _P, _I, _P, _P]),
    "kvz_hip_scaling_tables_pack": (_I, [_P, _P, _P, _P]),
    "kvz_hip_inter_residual_frame_sl": (_I, [_P, _P, _U, _P, _P, _U, _P, _P, _P, _P, _P, _P, _P, C.POINTER(ScalingTables), _P, _P]),
    "kvz_hip_intra_recon_frame_sl": (_I, [_P, _P, _U, _P, _P, _U, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.POINTER(ScalingTables), _P, _P]),
    "kvz_hip_inter_residual_frame_ts": (_I, [_P, _P, _U, _P, _P, _U, _P, _P, _P, _P, _P, _P, _P, C.POINTER(ScalingTables), C.POINTER(TrSkip), _P, _P, _P]),
    "kvz_hip_intra_recon_frame_ts": (_I, [_P, _P, _U, _P, _P, _U, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.POINTER(ScalingTables), C.POINTER(TrSkip), _P,
                                          _P, _P]),
    "kvz_hip_inter_residual_frame_ts_cabac": (_I, [_P, _P, _U, _P, _P, _U, _P, _P, _P, _P, _P, _P, _P, C.POINTER(ScalingTables), C.POINTER(TrSkip), _P,
                                                   C.POINTER(CoeffPricing), _P, _P]),
    "kvz_hip_intra_recon_frame_ts_cabac": (_I, [_P, _P, _U, _P, _P, _U, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.POINTER(ScalingTables), C.POINTER(TrSkip),
                                                _P, C.POINTER(CoeffPricing), _P, _P]),
    "kvz_hip_inter_residual_frame_rdoq": (_I, [_P, _P, _U, _P, _P, _U, _P, _P, _P, _P, _P, _P, _P, C.POINTER(ScalingTables), C.POINTER(RdoqSource), _P, _P]),
    "kvz_hip_intra_recon_frame_rdoq": (_I, [_P, _P, _U, _P, _P, _U, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.POINTER(ScalingTables), C.POINTER(RdoqSource),
                                            _P, _P]),
    "kvz_hip_inter_residual_frame_lossless": (_I, [_P, _P, _U, _P, _P, _U, _P, _P, _P, _P, _P, _P, C.POINTER(Lossless), _P]),
    "kvz_hip_intra_recon_frame_lossless": (_I, [_P, _P, _U, _P, _P, _U, _P, _P, _P, _P, _P, _P, _P, _P, C.POINTER(Lossless), _P]),
    "kvz_hip_inter_residual_frames": (_I, [C.POINTER(ChainPicture), _I, _P]),
    "kvz_hip_intra_recon_frames": (_I, [C.POINTER(ChainPicture), _I, _P]),
    "kvz_hip_inter_residual_frames_ts": (_I, [C.POINTER(ChainPictureTs), _I, _P]),
    "kvz_hip_intra_recon_frames_ts": (_I, [C.POINTER(ChainPictureTs), _I, _P]),
    "kvz_hip_inter_residual_frames_rdoq": (_I, [C.POINTER(ChainPictureRdoq), _I, _P]),
    "kvz_hip_intra_recon_frames_rdoq": (_I, [C.POINTER(ChainPictureRdoq), _I, _P]),
    "kvz_hip_cu_qp_frames": (_I, [C.POINTER(FilterPicture), _I, _P]),
    "kvz_hip_deblock_frames": (_I, [C.POINTER(FilterPicture), _I, _P]),
    "kvz_hip_sao_stats_frames": (_I, [C.POINTER(FilterPicture), _I, _P]),
    "kvz_hip_sao_frames": (_I, [C.POINTER(FilterPicture), _I, _P]),
    "kvz_hip_inter_recon_frames": (_I, [C.POINTER(ReconPicture), _I, C.POINTER(RefPicture), _I, _P]),
    "kvz_hip_picture_hash_frame": (_I, [_P, _P, _U, _P, _P, _U, _I, _I, _I, _P, _P, _P]),
    "kvz_hip_picture_hash_frames": (_I, [C.POINTER(HashPicture), _I, _P]),
    "kvz_hip_array_checksum_blocks": (_SZ, [_I, _I]),
    "kvz_hip_array_checksum_batch": (_I, [C.POINTER(HashPlane), _I, _P, _P, _P]),
    "kvz_hip_coeff_cost_batch": (_I, [_P, _P, _SZ, _P, _U, C.POINTER(CoeffCostParams), _P, _P]),
    "kvz_hip_rdoq_tables_pack": (_I, [_P, _P, _P, _P]),
    "kvz_hip_rdoq_batch": (_I, [_P, _P, _P, _SZ, _P, _P, _U, C.POINTER(RdoqTables), C.POINTER(RdoqParams), _P]),
    "kvz_hip_set_registrar": (None, [_P]),
    "kvz_hip_dropin_calls": (C.c_ulonglong, []),
    "kvz_hip_set_state_accessors": (None, [_P]),
    "kvz_strategy_register_picture_hip": (_I, [_P, C.c_uint8]),
    "kvz_strategy_register_dct_hip": (_I, [_P, C.c_uint8]),
    "kvz_strategy_register_quant_hip": (_I, [_P, C.c_uint8]),
    "kvz_strategy_register_ipol_hip": (_I, [_P, C.c_uint8]),
    "kvz_strategy_register_intra_hip": (_I, [_P, C.c_uint8]),
    "kvz_strategy_register_sao_hip": (_I, [_P, C.c_uint8]),
    "kvz_strategy_register_nal_hip": (_I, [_P, C.c_uint8]),
}


def load(path=None):
    """dlopen the library and bind every exported entry point.  Does not touch the GPU."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = path or LIB_PATH
    # One HIP runtime per process.  PyTorch wheels bundle their own libamdhip64; if this library is loaded first it brings in the
    # system's copy and a later `import torch` in the same process fails to see the device ("no ROCm-capable device").  A Python
    # host that has torch gets it loaded first, so that both share the runtime torch ships (a C host is not concerned).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(path):
        raise KvzHipError("%s not found: build it with __graft_entry__.build() (hipcc --offload-arch=gfx950); "
                          "kvazaar_amd has no CPU fallback" % path)
    L = C.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        f = getattr(L, name)          # AttributeError if the symbol is not exported
        f.restype = res
        f.argtypes = args
    _LIB = L
    return L


def check(rc, what=""):
    if rc != OK:
        L = load()
        raise KvzHipError("%s failed (rc=%d): %s" % (what or "kvz_hip call", rc, (L.kvz_hip_last_error() or b"").decode()))


def init(device=-1):
    L = load()
    check(L.kvz_hip_init(device), "kvz_hip_init")
    return L
