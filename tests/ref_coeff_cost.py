"""The compiled reference's own counting coder, reached with nothing but what libkvzref.so already exports: get_coeff_cabac_cost
(rdo.c:158-197) is kvz_encode_coeff_nxn (encode_coding_tree.c:103) on a copy of the CABAC state with only_count = 1, bits_left = 23 and
num_buffered_bytes = 0.  kvz_encode_coeff_nxn takes the cabac_data_t as an argument and reads of `state` only
state->encoder_control->cfg; encoder_control is the first member of encoder_state_t and cfg the first member of encoder_control_t, so a
"state" here is one pointer to a kvz_config made by kvz_config_alloc / _init / _parse.  TEST INFRASTRUCTURE."""
import ctypes as C

import numpy as np

import ref_lib

CTX_BYTES = 184


class CabacData(C.Structure):                  # cabac_data_t, cabac.h:41-88
    _fields_ = [("cur_ctx", C.c_void_p), ("low", C.c_uint32), ("range", C.c_uint32), ("buffered_byte", C.c_uint32),
                ("num_buffered_bytes", C.c_int32), ("bits_left", C.c_int32), ("only_count", C.c_int8), ("stream", C.c_void_p),
                ("ctx", C.c_uint8 * CTX_BYTES)]


assert C.sizeof(CabacData) == 224 and CabacData.ctx.offset == 40

available = ref_lib.available
_STATES = {}


def _lib():
    L = ref_lib.lib()
    if not getattr(L, "_coeff_cost_done", False):
        L.kvz_config_alloc.restype = C.c_void_p
        L.kvz_config_init.restype = C.c_int
        L.kvz_config_init.argtypes = [C.c_void_p]
        L.kvz_config_parse.restype = C.c_int
        L.kvz_config_parse.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
        L.kvz_encode_coeff_nxn.restype = None
        L.kvz_encode_coeff_nxn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint8, C.c_uint8, C.c_int8, C.c_int8]
        L._coeff_cost_done = True
    return L


def _state(signhide, trskip_enable, lossless):
    """(pointer to a one-pointer encoder_state_t, keep-alive) for a configuration; configurations are kept for the process"""
    key = (int(bool(signhide)), int(bool(trskip_enable)), int(bool(lossless)))
    if key not in _STATES:
        L = _lib()
        cfg = L.kvz_config_alloc()
        assert cfg and L.kvz_config_init(cfg) == 1
        for name, v in zip((b"signhide", b"transform-skip", b"lossless"), key):
            assert L.kvz_config_parse(cfg, name, b"1" if v else b"0") == 1, name
        # encoder_state_t starts with the encoder_control pointer, and encoder_control_t starts with the kvz_config, held by value
        _STATES[key] = ((C.c_void_p * 1)(cfg), cfg)
    return _STATES[key][0]


def scan_table(width, mode):
    """kvz_g_sig_last_scan[mode][log2(width) - 1] of the compiled reference (tables.c:67)"""
    L = _lib()
    tab = ((C.POINTER(C.c_uint32) * 5) * 3).in_dll(L, "kvz_g_sig_last_scan")
    return [int(tab[mode][width.bit_length() - 2][i]) for i in range(width * width)]


def coeff_cabac_cost(coeff, width, type_, scan_mode, rng, ctx, signhide=1, trskip_enable=1, lossless=0, tr_skip=0):
    """get_coeff_cabac_cost for one TU (tr_skip is kvz_encode_coeff_nxn's own argument; rdo.c passes 0).  ctx: 184 uc_state bytes,
    not written.  -> (bits, the context bytes after the call)"""
    L = _lib()
    c = np.ascontiguousarray(coeff, dtype=np.int16).ravel()
    assert c.size == width * width
    if not c.any():
        return 0, bytes(bytearray(ctx))
    buf = np.zeros(c.size + 8, dtype=np.int16)                   # 8-byte aligned: the reference reads four coefficients at a time
    off = ((-buf.ctypes.data) % 8) // 2
    buf[off:off + c.size] = c
    cab = CabacData()
    cab.range = int(rng)
    cab.only_count, cab.num_buffered_bytes, cab.bits_left = 1, 0, 23
    C.memmove(cab.ctx, bytes(bytearray(int(v) for v in ctx)), CTX_BYTES)
    L.kvz_encode_coeff_nxn(_state(signhide, trskip_enable, lossless), C.byref(cab), buf.ctypes.data + 2 * off, width, type_, scan_mode,
                           int(tr_skip))
    return (23 - cab.bits_left) + (cab.num_buffered_bytes << 3), bytes(cab.ctx)
