"""Host-side Python mirror of the batched C ABI (include/kvz_hip.h).

Two levels:
  * `DeviceBuffer` + the raw `*_batch` calls of `_lib.load()` work on device
    pointers (what bench.py times);
  * the convenience functions below take numpy arrays, stage them to HBM, run
    the HIP kernel and copy the result back -- used by the parity tests, which
    therefore always go through the C ABI and the GPU.
Names follow the reference's strategy types (strategies-picture.h:174-199,
strategies-dct.h:55-69, strategies-quant.h:58-62, strategies-ipol.h:65-74)."""
import contextlib
import ctypes as C

import numpy as np

from . import _lib
from ._lib import BlockPair, IpolBlock, QuantParams, KvzHipError, check

KINDS = {"dct": 0, "idct": 1, "dst": 2, "idst": 3, "trskip": 4, "itrskip": 5}


@contextlib.contextmanager
def tuned(**knobs):
    """with tuned(key=value, ...) as more: the tuning knobs (kvz_hip_set_tuning) set for the length of the block; more(key=value, ...)
    sets further ones inside it.  Every knob touched is back at its default (-1) afterwards, also when the block raises."""
    L = _lib.load()
    touched = set()

    def more(**kv):
        for k, v in kv.items():
            touched.add(k)
            check(L.kvz_hip_set_tuning(k.encode(), int(v)), "set_tuning %s" % k)
    try:
        more(**knobs)
        yield more
    finally:
        for k in touched:
            L.kvz_hip_set_tuning(k.encode(), -1)


class DeviceBuffer:
    """HBM allocation owned through kvz_hip_malloc/kvz_hip_free."""

    def __init__(self, nbytes):
        self.lib = _lib.init()
        self.nbytes = int(nbytes)
        self.ptr = self.lib.kvz_hip_malloc(max(self.nbytes, 16))
        if not self.ptr:
            raise KvzHipError("kvz_hip_malloc(%d) failed: %s" % (nbytes, self.lib.kvz_hip_last_error().decode()))

    @classmethod
    def from_numpy(cls, a, stream=None):
        a = np.ascontiguousarray(a)
        buf = cls(a.nbytes)
        if a.nbytes:
            check(buf.lib.kvz_hip_memcpy_h2d(buf.ptr, a.ctypes.data, a.nbytes, stream), "memcpy_h2d")
            check(buf.lib.kvz_hip_stream_sync(stream), "stream_sync")
        return buf

    def to_numpy(self, dtype, shape, stream=None):
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes <= max(self.nbytes, 16)
        if out.nbytes:
            check(self.lib.kvz_hip_memcpy_d2h(out.ctypes.data, self.ptr, out.nbytes, stream), "memcpy_d2h")
        return out

    def free(self):
        if self.ptr:
            self.lib.kvz_hip_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class PlaneView:
    """A plane that is a rectangle inside a larger uint8 buffer, the way the C ABI takes planes (pointer, stride, size):
    `buf` is the whole 2-D buffer and its row length the stride, the plane is buf[top:top + height, left:left + width], and the
    pointer handed to the entry is buffer + top * stride + left.  Every wrapper below that takes a plane as a 2-D array takes a
    PlaneView in its place; a plane the entry writes then comes back as the WHOLE buffer, so that the caller can look at the
    bytes around the plane as well (crop() cuts the plane out again)."""

    def __init__(self, buf, width, height, left=0, top=0):
        self.buf = np.ascontiguousarray(buf, dtype=np.uint8)
        self.width, self.height, self.left, self.top = int(width), int(height), int(left), int(top)
        assert self.buf.ndim == 2 and self.left >= 0 and self.top >= 0 and self.width >= 0 and self.height >= 0
        assert self.left + self.width <= self.buf.shape[1] and self.top + self.height <= self.buf.shape[0]

    @property
    def stride(self):
        return self.buf.shape[1]

    @property
    def offset(self):
        return self.top * self.stride + self.left

    def crop(self, buf=None):
        b = self.buf if buf is None else buf
        return b[self.top:self.top + self.height, self.left:self.left + self.width]


class _Staged:
    """one plane in device memory: .ptr is what the entry gets, .stride / .w / .h describe it, .shape is the buffer's"""

    def __init__(self, plane):
        if isinstance(plane, PlaneView):
            host, off = plane.buf, plane.offset
            self.stride, self.w, self.h = plane.stride, plane.width, plane.height
        else:
            host, off = np.ascontiguousarray(plane, dtype=np.uint8), 0
            self.stride, self.w, self.h = host.shape[1], host.shape[1], host.shape[0]
        self.shape = host.shape
        self.buf = DeviceBuffer.from_numpy(host)
        self.ptr = self.buf.ptr + off

    def download(self):
        """the whole buffer (= the plane when it was handed over as a compact array)"""
        return self.buf.to_numpy(np.uint8, self.shape)


def _pairs_array(pairs):
    """pairs: iterable of (x1, y1, x2, y2, w, h) -> contiguous BlockPair array as numpy int32 [n,6]"""
    a = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 6))
    return a


# ------------------------------------------------------------------ picture
def cost_nxn_batch(kind, n, blk1, blk2):
    """sad_NxN / satd_NxN over [count, n*n] uint8 block pairs -> uint32[count]"""
    L = _lib.init()
    blk1 = np.ascontiguousarray(blk1, dtype=np.uint8).reshape(-1, n * n)
    blk2 = np.ascontiguousarray(blk2, dtype=np.uint8).reshape(-1, n * n)
    count = blk1.shape[0]
    a, b, o = DeviceBuffer.from_numpy(blk1), DeviceBuffer.from_numpy(blk2), DeviceBuffer(4 * count)
    f = L.kvz_hip_sad_nxn_batch if kind == "sad" else L.kvz_hip_satd_nxn_batch
    check(f(n, a.ptr, b.ptr, count, o.ptr, None), "%s_%dx%d batch" % (kind, n, n))
    return o.to_numpy(np.uint32, (count,))


def cost_nxn_dual_batch(kind, n, preds, orig, pred_stride=1024, item_stride=2048):
    L = _lib.init()
    orig = np.ascontiguousarray(orig, dtype=np.uint8).reshape(-1, n * n)
    count = orig.shape[0]
    preds = np.ascontiguousarray(preds, dtype=np.uint8).reshape(count, item_stride)
    p, g, o = DeviceBuffer.from_numpy(preds), DeviceBuffer.from_numpy(orig), DeviceBuffer(8 * count)
    f = L.kvz_hip_sad_nxn_dual_batch if kind == "sad" else L.kvz_hip_satd_nxn_dual_batch
    check(f(n, p.ptr, pred_stride, item_stride, g.ptr, count, o.ptr, None), "%s_%dx%d_dual batch" % (kind, n, n))
    return o.to_numpy(np.uint32, (count, 2))


def _pair_call(fname, plane1, plane2, pairs, clamp):
    """plane1 / plane2: 2-D uint8 arrays (stride = width) or PlaneViews"""
    L = _lib.init()
    pa = _pairs_array(pairs)
    count = pa.shape[0]
    a, b, d, o = _Staged(plane1), _Staged(plane2), DeviceBuffer.from_numpy(pa), DeviceBuffer(4 * count)
    f = getattr(L, fname)
    if clamp:
        rc = f(a.ptr, a.stride, b.ptr, b.stride, b.w, b.h, d.ptr, count, o.ptr, None)
    else:
        rc = f(a.ptr, a.stride, b.ptr, b.stride, d.ptr, count, o.ptr, None)
    check(rc, fname)
    return o.to_numpy(np.uint32, (count,))


def reg_sad_batch(plane1, plane2, pairs):
    """reg_sad over (x1,y1,x2,y2,w,h) pairs inside 2-D uint8 planes"""
    return _pair_call("kvz_hip_reg_sad_batch", plane1, plane2, pairs, False)


def image_calc_sad_batch(pic, ref, pairs):
    return _pair_call("kvz_hip_image_calc_sad_batch", pic, ref, pairs, True)


def image_calc_satd_batch(pic, ref, pairs):
    return _pair_call("kvz_hip_image_calc_satd_batch", pic, ref, pairs, True)


def pixels_calc_ssd_batch(plane1, plane2, pairs):
    return _pair_call("kvz_hip_pixels_calc_ssd_batch", plane1, plane2, pairs, False)


def satd_any_size_quad_batch(preds, orig, pairs, pred_stride=64, pred_item_stride=64 * 64):
    """preds: uint8 [count*4, pred_item_stride]; orig: 2-D plane or PlaneView; pairs use (x1,y1,w,h)"""
    L = _lib.init()
    preds = np.ascontiguousarray(preds, dtype=np.uint8)
    pa = _pairs_array(pairs)
    count = pa.shape[0]
    p, g, d, o = DeviceBuffer.from_numpy(preds), _Staged(orig), DeviceBuffer.from_numpy(pa), DeviceBuffer(16 * count)
    check(L.kvz_hip_satd_any_size_quad_batch(p.ptr, pred_stride, pred_item_stride, g.ptr, g.stride, d.ptr, count,
                                             o.ptr, None), "satd_any_size_quad batch")
    return o.to_numpy(np.uint32, (count, 4))


def bipred_blend_batch(w, h, hi0, s0, hi1, s1):
    """s0/s1: [count, h, w] int16 (hi precision) or uint8 -> uint8 [count, h, w]"""
    L = _lib.init()
    s0 = np.ascontiguousarray(s0, dtype=np.int16 if hi0 else np.uint8).reshape(-1, h, w)
    s1 = np.ascontiguousarray(s1, dtype=np.int16 if hi1 else np.uint8).reshape(-1, h, w)
    count = s0.shape[0]
    a, b, o = DeviceBuffer.from_numpy(s0), DeviceBuffer.from_numpy(s1), DeviceBuffer(count * h * w)
    check(L.kvz_hip_bipred_blend_batch(w, h, int(hi0), a.ptr, int(hi1), b.ptr, o.ptr, count, None), "bipred blend")
    return o.to_numpy(np.uint8, (count, h, w))


def ctu_sad_grid_batch(pic, ref, ctus, mv_offsets):
    """pic, ref: 2-D planes or PlaneViews; ctus: (x, y, mvx, mvy) rows; mv_offsets: (dx, dy) rows -> uint32 [n_ctu, n_mv, 85]"""
    L = _lib.init()
    c = np.ascontiguousarray(np.asarray(ctus, dtype=np.int32).reshape(-1, 4))
    mv = np.ascontiguousarray(np.asarray(mv_offsets, dtype=np.int16).reshape(-1, 2))
    n, k = c.shape[0], mv.shape[0]
    a, b, dc, dm, o = _Staged(pic), _Staged(ref), DeviceBuffer.from_numpy(c), DeviceBuffer.from_numpy(mv), DeviceBuffer(4 * 85 * n * k)
    check(L.kvz_hip_ctu_sad_grid_batch(a.ptr, a.stride, a.w, a.h, b.ptr, b.stride, b.w, b.h, dc.ptr, n, dm.ptr, k, o.ptr, None),
          "ctu_sad_grid batch")
    return o.to_numpy(np.uint32, (n, k, 85))


# ------------------------------------------------------------------ dct
def transform_batch(kind, n, blocks):
    L = _lib.init()
    blocks = np.ascontiguousarray(blocks, dtype=np.int16).reshape(-1, n * n)
    count = blocks.shape[0]
    a, o = DeviceBuffer.from_numpy(blocks), DeviceBuffer(blocks.nbytes)
    check(L.kvz_hip_transform_batch(KINDS[kind], n, a.ptr, o.ptr, count, None), "%s %d batch" % (kind, n))
    return o.to_numpy(np.int16, blocks.shape)


# ------------------------------------------------------------------ quant
def _qparams(qp, slice_is_intra=0, signhide=0, quant_coeff=None, dequant_coeff=None):
    p = QuantParams()
    p.qp, p.slice_is_intra, p.signhide = int(qp), int(slice_is_intra), int(signhide)
    keep = []
    if quant_coeff is not None or dequant_coeff is not None:
        p.scaling_list = 1
        if quant_coeff is not None:
            q = DeviceBuffer.from_numpy(np.ascontiguousarray(quant_coeff, dtype=np.int32)); keep.append(q)
            p.quant_coeff = q.ptr
        if dequant_coeff is not None:
            d = DeviceBuffer.from_numpy(np.ascontiguousarray(dequant_coeff, dtype=np.int32)); keep.append(d)
            p.dequant_coeff = d.ptr
    return p, keep


def quant_batch(coef, w, qp, type_, scan_idx, slice_is_intra=0, signhide=0, quant_coeff=None):
    L = _lib.init()
    coef = np.ascontiguousarray(coef, dtype=np.int16).reshape(-1, w * w)
    count = coef.shape[0]
    p, keep = _qparams(qp, slice_is_intra, signhide, quant_coeff=quant_coeff)
    a, o = DeviceBuffer.from_numpy(coef), DeviceBuffer(coef.nbytes)
    check(L.kvz_hip_quant_batch(C.byref(p), a.ptr, o.ptr, w, type_, scan_idx, count, None), "quant batch")
    return o.to_numpy(np.int16, coef.shape)


def dequant_batch(q_coef, w, qp, type_, dequant_coeff=None):
    L = _lib.init()
    q_coef = np.ascontiguousarray(q_coef, dtype=np.int16).reshape(-1, w * w)
    count = q_coef.shape[0]
    p, keep = _qparams(qp, dequant_coeff=dequant_coeff)
    a, o = DeviceBuffer.from_numpy(q_coef), DeviceBuffer(q_coef.nbytes)
    check(L.kvz_hip_dequant_batch(C.byref(p), a.ptr, o.ptr, w, type_, count, None), "dequant batch")
    return o.to_numpy(np.int16, q_coef.shape)


def coeff_abs_sum_batch(coeffs, length):
    L = _lib.init()
    coeffs = np.ascontiguousarray(coeffs, dtype=np.int16).reshape(-1, length)
    count = coeffs.shape[0]
    a, o = DeviceBuffer.from_numpy(coeffs), DeviceBuffer(4 * count)
    check(L.kvz_hip_coeff_abs_sum_batch(a.ptr, length, count, o.ptr, None), "coeff_abs_sum batch")
    return o.to_numpy(np.uint32, (count,))


def quantize_residual_batch(ref_in, pred_in, w, qp, color, scan_order, cu_is_intra, slice_is_intra=0, signhide=0,
                            use_trskip=0, alias_rec=False, with_costs=False, quant_coeff=None, dequant_coeff=None):
    """-> (rec, coeff, has_coeffs) and, with_costs, (+ ssd(ref, rec), coeff_abs_sum) from the same launch.
    quant_coeff / dequant_coeff: per-coefficient scaling-list tables (w*w int32, raster order) of the quantisation and of
    the dequantisation; either may be left flat"""
    L = _lib.init()
    ref_in = np.ascontiguousarray(ref_in, dtype=np.uint8).reshape(-1, w * w)
    pred_in = np.ascontiguousarray(pred_in, dtype=np.uint8).reshape(-1, w * w)
    count = ref_in.shape[0]
    p, keep = _qparams(qp, slice_is_intra, signhide, quant_coeff, dequant_coeff)
    r, pr = DeviceBuffer.from_numpy(ref_in), DeviceBuffer.from_numpy(pred_in)
    rec = pr if alias_rec else DeviceBuffer(ref_in.nbytes)
    co, has = DeviceBuffer(2 * ref_in.size), DeviceBuffer(4 * count)
    if with_costs:
        ssd, sab = DeviceBuffer(4 * count), DeviceBuffer(4 * count)
        check(L.kvz_hip_quantize_residual_cost_batch(C.byref(p), int(cu_is_intra), w, color, scan_order, int(use_trskip),
                                                     r.ptr, pr.ptr, rec.ptr, co.ptr, has.ptr, ssd.ptr, sab.ptr, count, None),
              "quantize_residual_cost")
        return (rec.to_numpy(np.uint8, ref_in.shape), co.to_numpy(np.int16, ref_in.shape), has.to_numpy(np.int32, (count,)),
                ssd.to_numpy(np.uint32, (count,)), sab.to_numpy(np.uint32, (count,)))
    check(L.kvz_hip_quantize_residual_batch(C.byref(p), int(cu_is_intra), w, color, scan_order, int(use_trskip),
                                            r.ptr, pr.ptr, rec.ptr, co.ptr, has.ptr, count, None), "quantize_residual")
    return (rec.to_numpy(np.uint8, ref_in.shape), co.to_numpy(np.int16, ref_in.shape), has.to_numpy(np.int32, (count,)))


# ------------------------------------------------------------------ ipol
def sample_batch(kind, ref, blocks, ref_w=None, ref_h=None):
    """kind: luma|luma14|chroma|chroma14; blocks: (x, y, frac_x, frac_y, w, h); returns list of arrays.
    The plane is ref[:ref_h, :ref_w] (default: all of ref) with row stride ref.shape[1]."""
    L = _lib.init()
    ref = np.ascontiguousarray(ref, dtype=np.uint8)
    b = np.ascontiguousarray(np.asarray(blocks, dtype=np.int32).reshape(-1, 6))
    count = b.shape[0]
    sizes = (b[:, 4].astype(np.int64) * b[:, 5])
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    out14 = kind.endswith("14")
    esize = 2 if out14 else 1
    r, d, o = DeviceBuffer.from_numpy(ref), DeviceBuffer.from_numpy(b), DeviceBuffer.from_numpy(offs[:-1].copy())
    dst = DeviceBuffer(int(offs[-1]) * esize)
    f = L.kvz_hip_sample_luma_batch if kind.startswith("luma") else L.kvz_hip_sample_chroma_batch
    check(f(r.ptr, ref.shape[1], ref.shape[1] if ref_w is None else ref_w, ref.shape[0] if ref_h is None else ref_h,
            d.ptr, o.ptr, count, int(out14), dst.ptr, None),
          "sample %s batch" % kind)
    flat = dst.to_numpy(np.int16 if out14 else np.uint8, (int(offs[-1]),))
    return [flat[int(offs[i]):int(offs[i + 1])].reshape(int(b[i, 5]), int(b[i, 4])) for i in range(count)]


def search_frac_batch(pic, ref, pairs, ref_w=None, ref_h=None):
    """pairs: (x1, y1, x2, y2, w, h) with (x2,y2) the integer-pel position in ref.
    The reference plane is ref[:ref_h, :ref_w] (default: all of ref) with row stride ref.shape[1].
    Returns (costs uint32 [count,17], best int32 [count,2])"""
    L = _lib.init()
    pic = np.ascontiguousarray(pic, dtype=np.uint8)
    ref = np.ascontiguousarray(ref, dtype=np.uint8)
    pa = _pairs_array(pairs)
    count = pa.shape[0]
    a, b, d = DeviceBuffer.from_numpy(pic), DeviceBuffer.from_numpy(ref), DeviceBuffer.from_numpy(pa)
    co, be = DeviceBuffer(4 * 17 * count), DeviceBuffer(8 * count)
    check(L.kvz_hip_search_frac_batch(a.ptr, pic.shape[1], b.ptr, ref.shape[1], ref.shape[1] if ref_w is None else ref_w,
                                      ref.shape[0] if ref_h is None else ref_h, d.ptr, count, co.ptr, be.ptr, None),
          "search_frac batch")
    return co.to_numpy(np.uint32, (count, 17)), be.to_numpy(np.int32, (count, 2))


# ---- intra group ----
INTRA_LUMA, INTRA_FILTER_BOUNDARY, INTRA_RAW = 1, 2, 4


def intra_build_reference_batch(log2_width, color, plane, pic_w, pic_h, xy):
    """kvz_intra_build_reference for the PUs of `color` at the luma positions xy (count, 2), gathered on the device from
    the 2-D reconstruction plane of that colour; returns uint8 [count, 130] = kvz_intra_ref {left[65], top[65]}."""
    L = _lib.init()
    plane = np.ascontiguousarray(plane, dtype=np.uint8)
    xy = np.ascontiguousarray(xy, dtype=np.int32).reshape(-1, 2)
    count = xy.shape[0]
    p, q = DeviceBuffer.from_numpy(plane), DeviceBuffer.from_numpy(xy)
    out = DeviceBuffer(max(1, 130 * count))
    check(L.kvz_hip_intra_build_reference_batch(log2_width, color, p.ptr, plane.shape[1], pic_w, pic_h, q.ptr, count, out.ptr, None),
          "intra_build_reference batch")
    return out.to_numpy(np.uint8, (count, 130))


def intra_predict_batch(refs, log2_width, modes, flags=INTRA_LUMA | INTRA_FILTER_BOUNDARY):
    """refs: (count, 130) uint8 = kvz_intra_ref {left[65], top[65]}.  kvz_intra_predict for every PU x every mode of
    `modes`; returns uint8 [count, len(modes), N*N]."""
    L = _lib.init()
    refs = np.ascontiguousarray(refs, dtype=np.uint8).reshape(-1, 130)
    count, n = refs.shape[0], 1 << log2_width
    m = np.ascontiguousarray(modes, dtype=np.int8)
    r = DeviceBuffer.from_numpy(refs)
    out = DeviceBuffer(max(1, count * len(m) * n * n))
    check(L.kvz_hip_intra_predict_batch(log2_width, flags, r.ptr, count, m.ctypes.data, len(m), out.ptr, None), "intra_predict batch")
    return out.to_numpy(np.uint8, (count, len(m), n * n))


def intra_rough_batch(refs, log2_width, orig, flags=INTRA_LUMA | INTRA_FILTER_BOUNDARY, with_sad=False):
    """All 35 mode costs of search_intra_rough per PU: returns satd uint32 [count, 35] (and sad if with_sad)."""
    L = _lib.init()
    refs = np.ascontiguousarray(refs, dtype=np.uint8).reshape(-1, 130)
    count, n = refs.shape[0], 1 << log2_width
    orig = np.ascontiguousarray(orig, dtype=np.uint8).reshape(count, n * n)
    r, o = DeviceBuffer.from_numpy(refs), DeviceBuffer.from_numpy(orig)
    satd = DeviceBuffer(max(1, 4 * 35 * count))
    sad = DeviceBuffer(max(1, 4 * 35 * count)) if with_sad else None
    check(L.kvz_hip_intra_rough_batch(log2_width, flags, r.ptr, o.ptr, count, satd.ptr, sad.ptr if sad else None, None), "intra_rough batch")
    a = satd.to_numpy(np.uint32, (count, 35))
    return (a, sad.to_numpy(np.uint32, (count, 35))) if with_sad else a


# ---- AMVP / merge candidates of whole PUs ----
def inter_candidates_batch(params, cus, col_cus, ref_cus, pus):
    """kvz_hip_inter_candidates_batch: params = one kvz_hip_inter_params record (252 bytes), cus / col_cus / ref_cus = 2-D arrays of
    kvz_hip_cu_info records (20 bytes), pus = kvz_hip_me_pu records with x, y, width, height, pad set.  Returns (the completed
    descriptors as bytes [count, 64], the merge lists as bytes [count, 5, 12])."""
    L = _lib.init()
    params = np.ascontiguousarray(params)
    assert params.nbytes == 252
    pus = np.ascontiguousarray(pus)
    count = pus.shape[0]
    a, u = DeviceBuffer.from_numpy(np.ascontiguousarray(cus)), DeviceBuffer.from_numpy(pus)
    b = DeviceBuffer.from_numpy(np.ascontiguousarray(col_cus)) if col_cus is not None else None
    c = DeviceBuffer.from_numpy(np.ascontiguousarray(ref_cus)) if ref_cus is not None else None
    m = DeviceBuffer(max(1, 60 * count))
    check(L.kvz_hip_inter_candidates_batch(a.ptr, b.ptr if b else None, c.ptr if c else None, params.ctypes.data, u.ptr, count, m.ptr, None),
          "inter_candidates batch")
    return u.to_numpy(np.uint8, (count, 64)), m.to_numpy(np.uint8, (count, 5, 12))


def inter_candidates_multi_batch(pictures, pus):
    """kvz_hip_inter_candidates_multi_batch: pictures = list of (params, cus, col_cus, ref_cus) as inter_candidates_batch takes them;
    pus carry their picture in pad >> 2.  Returns (descriptors as bytes [count, 64], merge lists as bytes [count, 5, 12])."""
    import struct
    L = _lib.init()
    pus = np.ascontiguousarray(pus)
    count = pus.shape[0]
    keep, rec = [], b""
    for (params, cus, col_cus, ref_cus) in pictures:
        params = np.ascontiguousarray(params)
        assert params.nbytes == 252
        bufs = [DeviceBuffer.from_numpy(np.ascontiguousarray(m)) if m is not None else None for m in (cus, col_cus, ref_cus)]
        keep += bufs
        rec += struct.pack("<3Q", *[(b.ptr or 0) if b else 0 for b in bufs]) + params.tobytes() + struct.pack("<i", 0)
    assert len(rec) == 280 * len(pictures)
    table = DeviceBuffer.from_numpy(np.frombuffer(rec, dtype=np.uint8))
    u = DeviceBuffer.from_numpy(pus)
    m = DeviceBuffer(max(1, 60 * count))
    check(L.kvz_hip_inter_candidates_multi_batch(table.ptr, len(pictures), u.ptr, count, m.ptr, None), "inter_candidates multi batch")
    return u.to_numpy(np.uint8, (count, 64)), m.to_numpy(np.uint8, (count, 5, 12))


# ---- motion search of whole PUs ----
def search_pu_batch(pic, ref, pus, params, cabac=None, cost_to_beat=None):
    """pic, ref: 2-D planes or PlaneViews; pus: structured array laid out as kvz_hip_me_pu (64 bytes each), params: one
    kvz_hip_me_params record (96 bytes).
    cabac: kvz_hip_me_cabac snapshots (--mv-rdo); cost_to_beat: uint32 per PU (the best cost of the pictures searched before).
    Returns the raw results as int32 [count, 8] (= kvz_hip_me_result)."""
    L = _lib.init()
    pus = np.ascontiguousarray(pus)
    params = np.ascontiguousarray(params)
    assert pus.dtype.itemsize == 64 and params.nbytes == 96
    count = pus.shape[0]
    cb = tb = None
    if cost_to_beat is not None:
        tb = DeviceBuffer.from_numpy(np.ascontiguousarray(cost_to_beat, dtype=np.uint32))
        params = params.copy()
        params.view(np.uint8).reshape(-1)[88:96] = np.frombuffer(np.uint64(tb.ptr).tobytes(), dtype=np.uint8)
    if cabac is not None:                       # --mv-rdo: kvz_hip_me_cabac snapshots, staged to the device
        cb = DeviceBuffer.from_numpy(np.ascontiguousarray(cabac).view(np.uint8))
        params = params.copy()
        params.view(np.uint8).reshape(-1)[80:88] = np.frombuffer(np.uint64(cb.ptr).tobytes(), dtype=np.uint8)
        if int(params.view(np.int32).reshape(-1)[19]) == 0:      # n_cabac: the number of snapshots handed over
            params.view(np.int32).reshape(-1)[19] = len(cabac)
    a, b, d = _Staged(pic), _Staged(ref), DeviceBuffer.from_numpy(pus.view(np.uint8))
    out = DeviceBuffer(max(1, 32 * count))
    check(L.kvz_hip_search_pu_batch(a.ptr, a.stride, a.w, a.h, b.ptr, b.stride, b.w, b.h,
                                    d.ptr, count, params.ctypes.data, out.ptr, None), "search_pu batch")
    return out.to_numpy(np.int32, (count, 8))


def search_pu_multi_batch(pics, refs, pus, params):
    """kvz_hip_search_pu_multi_batch: pics / refs = lists of 2-D planes or PlaneViews of one size and one stride per list (the
    base offsets of PlaneViews may differ), pus carry their pair in pad >> 2.  Returns int32 [count, 8]."""
    L = _lib.init()
    dp, dr = [_Staged(p) for p in pics], [_Staged(r) for r in refs]
    assert len(dp) == len(dr) and all((p.stride, p.w, p.h) == (dp[0].stride, dp[0].w, dp[0].h) for p in dp)
    assert all((r.stride, r.w, r.h) == (dr[0].stride, dr[0].w, dr[0].h) for r in dr)
    pus = np.ascontiguousarray(pus)
    params = np.ascontiguousarray(params)
    assert pus.dtype.itemsize == 64 and params.nbytes == 96
    count = pus.shape[0]
    tp = DeviceBuffer.from_numpy(np.array([b.ptr for b in dp], dtype=np.uint64))
    tr = DeviceBuffer.from_numpy(np.array([b.ptr for b in dr], dtype=np.uint64))
    d = DeviceBuffer.from_numpy(pus.view(np.uint8))
    out = DeviceBuffer(max(1, 32 * count))
    check(L.kvz_hip_search_pu_multi_batch(tp.ptr, dp[0].stride, dp[0].w, dp[0].h, tr.ptr, dr[0].stride, dr[0].w, dr[0].h, len(dp), d.ptr, count,
                                          params.ctypes.data, out.ptr, None),
          "search_pu multi batch")
    return out.to_numpy(np.int32, (count, 8))


# ---- SAO group ----
def sao_edge_stats_batch(orig, rec, bw, bh):
    """-> int32 [count, 4 classes, 2 (sum, count), 5 categories]"""
    L = _lib.init()
    orig = np.ascontiguousarray(orig, dtype=np.uint8).reshape(-1, bw * bh)
    rec = np.ascontiguousarray(rec, dtype=np.uint8).reshape(-1, bw * bh)
    count = orig.shape[0]
    a, b, o = DeviceBuffer.from_numpy(orig), DeviceBuffer.from_numpy(rec), DeviceBuffer(max(1, 160 * count))
    check(L.kvz_hip_sao_edge_stats_batch(a.ptr, b.ptr, bw, bh, count, o.ptr, None), "sao_edge_stats")
    return o.to_numpy(np.int32, (count, 4, 2, 5))


def sao_edge_ddistortion_batch(orig, rec, bw, bh, offsets):
    """offsets int32 [count, 4, 5] -> int32 [count, 4]"""
    L = _lib.init()
    orig = np.ascontiguousarray(orig, dtype=np.uint8).reshape(-1, bw * bh)
    rec = np.ascontiguousarray(rec, dtype=np.uint8).reshape(-1, bw * bh)
    count = orig.shape[0]
    offs = np.ascontiguousarray(offsets, dtype=np.int32).reshape(count, 4, 5)
    a, b, f, o = DeviceBuffer.from_numpy(orig), DeviceBuffer.from_numpy(rec), DeviceBuffer.from_numpy(offs), DeviceBuffer(max(1, 16 * count))
    check(L.kvz_hip_sao_edge_ddistortion_batch(a.ptr, b.ptr, bw, bh, count, f.ptr, o.ptr, None), "sao_edge_ddistortion")
    return o.to_numpy(np.int32, (count, 4))


def sao_band_stats_batch(orig, rec, bw, bh):
    L = _lib.init()
    orig = np.ascontiguousarray(orig, dtype=np.uint8).reshape(-1, bw * bh)
    rec = np.ascontiguousarray(rec, dtype=np.uint8).reshape(-1, bw * bh)
    count = orig.shape[0]
    a, b, o = DeviceBuffer.from_numpy(orig), DeviceBuffer.from_numpy(rec), DeviceBuffer(max(1, 256 * count))
    check(L.kvz_hip_sao_band_stats_batch(a.ptr, b.ptr, bw, bh, count, o.ptr, None), "sao_band_stats")
    return o.to_numpy(np.int32, (count, 2, 32))


def sao_band_ddistortion_batch(orig, rec, bw, bh, band_pos, bands):
    L = _lib.init()
    orig = np.ascontiguousarray(orig, dtype=np.uint8).reshape(-1, bw * bh)
    rec = np.ascontiguousarray(rec, dtype=np.uint8).reshape(-1, bw * bh)
    count = orig.shape[0]
    bp = np.ascontiguousarray(band_pos, dtype=np.int32).reshape(count)
    bd = np.ascontiguousarray(bands, dtype=np.int32).reshape(count, 4)
    a, b, p, d, o = (DeviceBuffer.from_numpy(orig), DeviceBuffer.from_numpy(rec), DeviceBuffer.from_numpy(bp), DeviceBuffer.from_numpy(bd),
                     DeviceBuffer(max(1, 4 * count)))
    check(L.kvz_hip_sao_band_ddistortion_batch(a.ptr, b.ptr, bw, bh, count, p.ptr, d.ptr, o.ptr, None), "sao_band_ddistortion")
    return o.to_numpy(np.int32, (count,))


def sao_reconstruct_color_batch(plane, blocks, infos, color, new_rec=None):
    """plane: uint8 2-D plane or PlaneView (rec); blocks int32 [count, 5] (x, y, w, h, sao_index); infos int32 [n, 14];
    new_rec: the initial destination, a 2-D array or PlaneView of the plane's size (default: a copy of `plane`, so pixels
    outside every block read as the input's).  Returns the destination after the call (the whole buffer of a PlaneView)."""
    L = _lib.init()
    blocks = np.ascontiguousarray(blocks, dtype=np.int32).reshape(-1, 5)
    infos = np.ascontiguousarray(infos, dtype=np.int32).reshape(-1, 14)
    a, d = _Staged(plane), _Staged(plane if new_rec is None else new_rec)
    assert (d.w, d.h) == (a.w, a.h)
    b, f = DeviceBuffer.from_numpy(blocks), DeviceBuffer.from_numpy(infos)
    check(L.kvz_hip_sao_reconstruct_color_batch(a.ptr, a.stride, a.w, a.h, d.ptr, d.stride,
                                                b.ptr, blocks.shape[0], f.ptr, infos.shape[0], color, None), "sao_reconstruct")
    return d.download()


def bipred_cost_batch(pic, ref0, ref1, cands):
    """pic, ref0, ref1: 2-D planes or PlaneViews (the references of one size, each with its own stride);
    cands: iterable of (x, y, w, h, mv0x, mv0y, mv1x, mv1y) (quarter-pel vectors) -> uint32 [count] SATD costs"""
    L = _lib.init()
    rec = np.zeros(len(cands), dtype=np.dtype([("g", "<i4", (4,)), ("mv", "<i2", (4,))]))
    for i, c in enumerate(cands):
        rec[i]["g"] = c[:4]
        rec[i]["mv"] = c[4:8]
    a, b, d, e = _Staged(pic), _Staged(ref0), _Staged(ref1), DeviceBuffer.from_numpy(rec.view(np.uint8))
    assert (b.w, b.h) == (d.w, d.h)
    out = DeviceBuffer(max(1, 4 * len(rec)))
    check(L.kvz_hip_bipred_cost_batch(a.ptr, a.stride, a.w, a.h, b.ptr, b.stride, d.ptr, d.stride,
                                      b.w, b.h, e.ptr, len(rec), out.ptr, None), "bipred_cost batch")
    return out.to_numpy(np.uint32, (len(rec),))


# ---- tiles of a picture, for the *_tiles entries of the picture chain ----
TILE_GRID = np.dtype([("cols", "<i4"), ("rows", "<i4"), ("col_bd", "<i4", (48,)), ("row_bd", "<i4", (48,))])   # kvz_hip_tile_grid


def tile_grid(width, height, col_bd, row_bd):
    """one TILE_GRID record from the boundaries in LCUs, as encoder_control's tiles_col_bd / tiles_row_bd hold them: [0, ..., LCUs
    per row] and [0, ..., LCU rows].  The library checks them against width and height; this only refuses what does not fit the record."""
    col_bd, row_bd = [int(v) for v in col_bd], [int(v) for v in row_bd]
    if not (2 <= len(col_bd) <= 48 and 2 <= len(row_bd) <= 48):
        raise ValueError("1 to 47 tile columns and rows")
    g = np.zeros(1, dtype=TILE_GRID)
    g["cols"], g["rows"] = len(col_bd) - 1, len(row_bd) - 1
    g["col_bd"][0, :len(col_bd)], g["row_bd"][0, :len(row_bd)] = col_bd, row_bd
    return g


def uniform_tile_grid(width, height, cols, rows):
    """the reference's uniform spacing (encoder.c:437-458): tile i of c over n LCUs is (i + 1) n / c - i n / c LCUs wide"""
    lx, ly = (width + 63) // 64, (height + 63) // 64
    bd = lambda n, c: [0] + list(np.cumsum([(i + 1) * n // c - i * n // c for i in range(c)]))
    return tile_grid(width, height, bd(lx, cols), bd(ly, rows))


def _grid(tiles):
    """the record as the *_tiles entries take it (HOST, copied at the call); the caller keeps the array until the call returned"""
    g = np.ascontiguousarray(tiles)
    assert g.dtype == TILE_GRID and g.size == 1
    return g


# ---- deblocking ----
def deblock_frame(y, u, v, cus, prm, tiles=None):
    """y, u, v: uint8 planes or PlaneViews (u, v None with prm['chroma'] == 0; u and v share one stride); cus: kvz_hip_cu_info
    records [h/4, w/4] (20 bytes each); prm: one kvz_hip_deblock_params record (64 bytes).  Returns the filtered planes (the
    whole buffer of a PlaneView).  tiles: a TILE_GRID record (tile_grid / uniform_tile_grid) -> kvz_hip_deblock_frame_tiles."""
    L = _lib.init()
    cus = np.ascontiguousarray(cus)
    prm = np.ascontiguousarray(prm)
    assert cus.dtype.itemsize == 20 and prm.nbytes == 64
    dy, dc = _Staged(y), DeviceBuffer.from_numpy(cus.view(np.uint8))
    du = _Staged(u) if u is not None else None
    dv = _Staged(v) if v is not None else None
    assert du is None or dv is None or du.stride == dv.stride
    if tiles is None:
        check(L.kvz_hip_deblock_frame(dy.ptr, dy.stride, du.ptr if du else None, dv.ptr if dv else None, du.stride if du else 0,
                                      dy.w, dy.h, dc.ptr, prm.ctypes.data, None), "deblock_frame")
    else:
        g = _grid(tiles)
        check(L.kvz_hip_deblock_frame_tiles(dy.ptr, dy.stride, du.ptr if du else None, dv.ptr if dv else None, du.stride if du else 0,
                                            dy.w, dy.h, dc.ptr, g.ctypes.data, prm.ctypes.data, None), "deblock_frame_tiles")
    return (dy.download(), du.download() if du else None, dv.download() if dv else None)


# ---- motion compensation (inter recon) ----
REF_PICTURE = np.dtype([("y", "<u8"), ("u", "<u8"), ("v", "<u8"), ("stride_y", "<u4"), ("stride_c", "<u4"),
                        ("width", "<i4"), ("height", "<i4")])                                  # kvz_hip_ref_picture
INTER_PU = np.dtype([("x", "<i4"), ("y", "<i4"), ("width", "<i4"), ("height", "<i4"), ("mv", "<i2", (2, 2)),
                     ("mv_dir", "u1"), ("ref", "u1", (2,)), ("pad", "u1")])                    # kvz_hip_inter_pu
INTER_RECON_PARAMS = np.dtype([("chroma", "<i4"), ("n_refs", "<i4"), ("ref_LX", "u1", (2, 16))])   # kvz_hip_inter_recon_params


def ref_picture_table(planes, width, height):
    """kvz_hip_ref_picture records for device planes: planes = [(y, u, v, stride_y, stride_c)] with device pointers (u, v: 0 / None for 4:0:0)"""
    t = np.zeros(len(planes), dtype=REF_PICTURE)
    for i, (y, u, v, sy, sc) in enumerate(planes):
        t[i] = (y or 0, u or 0, v or 0, sy, sc, width, height)
    return t


class _Recon:
    """stages reference pictures and a destination for the two inter recon entries"""

    def __init__(self, refs, shape, chroma, dest):
        h, w = int(shape[0]), int(shape[1])
        self.h, self.w, self.chroma, self.keep = h, w, int(chroma), []
        planes = []
        for r in refs:
            arrs = [np.ascontiguousarray(p, dtype=np.uint8) if p is not None else None for p in (tuple(r) + (None, None))[:3]]
            bufs = [DeviceBuffer.from_numpy(p) if p is not None and (k == 0 or chroma) else None for k, p in enumerate(arrs)]
            self.keep += bufs
            planes.append((bufs[0].ptr, bufs[1].ptr if bufs[1] else 0, bufs[2].ptr if bufs[2] else 0, arrs[0].shape[1],
                           arrs[1].shape[1] if bufs[1] else 0))
        self.table = ref_picture_table(planes, w, h)
        if dest is None:
            dest = (np.zeros((h, w), np.uint8), np.zeros((h // 2, w // 2), np.uint8), np.zeros((h // 2, w // 2), np.uint8))
        self.dest = [np.ascontiguousarray(p, dtype=np.uint8) if p is not None and (k == 0 or chroma) else None
                     for k, p in enumerate((tuple(dest) + (None, None))[:3])]
        self.dbuf = [DeviceBuffer.from_numpy(p) if p is not None else None for p in self.dest]

    def dptr(self, k):
        return self.dbuf[k].ptr if self.dbuf[k] else None

    def stride_c(self):
        return self.dest[1].shape[1] if self.dest[1] is not None else 0

    def result(self):
        return tuple(b.to_numpy(np.uint8, p.shape) if b else None for b, p in zip(self.dbuf, self.dest))


def inter_recon_batch(refs, pus, shape, chroma=1, dest=None):
    """kvz_hip_inter_recon_batch.  refs: [(y, u, v)] uint8 planes of the reference pictures (u, v None for 4:0:0), each at least
    shape = (height, width) large -- a larger array gives a stride beyond the width; pus: INTER_PU records; dest: optional initial
    (y, u, v) destination planes (default zeros of the picture size; again a wider array gives a stride).  Returns (y, u, v)."""
    L = _lib.init()
    pus = np.ascontiguousarray(pus, dtype=INTER_PU)
    st = _Recon(refs, shape, chroma, dest)
    d = DeviceBuffer.from_numpy(pus.view(np.uint8))
    check(L.kvz_hip_inter_recon_batch(st.table.ctypes.data, len(st.table), d.ptr, len(pus), st.dptr(0), st.dest[0].shape[1],
                                      st.dptr(1), st.dptr(2), st.stride_c(), int(chroma), None), "inter_recon batch")
    return st.result()


def inter_recon_frame(refs, cus, ref_LX, width, height, chroma=1, dest=None):
    """kvz_hip_inter_recon_frame.  refs, dest: as inter_recon_batch; cus: kvz_hip_cu_info records [height / 4, width / 4] (20 bytes
    each); ref_LX: uint8 [2, 16].  Returns (y, u, v)."""
    L = _lib.init()
    cus = np.ascontiguousarray(cus)
    assert cus.dtype.itemsize == 20 and cus.shape == (height // 4, width // 4)
    st = _Recon(refs, (height, width), chroma, dest)
    prm = np.zeros(1, dtype=INTER_RECON_PARAMS)
    prm["chroma"], prm["n_refs"], prm["ref_LX"] = int(chroma), len(st.table), np.asarray(ref_LX, dtype=np.uint8).reshape(2, 16)
    c = DeviceBuffer.from_numpy(cus.view(np.uint8))
    check(L.kvz_hip_inter_recon_frame(st.dptr(0), st.dest[0].shape[1], st.dptr(1), st.dptr(2), st.stride_c(), width, height, c.ptr,
                                      st.table.ctypes.data, prm.ctypes.data, None), "inter_recon frame")
    return st.result()


class _OnDevice:
    """a 2-D uint8 device tensor used where it lies: the same face as _Staged; download() hands the tensor back"""

    def __init__(self, t):
        assert t.dim() == 2 and t.element_size() == 1 and t.stride(1) == 1 and t.is_cuda
        self.t, self.ptr, self.stride, self.w, self.h, self.shape = t, t.data_ptr(), t.stride(0), t.shape[1], t.shape[0], tuple(t.shape)

    def download(self):
        return self.t


def _plane(p):
    return _OnDevice(p) if hasattr(p, "data_ptr") else _Staged(p)


def inter_recon_frames(pictures, pool):
    """kvz_hip_inter_recon_frames: the prediction of up to 16 pictures over one pool of reference pictures, in one call.
    pictures: a list of dicts with
      cus      kvz_hip_cu_info records [height / 4, width / 4] (20 bytes each)
      refs     the picture's table of reference pictures as indices into pool (1..16 of them)
      ref_LX   uint8 [2, 16], indices into refs
      width, height
      chroma   optional, 1 (4:2:0, the default) or 0
      dest     optional initial (y, u, v) destination planes (default zeros of the picture size)
    pool: a list of (y, u, v) planes (u, v None where only 4:0:0 pictures name the entry; an entry may be None and is then left zero,
    for a slot that no picture names).  A pool picture has the size of the first picture that names it, or else of its y plane.
    A plane is a uint8 array or PlaneView, staged to the device (a wider array gives a stride), or a 2-D uint8 device tensor, used
    where it lies; cus likewise an array or a device tensor.  Returns [(y, u, v)] per picture: what the destination planes hold
    (arrays for staged planes -- the WHOLE buffer for a PlaneView -- and the tensors themselves for device tensors; None for the
    chroma planes of a 4:0:0 picture)."""
    L = _lib.init()
    size_of, keep = {}, []
    for p in pictures:
        for k in p["refs"]:
            size_of.setdefault(int(k), (int(p["width"]), int(p["height"])))
    table = (_lib.RefPicture * max(len(pool), 1))()
    for r, planes in enumerate(pool):
        if planes is None:
            continue
        st = [_plane(q) if q is not None else None for q in (tuple(planes) + (None, None))[:3]]
        keep.append(st)
        w, h = size_of.get(r, (st[0].w, st[0].h))
        table[r] = _lib.RefPicture(st[0].ptr, st[1].ptr if st[1] else None, st[2].ptr if st[2] else None, st[0].stride,
                                   st[1].stride if st[1] else 0, w, h)
    records, dests = (_lib.ReconPicture * max(len(pictures), 1))(), []
    for i, p in enumerate(pictures):
        w, h, chroma = int(p["width"]), int(p["height"]), int(p.get("chroma", 1))
        cus = p["cus"]
        if hasattr(cus, "data_ptr"):
            cus_ptr = cus.data_ptr()
        else:
            cus = np.ascontiguousarray(cus)
            assert cus.dtype.itemsize == 20 and cus.shape == (h // 4, w // 4)
            cus = DeviceBuffer.from_numpy(cus.view(np.uint8))
            cus_ptr = cus.ptr
        dest = p.get("dest")
        if dest is None:
            dest = (np.zeros((h, w), np.uint8), np.zeros((h // 2, w // 2), np.uint8), np.zeros((h // 2, w // 2), np.uint8))
        d = [_plane(q) if q is not None and (k == 0 or chroma) else None for k, q in enumerate((tuple(dest) + (None, None))[:3])]
        keep += [cus, d]
        dests.append(d)
        r = records[i]
        r.pred_y, r.pred_u, r.pred_v = d[0].ptr, d[1].ptr if d[1] else None, d[2].ptr if d[2] else None
        r.stride_y, r.stride_c, r.width, r.height, r.cus = d[0].stride, d[1].stride if d[1] else 0, w, h, cus_ptr
        refs = [int(k) for k in p["refs"]]
        r.refs[:len(refs)] = refs
        r.params.chroma, r.params.n_refs = chroma, len(refs)
        C.memmove(r.params.ref_LX, np.ascontiguousarray(p["ref_LX"], dtype=np.uint8).reshape(2, 16).ctypes.data, 32)
    check(L.kvz_hip_inter_recon_frames(records, len(pictures), table, len(pool), None), "inter_recon frames")
    check(L.kvz_hip_stream_sync(None), "stream_sync")
    return [tuple(q.download() if q else None for q in d) for d in dests]


# ---- residual coding of a picture's inter CUs ----
INTER_RESIDUAL_PARAMS = np.dtype([("qp", "<i4"), ("slice_is_intra", "<i4"), ("signhide", "<i4"), ("scaling_list", "<i4"),
                                  ("chroma", "<i4"), ("reserved", "<i4")])                      # kvz_hip_inter_residual_params
INTER_RESIDUAL_COST = np.dtype([("ssd_y", "<u4"), ("ssd_c", "<u4"), ("zero_ssd_y", "<u4"), ("zero_ssd_c", "<u4"),
                                ("coeff_abs_y", "<u4"), ("coeff_abs_c", "<u4")])                # kvz_hip_inter_residual_cost


def inter_residual_params(qp, slice_is_intra=0, signhide=0, chroma=1, scaling_list=0):
    p = np.zeros(1, dtype=INTER_RESIDUAL_PARAMS)
    p["qp"], p["slice_is_intra"], p["signhide"], p["scaling_list"], p["chroma"] = qp, slice_is_intra, signhide, scaling_list, chroma
    return p


def coeff_shapes(width, height):
    """shapes of the luma and chroma coefficient arrays: (LCUs, 4096) and (LCUs, 1024)"""
    n = ((width + 63) // 64) * ((height + 63) // 64)
    return (n, 4096), (n, 1024)


SL_TABLE_LEN = _lib.SL_TABLE_LEN                                   # KVZ_HIP_SL_TABLE_LEN: values per packed array


def sl_table_offset(size_id, list_id, rem):
    """where table (size_id = log2 N - 2, list 0..5, rem = qp_scaled % 6) begins in a packed array (kvz_hip_scaling_tables)"""
    assert 0 <= size_id < 4 and 0 <= list_id < 6 and 0 <= rem < 6
    return 36 * (0, 16, 80, 336)[size_id] + (6 * list_id + rem) * (16 << (2 * size_id))


def pack_scaling_tables(quant, dequant):
    """kvz_hip_scaling_tables_pack.  quant, dequant: [size_id][list][rem] -> N*N int32 values (nested sequences or dicts keyed
    (size_id, list, rem)), as scaling_list_t holds them after kvz_scalinglist_process; of the 32x32 lists only 0, 1 and 3 are read
    (the others may be missing or None).  -> (quant, dequant): two int32 arrays of SL_TABLE_LEN values.  Needs no device."""
    L = _lib.load()
    keep, ptrs = [], []
    for src in (quant, dequant):
        p = (C.c_void_p * 6 * 6 * 4)()
        for size_id in range(4):
            for list_id in range(6):
                for rem in range(6):
                    try:
                        t = src[(size_id, list_id, rem)] if isinstance(src, dict) else src[size_id][list_id][rem]
                    except (KeyError, IndexError):
                        t = None
                    if t is None:
                        continue
                    a = np.ascontiguousarray(t, dtype=np.int32).reshape(-1)
                    assert a.size == 16 << (2 * size_id)
                    keep.append(a)
                    p[size_id][list_id][rem] = a.ctypes.data
        ptrs.append(p)
    out = np.zeros(SL_TABLE_LEN, np.int32), np.zeros(SL_TABLE_LEN, np.int32)
    check(L.kvz_hip_scaling_tables_pack(C.addressof(ptrs[0]), C.addressof(ptrs[1]), out[0].ctypes.data, out[1].ctypes.data), "scaling_tables_pack")
    return out


TRSKIP = np.dtype([("bit_cost", "<i4"), ("reserved", "<i4"), ("lcu_bit_cost", "<u8")])           # kvz_hip_trskip


def inter_residual_frame(src, pred, cus, qp, chroma=1, slice_is_intra=0, signhide=0, coeff=None, cbf_out=None, costs=None, lcu_qp=None,
                         trskip=None, tr_skip=None, pricing=None, rdoq=None, scaling=None):
    """kvz_hip_inter_residual_frame.  src: (y, u, v) uint8 planes of the source picture (its luma shape is the picture size;
    u, v None for 4:0:0); pred: (y, u, v) planes holding the prediction, at least as large (a wider array gives a stride);
    cus: kvz_hip_cu_info records [height / 4, width / 4]; coeff / cbf_out / costs: optional initial contents of the outputs
    (default zeros).  Returns a dict: rec (y, u, v), coeff (y, u, v) as [LCUs, 4096 / 1024] int16, cus (with cbf_y set), cbf_out
    uint8 [height / 4, width / 4], costs INTER_RESIDUAL_COST [height / 4, width / 4].
    lcu_qp: int8 [LCUs] in raster order -> kvz_hip_inter_residual_frame_qp: every TU takes the QP of its LCU and qp is ignored.
    scaling: the pair of packed arrays of pack_scaling_tables -> kvz_hip_inter_residual_frame_sl (with or without lcu_qp).
    trskip: the bit cost of transform skip, (int)(lambda + 0.5) as one int or as an int32 array [LCUs] in raster order ->
    kvz_hip_inter_residual_frame_ts (with or without lcu_qp and scaling); the dict gains tr_skip, uint8 [height / 4, width / 4].
    tr_skip: optional initial contents of that array (default zeros).
    pricing (with trskip): dict(sets=COEFF_CTX [m], fast_limit=int, lcu_ctx=uint16 [LCUs] or None) -> kvz_hip_inter_residual_frame_ts_cabac:
    a trial is priced with CABAC on its LCU's set where the LCU's QP is at or above fast_limit.  An empty dict: that entry with
    pricing == NULL.
    rdoq (without trskip): dict(sets=COEFF_CTX [m], states=RDOQ_STATE [m], tables=(quant int32, err_scale float64) as pack_rdoq_tables
    makes them, lcu_ctx=uint16 [LCUs] or None, skip=0 | 1) -> kvz_hip_inter_residual_frame_rdoq (with or without lcu_qp and scaling):
    the TUs wider than 4, and the 4x4 TUs unless skip, take their levels from kvz_rdoq on the set of their LCU.  An empty dict: that
    entry with rdoq == NULL.  Together with trskip: ValueError."""
    return _residual_frame(None, src, pred, cus, qp, chroma, slice_is_intra, signhide, coeff, cbf_out, costs, lcu_qp, scaling=scaling,
                           trskip=trskip, tr_skip=tr_skip, pricing=pricing, rdoq=rdoq)


def intra_recon_frame(src, rec, cus, modes, qp, chroma=1, signhide=0, slice_is_intra=0, coeff=None, cbf_out=None, costs=None, lcu_qp=None,
                      tiles=None, trskip=None, tr_skip=None, pricing=None, rdoq=None, scaling=None):
    """kvz_hip_intra_recon_frame.  As inter_residual_frame; rec: (y, u, v) planes as the inter stages left them (the pixels of the
    intra CUs are not read); modes: uint8 [height / 4, width / 4, 2] = intra.mode, intra.mode_chroma per SCU.  Returns the same
    dict.  lcu_qp: int8 [LCUs] in raster order -> kvz_hip_intra_recon_frame_qp.  tiles: a TILE_GRID record ->
    kvz_hip_intra_recon_frame_tiles (with or without lcu_qp).  scaling: the pair of packed arrays of pack_scaling_tables ->
    kvz_hip_intra_recon_frame_sl (with or without lcu_qp and tiles).  trskip, tr_skip: as in inter_residual_frame ->
    kvz_hip_intra_recon_frame_ts (with or without lcu_qp, tiles and scaling).  pricing: as in inter_residual_frame ->
    kvz_hip_intra_recon_frame_ts_cabac.  rdoq: as in inter_residual_frame -> kvz_hip_intra_recon_frame_rdoq (with or without lcu_qp,
    tiles and scaling)."""
    cus = np.ascontiguousarray(cus)
    modes = np.ascontiguousarray(modes, dtype=np.uint8)
    assert modes.shape == cus.shape + (2,)
    return _residual_frame(modes, src, rec, cus, qp, chroma, slice_is_intra, signhide, coeff, cbf_out, costs, lcu_qp, tiles, scaling, trskip, tr_skip,
                           pricing, rdoq)


class _StagedPicture:
    """the arrays of one picture of a residual stage on the device: the source, the prediction (the inter stage) or the reconstruction
    so far (the intra stage), the coefficients, cbf_out, costs and cus, and modes for the intra stage (None: the inter stage).  coeff,
    cbf_out, costs: optional initial contents of the outputs, zeros by default"""

    def __init__(self, modes, src, pred, cus, chroma, coeff, cbf_out, costs):
        self.chroma = chroma = int(chroma)
        self.height, self.width = src[0].shape
        self.cus = np.ascontiguousarray(cus)
        assert self.cus.dtype.itemsize == 20 and self.cus.shape == (self.height // 4, self.width // 4)
        n = self.n = 3 if chroma else 1
        self.s = [np.ascontiguousarray(p, dtype=np.uint8) for p in src[:n]]
        self.r = [np.ascontiguousarray(p, dtype=np.uint8) for p in pred[:n]]
        self.ds, self.dr = [DeviceBuffer.from_numpy(p) for p in self.s], [DeviceBuffer.from_numpy(p) for p in self.r]
        shapes = coeff_shapes(self.width, self.height)
        self.co = [np.ascontiguousarray(coeff[k], dtype=np.int16).reshape(shapes[1 if k else 0]) if coeff is not None
                   else np.zeros(shapes[1 if k else 0], np.int16) for k in range(n)]
        self.dco = [DeviceBuffer.from_numpy(c) for c in self.co]
        self.cb = np.zeros(self.cus.shape, np.uint8) if cbf_out is None else np.ascontiguousarray(cbf_out, dtype=np.uint8).reshape(self.cus.shape)
        self.cs = (np.zeros(self.cus.shape, INTER_RESIDUAL_COST) if costs is None
                   else np.ascontiguousarray(costs, dtype=INTER_RESIDUAL_COST).reshape(self.cus.shape))
        self.dcb, self.dcs = DeviceBuffer.from_numpy(self.cb), DeviceBuffer.from_numpy(self.cs.view(np.uint8))
        self.dcu = DeviceBuffer.from_numpy(self.cus.view(np.uint8))
        self.dm = None
        if modes is not None:
            m = np.ascontiguousarray(modes, dtype=np.uint8)
            assert m.shape == self.cus.shape + (2,)
            self.dm = DeviceBuffer.from_numpy(m)

    def loose(self):
        """the arguments of a single-picture entry: (src table, rec planes and strides, cus), (coeff planes, cbf_out, costs)"""
        chroma, ds, dr, dco = self.chroma, self.ds, self.dr, self.dco
        self.table = ref_picture_table([(ds[0].ptr, ds[1].ptr if chroma else 0, ds[2].ptr if chroma else 0, self.s[0].shape[1],
                                         self.s[1].shape[1] if chroma else 0)], self.width, self.height)
        planes = (self.table.ctypes.data, dr[0].ptr, self.r[0].shape[1], dr[1].ptr if chroma else None, dr[2].ptr if chroma else None,
                  self.r[1].shape[1] if chroma else 0, self.dcu.ptr)
        return planes, (dco[0].ptr, dco[1].ptr if chroma else None, dco[2].ptr if chroma else None, self.dcb.ptr, self.dcs.ptr)

    def result(self):
        pad = (None,) * (3 - self.n)
        return {"rec": tuple(b.to_numpy(np.uint8, p.shape) for b, p in zip(self.dr, self.r)) + pad,
                "coeff": tuple(b.to_numpy(np.int16, c.shape) for b, c in zip(self.dco, self.co)) + pad,
                "cus": self.dcu.to_numpy(np.uint8, self.cus.shape + (20,)).view(self.cus.dtype).reshape(self.cus.shape),
                "cbf_out": self.dcb.to_numpy(np.uint8, self.cb.shape),
                "costs": self.dcs.to_numpy(np.uint8, self.cs.shape + (24,)).view(INTER_RESIDUAL_COST).reshape(self.cs.shape)}


def _residual_frame(modes, src, pred, cus, qp, chroma, slice_is_intra, signhide, coeff, cbf_out, costs, lcu_qp=None, tiles=None, scaling=None,
                    trskip=None, tr_skip=None, pricing=None, rdoq=None):
    """the staging both residual stages share; modes None: the inter stage; lcu_qp given: the _qp entries; tiles given (intra only): the
    _tiles entry; scaling given: the _sl entries, the packed arrays uploaded for the call; trskip given: the _ts entries"""
    if rdoq is not None and trskip is not None:
        raise ValueError("rdoq together with trskip: the _rdoq entries take no kvz_hip_trskip")
    L = _lib.init()
    st = _StagedPicture(modes, src, pred, cus, chroma, coeff, cbf_out, costs)
    width, height, cus = st.width, st.height, st.cus
    prm = inter_residual_params(qp, slice_is_intra, signhide, st.chroma, 0 if scaling is None else 1)
    sl = None
    if scaling is not None:
        tq, td = (np.ascontiguousarray(t, dtype=np.int32).reshape(SL_TABLE_LEN) for t in scaling)
        dtq, dtd = DeviceBuffer.from_numpy(tq), DeviceBuffer.from_numpy(td)
        sl = _lib.ScalingTables(dtq.ptr, dtd.ptr)
    planes, outs = st.loose()
    tail = (prm.ctypes.data, None)
    if lcu_qp is not None:
        lq = np.ascontiguousarray(lcu_qp, dtype=np.int8).reshape(lcu_count(width, height))
        dq = DeviceBuffer.from_numpy(lq)
        tail = (dq.ptr,) + tail
    dqp = dq.ptr if lcu_qp is not None else None
    dts = None
    assert pricing is None or trskip is not None
    if trskip is not None:
        ts = _lib.TrSkip(0, 0, None)
        if np.ndim(trskip) == 0:
            ts.bit_cost = int(trskip)
        else:
            dbc = DeviceBuffer.from_numpy(np.ascontiguousarray(trskip, dtype=np.int32).reshape(lcu_count(width, height)))
            ts.lcu_bit_cost = dbc.ptr
        tsk = np.zeros(cus.shape, np.uint8) if tr_skip is None else np.ascontiguousarray(tr_skip, dtype=np.uint8).reshape(cus.shape)
        dts = DeviceBuffer.from_numpy(tsk)
        g = _grid(tiles) if tiles is not None else None
        if pricing is not None:
            # the _ts_cabac entries: the sets and the optional index per LCU uploaded for the call
            pr_ref = None                                        # an empty dict: the entries with pricing == NULL
            if pricing:
                sets = np.ascontiguousarray(pricing["sets"], dtype=COEFF_CTX).ravel()
                dsets = DeviceBuffer.from_numpy(sets)
                dlc = None
                if pricing.get("lcu_ctx") is not None:
                    dlc = DeviceBuffer.from_numpy(np.ascontiguousarray(pricing["lcu_ctx"], dtype=np.uint16).reshape(lcu_count(width, height)))
                pr = _lib.CoeffPricing(dsets.ptr, len(sets), int(pricing["fast_limit"]), dlc.ptr if dlc is not None else None)
                pr_ref = C.byref(pr)
            if modes is None:
                assert tiles is None
                check(L.kvz_hip_inter_residual_frame_ts_cabac(*planes, *outs, dqp, C.byref(sl) if sl is not None else None, C.byref(ts), dts.ptr,
                                                              pr_ref, prm.ctypes.data, None), "inter_residual frame_ts_cabac")
            else:
                check(L.kvz_hip_intra_recon_frame_ts_cabac(*planes, st.dm.ptr, *outs, dqp, g.ctypes.data if g is not None else None,
                                                           C.byref(sl) if sl is not None else None, C.byref(ts), dts.ptr, pr_ref,
                                                           prm.ctypes.data, None), "intra_recon frame_ts_cabac")
        elif modes is None:
            assert tiles is None
            check(L.kvz_hip_inter_residual_frame_ts(*planes, *outs, dqp, C.byref(sl) if sl is not None else None, C.byref(ts), dts.ptr,
                                                    prm.ctypes.data, None), "inter_residual frame_ts")
        else:
            dm = st.dm
            check(L.kvz_hip_intra_recon_frame_ts(*planes, dm.ptr, *outs, dqp, g.ctypes.data if g is not None else None,
                                                 C.byref(sl) if sl is not None else None, C.byref(ts), dts.ptr, prm.ctypes.data, None),
                  "intra_recon frame_ts")
    elif rdoq is not None:
        # the _rdoq entries: the sets, the states, the two tables and the optional index per LCU uploaded for the call
        rq_ref = None                                            # an empty dict: the entries with rdoq == NULL
        if rdoq:
            sets = np.ascontiguousarray(rdoq["sets"], dtype=COEFF_CTX).ravel()
            states = np.ascontiguousarray(rdoq["states"], dtype=RDOQ_STATE).ravel()
            assert len(sets) == len(states)
            rq_q = np.ascontiguousarray(rdoq["tables"][0], dtype=np.int32).reshape(SL_TABLE_LEN)
            rq_e = np.ascontiguousarray(rdoq["tables"][1], dtype=np.float64).reshape(SL_TABLE_LEN)
            d_sets, d_states, d_rq, d_re = (DeviceBuffer.from_numpy(a) for a in (sets, states, rq_q, rq_e))
            d_lc = None
            if rdoq.get("lcu_ctx") is not None:
                d_lc = DeviceBuffer.from_numpy(np.ascontiguousarray(rdoq["lcu_ctx"], dtype=np.uint16).reshape(lcu_count(width, height)))
            rq = _lib.RdoqSource(d_sets.ptr, d_states.ptr, d_lc.ptr if d_lc is not None else None, _lib.RdoqTables(d_rq.ptr, d_re.ptr), len(sets),
                                 int(rdoq.get("skip", 0)))
            rq_ref = C.byref(rq)
        if modes is None:
            assert tiles is None
            check(L.kvz_hip_inter_residual_frame_rdoq(*planes, *outs, dqp, C.byref(sl) if sl is not None else None, rq_ref, prm.ctypes.data, None),
                  "inter_residual frame_rdoq")
        else:
            g = _grid(tiles) if tiles is not None else None
            check(L.kvz_hip_intra_recon_frame_rdoq(*planes, st.dm.ptr, *outs, dqp, g.ctypes.data if g is not None else None,
                                                   C.byref(sl) if sl is not None else None, rq_ref, prm.ctypes.data, None), "intra_recon frame_rdoq")
    elif modes is None:
        assert tiles is None
        if sl is not None:
            check(L.kvz_hip_inter_residual_frame_sl(*planes, *outs, dqp, C.byref(sl), prm.ctypes.data, None), "inter_residual frame_sl")
        else:
            entry = L.kvz_hip_inter_residual_frame if lcu_qp is None else L.kvz_hip_inter_residual_frame_qp
            check(entry(*planes, *outs, *tail), "inter_residual frame")
    else:
        dm = st.dm
        if sl is not None:
            g = _grid(tiles) if tiles is not None else None
            check(L.kvz_hip_intra_recon_frame_sl(*planes, dm.ptr, *outs, dqp, g.ctypes.data if g is not None else None, C.byref(sl), prm.ctypes.data,
                                                 None), "intra_recon frame_sl")
        elif tiles is not None:
            g = _grid(tiles)
            check(L.kvz_hip_intra_recon_frame_tiles(*planes, dm.ptr, *outs, dqp, g.ctypes.data, prm.ctypes.data, None),
                  "intra_recon frame_tiles")
        else:
            entry = L.kvz_hip_intra_recon_frame if lcu_qp is None else L.kvz_hip_intra_recon_frame_qp
            check(entry(*planes, dm.ptr, *outs, *tail), "intra_recon frame")
    out = st.result()
    if dts is not None:
        out["tr_skip"] = dts.to_numpy(np.uint8, cus.shape)
    return out


# ---- several independent pictures through the two residual stages in one call ----
MAX_CHAIN_PICTURES = _lib.MAX_CHAIN_PICTURES                       # KVZ_HIP_MAX_CHAIN_PICTURES


def inter_residual_frames(pictures):
    """kvz_hip_inter_residual_frames.  pictures: a list of up to MAX_CHAIN_PICTURES dicts, each with the arguments of
    inter_residual_frame by name (src, pred, cus, qp; optional chroma, slice_is_intra, signhide, coeff, cbf_out, costs, lcu_qp).
    Returns the list of inter_residual_frame's result dicts, one per picture."""
    return _chain_frames(False, pictures)


def intra_recon_frames(pictures):
    """kvz_hip_intra_recon_frames.  pictures: a list of up to MAX_CHAIN_PICTURES dicts, each with the arguments of intra_recon_frame
    by name (src, rec, cus, modes, qp; optional chroma, signhide, slice_is_intra, coeff, cbf_out, costs, lcu_qp).  Returns the list of
    intra_recon_frame's result dicts, one per picture."""
    return _chain_frames(True, pictures)


class _ChainPicture(_StagedPicture):
    """the arrays of one picture of a multi-picture call on the device, and its record"""

    def __init__(self, intra, src, cus, qp, pred=None, rec=None, modes=None, chroma=1, slice_is_intra=0, signhide=0, coeff=None, cbf_out=None,
                 costs=None, lcu_qp=None):
        assert modes is not None or not intra
        super().__init__(modes if intra else None, src, rec if intra else pred, cus, chroma, coeff, cbf_out, costs)
        chroma = self.chroma
        rec = _lib.ChainPicture()
        rec.src = _lib.RefPicture(self.ds[0].ptr, self.ds[1].ptr if chroma else None, self.ds[2].ptr if chroma else None, self.s[0].shape[1],
                                  self.s[1].shape[1] if chroma else 0, self.width, self.height)
        rec.rec_y, rec.stride_y = self.dr[0].ptr, self.r[0].shape[1]
        if chroma:
            rec.rec_u, rec.rec_v, rec.stride_c = self.dr[1].ptr, self.dr[2].ptr, self.r[1].shape[1]
            rec.coeff_u, rec.coeff_v = self.dco[1].ptr, self.dco[2].ptr
        rec.cus, rec.coeff_y, rec.cbf_out, rec.costs = self.dcu.ptr, self.dco[0].ptr, self.dcb.ptr, self.dcs.ptr
        if intra:
            rec.intra_modes = self.dm.ptr
        if lcu_qp is not None:
            self.dq = DeviceBuffer.from_numpy(np.ascontiguousarray(lcu_qp, dtype=np.int8).reshape(lcu_count(self.width, self.height)))
            rec.lcu_qp = self.dq.ptr
        rec.params = _lib.InterResidualParams(int(qp), int(slice_is_intra), int(signhide), 0, chroma, 0)
        self.record = rec


def _chain_frames(intra, pictures):
    L = _lib.init()
    staged = [_ChainPicture(intra, **p) for p in pictures]
    records = (_lib.ChainPicture * max(len(staged), 1))(*[st.record for st in staged])
    entry = L.kvz_hip_intra_recon_frames if intra else L.kvz_hip_inter_residual_frames
    check(entry(records, len(staged), None), "intra_recon frames" if intra else "inter_residual frames")
    return [st.result() for st in staged]


# ---- several independent pictures with tiles, scaling lists and transform skip ----
CHAIN_TILE_BOUNDS = _lib.CHAIN_TILE_BOUNDS                         # KVZ_HIP_CHAIN_TILE_BOUNDS


def inter_residual_frames_ts(pictures):
    """kvz_hip_inter_residual_frames_ts.  pictures: as for inter_residual_frames, each dict with the optional keys
    tables=(quant, dequant), the packed arrays of scaling_tables_pack, and trskip=dict(bit_cost=..., lcu_bit_cost=...), either of the two
    (tr_skip_out=...: what the array of choices holds before the call, zeros by default).  Either every picture carries tables or none
    does, and the same for trskip.  grid is accepted and ignored: the stage does not depend on tiles.  Returns inter_residual_frames'
    list of dicts, with "tr_skip_out" where trskip was given."""
    return _chain_frames_ts(False, pictures)


def intra_recon_frames_ts(pictures):
    """kvz_hip_intra_recon_frames_ts.  pictures: as for intra_recon_frames, each dict with the optional keys grid=(col_bd, row_bd), the
    tile boundaries in LCUs as tile_grid takes them, and tables / trskip / tr_skip_out as for inter_residual_frames_ts.  Tiled pictures
    may stand beside untiled ones."""
    return _chain_frames_ts(True, pictures)


class _ChainPictureTs(_ChainPicture):
    """_ChainPicture with the grid, the tables and the transform-skip arguments of one picture, and the 200-byte record"""

    def __init__(self, intra, grid=None, tables=None, trskip=None, tr_skip_out=None, **plain):
        super().__init__(intra, **plain)
        height, width = plain["src"][0].shape
        rec = _lib.ChainPictureTs()
        rec.pic = self.record
        self.dts = None
        if grid is not None and intra:
            self.grid = _lib.TileGrid.from_buffer_copy(tile_grid(width, height, grid[0], grid[1]).tobytes())
            rec.grid = C.pointer(self.grid)
        if tables is not None:
            self.dt = [DeviceBuffer.from_numpy(np.ascontiguousarray(t, dtype=np.int32).reshape(SL_TABLE_LEN)) for t in tables]
            rec.tables = _lib.ScalingTables(self.dt[0].ptr, self.dt[1].ptr)
            rec.pic.params.scaling_list = 1
        if trskip is not None:
            self.ts = _lib.TrSkip(int(trskip.get("bit_cost", 0)), 0, None)
            if trskip.get("lcu_bit_cost") is not None:
                self.dbc = DeviceBuffer.from_numpy(np.ascontiguousarray(trskip["lcu_bit_cost"], dtype=np.int32).reshape(lcu_count(width, height)))
                self.ts.lcu_bit_cost = self.dbc.ptr
            tsk = (np.zeros(self.cus.shape, np.uint8) if tr_skip_out is None
                   else np.ascontiguousarray(tr_skip_out, dtype=np.uint8).reshape(self.cus.shape))
            self.dts = DeviceBuffer.from_numpy(tsk)
            rec.ts, rec.tr_skip_out = C.pointer(self.ts), self.dts.ptr
        self.record_ts = rec

    def result(self):
        out = super().result()
        if self.dts is not None:
            out["tr_skip_out"] = self.dts.to_numpy(np.uint8, self.cus.shape)
        return out


def _chain_frames_ts(intra, pictures):
    L = _lib.init()
    staged = [_ChainPictureTs(intra, **p) for p in pictures]
    records = (_lib.ChainPictureTs * max(len(staged), 1))(*[st.record_ts for st in staged])
    entry = L.kvz_hip_intra_recon_frames_ts if intra else L.kvz_hip_inter_residual_frames_ts
    check(entry(records, len(staged), None), "intra_recon frames_ts" if intra else "inter_residual frames_ts")
    return [st.result() for st in staged]


# ---- several independent pictures with RDOQ ----
def inter_residual_frames_rdoq(pictures):
    """kvz_hip_inter_residual_frames_rdoq.  pictures: as for inter_residual_frames, each dict with the optional keys tables=(quant,
    dequant), the packed arrays of scaling_tables_pack, and rdoq=dict(sets=..., states=..., tables=(quant, err_scale), lcu_ctx=...,
    skip=0 | 1) as inter_residual_frame takes it.  Either every picture carries tables or none does, and the same for rdoq; skip and
    the RDOQ tables are the call's: tables with the same values are uploaded once and shared, as the entry requires.  grid is accepted
    and ignored: the stage does not depend on tiles.  Returns inter_residual_frames' list of dicts."""
    return _chain_frames_rdoq(False, pictures)


def intra_recon_frames_rdoq(pictures):
    """kvz_hip_intra_recon_frames_rdoq.  pictures: as for intra_recon_frames, each dict with the optional keys grid=(col_bd, row_bd),
    the tile boundaries in LCUs as tile_grid takes them, and tables / rdoq as for inter_residual_frames_rdoq.  Tiled pictures may stand
    beside untiled ones; every picture has its own context sets, states and lcu_ctx."""
    return _chain_frames_rdoq(True, pictures)


class _ChainPictureRdoq(_ChainPictureTs):
    """_ChainPictureTs without transform skip, with the kvz_hip_rdoq_source of one picture, and the 192-byte record.  shared: the RDOQ
    tables already on the device for this call, [(quant, err_scale, device quant, device err_scale)]"""

    def __init__(self, intra, shared, rdoq=None, **plain):
        super().__init__(intra, **plain)
        assert self.dts is None, "rdoq together with trskip: the _rdoq entries take no kvz_hip_trskip"
        height, width = plain["src"][0].shape
        rec = _lib.ChainPictureRdoq()
        rec.pic, rec.grid, rec.tables = self.record_ts.pic, self.record_ts.grid, self.record_ts.tables
        if rdoq is not None:
            sets = np.ascontiguousarray(rdoq["sets"], dtype=COEFF_CTX).ravel()
            states = np.ascontiguousarray(rdoq["states"], dtype=RDOQ_STATE).ravel()
            assert len(sets) == len(states)
            rq_q = np.ascontiguousarray(rdoq["tables"][0], dtype=np.int32).reshape(SL_TABLE_LEN)
            rq_e = np.ascontiguousarray(rdoq["tables"][1], dtype=np.float64).reshape(SL_TABLE_LEN)
            same = [t for t in shared if np.array_equal(t[0], rq_q) and np.array_equal(t[1], rq_e)]
            if not same:
                shared.append((rq_q, rq_e, DeviceBuffer.from_numpy(rq_q), DeviceBuffer.from_numpy(rq_e)))
                same = shared[-1:]
            self.d_rq = [DeviceBuffer.from_numpy(sets), DeviceBuffer.from_numpy(states), same[0][2], same[0][3]]
            self.d_lc = None
            if rdoq.get("lcu_ctx") is not None:
                self.d_lc = DeviceBuffer.from_numpy(np.ascontiguousarray(rdoq["lcu_ctx"], dtype=np.uint16).reshape(lcu_count(width, height)))
            # the staged kvz_hip_rdoq_source stays alive with the picture, over the call
            self.rq = _lib.RdoqSource(self.d_rq[0].ptr, self.d_rq[1].ptr, self.d_lc.ptr if self.d_lc is not None else None,
                                      _lib.RdoqTables(self.d_rq[2].ptr, self.d_rq[3].ptr), len(sets), int(rdoq.get("skip", 0)))
            rec.rdoq = C.pointer(self.rq)
        self.record_rdoq = rec


def _chain_frames_rdoq(intra, pictures):
    L = _lib.init()
    shared = []
    staged = [_ChainPictureRdoq(intra, shared, **p) for p in pictures]
    records = (_lib.ChainPictureRdoq * max(len(staged), 1))(*[st.record_rdoq for st in staged])
    entry = L.kvz_hip_intra_recon_frames_rdoq if intra else L.kvz_hip_inter_residual_frames_rdoq
    check(entry(records, len(staged), None), "intra_recon frames_rdoq" if intra else "inter_residual frames_rdoq")
    return [st.result() for st in staged]


# ---- lossless coding: the two residual stages of a picture coded with --lossless ----
def inter_residual_frame_lossless(src, pred, cus, chroma=1, implicit_rdpcm=0, coeff=None, cbf_out=None, costs=None):
    """kvz_hip_inter_residual_frame_lossless.  Arguments and the returned dict as inter_residual_frame, without a QP: coeff = source -
    prediction, rec = source.  implicit_rdpcm is carried in the struct and does not apply to inter CUs."""
    return _lossless_frame(None, src, pred, cus, chroma, implicit_rdpcm, None, coeff, cbf_out, costs)


def intra_recon_frame_lossless(src, rec, cus, modes, chroma=1, implicit_rdpcm=0, tiles=None, coeff=None, cbf_out=None, costs=None):
    """kvz_hip_intra_recon_frame_lossless.  As intra_recon_frame without a QP; the reference pixels come from the source planes and rec
    is only written.  implicit_rdpcm: DPCM for TUs in modes 10 and 26, and no boundary filter.  tiles: a TILE_GRID record or None."""
    cus = np.ascontiguousarray(cus)
    modes = np.ascontiguousarray(modes, dtype=np.uint8)
    assert modes.shape == cus.shape + (2,)
    return _lossless_frame(modes, src, rec, cus, chroma, implicit_rdpcm, tiles, coeff, cbf_out, costs)


def _lossless_frame(modes, src, pred, cus, chroma, implicit_rdpcm, tiles, coeff, cbf_out, costs):
    """the staging of the two lossless entries; modes None: the inter stage"""
    L = _lib.init()
    st = _StagedPicture(modes, src, pred, cus, chroma, coeff, cbf_out, costs)
    ll = _lib.Lossless(st.chroma, int(implicit_rdpcm), (0, 0))
    planes, outs = st.loose()
    if modes is None:
        check(L.kvz_hip_inter_residual_frame_lossless(*planes, *outs, C.byref(ll), None), "inter_residual frame_lossless")
    else:
        dm = st.dm
        g = _grid(tiles) if tiles is not None else None
        check(L.kvz_hip_intra_recon_frame_lossless(*planes, dm.ptr, *outs, g.ctypes.data if g is not None else None, C.byref(ll), None),
              "intra_recon frame_lossless")
    return st.result()


# ---- the QP map of a picture whose QP changes per LCU ----
CU_QP_PARAMS = np.dtype([("start_qp", "<i4"), ("chain_lcus", "<i4")])                            # kvz_hip_cu_qp_params
CU_QP_TILES_PARAMS = np.dtype([("start_qp", "<i4"), ("chain_rows", "<i4")])                      # kvz_hip_cu_qp_tiles_params


def cu_qp_frame(cus, cbf, lcu_qp, start_qp, chain_lcus=0):
    """kvz_hip_cu_qp_frame.  cus: kvz_hip_cu_info records [height / 4, width / 4]; cbf: the cbf_out array of the residual stages,
    uint8 of the same shape; lcu_qp: int8 [LCUs] in raster order; start_qp: the picture's QP; chain_lcus: 0 = one chain, LCUs per
    row = a chain per LCU row.  Returns (cus with qp written, lcu_last_qp int8 [LCUs]: the QP predictor on entry to each LCU)."""
    prm = np.zeros(1, dtype=CU_QP_PARAMS)
    prm["start_qp"], prm["chain_lcus"] = start_qp, chain_lcus
    return _cu_qp(cus, cbf, lcu_qp, prm, None)


def cu_qp_frame_tiles(cus, cbf, lcu_qp, start_qp, tiles, chain_rows=0):
    """kvz_hip_cu_qp_frame_tiles.  As cu_qp_frame; tiles: a TILE_GRID record (None: one tile); the chains are the tiles (chain_rows = 0)
    or the LCU rows of the tiles (chain_rows = 1).  lcu_last_qp stays in picture raster order."""
    prm = np.zeros(1, dtype=CU_QP_TILES_PARAMS)
    prm["start_qp"], prm["chain_rows"] = start_qp, chain_rows
    return _cu_qp(cus, cbf, lcu_qp, prm, (None if tiles is None else _grid(tiles),))


def _cu_qp(cus, cbf, lcu_qp, prm, grid):
    """the staging both QP-map entries share; grid: None for the untiled entry, else (TILE_GRID record or None,)"""
    L = _lib.init()
    cus = np.ascontiguousarray(cus)
    assert cus.dtype.itemsize == 20 and cus.ndim == 2
    height, width = 4 * cus.shape[0], 4 * cus.shape[1]
    cb = np.ascontiguousarray(cbf, dtype=np.uint8).reshape(cus.shape)
    n = lcu_count(width, height)
    lq = np.ascontiguousarray(lcu_qp, dtype=np.int8).reshape(n)
    dcu, dcb, dq, dl = DeviceBuffer.from_numpy(cus.view(np.uint8)), DeviceBuffer.from_numpy(cb), DeviceBuffer.from_numpy(lq), DeviceBuffer(n)
    if grid is None:
        check(L.kvz_hip_cu_qp_frame(dcu.ptr, dcb.ptr, width, height, dq.ptr, dl.ptr, prm.ctypes.data, None), "cu_qp frame")
    else:
        check(L.kvz_hip_cu_qp_frame_tiles(dcu.ptr, dcb.ptr, width, height, dq.ptr, dl.ptr, None if grid[0] is None else grid[0].ctypes.data,
                                          prm.ctypes.data, None), "cu_qp frame_tiles")
    return dcu.to_numpy(np.uint8, cus.shape + (20,)).view(cus.dtype).reshape(cus.shape), dl.to_numpy(np.int8, (n,))


# ---- SAO of a whole picture ----
SAO_LCU_STATS = np.dtype([("edge", "<i4", (4, 2, 5)), ("band", "<i4", (2, 32))])                # kvz_hip_sao_lcu_stats
SAO_LCU_CAND = np.dtype([("edge_offsets", "<i4", (4, 5)), ("edge_ddist", "<i4", (4,)), ("band_offsets", "<i4", (4,)),
                         ("band_position", "<i4"), ("band_ddist", "<i4")])                      # kvz_hip_sao_lcu_cand
SAO_INFO = np.dtype([("type", "<i4"), ("eo_class", "<i4"), ("band_position", "<i4", (2,)), ("offsets", "<i4", (10,))])   # kvz_hip_sao_info


def lcu_count(width, height):
    return ((width + 63) // 64) * ((height + 63) // 64)


def _stage_planes(planes, chroma):
    st = [_Staged(p) for p in planes[:3 if chroma else 1]]
    assert not chroma or (st[1].stride == st[2].stride and (st[1].w, st[1].h) == (st[2].w, st[2].h) == (st[0].w // 2, st[0].h // 2))
    return st


def sao_stats_frame(src, rec, chroma=1, with_cands=True):
    """kvz_hip_sao_stats_frame.  src, rec: (y, u, v) uint8 planes or PlaneViews of the source and the deblocked picture (u, v None
    for 4:0:0; u and v share one stride).  Returns (stats, cands): SAO_LCU_STATS / SAO_LCU_CAND records [planes, LCUs] (cands None
    without with_cands)."""
    L = _lib.init()
    chroma = int(chroma)
    s, r = _stage_planes(src, chroma), _stage_planes(rec, chroma)
    w, h = s[0].w, s[0].h
    assert (r[0].w, r[0].h) == (w, h)
    table = ref_picture_table([(s[0].ptr, s[1].ptr if chroma else 0, s[2].ptr if chroma else 0, s[0].stride, s[1].stride if chroma else 0)], w, h)
    n = (3 if chroma else 1) * lcu_count(w, h)
    ds = DeviceBuffer(n * SAO_LCU_STATS.itemsize)
    dc = DeviceBuffer(n * SAO_LCU_CAND.itemsize) if with_cands else None
    check(L.kvz_hip_sao_stats_frame(table.ctypes.data, r[0].ptr, r[0].stride, r[1].ptr if chroma else None, r[2].ptr if chroma else None,
                                    r[1].stride if chroma else 0, chroma, ds.ptr, dc.ptr if dc else None, None), "sao_stats_frame")
    shape = (3 if chroma else 1, n // (3 if chroma else 1))
    stats = ds.to_numpy(np.uint8, (n * SAO_LCU_STATS.itemsize,)).view(SAO_LCU_STATS).reshape(shape)
    cands = dc.to_numpy(np.uint8, (n * SAO_LCU_CAND.itemsize,)).view(SAO_LCU_CAND).reshape(shape) if dc else None
    return stats, cands


def sao_frame(rec, sao_luma, sao_chroma=None, chroma=1, dst=None, tiles=None):
    """kvz_hip_sao_frame.  rec: (y, u, v) uint8 planes or PlaneViews of the deblocked picture; sao_luma / sao_chroma: int32
    [LCUs, 14] or SAO_INFO records in raster order; dst: the initial destination planes (arrays or PlaneViews of the picture's
    size; default zeros).  Returns the destination (y, u, v) after the call (the whole buffer of a PlaneView).  tiles: a TILE_GRID
    record -> kvz_hip_sao_frame_tiles."""
    L = _lib.init()
    chroma = int(chroma)
    r = _stage_planes(rec, chroma)
    w, h = r[0].w, r[0].h
    if dst is None:
        dst = [np.zeros((h >> (1 if k else 0), w >> (1 if k else 0)), np.uint8) for k in range(3)]
    d = _stage_planes(dst, chroma)
    assert (d[0].w, d[0].h) == (w, h)
    n = lcu_count(w, h)
    infos = [np.ascontiguousarray(a).view(np.int32).reshape(n, 14) if a is not None and np.asarray(a).dtype == SAO_INFO
             else (np.ascontiguousarray(a, dtype=np.int32).reshape(n, 14) if a is not None else None) for a in (sao_luma, sao_chroma)]
    di = [DeviceBuffer.from_numpy(a) if a is not None else None for a in infos]
    args = (r[0].ptr, r[0].stride, r[1].ptr if chroma else None, r[2].ptr if chroma else None, r[1].stride if chroma else 0,
            d[0].ptr, d[0].stride, d[1].ptr if chroma else None, d[2].ptr if chroma else None, d[1].stride if chroma else 0,
            w, h, di[0].ptr, di[1].ptr if di[1] else None, chroma)
    if tiles is None:
        check(L.kvz_hip_sao_frame(*args, None), "sao_frame")
    else:
        g = _grid(tiles)
        check(L.kvz_hip_sao_frame_tiles(*args, g.ctypes.data, None), "sao_frame_tiles")
    out = [p.download() for p in d]
    return tuple(out + [None] * (3 - len(out)))


# ---- several independent pictures through the QP map, deblocking and SAO in one call each ----
def cu_qp_frames(pictures):
    """kvz_hip_cu_qp_frames.  pictures: a list of up to MAX_CHAIN_PICTURES dicts, each with the arguments of cu_qp_frame_tiles by name
    (cus, cbf, lcu_qp, start_qp; optional tiles, chain_rows).  Returns the list of cu_qp_frame_tiles' results, one per picture."""
    return _filter_frames("kvz_hip_cu_qp_frames", [_FilterPicture.cu_qp(**p) for p in pictures])


def deblock_frames(pictures):
    """kvz_hip_deblock_frames.  pictures: a list of up to MAX_CHAIN_PICTURES dicts, each with the arguments of deblock_frame by name
    (y, u, v, cus, prm; optional tiles).  Returns the list of deblock_frame's results, one per picture."""
    return _filter_frames("kvz_hip_deblock_frames", [_FilterPicture.deblock(**p) for p in pictures])


def sao_stats_frames(pictures):
    """kvz_hip_sao_stats_frames.  pictures: a list of up to MAX_CHAIN_PICTURES dicts, each with the arguments of sao_stats_frame by name
    (src, rec; optional chroma, with_cands).  Returns the list of sao_stats_frame's results, one per picture."""
    return _filter_frames("kvz_hip_sao_stats_frames", [_FilterPicture.sao_stats(**p) for p in pictures])


def sao_frames(pictures):
    """kvz_hip_sao_frames.  pictures: a list of up to MAX_CHAIN_PICTURES dicts, each with the arguments of sao_frame by name (rec,
    sao_luma; optional sao_chroma, chroma, dst, tiles).  Returns the list of sao_frame's results, one per picture."""
    return _filter_frames("kvz_hip_sao_frames", [_FilterPicture.sao(**p) for p in pictures])


class _FilterPicture:
    """the arrays of one picture of kvz_hip_cu_qp_frames / _deblock_frames / _sao_stats_frames / _sao_frames on the device, the record
    with the fields its entry reads, and how the entry's outputs come back"""

    def __init__(self, width, height, chroma, tiles=None):
        self.keep = []
        self.record = rec = _lib.FilterPicture()
        rec.width, rec.height, rec.chroma = width, height, int(chroma)
        rec.deblock.chroma = int(chroma)
        if tiles is not None:
            self.grid = _lib.TileGrid.from_buffer_copy(_grid(tiles).tobytes())
            rec.grid = C.pointer(self.grid)

    def _rec_planes(self, planes, chroma):
        r = _stage_planes(planes, chroma)
        rec = self.record
        rec.rec_y, rec.stride_y = r[0].ptr, r[0].stride
        if chroma:
            rec.rec_u, rec.rec_v, rec.stride_c = r[1].ptr, r[2].ptr, r[1].stride
        return r

    def _cus(self, cus):
        cus = np.ascontiguousarray(cus)
        assert cus.dtype.itemsize == 20 and cus.ndim == 2
        dcu = DeviceBuffer.from_numpy(cus.view(np.uint8))
        self.record.cus = dcu.ptr
        return cus, dcu

    @classmethod
    def cu_qp(cls, cus, cbf, lcu_qp, start_qp, tiles=None, chain_rows=0):
        cus = np.ascontiguousarray(cus)
        height, width = 4 * cus.shape[0], 4 * cus.shape[1]
        self = cls(width, height, 1, tiles)
        cus, dcu = self._cus(cus)
        n = lcu_count(width, height)
        dcb = DeviceBuffer.from_numpy(np.ascontiguousarray(cbf, dtype=np.uint8).reshape(cus.shape))
        dq, dl = DeviceBuffer.from_numpy(np.ascontiguousarray(lcu_qp, dtype=np.int8).reshape(n)), DeviceBuffer(n)
        rec = self.record
        rec.cbf, rec.lcu_qp, rec.lcu_last_qp = dcb.ptr, dq.ptr, dl.ptr
        rec.cu_qp = _lib.CuQpTilesParams(int(start_qp), int(chain_rows))
        self.keep += [dcb, dq]
        self.result = lambda: (dcu.to_numpy(np.uint8, cus.shape + (20,)).view(cus.dtype).reshape(cus.shape), dl.to_numpy(np.int8, (n,)))
        return self

    @classmethod
    def deblock(cls, y, u, v, cus, prm, tiles=None):
        prm = np.ascontiguousarray(prm)
        assert prm.nbytes == 64
        params = _lib.DeblockParams.from_buffer_copy(prm.tobytes())
        chroma = 1 if params.chroma else 0
        h, w = (y.height, y.width) if isinstance(y, PlaneView) else np.asarray(y).shape
        self = cls(w, h, params.chroma, tiles)
        planes = self._rec_planes((y, u, v), chroma)
        self.record.deblock = params
        self.keep.append(self._cus(cus)[1])
        self.result = lambda: tuple([p.download() for p in planes] + [None] * (3 - len(planes)))
        return self

    @classmethod
    def sao_stats(cls, src, rec, chroma=1, with_cands=True):
        chroma = int(chroma)
        s = _stage_planes(src, chroma)
        w, h = s[0].w, s[0].h
        self = cls(w, h, chroma)
        r = self._rec_planes(rec, chroma)
        assert (r[0].w, r[0].h) == (w, h)
        self.record.src = _lib.RefPicture(s[0].ptr, s[1].ptr if chroma else None, s[2].ptr if chroma else None, s[0].stride,
                                          s[1].stride if chroma else 0, w, h)
        planes = 3 if chroma else 1
        n = planes * lcu_count(w, h)
        ds = DeviceBuffer(n * SAO_LCU_STATS.itemsize)
        dc = DeviceBuffer(n * SAO_LCU_CAND.itemsize) if with_cands else None
        self.record.stats, self.record.cands = ds.ptr, dc.ptr if dc else None
        self.keep += [s, r]
        shape = (planes, n // planes)
        self.result = lambda: (ds.to_numpy(np.uint8, (n * SAO_LCU_STATS.itemsize,)).view(SAO_LCU_STATS).reshape(shape),
                               dc.to_numpy(np.uint8, (n * SAO_LCU_CAND.itemsize,)).view(SAO_LCU_CAND).reshape(shape) if dc else None)
        return self

    @classmethod
    def sao(cls, rec, sao_luma, sao_chroma=None, chroma=1, dst=None, tiles=None):
        chroma = int(chroma)
        first = rec[0]
        h, w = (first.height, first.width) if isinstance(first, PlaneView) else np.asarray(first).shape
        self = cls(w, h, chroma, tiles)
        self.keep.append(self._rec_planes(rec, chroma))
        if dst is None:
            dst = [np.zeros((h >> (1 if k else 0), w >> (1 if k else 0)), np.uint8) for k in range(3)]
        d = _stage_planes(dst, chroma)
        assert (d[0].w, d[0].h) == (w, h)
        n = lcu_count(w, h)
        infos = [np.ascontiguousarray(a).view(np.int32).reshape(n, 14) if a is not None and np.asarray(a).dtype == SAO_INFO
                 else (np.ascontiguousarray(a, dtype=np.int32).reshape(n, 14) if a is not None else None) for a in (sao_luma, sao_chroma)]
        di = [DeviceBuffer.from_numpy(a) if a is not None else None for a in infos]
        rc = self.record
        rc.dst_y, rc.dst_stride_y = d[0].ptr, d[0].stride
        if chroma:
            rc.dst_u, rc.dst_v, rc.dst_stride_c = d[1].ptr, d[2].ptr, d[1].stride
        rc.sao_luma, rc.sao_chroma = di[0].ptr, di[1].ptr if di[1] else None
        self.keep += [di]
        self.result = lambda: tuple([p.download() for p in d] + [None] * (3 - len(d)))
        return self


def _filter_frames(entry, staged):
    L = _lib.init()
    records = (_lib.FilterPicture * max(len(staged), 1))(*[st.record for st in staged])
    check(getattr(L, entry)(records, len(staged), None), entry[len("kvz_hip_"):])
    return [st.result() for st in staged]


# ---- the last stage of the chain: the SEI checksum and the squared error of a reconstructed picture; array_checksum of planes ----
LCU_HASH = np.dtype([("checksum", "<u4", (3,)), ("sse", "<u4", (3,))])                            # kvz_hip_lcu_hash
PICTURE_HASH = np.dtype([("checksum", "<u4", (3,)), ("n_lcu", "<u4"), ("sse", "<u8", (3,))])      # kvz_hip_picture_hash


class _HashPicture:
    """the planes of one picture of kvz_hip_picture_hash_frame(s) on the device, its kvz_hip_hash_picture record with output arrays of
    its own, and how the outputs come back.  fill: the byte that the output arrays hold before the call."""

    def __init__(self, rec, src=None, chroma=1, fill=0):
        chroma = int(chroma)
        r = _stage_planes(rec, chroma)
        w, h = r[0].w, r[0].h
        self.record = p = _lib.HashPicture()
        p.width, p.height, p.chroma = w, h, chroma
        p.rec_y, p.stride_y = r[0].ptr, r[0].stride
        if chroma:
            p.rec_u, p.rec_v, p.stride_c = r[1].ptr, r[2].ptr, r[1].stride
        self.keep = [r]
        if src is not None:
            s = _stage_planes(src, chroma)
            assert (s[0].w, s[0].h) == (w, h)
            p.src = _lib.RefPicture(s[0].ptr, s[1].ptr if chroma else None, s[2].ptr if chroma else None, s[0].stride,
                                    s[1].stride if chroma else 0, w, h)
            self.keep.append(s)
        self.n_lcu = lcu_count(w, h)
        self.lcu_out = DeviceBuffer.from_numpy(np.full(self.n_lcu * LCU_HASH.itemsize, fill, np.uint8))
        self.out = DeviceBuffer.from_numpy(np.full(PICTURE_HASH.itemsize, fill, np.uint8))
        p.lcu_out, p.out = self.lcu_out.ptr, self.out.ptr

    def call_single(self, L, stream=None):
        """kvz_hip_picture_hash_frame with the record's fields -> its return code"""
        p = self.record
        return L.kvz_hip_picture_hash_frame(C.byref(p.src) if p.src.y else None, p.rec_y, p.stride_y, p.rec_u, p.rec_v, p.stride_c, p.width, p.height,
                                            p.chroma, p.lcu_out, p.out, stream)

    def result(self):
        """(LCU_HASH records [LCUs], the PICTURE_HASH record)"""
        return (self.lcu_out.to_numpy(np.uint8, (self.n_lcu * LCU_HASH.itemsize,)).view(LCU_HASH),
                self.out.to_numpy(np.uint8, (PICTURE_HASH.itemsize,)).view(PICTURE_HASH)[0])


def picture_hash_frame(rec, src=None, chroma=1):
    """kvz_hip_picture_hash_frame.  rec, src: (y, u, v) uint8 planes or PlaneViews of the reconstruction and of the source (u, v None
    for 4:0:0; u and v share one stride); src None: checksum only.  Returns (lcu, picture): LCU_HASH records in raster order over the
    LCUs and the PICTURE_HASH record."""
    L = _lib.init()
    st = _HashPicture(rec, src, chroma)
    check(st.call_single(L), "picture_hash_frame")
    return st.result()


def picture_hash_frames(pictures):
    """kvz_hip_picture_hash_frames.  pictures: a list of up to MAX_CHAIN_PICTURES dicts, each with the arguments of picture_hash_frame
    by name (rec; optional src, chroma).  Returns the list of picture_hash_frame's results, one per picture."""
    L = _lib.init()
    staged = [_HashPicture(**p) for p in pictures]
    records = (_lib.HashPicture * max(len(staged), 1))(*[st.record for st in staged])
    check(L.kvz_hip_picture_hash_frames(records, len(staged), None), "picture_hash_frames")
    return [st.result() for st in staged]


def array_checksum_batch(planes):
    """kvz_hip_array_checksum_batch.  planes: up to MAX_HASH_PLANES uint8 planes or PlaneViews (any size, stride and offset).  Returns
    the checksums, uint32 [planes]."""
    L = _lib.init()
    st = [_Staged(p) for p in planes]
    records = (_lib.HashPlane * max(len(st), 1))(*[_lib.HashPlane(p.ptr, p.w, p.h, p.stride, 0) for p in st])
    blocks = sum(L.kvz_hip_array_checksum_blocks(p.w, p.h) for p in st)
    scratch, out = DeviceBuffer(4 * blocks), DeviceBuffer(4 * len(st))
    check(L.kvz_hip_array_checksum_batch(records, len(st), scratch.ptr, out.ptr, None), "array_checksum_batch")
    return out.to_numpy(np.uint32, (len(st),))


# ---- coefficient pricing with CABAC ----
COEFF_CTX = np.dtype([("range", "<u2"), ("reserved", "<u2"), ("ctx", "u1", (140,))])              # kvz_hip_coeff_ctx
COEFF_COST_DESC = np.dtype([("offset", "<u4"), ("width", "u1"), ("type", "u1"), ("scan_mode", "u1"), ("tr_skip", "u1"),
                            ("ctx_index", "<u4")])                                                # kvz_hip_coeff_cost_desc
CABAC_CTX_BYTES = 184        # sizeof cabac_data_t.ctx (cabac.h:53-87)


def coeff_ctx_from_dump(ctx184, cabac_range):
    """A kvz_hip_coeff_ctx record cut from a dump of the reference's context block: the 184 bytes of cabac_data_t.ctx and
    cabac.range.  Bytes 32..167 (cu_sig_coeff_group_model[0] .. cu_abs_model_chroma[1]) become ctx[0..135], bytes 182 / 183
    (transform_skip_model_luma / _chroma) ctx[136] / ctx[137]."""
    d = np.frombuffer(bytes(bytearray(ctx184)), dtype=np.uint8)
    if d.size != CABAC_CTX_BYTES:
        raise ValueError("a context dump is %d bytes, not %d" % (CABAC_CTX_BYTES, d.size))
    if not 256 <= int(cabac_range) <= 510:
        raise ValueError("cabac.range lies in 256..510")
    rec = np.zeros((), dtype=COEFF_CTX)
    rec["range"] = int(cabac_range)
    rec["ctx"][:136] = d[32:168]
    rec["ctx"][136:138] = d[182:184]
    return rec


def coeff_cost_batch(coeffs, descs, ctx_sets, signhide=1, trskip_enable=1, lossless=0, bits=None):
    """kvz_hip_coeff_cost_batch.  coeffs: int16 array holding the TUs; descs [n] COEFF_COST_DESC; ctx_sets [m] COEFF_CTX.
    bits: what bits_out holds before the call (a skipped descriptor keeps its value), zeros by default.  Returns uint32 [n]."""
    L = _lib.init()
    coeffs = np.ascontiguousarray(coeffs, dtype=np.int16).ravel()
    descs = np.ascontiguousarray(descs, dtype=COEFF_COST_DESC)
    ctx_sets = np.ascontiguousarray(ctx_sets, dtype=COEFF_CTX).ravel()
    n = len(descs)
    bits = np.zeros(n, dtype=np.uint32) if bits is None else np.ascontiguousarray(bits, dtype=np.uint32)
    assert bits.shape == (n,)
    d_c, d_d, d_s, d_b = (DeviceBuffer.from_numpy(a) for a in (coeffs, descs, ctx_sets, bits))
    prm = _lib.CoeffCostParams(int(signhide), int(trskip_enable), int(lossless), 0)
    check(L.kvz_hip_coeff_cost_batch(d_c.ptr, d_d.ptr, n, d_s.ptr, len(ctx_sets), C.byref(prm), d_b.ptr, None), "coeff_cost_batch")
    return d_b.to_numpy(np.uint32, (n,))


# ---- rate-distortion optimised quantisation ----
RDOQ_STATE = np.dtype([("lambda", "<f8"), ("qp", "i1"), ("root_cbf", "u1"), ("qt_cbf_luma", "u1", (4,)), ("qt_cbf_chroma", "u1", (4,)),
                       ("reserved", "u1", (6,))])                                                   # kvz_hip_rdoq_state
RDOQ_DESC = np.dtype([("src_offset", "<u4"), ("dst_offset", "<u4"), ("width", "u1"), ("type", "u1"), ("scan_mode", "u1"), ("block_type", "u1"),
                      ("tr_depth", "u1"), ("reserved", "u1"), ("ctx_index", "<u2")])              # kvz_hip_rdoq_desc
CU_INTRA, CU_INTER = 1, 2    # cu.h:39-41: kvz_hip_rdoq_desc.block_type


def rdoq_state_from_dump(ctx184, lam, qp):
    """A kvz_hip_rdoq_state record cut from a dump of the reference's context block (the 184 bytes of cabac_data_t.ctx) plus
    state->lambda and state->qp: bytes 16..19 (qt_cbf_model_luma) and 20..23 (qt_cbf_model_chroma) and byte 181 (cu_qt_root_cbf_model).
    coeff_ctx_from_dump cuts the kvz_hip_coeff_ctx record of the same index from the same dump."""
    d = np.frombuffer(bytes(bytearray(ctx184)), dtype=np.uint8)
    if d.size != CABAC_CTX_BYTES:
        raise ValueError("a context dump is %d bytes, not %d" % (CABAC_CTX_BYTES, d.size))
    if not 0 <= int(qp) <= 51:
        raise ValueError("state->qp lies in 0..51")
    rec = np.zeros((), dtype=RDOQ_STATE)
    rec["lambda"], rec["qp"], rec["root_cbf"] = float(lam), int(qp), d[181]
    rec["qt_cbf_luma"], rec["qt_cbf_chroma"] = d[16:20], d[20:24]
    return rec


def pack_rdoq_tables(quant, error_scale):
    """kvz_hip_rdoq_tables_pack.  quant (int32) and error_scale (float64): [size_id][list][rem] -> N*N values (nested sequences or dicts
    keyed (size_id, list, rem)), as scaling_list_t holds them after kvz_scalinglist_process; of the 32x32 lists only 0, 1 and 3 are read.
    -> (quant int32, err_scale float64): two arrays of SL_TABLE_LEN values.  Needs no device."""
    L = _lib.load()
    keep, ptrs = [], []
    for src, dt in ((quant, np.int32), (error_scale, np.float64)):
        p = (C.c_void_p * 6 * 6 * 4)()
        for size_id in range(4):
            for list_id in range(6):
                for rem in range(6):
                    try:
                        t = src[(size_id, list_id, rem)] if isinstance(src, dict) else src[size_id][list_id][rem]
                    except (KeyError, IndexError):
                        t = None
                    if t is None:
                        continue
                    a = np.ascontiguousarray(t, dtype=dt).reshape(-1)
                    assert a.size == 16 << (2 * size_id)
                    keep.append(a)
                    p[size_id][list_id][rem] = a.ctypes.data
        ptrs.append(p)
    out = np.zeros(SL_TABLE_LEN, np.int32), np.zeros(SL_TABLE_LEN, np.float64)
    check(L.kvz_hip_rdoq_tables_pack(C.addressof(ptrs[0]), C.addressof(ptrs[1]), out[0].ctypes.data, out[1].ctypes.data), "rdoq_tables_pack")
    return out


def rdoq_batch(coef, descs, ctx_sets, states, tables, signhide=1, dest=None):
    """kvz_hip_rdoq_batch.  coef: int16 array holding the TUs; descs [n] RDOQ_DESC; ctx_sets [m] COEFF_CTX and states [m] RDOQ_STATE, index-
    parallel; tables = (quant int32, err_scale float64), the packed arrays of pack_rdoq_tables.  dest: what the destination array holds
    before the call (a skipped descriptor keeps its values), zeros of coef's size by default.  Returns the destination array, int16."""
    L = _lib.init()
    coef = np.ascontiguousarray(coef, dtype=np.int16).ravel()
    descs = np.ascontiguousarray(descs, dtype=RDOQ_DESC)
    ctx_sets = np.ascontiguousarray(ctx_sets, dtype=COEFF_CTX).ravel()
    states = np.ascontiguousarray(states, dtype=RDOQ_STATE).ravel()
    assert len(states) == len(ctx_sets)
    quant = np.ascontiguousarray(tables[0], dtype=np.int32).ravel()
    err = np.ascontiguousarray(tables[1], dtype=np.float64).ravel()
    assert quant.size == SL_TABLE_LEN and err.size == SL_TABLE_LEN
    dest = np.zeros(coef.size, dtype=np.int16) if dest is None else np.ascontiguousarray(dest, dtype=np.int16).ravel()
    d_c, d_o, d_d, d_s, d_t, d_q, d_e = (DeviceBuffer.from_numpy(a) for a in (coef, dest, descs, ctx_sets, states, quant, err))
    tab = _lib.RdoqTables(d_q.ptr, d_e.ptr)
    prm = _lib.RdoqParams(int(signhide))
    check(L.kvz_hip_rdoq_batch(d_c.ptr, d_o.ptr, d_d.ptr, len(descs), d_s.ptr, d_t.ptr, len(ctx_sets), C.byref(tab), C.byref(prm), None), "rdoq_batch")
    return d_o.to_numpy(np.int16, (dest.size,))


# ---- tile halo exchange: batched rectangle copies on device pointers ----
def copy_rects(rects, stream=None):
    """kvz_hip_copy_rects_batch: rects = [(src, dst, src_stride, dst_stride, w, h)] with device pointers (ints), at most
    _lib.MAX_RECTS of them, copied by one launch on `stream` (a kvz_hip_stream / hipStream_t handle, None = the library's)."""
    L = _lib.init()
    rects = list(rects)
    arr = (_lib.RectCopy * max(1, len(rects)))(*[_lib.RectCopy(*r) for r in rects])
    check(L.kvz_hip_copy_rects_batch(arr, len(rects), stream), "copy_rects_batch")


def tile_plane(ext_ptr, device, stride, ext_rect, own_rect):
    """a kvz_hip_tile_plane record: ext_rect / own_rect = (x, y, w, h) in frame coordinates (TileShard.ext / .own)"""
    return _lib.TilePlane(ext_ptr, device, stride, *(tuple(ext_rect) + tuple(own_rect)))


def tile_halo_exchange(self_plane, neighbours, stream=None):
    """kvz_hip_tile_halo_exchange: self_plane pushes its pixels into the extended buffers of `neighbours` (TilePlane records) in one
    launch on `stream` of self_plane.device (the calling thread must work on it)."""
    L = _lib.load()
    nbs = list(neighbours)
    arr = (_lib.TilePlane * max(1, len(nbs)))(*nbs)
    check(L.kvz_hip_tile_halo_exchange(C.byref(self_plane), arr if nbs else None, len(nbs), stream), "tile_halo_exchange")


# ---- search service: requests of many host threads in shared launches (include/kvz_hip.h, "search service") ----
class MeService:
    """kvz_hip_me_service: resident luma planes in numbered slots + kvz_hip_me_service_search, callable from many threads."""

    def __init__(self, width, height, max_pictures=8, max_threads=64):
        self.lib = _lib.init()
        cfg = np.zeros(8, dtype=np.int32)
        cfg[:4] = (width, height, max_pictures, max_threads)
        self.w, self.h = int(width), int(height)
        self.ptr = self.lib.kvz_hip_me_service_create(cfg.ctypes.data)
        if not self.ptr:
            raise KvzHipError("kvz_hip_me_service_create failed: %s" % self.lib.kvz_hip_last_error().decode())

    def put_plane(self, slot, plane):
        plane = np.ascontiguousarray(plane, dtype=np.uint8)
        assert plane.shape == (self.h, self.w)
        check(self.lib.kvz_hip_me_service_put_rect(self.ptr, slot, plane.ctypes.data, self.w, 0, 0, self.w, self.h), "me_service_put_rect")

    def put_rect(self, slot, plane, x, y, w, h):
        """rectangle (x, y, w, h) of a full host plane"""
        plane = np.ascontiguousarray(plane, dtype=np.uint8)
        check(self.lib.kvz_hip_me_service_put_rect(self.ptr, slot, plane.ctypes.data + y * plane.shape[1] + x, plane.shape[1], x, y, w, h),
              "me_service_put_rect")

    def search(self, request):
        """request: one record laid out as kvz_hip_me_request (1200 bytes).  Returns int32 [n_refs, 8] (= kvz_hip_me_result)."""
        request = np.ascontiguousarray(request)
        assert request.nbytes == 1200
        n = int(request.view(np.int32).reshape(-1)[1])
        out = np.zeros((max(n, 1), 8), dtype=np.int32)
        check(self.lib.kvz_hip_me_service_search(self.ptr, request.ctypes.data, out.ctypes.data), "me_service_search")
        return out[:n]

    def stats(self):
        s = np.zeros(11, dtype=np.uint64)
        check(self.lib.kvz_hip_me_service_get_stats(self.ptr, s.ctypes.data), "me_service_get_stats")
        return dict(zip(("requests", "units", "batches", "launches", "max_batch_units", "rects", "rect_bytes", "wait_ns", "tables", "table_bytes", "table_ns"),
                        (int(v) for v in s)))

    def sad_tables(self, pic_slot, ref_slots, ctu_x, ctu_y, rng):
        """kvz_hip_me_service_sad_tables -> uint32 [n_refs, 2 rng + 1 (dy), 2 rng + 1 (dx), 85] (a copy of the thread's table)"""
        import ctypes as C
        refs = np.ascontiguousarray(ref_slots, dtype=np.int32)
        p = self.lib.kvz_hip_me_service_sad_tables(self.ptr, pic_slot, len(refs), refs.ctypes.data, ctu_x, ctu_y, rng)
        if not p:
            raise KvzHipError("kvz_hip_me_service_sad_tables failed: %s" % self.lib.kvz_hip_last_error().decode())
        side = 2 * rng + 1
        n = len(refs) * side * side * 85
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint32)), shape=(n,)).reshape(len(refs), side, side, 85).copy()

    def close(self):
        if self.ptr:
            self.lib.kvz_hip_me_service_destroy(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
