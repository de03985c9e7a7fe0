"""The rule of the decoded-picture-hash checksum and of the per-plane squared error in plain numpy, with a list of deliberate errors.

  checksum = ( sum over y, x of  data[y * stride + x] ^ mask(x, y) )  mod 2^32
  mask(x, y) = ((x & 255) ^ (y & 255) ^ (x >> 8) ^ (y >> 8)) & 255          (nal-generic.c:45-69)
  the SEI carries the 32 bits big-endian; sse = sum of (src - rec)^2 as an exact integer.

A plane is a 2-D uint8 buffer whose row length is the stride; the plane is buf[:height, :width].  A Rule without arguments is the
rule; Rule(fault) is the rule with one of FAULTS planted, which tests/test_picture_hash_model.py shows to be noticed by at least one
case of tests/picture_hash_cases.py.  TEST INFRASTRUCTURE."""
import numpy as np

LCU_HASH = np.dtype([("checksum", "<u4", (3,)), ("sse", "<u4", (3,))])                            # kvz_hip_lcu_hash
PICTURE_HASH = np.dtype([("checksum", "<u4", (3,)), ("n_lcu", "<u4"), ("sse", "<u8", (3,))])      # kvz_hip_picture_hash

FAULTS = ("x_hi_dropped",            # x >> 8 left out of the mask
          "y_hi_dropped",            # y >> 8 left out of the mask
          "mask_not_cut",            # x ^ y ^ (x >> 8) ^ (y >> 8) without the cut to 8 bits
          "stride_as_width",         # the sum runs over stride columns
          "width_as_stride",         # the rows are taken width bytes apart
          "luma_coords_for_chroma",  # a chroma pixel masked with the luma position 2x, 2y
          "chroma_rounded_up",       # chroma planes of (w + 1) / 2 x (h + 1) / 2
          "saturating_sum",          # the sum stops at 2^32 - 1
          "little_endian",           # the SEI bytes in the host's order
          "sse_in_32_bits")          # the picture's sse wraps at 2^32


class Rule:
    def __init__(self, fault=None):
        assert fault is None or fault in FAULTS
        self.fault = fault

    def mask(self, width, height, x0=0, y0=0, scale=1):
        """int64 [height, width]: the masks of the pixels (x0 + x, y0 + y)"""
        yy, xx = np.mgrid[y0:y0 + height, x0:x0 + width].astype(np.int64) * scale
        m = xx ^ yy
        if self.fault != "x_hi_dropped":
            m = m ^ (xx >> 8)
        if self.fault != "y_hi_dropped":
            m = m ^ (yy >> 8)
        return m if self.fault == "mask_not_cut" else m & 255

    def pixels(self, buf, width, height):
        """the plane's pixels as the rule reads them, int64 [height, width']"""
        buf = np.asarray(buf, dtype=np.uint8)
        if self.fault == "stride_as_width":
            width = buf.shape[1]
        if self.fault == "width_as_stride":
            return buf.reshape(-1)[:width * height].reshape(height, width).astype(np.int64)
        return buf[:height, :width].astype(np.int64)

    def wrap(self, total):
        total = int(total)
        return min(total, 2 ** 32 - 1) if self.fault == "saturating_sum" else total % 2 ** 32

    def block_sum(self, buf, width, height, x, y, w, h, scale=1):
        """the exact share of the rectangle (x, y, w, h) in the plane's sum, before any wrapping"""
        p = self.pixels(buf, width, height)[y:y + h, x:x + w]
        return int((p ^ self.mask(p.shape[1], p.shape[0], x, y, scale)).sum())

    def plane_checksum(self, buf, width, height, scale=1):
        p = self.pixels(buf, width, height)
        return self.wrap(self.block_sum(buf, width, height, 0, 0, p.shape[1], p.shape[0], scale))

    def sei_bytes(self, checksum):
        return int(checksum).to_bytes(4, "little" if self.fault == "little_endian" else "big")

    def chroma_size(self, width, height):
        return ((width + 1) >> 1, (height + 1) >> 1) if self.fault == "chroma_rounded_up" else (width >> 1, height >> 1)

    def picture(self, rec, src, width, height, chroma):
        """rec, src: (y, u, v) buffers (u, v unused for 4:0:0; src None: checksum only) -> (LCU_HASH [LCUs] in raster order, PICTURE_HASH)"""
        nx, ny = (width + 63) // 64, (height + 63) // 64
        lcus = np.zeros(nx * ny, dtype=LCU_HASH)
        pic = np.zeros((), dtype=PICTURE_HASH)
        pic["n_lcu"] = nx * ny
        for c in range(3 if chroma else 1):
            (pw, ph), bs = ((width, height), 64) if c == 0 else (self.chroma_size(width, height), 32)
            scale = 2 if c and self.fault == "luma_coords_for_chroma" else 1
            total, sse = 0, 0
            for ly in range(ny):
                for lx in range(nx):
                    x, y = lx * bs, ly * bs
                    w, h = max(min(bs, pw - x), 0), max(min(bs, ph - y), 0)
                    s = self.block_sum(rec[c], pw, ph, x, y, w, h, scale)
                    lcus[ly * nx + lx]["checksum"][c] = s
                    total += s
                    if src is not None:
                        d = self.pixels(src[c], pw, ph)[y:y + h, x:x + w] - self.pixels(rec[c], pw, ph)[y:y + h, x:x + w]
                        e = int((d * d).sum())
                        lcus[ly * nx + lx]["sse"][c] = e
                        sse += e
            pic["checksum"][c] = self.wrap(total)
            pic["sse"][c] = sse % 2 ** 32 if self.fault == "sse_in_32_bits" else sse
        return lcus, pic


RULE = Rule()


def plane_checksum(buf, width, height):
    return RULE.plane_checksum(buf, width, height)


def plane_sse(a, b, width, height):
    d = np.asarray(a)[:height, :width].astype(np.int64) - np.asarray(b)[:height, :width].astype(np.int64)
    return int((d * d).sum())


def picture(rec, src, width, height, chroma):
    return RULE.picture(rec, src, width, height, chroma)
