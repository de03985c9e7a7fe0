"""The seeded inputs of the picture-hash tests: planes for kvz_hip_array_checksum_batch and the array_checksum strategy, pictures for
kvz_hip_picture_hash_frame(s).  Everything is regenerated from seeds (the wrap plane from a formula); tests/golden/picture_hash.npz
holds only the reference's results for them.  TEST INFRASTRUCTURE."""
import numpy as np

import picture_hash_model as M

# (name, width, height, stride): sizes below, at and across the 8-pixel and 256-pixel periods of the mask, odd sizes, padded strides
PLANES = (("1x1", 1, 1, 1), ("13x7", 13, 7, 29), ("8x8", 8, 8, 8), ("264x264", 264, 264, 272), ("528x264", 528, 264, 528),
          ("260x260", 260, 260, 300), ("520x520", 520, 520, 520))
WRAP = ("wrap", 4352, 4096, 4352)             # data = 255 ^ mask: every pixel adds 255 and the sum passes 2^32
WRAP_CHECKSUM = 250609664                     # (255 * 4352 * 4096) mod 2^32


def plane(name):
    """-> (buf uint8 [height, stride], width, height): the plane is buf[:, :width], the bytes right of it are random as well"""
    if name == "wrap":
        _, w, h, s = WRAP
        return (255 ^ M.RULE.mask(w, h)).astype(np.uint8), w, h
    i = [p[0] for p in PLANES].index(name)
    _, w, h, s = PLANES[i]
    return np.random.default_rng(4100 + i).integers(0, 256, (h, s), dtype=np.uint8), w, h


# (name, width, height): one LCU, ragged LCUs, chroma across x = 256, chroma across 256 both ways; each in 4:2:0 and 4:0:0
PICTURE_SIZES = (("8x8", 8, 8), ("72x40", 72, 40), ("528x264", 528, 264), ("520x520", 520, 520))
PICTURES = tuple((n + ("" if c else "_mono"), w, h, c) for (n, w, h) in PICTURE_SIZES for c in (1, 0))
EXTREME = ("520x520_extreme", 520, 520, 1)    # source 0 against reconstruction 255: a picture sse of 1.76e10, beyond 32 bits
PAD_ROWS = 2                                  # rows below the picture, never to be read


def strides(width, kind):
    """padded and unequal: luma and chroma, source and reconstruction each get a stride of their own (multiples of 4)"""
    return {"rec": (width + 24, width // 2 + 12), "src": (width + 8, width // 2 + 20)}[kind]


def picture(name):
    """-> (rec, src, width, height, chroma): rec, src = (y, u, v) buffers [rows + PAD_ROWS, stride] (u, v None for 4:0:0), the planes in
    their top left corners, everything around them random"""
    every = PICTURES + (EXTREME,)
    i = [p[0] for p in every].index(name)
    _, w, h, chroma = every[i]
    g = np.random.default_rng(4200 + i)
    out = {}
    for kind in ("src", "rec"):
        sy, sc = strides(w, kind)
        planes = []
        for k in range(3 if chroma else 1):
            pw, ph, s = (w, h, sy) if k == 0 else (w // 2, h // 2, sc)
            buf = g.integers(0, 256, (ph + PAD_ROWS, s), dtype=np.uint8)
            if name == EXTREME[0]:
                buf[:ph, :pw] = 0 if kind == "src" else 255
            elif kind == "rec":
                # coding-like noise on the source, so that the squared error is not that of two unrelated pictures
                noise = g.integers(-6, 7, (ph, pw))
                buf[:ph, :pw] = np.clip(out["src"][k][:ph, :pw].astype(np.int64) + noise, 0, 255)
            planes.append(buf)
        out[kind] = tuple(planes + [None] * (3 - len(planes)))
    return out["rec"], out["src"], w, h, chroma


def repoison(planes, width, height, chroma, seed):
    """copies of the buffers with everything right of the width and below the height replaced"""
    g = np.random.default_rng(seed)
    out = []
    for k, buf in enumerate(planes[:3 if chroma else 1]):
        pw, ph = (width, height) if k == 0 else (width // 2, height // 2)
        new = g.integers(0, 256, buf.shape, dtype=np.uint8)
        new[:ph, :pw] = buf[:ph, :pw]
        out.append(new)
    return tuple(out + [None] * (3 - len(out)))


# the pictures of tests/golden/sao_frame.npz whose dst planes the golden also hashes: (name, chroma)
SAO_FIXTURE = (("ragged", 1), ("mono", 0), ("one", 1), ("tiny", 1))
