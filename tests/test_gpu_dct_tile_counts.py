"""The matrix-core transform tiles (dct32_mfma_core.h: one 32x32 block, four 16x16 or sixty-four 4x4 blocks per tile, one tile per
wave, four waves per workgroup) at block counts on both sides of one wave, one workgroup and a ragged last tile, with the extreme
int16 values in the mix -- bit-exact against the oracle.  The fused quantize_residual kernels share the tile layout."""
import numpy as np
import pytest

import oracle_lib as O
from patterns import rng

pytestmark = pytest.mark.gpu

COUNTS = (1, 2, 3, 4, 5, 7, 8, 9, 65)


@pytest.fixture(scope="module")
def api():
    from kvazaar_amd import api as a, _lib
    _lib.init(0)
    return a


def _blocks(n, count, seed):
    """random int16 blocks; every third block starts with a run of -32768, 32767 and 0, block 1 is all -32768, block 2 all 32767,
    block 4 all zero (int16 has no +32768: 32767 stands in for it)"""
    g = rng(seed)
    x = g.integers(-32768, 32768, (count, n * n)).astype(np.int16)
    x[::3, 0:3] = (-32768, 32767, 0)
    if count > 1:
        x[1] = -32768
    if count > 2:
        x[2] = 32767
    if count > 4:
        x[4] = 0
    return x


@pytest.mark.parametrize("kind,n", [("dct", 32), ("idct", 32), ("dct", 16), ("idct", 16), ("dct", 4), ("idct", 4), ("dst", 4), ("idst", 4)])
def test_transform_tile_counts(api, kind, n):
    for count in COUNTS:
        x = _blocks(n, count, 7000 + 10 * n + count)
        np.testing.assert_array_equal(api.transform_batch(kind, n, x), O.transform_many(kind, n, x, threads=1),
                                      err_msg="%s %dx%d, %d blocks" % (kind, n, n, count))
        # residual-sized values (what an encoder feeds the forward transform, and small coefficients for the inverse)
        y = rng(7500 + 10 * n + count).integers(-255, 256, (count, n * n)).astype(np.int16)
        np.testing.assert_array_equal(api.transform_batch(kind, n, y), O.transform_many(kind, n, y, threads=1),
                                      err_msg="%s %dx%d, %d blocks (residuals)" % (kind, n, n, count))


@pytest.mark.parametrize("n", [8, 16, 32])
def test_quantize_residual_tile_counts(api, n):
    for count in (1, 5, 17):
        g = rng(7900 + n + count)
        ref_in = g.integers(0, 256, (count, n * n), dtype=np.uint8)
        pred = np.clip(ref_in.astype(np.int32) + g.integers(-50, 51, ref_in.shape), 0, 255).astype(np.uint8)
        pred[0] = 255 - ref_in[0]                                # extreme residuals
        if count > 1:
            pred[1] = ref_in[1]                                  # a TU that quantises to nothing
        for qp in (12, 32):
            got = api.quantize_residual_batch(ref_in, pred, n, qp, 0, 0, 0)
            want = O.quantize_residual_batch(ref_in, pred, n, qp, 0, 0, 0)
            for a, b, nm in zip(got, want, ("rec", "coeff", "has")):
                np.testing.assert_array_equal(a, b, err_msg="%s %dx%d, %d TUs, qp %d" % (nm, n, n, count, qp))
