"""GPU: the kernel variants around the defaults, bit for bit against the oracle.

  * scaling lists through every fused quantize_residual kernel that takes them (the matrix-core tile kernel at 8 / 16 / 32,
    the 4x4 lane kernel, the LDS kernel) and through quant / dequant with sign hiding -- random tables that are asymmetric
    in raster order, list values 1 and 255 included, separate quantisation and dequantisation tables and each alone;
  * the kernels the tuning knobs select ("dct4_tile" 0, "dct_pipe" 1, "pipe" 1, "qr_tile_pipe" 0, KVZ_HIP_DCT32_VALU);
  * the later trips of the grid-stride loops: every "*_wgs_per_cu" cap set to 1 and to 3 with a count from the launcher's
    own formula that gives every wave at least two blocks and leaves the last sweep ragged, and a cap of 0 (counts as 1).
Every knob is restored to its default (-1) whatever happens."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
from patterns import rng

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUANT_SCALES = (26214, 23302, 20560, 18396, 16384, 14564)      # scalinglist.c:66
INV_QUANT_SCALES = (40, 45, 51, 57, 64, 72)                    # scalinglist.c:67
TABLES = ("both", "quant", "dequant")                          # which of the two tables a call is given


@pytest.fixture(scope="module")
def env():
    import torch
    from kvazaar_amd import _lib, api
    L = _lib.init(0)
    return api, _lib, L, torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture
def knobs(env):
    """knobs(key=value, ...) sets tuning knobs; every knob set is back at its default after the test"""
    with env[0].tuned() as set_:
        yield set_


def sweeps(per_wg, cap, cus):
    """a count for a grid-stride launch of `cap` workgroups per CU that take `per_wg` items per sweep: two full sweeps, half
    of a third and 3 more (a part-filled last workgroup / tile)"""
    sweep = per_wg * cap * cus
    return 2 * sweep + sweep // 2 + 3


def tables(w, qp, seed, which="both"):
    """(quant_coeff, dequant_coeff) in the legal range: qc = scale * 16 / v, dq = inv_scale * v for list values v in 1 .. 255
    (scalinglist.c:306-330), a different list for each, neither symmetric; v = 1 drives the level into the int16 clip and
    needs the 64-bit product, v = 255 the largest dequantisation factor"""
    g = rng(seed)

    def lst():
        v = g.integers(1, 256, w * w)
        v[g.choice(w * w, 2 + w // 4, replace=False)] = 1
        v[g.choice(w * w, 2 + w // 4, replace=False)] = 255
        v[0], v[1], v[w] = 1, 255, 40
        return v
    qt = ((QUANT_SCALES[qp % 6] << 4) // lst()).astype(np.int32)
    dt = (INV_QUANT_SCALES[qp % 6] * lst()).astype(np.int32)
    assert not (qt.reshape(w, w) == qt.reshape(w, w).T).all() and not (dt.reshape(w, w) == dt.reshape(w, w).T).all()
    return (qt if which != "dequant" else None), (dt if which != "quant" else None)


def residual_pairs(w, count, seed):
    """ref / pred TUs: random differences, TUs without residual, and the extremes (flat 255 against 0, checkerboards)"""
    g = rng(seed)
    ref = g.integers(0, 256, (count, w * w), dtype=np.uint8)
    pred = np.clip(ref.astype(np.int32) + g.integers(-70, 71, ref.shape), 0, 255).astype(np.uint8)
    pred[1::5] = ref[1::5]
    ref[2::7], pred[2::7] = 255, 0
    ref[3::11], pred[3::11] = 0, 255
    ref[4::13, ::2], pred[4::13, ::2] = 0, 255
    return ref, pred


def check_qr(api, ref, pred, w, qp, color, intra, qt, dt, signhide=0, scan=0, trskip=0, costs=False, alias=False, msg=""):
    many = ref.shape[0] > 256
    fn = O.quantize_residual_many if many else O.quantize_residual_batch
    want = fn(ref, pred, w, qp, color, scan, intra, intra, signhide, trskip, quant_coeff=qt, dequant_coeff=dt)
    got = api.quantize_residual_batch(ref, pred, w, qp, color, scan, intra, intra, signhide, trskip, alias_rec=alias,
                                      with_costs=costs, quant_coeff=qt, dequant_coeff=dt)
    tag = "%s w=%d count=%d qp=%d color=%d intra=%d sh=%d scan=%d ts=%d costs=%d alias=%d" % (
        msg, w, ref.shape[0], qp, color, intra, signhide, scan, trskip, costs, alias)
    for a, b, nm in zip(got[:3], want, ("rec", "coeff", "has")):
        np.testing.assert_array_equal(a, b, err_msg="%s %s" % (nm, tag))
    if costs:
        if many:   # the same two sums in numpy over the whole launch
            ssd = ((ref.astype(np.int64) - want[0].astype(np.int64)) ** 2).sum(axis=1)
            sab = np.abs(want[1].astype(np.int64)).sum(axis=1)
        else:
            ssd = [O.pixels_calc_ssd(ref[i], 0, want[0][i], 0, w, w, w) for i in range(ref.shape[0])]
            sab = [O.coeff_abs_sum(want[1][i]) for i in range(ref.shape[0])]
        np.testing.assert_array_equal(got[3], ssd, err_msg="ssd " + tag)
        np.testing.assert_array_equal(got[4], sab, err_msg="coeff_abs_sum " + tag)


def _qps(w):
    """QPs below and at / above the dequantisation's switch to clip-and-shift (luma qp >= 6 * (log2 w + 3))"""
    sw = 6 * {4: 5, 8: 6, 16: 7, 32: 8}[w]
    return (3, sw - 1, min(sw + 1, 51))


# ------------------------------------------------------------------ scaling lists through the fused kernels
@pytest.mark.parametrize("n", [8, 16, 32])
def test_tile_kernel_with_tables(env, knobs, n):
    """the matrix-core tile kernel's non-flat branches: per-coefficient quant factors through the kappa / lane layout, dequant
    modes 1 and 2; the plain and the cost entry (8x8 costs: the LDS kernel), both pipe settings; 1 TU, a part-filled tile,
    and several sweeps with a ragged tail (qr{n}_wgs_per_cu = 1); rec_out aliasing pred_in"""
    api, _, _, cus = env
    tus = (32 // n) ** 2
    big = sweeps(4 * tus, 1, cus)
    for count in (1, max(tus - 3, 2), big):
        ref, pred = residual_pairs(n, count, 300 + n + count)
        knobs(**{"qr%d_wgs_per_cu" % n: 1})
        for which in TABLES:
            for qp in (_qps(n) if count < big else _qps(n)[1:]):
                qt, dt = tables(n, qp, 7 * qp + n, which)
                for color in (((0, 1, 2) if n < 32 else (0,)) if count < big else (0,)):
                    for pipe in (1, 0):
                        knobs(qr_tile_pipe=pipe)
                        for costs in (False, True):
                            check_qr(api, ref, pred, n, qp, color, 0, qt, dt, costs=costs, msg="%s pipe=%d" % (which, pipe))
    knobs(qr_tile_pipe=-1)
    qt, dt = tables(n, 40, 99)
    ref, pred = residual_pairs(n, big, 77)
    check_qr(api, ref, pred, n, 40, 0, 1, qt, dt, alias=True)


@pytest.mark.parametrize("kind", ["dst", "dct", "trskip"])
def test_4x4_lane_kernel_with_tables(env, knobs, kind):
    """the FLAT = false instantiation of the 4x4 lane kernel (DST of intra luma, DCT, transform skip); its grid stride at qr4 = 1"""
    api, _, _, cus = env
    color, intra, ts = {"dst": (0, 1, 0), "dct": (2, 1, 0), "trskip": (1, 0, 1)}[kind]
    big = sweeps(256, 1, cus)
    knobs(qr4_wgs_per_cu=1)
    for count in (1, 3, 1000, big):
        ref, pred = residual_pairs(4, count, 400 + count)
        for which in TABLES:
            for qp in _qps(4):
                qt, dt = tables(4, qp, 11 * qp + count, which)
                check_qr(api, ref, pred, 4, qp, color, intra, qt, dt, trskip=ts, costs=count < big, alias=count == big,
                         msg="%s %s" % (kind, which))
    # same call with color 0 inter: plain DCT of luma
    qt, dt = tables(4, 30, 5)
    ref, pred = residual_pairs(4, 700, 5)
    check_qr(api, ref, pred, 4, 30, 0, 0, qt, dt, trskip=ts)


@pytest.mark.parametrize("n", [4, 8, 16, 32])
def test_lds_kernel_with_tables(env, knobs, n):
    """the LDS quantize_residual kernel with tables, reached through every route that selects it: qr_tile_kernel = 0 /
    qr4_lane_kernel = 0, sign hiding (every scan), and the 8x8 cost entry with tables; grid stride at qr = 1"""
    api, _, _, cus = env
    big = sweeps(256 // n, 1, cus)
    knobs(qr_wgs_per_cu=1)
    for count in (1, 5, big):
        ref, pred = residual_pairs(n, count, 500 + n + count)
        for which in TABLES:
            for qp in (_qps(n) if count < big else _qps(n)[:1]):
                qt, dt = tables(n, qp, 13 * qp + n, which)
                for color in ((0, 1, 2) if n < 32 else (0,)):
                    intra = color != 1
                    # sign hiding: the LDS kernel whatever the knobs say
                    for scan in ((0, 1, 2) if count < big else (0,)):
                        check_qr(api, ref, pred, n, qp, color, intra, qt, dt, signhide=1, scan=scan, costs=scan == 1,
                                 trskip=int(n == 4 and scan == 2), msg="signhide " + which)
                    knobs(qr_tile_kernel=0, qr4_lane_kernel=0)
                    check_qr(api, ref, pred, n, qp, color, intra, qt, dt, costs=color == 2, msg="knobs " + which)
                    knobs(qr_tile_kernel=-1, qr4_lane_kernel=-1)
                    if n == 8:
                        check_qr(api, ref, pred, n, qp, color, intra, qt, dt, costs=True, msg="8x8 cost " + which)
    qt, dt = tables(n, 27, 3)
    ref, pred = residual_pairs(n, 300, 9)
    check_qr(api, ref, pred, n, 27, 0, 1, qt, dt, signhide=1, alias=True)


@pytest.mark.parametrize("w", [4, 8, 16, 32])
def test_quant_sign_hiding_and_dequant_with_tables(env, knobs, w):
    """quant_batch with a table and sign hiding (every scan; the sign-hiding pass re-derives delta_u from the table),
    dequant_batch with a table in both modes; quant = 1 gives the elementwise kernels a second sweep"""
    api, _, _, cus = env
    g = rng(600 + w)
    count = sweeps(2048 // (w * w) if w < 32 else 2, 1, cus) if w >= 16 else 700
    coef = g.integers(-3000, 3001, (count, w * w)).astype(np.int16)
    coef[1::9] = g.integers(-32768, 32768, coef[1::9].shape)
    coef[2::9] = 0
    coef[3::9, ::5] = 1
    knobs(quant_wgs_per_cu=1)
    for qp in _qps(w):
        qt, dt = tables(w, qp, 17 * qp + w)
        for type_ in ((0,) if w == 32 else (0, 2)):
            for scan in (0, 1, 2):
                for intra_slice in (0, 1):
                    got = api.quant_batch(coef, w, qp, type_, scan, intra_slice, 1, quant_coeff=qt)
                    want = O.quant_batch(coef, w, qp, type_, scan, intra_slice, 1, quant_coeff=qt)
                    np.testing.assert_array_equal(got, want, err_msg="qp=%d type=%d scan=%d" % (qp, type_, scan))
            np.testing.assert_array_equal(api.dequant_batch(want, w, qp, type_, dequant_coeff=dt),
                                          O.dequant_batch(want, w, qp, type_, dequant_coeff=dt), err_msg="dequant qp=%d" % qp)


# ------------------------------------------------------------------ flat-path kernels the knobs select
def _extreme_blocks(n, count, seed):
    g = rng(seed)
    x = g.integers(-255, 256, (count, n * n)).astype(np.int16)
    x[::9] = g.integers(-32768, 32768, x[::9].shape)
    x[3::101] = 32767
    x[5::101] = -32768
    return x


def _check_transform(api, kind, n, x, msg=""):
    want = O.transform_many(kind, n, x) if x.shape[0] > 256 else O.transform_batch(kind, n, x)
    np.testing.assert_array_equal(api.transform_batch(kind, n, x), want, err_msg="%s %d count=%d %s" % (kind, n, x.shape[0], msg))


@pytest.mark.parametrize("kind", ["dct", "idct", "dst", "idst"])
def test_dct4_lds_kernel(env, knobs, kind):
    """dct4_tile = 0: the LDS transform_kernel<4, *>; its grid stride at dct = 1"""
    api, _, _, cus = env
    knobs(dct4_tile=0, dct_wgs_per_cu=1)
    for count in (1, 63, sweeps(64, 1, cus)):
        _check_transform(api, kind, 4, _extreme_blocks(4, count, 700 + count), "dct4_tile=0")


def test_dct32_pipe(env, knobs):
    """dct_pipe = 1: the hand-placed wait of the 32x32 matrix-core transform, forward and inverse, with its grid stride"""
    api, _, _, cus = env
    knobs(dct_pipe=1)
    for cap in (-1, 1, 3):
        knobs(dct32_wgs_per_cu=cap, idct32_wgs_per_cu=cap)
        for count in ((1, 5, 1001) if cap < 0 else (sweeps(4, cap, cus),)):
            x = _extreme_blocks(32, count, 710 + count)
            for kind in ("dct", "idct"):
                _check_transform(api, kind, 32, x, "dct_pipe=1 cap=%d" % cap)


def test_pipe_register_kernels(env, knobs):
    """pipe = 1: the prefetching 4x4 lane kernel (flat) and the 8x8 register kernel (qr8_tile_kernel = 0), each past its
    first sweep"""
    api, _, _, cus = env
    knobs(pipe=1, qr8_tile_kernel=0)
    for cap in (1, 3):
        knobs(qr4_wgs_per_cu=cap, qr8_wgs_per_cu=cap)
        for n, per_wg in ((4, 256), (8, 32)):
            for count in ((1, 3, 77) if cap == 1 else ()) + (sweeps(per_wg, cap, cus),):
                ref, pred = residual_pairs(n, count, 720 + n + count)
                for qp, color, intra in ((4, 0, 1), (30, 0, 0), (45, 2, 1)):
                    check_qr(api, ref, pred, n, qp, color, intra, None, None, msg="pipe=1 cap=%d" % cap)


_VALU_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import oracle_lib as O
from kvazaar_amd import _lib, api
from patterns import rng
L = _lib.init(0)
g = rng(730)
cus = int(sys.argv[2])
for n in (16, 32):
    for count in (1, 7, 2 * cus * 256 // n + 5):         # dct = 1: 256 / n blocks per workgroup, one workgroup per CU
        x = g.integers(-255, 256, (count, n * n)).astype(np.int16)
        x[::9] = g.integers(-32768, 32768, x[::9].shape)
        x[3::101] = 32767; x[5::101] = -32768
        for cap in (-1, 1):
            L.kvz_hip_set_tuning(b"dct_wgs_per_cu", cap)
            for kind in ("dct", "idct"):
                got = api.transform_batch(kind, n, x)
                want = O.transform_many(kind, n, x)
                if not (got == want).all():
                    print("MISMATCH", kind, n, count, cap); sys.exit(3)
print("VALU_OK")
"""


def test_dct32_valu_kernels_in_a_child(env):
    """KVZ_HIP_DCT32_VALU=1 (read once per process): the VALU / LDS 16x16 and 32x32 kernels, forward and inverse, in a fresh
    process under a time limit"""
    env_ = dict(os.environ, KVZ_HIP_DCT32_VALU="1")
    r = subprocess.run([sys.executable, "-c", _VALU_CHILD, ROOT, str(env[3])], env=env_, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=300)
    assert r.returncode == 0 and "VALU_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ------------------------------------------------------------------ grid-stride loops past the first sweep
@pytest.mark.parametrize("cap", [1, 3])
def test_grid_stride_transforms_and_costs(env, knobs, cap):
    """sad / satd8 / dct (8x8 LDS) / dct4 / dct16 / dct32 and their inverses with every wave taking two blocks or more and a
    ragged last sweep; dct32 with both pipe settings"""
    api, _, _, cus = env
    knobs(sad_wgs_per_cu=cap, satd8_wgs_per_cu=cap, dct_wgs_per_cu=cap, dct4_wgs_per_cu=cap, idct4_wgs_per_cu=cap,
          dct16_wgs_per_cu=cap, idct16_wgs_per_cu=cap, dct32_wgs_per_cu=cap, idct32_wgs_per_cu=cap)
    g = rng(800 + cap)
    for kind, n, per_wg in (("sad", 8, 1024 // 4), ("sad", 32, 1024 // 64), ("satd", 8, 256)):
        count = sweeps(per_wg, cap, cus)
        a = g.integers(0, 256, (count, n * n), dtype=np.uint8)
        b = np.clip(a.astype(np.int32) + g.integers(-40, 41, a.shape), 0, 255).astype(np.uint8)
        b[::7] = 255 - a[::7]
        np.testing.assert_array_equal(api.cost_nxn_batch(kind, n, a, b), O.cost_nxn_many(kind, n, a, b), err_msg="%s %d" % (kind, n))
    for kinds, n, per_wg in ((("dct", "idct"), 8, 256 // 8), (("dct", "idct", "dst", "idst"), 4, 256),
                             (("dct", "idct"), 16, 16), (("dct", "idct"), 32, 4)):
        x = _extreme_blocks(n, sweeps(per_wg, cap, cus), 810 + n)
        for kind in kinds:
            for pipe in ((0, 1) if n == 32 else (0,)):
                knobs(dct_pipe=pipe)
                _check_transform(api, kind, n, x, "cap=%d dct_pipe=%d" % (cap, pipe))


@pytest.mark.parametrize("cap", [1, 3])
def test_grid_stride_quant_kernels(env, knobs, cap):
    """quant / dequant, the LDS quantize_residual kernel (qr), the 4x4 lane kernel (qr4, both pipe settings), the 8x8 tile and
    register kernels (qr8 caps both; register kernel with both pipe settings), the 16x16 / 32x32 tile kernels (qr16 / qr32,
    both qr_tile_pipe settings) -- flat scaling, each past its first sweep with a ragged tail"""
    api, _, _, cus = env
    knobs(quant_wgs_per_cu=cap, qr_wgs_per_cu=cap, qr4_wgs_per_cu=cap, qr8_wgs_per_cu=cap, qr16_wgs_per_cu=cap,
          qr32_wgs_per_cu=cap)
    g = rng(900 + cap)
    w = 16
    coef = g.integers(-4000, 4001, (sweeps(2048 // (w * w), cap, cus), w * w)).astype(np.int16)
    q = api.quant_batch(coef, w, 22, 0, 0)
    np.testing.assert_array_equal(q, O.quant_batch(coef, w, 22, 0, 0))
    np.testing.assert_array_equal(api.dequant_batch(q, w, 22, 0), O.dequant_batch(q, w, 22, 0))
    # LDS kernel: 256 / n TUs per workgroup
    knobs(qr_tile_kernel=0, qr4_lane_kernel=0)
    for n in (4, 32):
        ref, pred = residual_pairs(n, sweeps(256 // n, cap, cus), 910 + n)
        check_qr(api, ref, pred, n, 27, 0, 1, None, None, msg="lds cap=%d" % cap)
    knobs(qr_tile_kernel=-1, qr4_lane_kernel=-1)
    ref, pred = residual_pairs(4, sweeps(256, cap, cus), 920)
    for pipe in (0, 1):
        knobs(pipe=pipe)
        check_qr(api, ref, pred, 4, 32, 0, 1, None, None, costs=pipe == 0, msg="qr4 pipe=%d" % pipe)
    ref, pred = residual_pairs(8, max(sweeps(64, cap, cus), sweeps(32, cap, cus)), 930)
    for tile8, pipe in ((1, 0), (0, 0), (0, 1)):
        knobs(qr8_tile_kernel=tile8, pipe=pipe)
        check_qr(api, ref, pred, 8, 30, 1, 0, None, None, msg="qr8 tile=%d pipe=%d" % (tile8, pipe))
    knobs(qr8_tile_kernel=-1, pipe=-1)
    for n in (16, 32):
        ref, pred = residual_pairs(n, sweeps(4 * (32 // n) ** 2, cap, cus), 940 + n)
        for pipe in (1, 0):
            knobs(qr_tile_pipe=pipe)
            for costs in (False, True):
                check_qr(api, ref, pred, n, 25, 0, 0, None, None, costs=costs, msg="qr%d pipe=%d" % (n, pipe))


def test_zero_caps_count_as_one(env, knobs):
    """a "*_wgs_per_cu" of 0 launches one workgroup per CU, not an empty grid"""
    api, _, _, cus = env
    knobs(sad_wgs_per_cu=0, dct_wgs_per_cu=0, dct4_wgs_per_cu=0, dct16_wgs_per_cu=0, idct32_wgs_per_cu=0, qr4_wgs_per_cu=0,
          qr8_wgs_per_cu=0, qr32_wgs_per_cu=0, quant_wgs_per_cu=0)
    g = rng(950)
    a = g.integers(0, 256, (sweeps(256, 1, cus), 64), dtype=np.uint8)
    b = g.integers(0, 256, a.shape, dtype=np.uint8)
    np.testing.assert_array_equal(api.cost_nxn_batch("sad", 8, a, b), O.cost_nxn_many("sad", 8, a, b))
    for kind, n, per_wg in (("dct", 8, 32), ("dct", 4, 256), ("dct", 16, 16), ("idct", 32, 4)):
        _check_transform(api, kind, n, _extreme_blocks(n, sweeps(per_wg, 1, cus), 960 + n), "cap 0")
    for n, per_wg in ((4, 256), (8, 64), (32, 4)):
        ref, pred = residual_pairs(n, sweeps(per_wg, 1, cus), 970 + n)
        check_qr(api, ref, pred, n, 29, 0, 1, None, None, msg="cap 0")
    coef = g.integers(-900, 901, (sweeps(2, 1, cus), 1024)).astype(np.int16)
    np.testing.assert_array_equal(api.quant_batch(coef, 32, 20, 0, 0), O.quant_batch(coef, 32, 20, 0, 0))
